"""E, r and rho on near-singular environments, every status, D = 2 .. 16 (GPU, through EnergyEngine).

The other GPU tests compare density matrices, environments and energies on Haar tensors (smallest eigenvalue of r ~1e-2)
and only where the status is 0.  Here the rows are the family of tests/conditioning_cases.py - near-product tensors behind
a random gauge, smallest eigenvalue of r from 1e-2 down to the rounding noise of r, either sign - and EVERY row of status
0 or 2 is compared with the mpmath reference (1e-10 for E, r, rho: BASELINE.json): status 2 (QMPS_STATUS_NOT_PD) is no
error status, the optimisers use such energies.  A row whose reference lam_min is at or above the band must be status 0,
a status-2 row must lie below it; inside the band either status is right and the numbers are checked all the same.
The band: 1e-13 at D = 2, 4 (the error of r, 3e-15 measured, plus the backward error of a 4 x 4 LDL^H, a few eps ||r||,
with a margin of ~30), 1e-12 at D = 8, 16 (larger factorisations).

Worst figures measured on one MI355X are in the docstrings of the tests and in profiles/EXPERIMENTS.md."""
import numpy as np
import pytest

from tests import conditioning_cases as CC

pytestmark = pytest.mark.gpu

SMALL_T = 3e-5            # the strengths 1e-5 .. 1e-9 of the sweep: the D = 4 rows split between status 0 and status 2


def collect(eng, A, h, **kw):
    """One-shot call with the engine's selected solver; everything the engine can report about the batch."""
    E, it, st = eng.energies(A, h, **kw)
    cost = eng.summed_cost().copy()
    return {'E': E.copy(), 'iters': it.copy(), 'status': st.copy(), 'r': eng.environments().copy(), 'rho': eng.rdm().copy(), 'cost': cost}


def same_bits(a, b, keys=('E', 'r', 'rho', 'iters', 'status')):
    return [k for k in keys if not np.array_equal(a[k], b[k])]


@pytest.fixture(scope='module')
def d4():
    """The D = 4 rows, shuffled once: 1 864 rows (not a multiple of 16: the last wave is ragged)."""
    fam = CC.family(4)
    B = len(fam['A'])
    assert B % 16 != 0
    perm = np.random.default_rng(4242).permutation(B)
    return {'fam': fam, 'perm': perm, 'A': np.ascontiguousarray(fam['A'][perm]), 'h': CC.hamiltonian_terms(), 'B': B}


@pytest.fixture(scope='module')
def d4_direct(d4, engine_factory):
    eng = engine_factory(4, 8192)
    eng.set_solver('direct', handoff=0)
    return collect(eng, d4['A'], d4['h'])


def test_fused_direct_d4_every_status(d4, d4_direct, engine_factory):
    """energy_direct_d4_kernel (E, r, iterations, status) and energy_only_d4_kernel's rho route (eng.rdm()) on the shuffled family:
    all rows of status 0 or 2 against the reference, the status band, rho against two_site_rdm of the kernel's own r (1e-13), r against
    oracle.env_direct where accepted in one step (1e-12), summed_cost against E.sum(0), and the launch without the environment store.
    Conditions on the test itself: no row is status 1; among the rows with t <= 3e-5 at least a fifth is status 0 and at least a fifth
    status 2; at least 10 aligned groups of 16 consecutive rows (the evaluations of one wave) hold both statuses.
    Measured on one MI355X, 1 864 rows: r 7.2e-15, rho 6.4e-15, E 2.1e-14, rho against its own r 2.4e-15, r against env_direct 7.2e-15,
    |tr rho - 1| 6.9e-15, smallest eigenvalue of rho -3.1e-15, rho exactly Hermitian; 1 522 rows status 0, none status 1, 342 status 2
    (877 rows inside the band); 109 of the 116 full waves hold both statuses; the 136 rows of the ungauged slice, and only they, take
    the power fall-back."""
    out, A, h, B, perm = d4_direct, d4['A'], d4['h'], d4['B'], d4['perm']
    st = out['status']
    CC.compare(4, out, h, 'fused direct kernel', rows=perm, one_step=True, rho_self=True)
    assert not np.any(st == 1)
    t, gauged = d4['fam']['t'][perm], d4['fam']['gauged'][perm]
    small = (t > 0) & (t <= SMALL_T)
    mixed = sum(1 for g in range(B // 16) if len(set(st[16 * g:16 * g + 16])) > 1)
    print(f'status 2 among t <= 3e-5: {(st[small] == 2).mean():.3f}; waves with both statuses: {mixed} of {B // 16}; '
          f'iterations > 1: {(out["iters"] > 1).sum()} ({(out["iters"][~gauged] > 1).sum()} of the ungauged slice)')
    assert (st[small] == 0).mean() >= 0.2 and (st[small] == 2).mean() >= 0.2
    assert mixed >= 10
    assert np.all(out['iters'][gauged] == 1)
    assert np.abs(out['cost'] - out['E'].sum(0)).max() < 1e-10
    # without the environment store: the same kernel, the same numbers
    eng = engine_factory(4, 8192)
    eng.set_tensors(A)
    eng.set_hamiltonian(h)
    eng.launch(B, solver='direct', store_env=False)
    E2, it2, st2 = eng.results(B)
    assert np.array_equal(E2, out['E']) and np.array_equal(it2, out['iters']) and np.array_equal(st2, st)
    eng.cost_launch(B)
    assert np.abs(eng.get_cost() - E2.sum(0)).max() < 1e-10


def test_no_result_depends_on_the_wave_mates_d4(d4, d4_direct, engine_factory):
    """DirectD4::density takes the Y = B r route in a wave-uniform branch when ANY evaluation of the wave fails the
    positive-definiteness test, with a select per evaluation: E, r, rho, iterations and status of a row must not depend on the
    other fifteen evaluations of its wave.  The same rows under a second permutation, and 32 rows (16 of status 2) as batches of
    one: bit-identical.  The energy-only launch under a permutation likewise.  Measured on one MI355X: identical throughout."""
    A, h, B, perm = d4['A'], d4['h'], d4['B'], d4['perm']
    eng = engine_factory(4, 8192)
    eng.set_solver('direct', handoff=0)
    p2 = np.random.default_rng(4243).permutation(B)
    second = collect(eng, A[p2], h)
    first = {k: d4_direct[k][p2] for k in ('E', 'r', 'rho', 'iters', 'status')}
    assert same_bits(first, second) == []
    st = d4_direct['status']
    rng = np.random.default_rng(4244)
    chosen = np.concatenate([rng.choice(np.flatnonzero(st == 2), 16, replace=False), rng.choice(np.flatnonzero(st == 0), 16, replace=False)])
    for b in chosen:
        alone = collect(eng, A[b:b + 1], h)
        assert same_bits({k: d4_direct[k][b:b + 1] for k in first}, alone) == [], b
    # energy-only launch on resident environments, rows permuted together with their environments
    for n_terms in (2, 3):
        eng.set_tensors(A)
        eng.set_hamiltonian(h[:n_terms])
        eng.set_env_guess(d4_direct['r'])
        eng.launch_energy_only(B)
        E1, _, _ = eng.results(B)
        eng.set_tensors(A[p2])
        eng.set_env_guess(d4_direct['r'][p2])
        eng.launch_energy_only(B)
        E2, _, _ = eng.results(B)
        assert np.array_equal(E1[p2], E2), n_terms


@pytest.mark.parametrize('n_terms', [1, 2, 3])
def test_energy_only_kernel_d4(n_terms, d4, d4_direct, engine_factory):
    """energy_only_d4_kernel on the resident environments of the batch: the density-matrix-free route (one or two terms) and the rho
    route (three), also with the environments rescaled by random positive factors (the pass normalises by the trace): all rows
    against the reference energies (1e-10) and against the fused kernel's (1e-12: the same environments, another contraction order).
    Measured on one MI355X (n_terms 1 / 2 / 3): against the reference 2.3e-14 / 2.2e-14 / 2.1e-14 as stored, 2.6e-14 / 2.6e-14 / 2.4e-14
    rescaled; against the fused kernel 4.0e-15 / 4.0e-15 / 3.6e-15 and 6.7e-15 / 6.7e-15 / 4.9e-15."""
    A, B, perm = d4['A'], d4['B'], d4['perm']
    h = d4['h'][3 - n_terms:]                    # the non-Hermitian term is in every selection
    Eref = CC.reference_energies(4, h)[perm]
    eng = engine_factory(4, 8192)
    eng.set_hamiltonian(h)
    eng.set_tensors(A)
    eng.launch(B, solver='direct', store_env=True)
    E0, _, st = eng.results(B)
    assert np.array_equal(st, d4_direct['status']) and np.array_equal(E0, d4_direct['E'][:, 3 - n_terms:])
    r = eng.environments(B)
    rng = np.random.default_rng(4245)
    worst = []
    for scale in (None, rng.uniform(0.5, 3.0, size=(B, 1, 1))):
        if scale is not None:
            eng.set_env_guess(r * scale)
        eng.launch_energy_only(B)
        E1, _, st1 = eng.results(B)
        worst.append((float(np.abs(E1 - Eref).max()), float(np.abs(E1 - E0).max())))
        assert np.array_equal(st1, st)             # the pass without a positive-definiteness test leaves the statuses alone
    print(f'conditioning D=4 energy-only n_terms={n_terms}: (against the reference, against the fused kernel) as stored {worst[0]}, rescaled {worst[1]}')
    for ref_err, self_err in worst:
        assert ref_err < CC.E_TOL and self_err < 1e-12


@pytest.mark.parametrize('solver', ['squaring', 'plain', 'plain_lane'])
def test_other_solvers_d4(solver, d4, d4_direct, engine_factory, monkeypatch):
    """The same rows through the squaring solver (from the start: hand-off 0) and the plain power iteration, the latter with the row
    kernel and with the lane kernel (QMPS_POWER_LANE=1): every row of status 0 or 2 against the reference; the statuses may differ from
    the direct kernel's only inside the band (outside it every row is status 0 on every path).
    Measured on one MI355X (squaring / plain row kernel / plain lane kernel): r 5.7e-15 / 4.7e-13 / 4.7e-13, rho 6.3e-15 / 4.0e-13 / 4.0e-13,
    E 9.3e-15 / 1.7e-12 / 1.7e-12, rho against its own r 2.4e-15 / 2.6e-15 / 2.1e-15; status 0 : 2 = 1 340 : 524 / 1 520 : 344 / 1 451 : 413, none
    status 1; 322 / 290 / 305 statuses differ from the direct kernel's, the largest reference lam_min among those rows 1.4e-15."""
    A, h, perm = d4['A'], d4['h'], d4['perm']
    eng = engine_factory(4, 8192)
    try:
        if solver == 'plain_lane':
            monkeypatch.setenv('QMPS_POWER_LANE', '1')
        else:
            monkeypatch.delenv('QMPS_POWER_LANE', raising=False)
        eng.set_solver('squaring' if solver == 'squaring' else 'plain', handoff=0)
        out = collect(eng, A, h)
    finally:
        monkeypatch.delenv('QMPS_POWER_LANE', raising=False)
        eng.set_solver('direct', handoff=0)
    CC.compare(4, out, h, solver, rows=perm, rho_self=True)
    lam = CC.references(4)['lam_min'][perm]
    differ = out['status'] != d4_direct['status']
    print(f'conditioning D=4 {solver}: statuses that differ from the direct kernel\'s: {differ.sum()}, largest lam_min among them '
          f'{lam[differ].max() if differ.any() else 0.0:.2e}; iterations max {out["iters"].max()}')
    assert not np.any(differ & (lam >= CC.BAND[4]))
    assert np.abs(out['cost'] - out['E'].sum(0)).max() < 1e-10


@pytest.mark.parametrize('D,solver', [(2, 'direct'), (2, 'squaring'), (2, 'plain'), (8, 'direct'), (8, 'plain'), (16, 'squaring'), (16, 'plain')])
def test_other_bond_dimensions(D, solver, engine_factory):
    """D = 2 (the 4 x 4 solve in the lane, the squaring tail, the plain iteration), D = 8 (the wave-per-evaluation direct solve behind the
    block kernel; its plain iteration) and D = 16 (the matrix-core power iteration with the Krylov fall-back - the library's default
    there - and alone): the gauged sweep, 19 strengths x 32 rows (D = 16: 7 x 8), in a fixed shuffle.  Same assertions: every row of
    status 0 or 2 against the reference, the status band (1e-13 at D = 2, 1e-12 at D = 8 and 16: all three kernels test the pivots of
    a Cholesky / LDL^H factorisation for > 0), both statuses present, r against oracle.env_direct where the direct solves accept.
    Measured on one MI355X (r, rho, E; status 0 : 2; none status 1 anywhere):
      D = 2  direct 3.0e-15, 2.2e-15, 6.2e-15; 542 : 66 (r against env_direct 3.2e-15)   squaring 3.4e-15, 2.2e-15, 6.2e-15; 548 : 60
             plain 1.1e-12, 4.1e-13, 6.5e-13; 565 : 43            (186 of 608 rows inside the band)
      D = 8  direct 3.2e-15, 3.2e-15, 7.1e-15; 297 : 311 (r against env_direct 3.5e-15)  plain 1.7e-13, 1.3e-13, 3.6e-13; 296 : 312
             (394 of 608 rows inside the band; rho Hermitian to 1.5e-16)
      D = 16 squaring and plain alike (the power iteration converges before the Krylov hand-over): 4.1e-14, 3.0e-14, 1.1e-13; 24 : 32
             (40 of 56 rows inside the band; rho Hermitian to 3.0e-16)."""
    fam = CC.family(D)
    B = len(fam['A'])
    perm = np.random.default_rng(4250 + D).permutation(B)
    A = np.ascontiguousarray(fam['A'][perm])
    h = CC.hamiltonian_terms()
    eng = engine_factory(D, 4096)
    default = 'squaring' if D == 16 else 'direct'
    try:
        eng.set_solver(solver, handoff=0)
        out = collect(eng, A, h)
    finally:
        eng.set_solver(default, handoff=0)
    CC.compare(D, out, h, solver, rows=perm, one_step=(solver == 'direct'))
    st = out['status']
    print(f'conditioning D={D} {solver}: iterations max {out["iters"].max()}, rows with iterations > 1: {(out["iters"] > 1).sum()}')
    assert np.any(st == 0) and np.any(st == 2)
    if solver == 'direct':
        assert not np.any(st == 1) and np.all(out['iters'] == 1)
    assert np.abs(out['cost'] - out['E'].sum(0)).max() < 1e-10
