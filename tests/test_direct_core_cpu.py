"""The mathematics of the D = 4 direct-solve kernel (qmps_amd/csrc/qmps_direct_core.h - the very source the GPU
kernel is compiled from) run on the CPU in a four-lane lock-step emulation and compared with the oracle.
CPU only: the GPU parity tests proper are in test_direct_gpu.py."""
import numpy as np
import pytest

from oracle import qmps_oracle as O
from tests import direct_emu as EMU

H3 = lambda rng: np.stack([O.hamiltonian_matrix({'ZZ': -1, 'X': 1}),
                           O.hamiltonian_matrix({'XX': 1, 'YY': 1, 'ZZ': 0.5}),
                           rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))])


def test_golden_vectors_d4(golden):
    out = EMU.energies_d4(golden['ref_A_D4'], golden['ref_h_tfim'])
    assert np.all(out['status'] == 0) and np.all(out['iters'] == 1)
    assert np.abs(out['E'][:, 0] - golden['oracle_E_closed_D4']).max() < 1e-12
    assert np.abs(out['E'][:, 0] - golden['oracle_E_statevec_D4']).max() < 1e-12
    assert np.abs(out['r'] - golden['oracle_r_D4']).max() < 1e-12


def test_haar_batch_against_the_oracle():
    rng = np.random.default_rng(11)
    A = O.unitary_to_tensor(O.haar_unitaries(rng, 8, 400))
    h = H3(rng)
    out = EMU.energies_d4(A, h)
    assert np.all(out['status'] == 0) and np.all(out['iters'] == 1) and out['resid'].max() < 1e-14
    assert np.abs(out['E_lean'] - out['E']).max() < 1e-13          # the density-matrix-free route of the energy-only kernel
    for b in range(0, 400, 7):
        r, it, st = O.env_direct(A[b])
        assert (it, st) == (1, 0)
        assert np.abs(out['r'][b] - r).max() < 1e-13
        assert np.abs(out['rho'][b] - O.two_site_rdm(A[b], r)).max() < 1e-13
        for t in range(3):
            assert abs(out['E'][b, t] - O.energy_closed_form(A[b], h[t], r)) < 1e-13
        _, rr = O.env_dense_eig(A[b])          # and the reference's own route: the dominant eigen-matrix
        assert np.abs(out['r'][b] - rr).max() < 1e-12


def test_ansatz_family_d4():
    """ShallowCNOT depth-2 tensors (the optimisers' default ansatz, represent.py:288-310): structured, far from Haar."""
    rng = np.random.default_rng(12)
    A = np.stack([O.unitary_to_tensor(O.shallow_cnot_unitary(4, rng.standard_normal(4))) for _ in range(300)])
    h = O.hamiltonian_matrix({'ZZ': -1, 'X': 1})
    out = EMU.energies_d4(A, h)
    ok = out['status'] == 0
    assert ok.mean() > 0.95
    for b in np.flatnonzero(ok)[::5]:
        assert abs(out['E'][b, 0] - O.energy_closed_form(A[b], h)) < 1e-11


def test_fallback_non_isometric_and_degenerate():
    rng = np.random.default_rng(13)
    A = O.unitary_to_tensor(O.haar_unitaries(rng, 8, 60))
    A = A * rng.uniform(0.6, 1.5, size=(60, 1, 1, 1)) + 0.05 * (rng.standard_normal(A.shape) + 1j * rng.standard_normal(A.shape))
    h = O.hamiltonian_matrix({'ZZ': -1, 'X': 1})
    out = EMU.energies_d4(A, h, max_iter=100000)
    assert np.all(out['status'] == 0) and np.all(out['iters'] > 1)
    for b in range(60):
        r, it, st = O.env_direct(A[b], max_iter=100000)
        assert st == 0 and it == out['iters'][b]
        assert np.abs(out['r'][b] - r).max() < 1e-12
        assert np.abs(out['r'][b] - O.env_dense_eig(A[b])[1]).max() < 1e-10
    # the iteration cap is reported, not hidden: 1 verification step + 2^1 squared steps <= 3
    cut = EMU.energies_d4(A[:5], h, max_iter=3)
    assert np.all(cut['status'] == 1) and np.all(cut['iters'] == 3)
    # product state |00..0>: rank-one environment -> not positive definite (the reference's LinAlgError branch)
    U = np.eye(8, dtype=complex)[None]
    out = EMU.energies_d4(O.unitary_to_tensor(U), h)
    assert out['status'][0] == 2 and abs(out['E'][0, 0] + 1.0) < 1e-12
    E, it, st = O.energy_direct(O.unitary_to_tensor(U)[0], h)
    assert st == 2 and abs(E + 1.0) < 1e-12


def test_near_singular_environments_every_status():
    """The family of tests/conditioning_cases.py at D = 4 through the emulation: the gauged sweep t = 1 .. 1e-9 (19 strengths x 64), the
    ungauged slice (the elimination is not accepted: the power method 2^m steps at a time) and 512 Haar rows.  r, rho, E (three terms, one
    not Hermitian) and E_lean of EVERY row of status 0 or 2 against the mpmath reference within 1e-10, rho Hermitian with trace 1 and no
    eigenvalue below -1e-13, rho against two_site_rdm of the kernel's own r within 1e-13, r against oracle.env_direct within 1e-12 where both
    accept the solve in one step; status 0 wherever the reference's smallest eigenvalue is >= 1e-13, status 2 only below.  Both routes of
    DirectD4::density carry weight: among the rows with t <= 3e-5 at least a fifth is status 2 (the Y = B r route) and at least a fifth
    status 0 (the LDL^H route at pivots of ~1e-16).
    Measured: r 5.8e-15, rho 6.4e-15, E 1.2e-14, E_lean 1.1e-14, rho against its own r 1.0e-15, r against env_direct 2.8e-15, trace 6.2e-15,
    smallest eigenvalue of rho -3.2e-15, rho exactly Hermitian; 1 459 rows status 0, 405 status 2, none status 1.
    With one sign flipped in the LDL^H branch of density() (G_tau = B_tau L) or in its Y = B r branch the assertion
    `fig['r'] < R_TOL and fig['rho'] < R_TOL and fig['E'] < E_TOL` of conditioning_cases.compare fails (rho off by 0.6 / 0.5, E by 3.0 / 1.3);
    the second flip passes every other test of this file."""
    from tests import conditioning_cases as CC
    fam = CC.family(4)
    h = CC.hamiltonian_terms()
    out = EMU.energies_d4(fam['A'], h)
    CC.compare(4, out, h, 'emulation', one_step=True, rho_self=True)
    st, it = out['status'], out['iters']
    assert not np.any(st == 1)
    assert np.all(it[fam['gauged']] == 1)
    small = fam['gauged'] & (fam['t'] > 0) & (fam['t'] <= 3e-5)          # the strengths 1e-5 .. 1e-9 of the sweep
    assert (st[small] == 2).mean() >= 0.2 and (st[small] == 0).mean() >= 0.2, (st[small] == 2).mean()
    # the ungauged slice leaves the one-step solve (a pivot below 1e-10 without pivoting) and comes back with status 0 or 2 all the same
    un = ~fam['gauged']
    assert (it[un] > 1).mean() > 0.5 and np.all(np.log2(it[un & (it > 1)] - 1) % 1 == 0)


@pytest.mark.parametrize('D', [2, 4, 8, 16])
def test_double_precision_references_against_mpmath(D):
    """oracle.env_direct (pivoted LU) against the mpmath solve of the same system on the rows that have one (tests/conditioning_cases.py):
    it is the reference of the rows mpmath is too slow for.  1e-13: backward error N eps times the condition number 1 / gap <= ~1e3 of the
    system.  Measured 7.2e-16, 6.7e-16, 9.4e-16, 9.0e-16 at D = 2, 4, 8, 16 (the dense eigen-solve: 3.7e-12 at D = 2)."""
    from tests import conditioning_cases as CC
    fam, ref, dref = CC.family(D), CC.references(D), CC.direct_references(D)
    ex = np.flatnonzero(fam['exact'])
    assert all(dref[b][1:] == (1, 0) for b in ex)
    assert max(np.abs(dref[b][0] - ref['r'][b]).max() for b in ex) < 1e-13
    assert np.abs(np.einsum('bsij,bsik->bjk', fam['A'].conj(), fam['A']) - np.eye(D)).max() < 1e-13
    # the reference rho is oracle.two_site_rdm in double on the rounded r: against the same contraction in mpmath on a few rows.  1e-14: entries
    # of modulus <= 1, sums of at most 2 D^2 products (~50 eps at D = 16).  Measured 5.6e-16 at most.
    worst = max(np.abs(CC.two_site_rdm_mp(fam['A'][b], ref['r'][b]) - ref['rho'][b]).max() for b in ex[::max(1, len(ex) // 4)][:4])
    print(f'reference rho against mpmath D={D}: {worst:.2e}')
    assert worst < 1e-14
