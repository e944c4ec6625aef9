"""The two-site cell, brick-wall and SU(N) kernels at their edges (GPU): the kernels behind NonSparseFullTwoSiteEnergyOptimizer, new_tdvp
and NonSparseFullEnergyOptimizer held to the standard of the main path - an mpmath reference, every status compared, inputs where the
solves change branch, and bit-identical results wherever an evaluation sits in a batch.  Rows, references and the conditions they meet:
tests/side_kernel_cases.py (proved on the references alone by tests/test_side_kernel_cases_cpu.py).

Worst figures measured on one MI355X are in the docstrings of the tests and in profiles/EXPERIMENTS.md."""
import numpy as np
import pytest

import side_kernel_cases as SK
from oracle import qmps_oracle as O
from qmps_amd import new_tdvp as NT
from tests import conditioning_cases as CC

pytestmark = pytest.mark.gpu


def fmt(fig):
    return ' '.join(f'{k}={v:.2e}' if isinstance(v, float) else f'{k}={v}' for k, v in fig.items())


def bits_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. two-site unit cell (qmps_cell2.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def run_cells(eng, U1, U2, h):
    E, it, st = eng.cell2_energies(U1, U2, h)
    return {'E': E.copy(), 'iters': it.copy(), 'status': st.copy()}


def cells_differ(a, b):
    return [k for k in ('E', 'iters', 'status') if bits_differ(a[k], b[k])]


@pytest.fixture(scope='module')
def cells(engine_factory):
    fam, ref = SK.cell_family(), SK.cell_references()
    perm = SK.cell_shuffle()
    c = {'fam': fam, 'ref': ref, 'perm': perm, 'U1': np.ascontiguousarray(fam['U1'][perm]), 'U2': np.ascontiguousarray(fam['U2'][perm]),
         'h': CC.hamiltonian_terms(), 'eng': engine_factory(2)}
    c['out'] = run_cells(c['eng'], c['U1'], c['U2'], c['h'])
    return c


def test_two_site_cell_every_status(cells):
    """cell2_lane_kernel on the 169 shuffled cells, three terms (the last complex and not Hermitian): no row is status 1; every row of
    status 0 or 2 within 1e-10 of the mpmath reference on every term; lam_min (the smaller of r12's and r21's) at or above 1e-13 means
    status 0, a status-2 row lies below; at least a fifth of the 80 rows with t <= 1e-5 in each status; iterations == 1 on the gauged and
    Haar rows, > 1 on every ungauged row with t <= 1e-6 (the power loop after a rejected 4 x 4 solve).
    Measured on one MI355X: max |dE| 4.4e-15 over all rows and terms (per strength 8.9e-16 .. 4.4e-15, Haar 8.9e-16); 142 rows status 0,
    none status 1, 27 status 2 (61 rows inside the band; the largest reference lam_min of a status-2 row 9.7e-17); of the 80 rows with
    t <= 1e-5, 53 status 0 and 27 status 2 (gauged t = 1e-8 / 1e-9 / 1e-10 / 1e-11: 6 / 8 / 6 / 7 of 8; every other strength 0); iterations
    3, 2, 2 on the ungauged rows at t = 1e-6, 1e-7, 1e-9 (the power loop starts from 1 / D and a near-product map is nearly a projection),
    1 on every other row, the ungauged t = 1e-4 included."""
    out, fam, ref, perm = cells['out'], cells['fam'], cells['ref'], cells['perm']
    st, it = out['status'], out['iters']
    t, gauged, lam = fam['t'][perm], fam['gauged'][perm], ref['lam_min'][perm]
    err = np.abs(out['E'] - ref['E'][perm]).max(axis=1)
    for tt in sorted(set(t), reverse=True):
        for g in (True, False):
            m = (t == tt) & (gauged == g)
            if m.any():
                print(f'cell2 t={tt:g} {"gauged" if g else "ungauged"}: rows {m.sum()} max |dE| {err[m].max():.2e} status 0/1/2 '
                      f'{(st[m] == 0).sum()}/{(st[m] == 1).sum()}/{(st[m] == 2).sum()} iterations {it[m].min()}..{it[m].max()}')
    small = (t > 0) & (t <= SK.CELL_SMALL_T)
    fig = {'rows': len(st), 'status0': int((st == 0).sum()), 'status1': int((st == 1).sum()), 'status2': int((st == 2).sum()),
           'E': float(err[st != 1].max()), 'in_band': int((lam < CC.BAND[2]).sum()), 'small_rows': int(small.sum()),
           'small_status0': int((st[small] == 0).sum()), 'small_status2': int((st[small] == 2).sum()),
           'largest_lam_min_of_a_status2_row': float(lam[st == 2].max()) if np.any(st == 2) else 0.0}
    print('cell2: ' + fmt(fig))
    assert not np.any(st == 1)
    assert fig['E'] < CC.E_TOL, fig
    wrong0 = np.flatnonzero((lam >= CC.BAND[2]) & (st != 0))
    wrong2 = np.flatnonzero((st == 2) & ~(lam < CC.BAND[2]))
    assert len(wrong0) == 0, ('lam_min >= band but status != 0', perm[wrong0], lam[wrong0], st[wrong0])
    assert len(wrong2) == 0, ('status 2 outside the band', perm[wrong2], lam[wrong2])
    assert (st[small] == 0).mean() >= 0.2 and (st[small] == 2).mean() >= 0.2, fig
    assert np.all(it[gauged] == 1)
    power = ~gauged & (t <= SK.CELL_POWER_T)
    assert power.sum() == 3 * SK.CELL_PER_T and np.all(it[power] > 1), it[power]


def test_two_site_cell_does_not_depend_on_the_lane_mates(cells):
    """One evaluation per lane, 64 per workgroup: the same cells under a second permutation, and 16 of them (8 of each status) as batches
    of one - E, iterations and status bit-identical.  Measured on one MI355X: identical throughout."""
    out, eng, h = cells['out'], cells['eng'], cells['h']
    B = len(out['status'])
    p2 = np.random.default_rng(9210).permutation(B)
    second = run_cells(eng, cells['U1'][p2], cells['U2'][p2], h)
    assert cells_differ({k: v[p2] for k, v in out.items()}, second) == []
    rng = np.random.default_rng(9211)
    st = out['status']
    chosen = np.concatenate([rng.choice(np.flatnonzero(st == 2), 8, replace=False), rng.choice(np.flatnonzero(st == 0), 8, replace=False)])
    for b in chosen:
        alone = run_cells(eng, cells['U1'][b:b + 1], cells['U2'][b:b + 1], h)
        assert cells_differ({k: v[b:b + 1] for k, v in out.items()}, alone) == [], b


def test_two_site_cell_terms_one_by_one(cells):
    """n_terms = 3 in one call against three calls with one term each: bit-identical energies, iterations and statuses.
    Measured on one MI355X: identical."""
    out, eng, h = cells['out'], cells['eng'], cells['h']
    for q in range(3):
        one = run_cells(eng, cells['U1'], cells['U2'], h[q:q + 1])
        assert not bits_differ(one['E'][:, 0], out['E'][:, q]), q
        assert not bits_differ(one['iters'], out['iters']) and not bits_differ(one['status'], out['status']), q


@pytest.mark.parametrize('B', SK.CELL_BATCHES)
def test_two_site_cell_batch_edges(B, cells):
    """A pool of 41 cells of the family (both statuses, both solve branches) tiled to B = 1, 63, 64, 65 (one lane, a ragged wave, a full
    one, one lane of a second workgroup) and 4 141 (65 workgroups): every copy bit-identical to the first of its member and within 1e-10 of
    the reference.  Measured on one MI355X: max |dE| 2.2e-15 at every B; 15 of the 41 pool members status 2 (1 010 of 4 141 rows), none
    status 1, up to 3 iterations; no copy differs."""
    pool = SK.cell_pool()
    rows = SK.tile(pool, B)
    out = run_cells(cells['eng'], cells['fam']['U1'][rows], cells['fam']['U2'][rows], cells['h'])
    err = float(np.abs(out['E'] - cells['ref']['E'][rows]).max())
    print(f'cell2 batch {B}: max |dE| {err:.2e}, status 0/1/2 {[(int((out["status"] == s).sum())) for s in (0, 1, 2)]}, '
          f'iterations max {out["iters"].max()}')
    for k in ('E', 'iters', 'status'):
        assert len(SK.differing_copies(out[k])) == 0, k
    assert not np.any(out['status'] == 1) and err < CC.E_TOL
    first = run_cells(cells['eng'], cells['fam']['U1'][pool[:min(B, SK.POOL)]], cells['fam']['U2'][pool[:min(B, SK.POOL)]], cells['h'])
    assert cells_differ(first, {k: v[:SK.POOL] for k, v in out.items()}) == []


def test_two_site_cell_from_su_parameters(cells):
    """eng.cell2_energies_su on 41 rows of 30 standard-normal parameters (U1 = U4(p[:15]), U2 = U4(p[15:]) built by su_exp_kernel<4>, ten
    full workgroups and one evaluation in the eleventh) against eng.cell2_energies of the host mirror's unitaries and against the
    oracle's two 4-qubit circuits, 1e-10 on every term.
    Measured on one MI355X: 5.3e-15 against the host-built unitaries, 5.1e-15 against the oracle (host-built against the oracle 8.9e-16);
    every row status 0 in one step."""
    pool, eng, h = SK.cell_su_pool(), cells['eng'], cells['h']
    E, it, st = eng.cell2_energies_su(pool['P'], h)
    Eh, ith, sth = eng.cell2_energies(pool['U1'], pool['U2'], h)
    Eo = np.array([[O.two_site_cell_energy(u1, u2, hq) for hq in h] for u1, u2 in zip(pool['U1'], pool['U2'])])
    fig = {'against_host_unitaries': float(np.abs(E - Eh).max()), 'against_oracle': float(np.abs(E - Eo).max()),
           'host_unitaries_against_oracle': float(np.abs(Eh - Eo).max())}
    print('cell2 from SU parameters: ' + fmt(fig))
    assert np.all(st == 0) and np.all(sth == 0) and np.array_equal(it, ith)
    assert max(fig.values()) < CC.E_TOL, fig


# ---------------------------------------------------------------------------------------------------------------------------
# 2. brick-wall kernels (qmps_brickwall.hip)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', [0, 1])
def test_brickwall_environment_every_row(side):
    """bw_env_kernel through _Environment._env (40 squarings, tol 1e-13) on the 1 062 rows of side_kernel_cases.bw_rows, right and left:
    the matrix against the oracle's (1e-13); every status-0 row: eta within 1e-9 of the reference's leading set (largest
    Re + 1e-6 Im), ||M v - eta v|| < 1e-9, unit norm (1e-12), an entry of largest modulus real and positive; Im(eta) > 0 on every real
    matrix that leads with a conjugate pair (the tilt alone decides there); status 1 only where the reference explains it (nilpotent M, or
    two different leading eigenvalues closer than 1e-8 under the tilted order) - on the Haar-orthogonal, Haar-unitary and state-like rows
    never.
    Measured on one MI355X (right / left): matrix 4.4e-16 / 3.4e-16; 1 056 / 1 053 rows status 0, 6 / 9 status 1, every one of them a
    nilpotent grid matrix (190 / 187 further nilpotent ones come back status 0); eta 9.3e-10 on both sides - 2^-30, on nilpotent matrices
    only, where the exact eigenvalue is 0 and the acceptance at round 30 takes the Rayleigh quotient of a Jordan chain; 1.7e-13 / 9.3e-14
    on the Haar-orthogonal, 8.1e-14 / 6.1e-14 on the Haar-unitary, 6.2e-15 / 6.6e-15 on the state-like rows; residual 9.9e-14 / 8.7e-14;
    norm 3.3e-16; phase 3.8e-17; all 36 / 36 leading conjugate pairs (smallest |Im| 1.28e-2) returned with Im(eta) > 0.  The entry point
    does not report the number of squarings."""
    rows, M, cls = SK.bw_rows(), SK.bw_matrices(side), SK.bw_classes(side)
    env = NT.LeftEnvironment() if side else NT.RightEnvironment()
    mat, eta, vec, st, _ = env._env(rows['U1'], rows['U2'], rows['U1p'], rows['U2p'], True)
    kind = rows['kind']
    n = len(kind)
    d_eta, resid, norm, phase = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for k in range(n):
        lead = SK.leading_eigenpair(M[k])
        v = vec[k].reshape(-1)
        d_eta[k] = np.abs(lead - eta[k]).min()
        resid[k] = np.linalg.norm(M[k] @ v - eta[k] * v)
        norm[k] = abs(np.linalg.norm(v) - 1.0)
        # (several entries may share the largest modulus to rounding: one of them carries the phase convention)
        big = np.flatnonzero(np.abs(v) >= np.abs(v).max() - 1e-12)
        phase[k] = min(abs(v[j].imag) if v[j].real > 0 else np.inf for j in big)
    ok = st == 0
    pairs = (kind == 'a') & (cls['pair_im'] >= SK.PAIR_IM)
    fig = {'rows': n, 'status0': int(ok.sum()), 'status1': int((st == 1).sum()), 'other_status': int((~ok & (st != 1)).sum()),
           'matrix': float(np.abs(mat - M).max()), 'eta': float(d_eta[ok].max()), 'residual': float(resid[ok].max()),
           'norm': float(norm[ok].max()), 'phase': float(phase[ok].max()), 'leading_pairs': int(pairs.sum()),
           'smallest_pair_im': float(cls['pair_im'][pairs].min()), 'pairs_with_positive_im': int((eta.imag[pairs] > 0).sum())}
    for c in 'abcd':
        m = kind == c
        s1 = m & (st == 1)
        fig[f'status1_{c}'] = int(s1.sum())
        fig[f'status1_{c}_nilpotent'] = int((cls['cls'][s1] == 'nilpotent').sum())
        fig[f'status1_{c}_close'] = int((cls['cls'][s1] == 'close').sum())
        fig[f'nilpotent_{c}_status0'] = int((cls['cls'][m & ok] == 'nilpotent').sum())
    print(f'bw_env side {side}: ' + fmt(fig))
    assert fig['matrix'] < 1e-13
    assert fig['other_status'] == 0
    unexplained = np.flatnonzero((st == 1) & (cls['cls'] == None))                      # noqa: E711 (object array)
    assert len(unexplained) == 0, ('status 1 that the reference does not explain', unexplained[:8], kind[unexplained][:8])
    assert np.all(st[kind != 'd'] == 0)
    bad = np.flatnonzero(ok & (d_eta >= 1e-9))
    assert len(bad) == 0, ('status 0 with an eigenvalue outside the leading set', bad[:8], eta[bad][:8], [SK.leading_eigenpair(M[k]) for k in bad[:4]])
    assert fig['residual'] < 1e-9 and fig['norm'] < 1e-12 and fig['phase'] < 1e-15, fig
    assert fig['leading_pairs'] >= 30 and fig['pairs_with_positive_im'] == fig['leading_pairs'], fig


@pytest.mark.parametrize('B', SK.BW_BATCHES)
def test_brickwall_per_item_operators(B):
    """bw_expval (two and four sites) with an operator per item (o_shared = 0) and bw_manifold with shared / per-item boundary matrices
    (m_shared) and shared / per-item W (w_shared), all four combinations: a pool of 41 items tiled to B = 1, 63, 64, 65, 130 against the
    oracle (1e-12; four sites 1e-11: the tolerances of the shared forms in test_brickwall_gpu.py), every copy bit-identical.
    Measured on one MI355X (the same at every B >= 63): two sites 5.6e-16, four sites 2.7e-15, manifold 5.0e-16 (both per item), 7.1e-16
    (W shared), 5.0e-16 (boundary matrices shared), 6.7e-16 (both shared); no copy differs."""
    p = SK.bw_pool()
    t = {k: SK.tile(p[k], B) for k in ('U1', 'U2', 'U1p', 'U2p', 'O2', 'O4', 'Mr', 'Ml', 'W')}
    member = np.arange(B) % SK.POOL
    oc, mo = NT.OverlapCalculator(), NT.ManifoldOverlap()
    fig = {}
    e2 = oc._expval(t['U1'], t['U2'], t['O2'], 2)
    e4 = oc._expval(t['U1'], t['U2'], t['O4'], 4)
    fig['expval2'] = float(np.abs(e2 - p['e2'][member]).max())
    fig['expval4'] = float(np.abs(e4 - p['e4'][member]).max())
    results = {'expval2': e2, 'expval4': e4}
    for ms in (0, 1):
        for ws in (0, 1):
            Mr, Ml = (p['Mr'][0], p['Ml'][0]) if ms else (t['Mr'], t['Ml'])
            W = p['W'][0] if ws else t['W']
            ov = mo.circuit(t['U1'], t['U2'], t['U1p'], t['U2p'], Mr, Ml, W)
            name = f'manifold_m{"shared" if ms else "item"}_w{"shared" if ws else "item"}'
            fig[name] = float(np.abs(ov - p['ov', ms, ws][member]).max())
            results[name] = ov
    print(f'brick-wall per-item operators B={B}: ' + fmt(fig))
    for name, r in results.items():
        assert r.shape == (B,) and len(SK.differing_copies(r)) == 0, name
        assert fig[name] < (1e-11 if name == 'expval4' else 1e-12), (name, fig)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. SU(N) (qmps_su.hip)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def su_engine(engine_factory):
    return engine_factory(2, 4096)


@pytest.mark.parametrize('N', SK.SU_N)
def test_su_unitaries_do_not_depend_on_the_batch_mates(N, su_engine):
    """su_exp_kernel: 32 parameter rows - eight standard-normal ones, each followed by rows scaled by 6, 300 and 1e5, so that at N = 4 every
    workgroup of four evaluations mixes all sizes - against the eight standard-normal rows as a batch of their own, all 32 rows as batches
    of one, and the batch in a second order: bit-identical unitaries.  (At N = 4 the evaluations of a workgroup used to share the largest
    scaling exponent among them.  Measured on one MI355X before every evaluation kept its own exponent: N = 4 failed - the standard-normal
    rows differed by up to 1.18e-10 from the same rows alone and as batches of one, 1.00e-10 between the two orders; N = 8, 16, 32, one
    evaluation per workgroup, identical.  With the kernel as it is now: identical at every N.)"""
    sp = SK.su_params(N)
    P = sp['P']
    U = su_engine.su_unitaries(P, N)
    normal = np.flatnonzero(sp['scale'] == 1.0)
    alone = su_engine.su_unitaries(P[normal], N)
    single = np.concatenate([su_engine.su_unitaries(P[k:k + 1], N) for k in range(len(P))])
    p2 = np.random.default_rng(9410 + N).permutation(len(P))
    second = su_engine.su_unitaries(P[p2], N)
    diff = {'normal_rows_alone': float(np.abs(U[normal] - alone).max()), 'batches_of_one': float(np.nanmax(np.abs(U - single))),
            'batches_of_one_normal_and_6x': float(np.abs(U - single)[sp['scale'] <= 6.0].max()),
            'second_order': float(np.nanmax(np.abs(U[p2] - second)))}
    print(f'SU({N}) largest difference between the same row in different batches: ' + fmt(diff))
    assert not bits_differ(U[normal], alone)
    assert not bits_differ(U, single)
    assert not bits_differ(U[p2], second)


def test_two_site_cell_su_energies_do_not_depend_on_the_batch_mates(cells):
    """eng.cell2_energies_su: twelve standard-normal rows of 30 parameters with a row scaled by 1e5 in every workgroup of four, against the
    same twelve rows in a batch without those - energies, iterations and statuses bit-identical.
    Measured on one MI355X: identical (with the shared exponent all 12 rows differed, by up to 4.45e-10)."""
    mixed, eng, h = SK.cell_su_mixed(), cells['eng'], cells['h']
    keep = np.setdiff1d(np.arange(len(mixed['P'])), mixed['big'])
    E, it, st = eng.cell2_energies_su(mixed['P'], h)
    E2, it2, st2 = eng.cell2_energies_su(mixed['P'][keep], h)
    print(f'cell2 from SU parameters beside a 1e5-sized row: max |dE| {np.abs(E[keep] - E2).max():.2e}, rows that differ '
          f'{int(np.any(E[keep] != E2, axis=1).sum())} of {len(keep)}')
    assert not bits_differ(E[keep], E2) and np.array_equal(it[keep], it2) and np.array_equal(st[keep], st2)


@pytest.mark.parametrize('N', SK.SU_N)
def test_su_unitaries_against_the_reference(N, su_engine):
    """The standard-normal and 6 x rows against mpmath's expm of the host mirror's generator (N = 4, 8) or the host mirror itself
    (scipy, N = 16, 32): 1e-12 for the unitary and for U^H U - 1.  The 300 x and 1e5 x rows must be finite; their unitarity defect is
    printed (no bound: the conditioning of exp at that norm has not been measured).
    Measured on one MI355X (error 1 x, 6 x; defect 1 x, 6 x, 300 x, 1e5 x):
      N = 4   1.2e-15, 6.1e-15;  2.2e-15, 1.8e-14, 4.8e-13, 1.5e-10
              (with the exponent shared by the workgroup: 1.18e-10, 9.8e-11;  2.2e-10, 2.1e-10, 2.5e-10, 1.5e-10)
      N = 8   2.2e-15, 9.9e-15;  4.9e-15, 2.3e-14, 2.5e-12, 6.4e-10
      N = 16  6.0e-15, 1.4e-14;  1.3e-14, 5.3e-14, 1.5e-12, 8.4e-10
      N = 32  9.6e-15, 2.0e-14;  2.5e-14, 6.4e-14, 3.2e-12, 1.2e-9"""
    sp = SK.su_params(N)
    U = su_engine.su_unitaries(sp['P'], N)
    rows, ref = SK.su_references(N)
    defect = np.abs(np.einsum('bki,bkj->bij', U.conj(), U) - np.eye(N)).reshape(len(U), -1).max(axis=1)
    fig = {}
    for s in SK.SU_SCALES:
        m = sp['scale'] == s
        if s <= 6.0:
            fig[f'error_{s:g}x'] = float(np.abs(U[m] - ref[np.isin(rows, np.flatnonzero(m))]).max())
        fig[f'defect_{s:g}x'] = float(defect[m].max())
    print(f'SU({N}) against {"mpmath expm" if N in SK.SU_MP_N else "the host mirror"}: ' + fmt(fig))
    assert np.all(np.isfinite(U.view(np.float64)))
    for s in (1.0, 6.0):
        assert fig[f'error_{s:g}x'] < SK.SU_TOL and fig[f'defect_{s:g}x'] < SK.SU_TOL, fig


@pytest.mark.parametrize('D', [2, 4, 8, 16])
def test_su_tensor_output(D, engine_factory):
    """eng.energies_from_su (su_exp_kernel with out_tensor = 1 writes the state tensor, then the energy kernels of that D) on 13
    standard-normal rows - at N = 4 three full workgroups and one evaluation in a fourth, whose shadow lanes must not write - against
    oracle.energy_closed_form of unitary_to_tensor(SU(p)) built on the host, 1e-10 on all three terms; the pool tiled to B = 41, 42, 43
    (4 k + 1, 4 k + 2, 4 k + 3): every copy bit-identical.
    Measured on one MI355X (D = 2 / 4 / 8 / 16): max |dE| 8.0e-15 / 2.7e-14 / 9.1e-15 / 9.7e-14, every row status 0 (one step; up to 90 power
    steps at D = 16); no copy differs."""
    pool, h = SK.su_tensor_pool(D), CC.hamiltonian_terms()
    eng = engine_factory(D, 4096)
    E, it, st = eng.energies_from_su(pool['P'], h)
    err = float(np.abs(E - pool['E']).max())
    print(f'SU({2 * D}) tensor output D={D}: max |dE| {err:.2e}, statuses {sorted(set(st.tolist()))}, iterations max {it.max()}')
    assert not np.any(st == 1) and err < CC.E_TOL
    n = SK.SU_TENSOR_POOL
    for B in SK.SU_TENSOR_BATCHES:
        Et, itt, stt = eng.energies_from_su(SK.tile(pool['P'], B), h)
        for name, r in (('E', Et), ('iters', itt), ('status', stt)):
            assert len(SK.differing_copies(r, n)) == 0, (B, name)
        assert not bits_differ(Et[:n], E) and float(np.abs(Et - pool['E'][np.arange(B) % n]).max()) < CC.E_TOL, B
