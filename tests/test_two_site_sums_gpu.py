"""GPU: qmps_correlator_sums_two_site - the sums over all distances of the connected two-point functions of two-site operators, the
three overlapping distances and the energy variance per site - against the long-double reference of tests/two_site_sum_cases.py.  The
kernel-alone comparison gives the environments by set_env_guess from the oracle's direct solve, so no solver error is in it; the rest
checks the one-site limit, the product states, energy_variance on a solved batch, and the contract of the call: positions in the batch,
window, fused-ansatz batches, untouched state, argument errors, degenerate fixed points and unusable environments.

Worst err / bound of the kernel-alone comparison measured on an MI355X: see profiles/EXPERIMENTS.md."""
import numpy as np
import pytest

import correlator_cases as K
import resident_cases as RS
import structure_factor_cases as S
import two_site_sum_cases as T2
from qmps_amd import _lib

pytestmark = pytest.mark.gpu


def _given(engine_factory, D, A, r):
    """Engine with tensors and environments given verbatim (nothing is solved)."""
    eng = engine_factory(D)
    eng.set_tensors(np.ascontiguousarray(A))
    eng.set_hamiltonian(RS.H_TFIM)
    eng.set_env_guess(np.ascontiguousarray(r))
    return eng


def _haar(engine_factory, D):
    rows = K.HAAR_B if D <= 8 else T2.haar_rows(D)
    return _given(engine_factory, D, K.haar_tensors(D)[:rows], S.haar_environments(D, rows))


def _check(G, one, near, ref, rows, m, n_z, D, what):
    Gr, oner, nearr, bnd = ref
    rows = np.arange(rows) if np.isscalar(rows) else rows
    err = np.abs(G - Gr[rows][:, :n_z, :m, :m]).astype(float).max(axis=(2, 3))
    ratio = float((err / bnd[rows][:, :n_z]).max())
    e1 = max(float(np.abs(one - oner[rows][:, :m]).max()), float(np.abs(near - nearr[rows][:, :m, :m]).max()))
    print(f'two-site sums D={D} {what} B={len(rows)} m={m} n_z={n_z}: G err / bound {ratio:.3f}, one, near err / bound {e1 / T2.bound_near():.3f}')
    assert ratio <= 1.0, (what, D, len(rows), m, n_z, ratio)
    assert e1 <= T2.bound_near(), (what, D, len(rows), m, n_z, e1)
    return ratio, e1


@pytest.mark.parametrize('D', T2.DS)
def test_kernel_alone_within_the_rounding_bound(engine_factory, D):
    """Haar tensors and the small-gap family with the oracle's direct-solve environments given by set_env_guess; G elementwise within
    bound(b, j) of the long-double reference, one and near within bound_near().  D <= 8: B in (1, 17, 65, 130) x n_ops in (1, 2, 3, 4) x n_z
    in (1, 2, 6); D = 16: B in (1, 5), n_ops in (1, 4), n_z in (1, 3)."""
    eng = _haar(engine_factory, D)
    ref = T2.haar_reference(D)
    batches, n_ops, n_zs = (T2.BATCHES, T2.N_OPS, T2.N_Z) if D <= 8 else (T2.D16_BATCHES, T2.D16_N_OPS, T2.D16_N_Z)
    worst, worst_near = 0.0, 0.0
    for B in batches:
        for m in n_ops:
            for n_z in n_zs:
                G, one, near = eng.correlator_sums(T2.generic_ops()[:m], T2.Z[:n_z], B=B, want_one_site=True, want_site=True)
                assert G.shape == (B, n_z, m, m) and one.shape == (B, m) and near.shape == (B, m, m, 3) and G.dtype == np.complex128
                ratio, e1 = _check(G, one, near, ref, B, m, n_z, D, 'Haar')
                worst, worst_near = max(worst, ratio), max(worst_near, e1)
    print(f'two-site sums D={D} Haar: worst G err / bound {worst:.3f}, worst |one, near - long double| {worst_near:.2e} (bound {T2.bound_near():.2e})')
    Af, rf, _ = S.family(D)
    zf = T2.points(D)
    eng = _given(engine_factory, D, Af, rf)
    R = Af.shape[0]
    assert eng.tensors(R).tobytes() == Af.tobytes() and eng.environments(R).tobytes() == rf.tobytes()
    G, one, near = eng.correlator_sums(T2.generic_ops(), zf, B=R, want_one_site=True, want_site=True)
    ratio, e1 = _check(G, one, near, T2.family_reference(D), R, 4, len(zf), D, 'family')
    print(f'two-site sums D={D} family: worst G err / bound {ratio:.3f}')
    # G without the optional outputs is the same G
    assert eng.correlator_sums(T2.generic_ops(), zf, B=R).tobytes() == G.tobytes()


@pytest.mark.parametrize('D', T2.DS)
def test_embedded_operator_against_the_one_site_structure_factor(engine_factory, D):
    """The GPU two-site S of O (x) 1 and of 1 (x) O against the GPU one-site structure_factor of O at k = 0, 0.7, pi, within the sum of the
    two modules' bounds (S_OO is one-site `site - one one` within 3 correlator bounds plus two sums)."""
    eng = _haar(engine_factory, D)
    B = 17 if D <= 8 else 2
    A, r = K.haar_tensors(D)[:B], S.haar_environments(D, B)
    k = np.array([0.0, 0.7, np.pi])
    O1 = K.generic_ops()[0]
    S2 = eng.structure_factor(T2.embedded_ops(O1), k, B=B)
    S1 = eng.structure_factor(O1, k, B=B)[:, :, 0, 0]
    assert S2.shape == (B, 3, 2, 2)
    b1 = S.bound(A, r, S.k_to_z(k))
    granted = T2.bound_S(A, r, k) + b1[:, 0::2] + b1[:, 1::2] + 3 * K.bound(D, 1)
    err = np.maximum(np.abs(S2[:, :, 0, 0] - S1), np.abs(S2[:, :, 1, 1] - S1))
    print(f'two-site S of the embedded operator D={D}: |S2 - S1| / granted {float((err / granted).max()):.3f}')
    assert np.all(err <= granted)


@pytest.mark.parametrize('D', T2.DS)
def test_product_rows_against_the_closed_form(engine_factory, D):
    """cos th/2 |0> + sin th/2 |1> at every D: the variance per site of sum ZZ is 1 + 2 c^2 - 3 c^4; th = 0, an eigenstate, gives 0."""
    A, r, c = T2.product_rows(D)
    eng = _given(engine_factory, D, A, r)
    var = eng.energy_variance(T2.ZZ, B=3)
    assert var.shape == (3, 1) and var.dtype == np.float64
    err = np.abs(var[:, 0] - T2.zz_variance(c))
    print(f'product rows D={D}: variance {var[:, 0]}, error {err.max():.2e}')
    assert np.all(err <= T2.bound_S(A, r, [0.0])[:, 0])
    zs = np.array([1.0, 0.5 + 0.25j])
    G = eng.correlator_sums(T2.ZZ, zs, B=3)
    assert np.all(np.abs(G[:, :, 0, 0]) <= T2.bound(A, r, zs))      # b_c vanishes on a product state: no correlations beyond n = 1
    assert not G[0].any()                                           # th = 0: exactly


@pytest.mark.parametrize('D', T2.DS)
def test_energy_variance_of_a_solved_batch(engine_factory, D):
    """A TFIM batch solved on the device: energy_variance() of the resident Hamiltonian against the reference evaluated at the device's
    own environments()."""
    eng = engine_factory(D)
    B = 17 if D <= 8 else 2
    RS.solve(eng, K.haar_tensors(D)[:B], D)
    assert np.all(eng.results(B)[2] == 0)
    A, r = eng.tensors(B), eng.environments(B)
    var = eng.energy_variance(B=B)
    assert var.shape == (B, 1)
    z = S.k_to_z([0.0])
    G, one, near = T2.reference(A, r, RS.H_TFIM[None], z)
    want = T2.structure_factor(G, one, near, z)[:, 0, 0, 0].real.astype(float)
    scale = max(1.0, np.linalg.norm(RS.H_TFIM, 2)) ** 2               # (the bounds are stated for operators of unit spectral norm)
    err = np.abs(var[:, 0] - want)
    print(f'energy_variance D={D}: sigma^2 in [{var.min():.3f}, {var.max():.3f}], |error| / granted {float((err / (scale * T2.bound_S(A, r, [0.0])[:, 0])).max()):.3f}')
    assert np.all(err <= scale * T2.bound_S(A, r, [0.0])[:, 0])
    assert np.all(var >= -scale * T2.bound_S(A, r, [0.0]))
    # an explicit h of several terms: each column is the variance of its own term
    both = eng.energy_variance(np.stack([RS.H_TFIM, T2.ZZ, RS.H_TFIM, T2.ZZ, RS.H_TFIM]), B=B)
    granted = 2 * scale * T2.bound_S(A, r, [0.0])[:, 0]
    assert both.shape == (B, 5) and both[:, 0].tobytes() == both[:, 2].tobytes() and both[:, 1].tobytes() == both[:, 3].tobytes()
    assert np.all(np.abs(both[:, 0] - var[:, 0]) <= granted) and np.all(np.abs(both[:, 4] - var[:, 0]) <= granted)      # (the fifth term: a second call)


@pytest.mark.parametrize('D', T2.DS)
def test_same_input_at_several_positions_gives_the_same_bytes(engine_factory, D):
    """One (tensor, environment) pair tiled over the batch: every position computes the same bytes (lane, group and workgroup tails)."""
    B = 70 if D <= 8 else 5
    A = np.repeat(K.haar_tensors(D)[3:4], B, axis=0)
    r = np.repeat(S.haar_environments(D, 4)[3:4], B, axis=0)
    eng = _given(engine_factory, D, A, r)
    G, one, near = eng.correlator_sums(T2.generic_ops(), T2.Z[:3], B=B, want_one_site=True, want_site=True)
    for x in (G, one, near):
        assert all(x[b].tobytes() == x[0].tobytes() for b in range(1, B))


@pytest.mark.parametrize('D', T2.DS)
def test_window(engine_factory, D):
    eng = _haar(engine_factory, D)
    ops = T2.generic_ops()[:3]
    z = T2.Z[:2]
    n, first, count = (K.HAAR_B, 64, 66) if D <= 8 else (T2.haar_rows(D), 2, 3)
    full = eng.correlator_sums(ops, z, B=n, want_one_site=True, want_site=True)
    eng.set_window(first)
    part = eng.correlator_sums(ops, z, B=count, want_one_site=True, want_site=True)
    eng.set_window(0)
    for f, p in zip(full, part):
        assert np.array_equal(p, f[first:first + count])
    rows = min(n, 5)
    _check(full[0][:rows], full[1][:rows], full[2][:rows], T2.haar_reference(D), rows, 3, 2, D, 'window')


@pytest.mark.parametrize('D', (2, 4))
def test_fused_ansatz_batch(engine_factory, D):
    """ShallowCNOT parameters: the tensors are built on the device, d_A is materialised by the call; without resident environments
    the call refuses (QMPS_ERR_STATE)."""
    eng = engine_factory(D)
    P = K.ansatz_params(D)
    R = P.shape[0]
    ops = np.concatenate([T2.hermitian_ops(), T2.generic_ops()[:1]])
    z = T2.Z[2:5]
    eng.set_hamiltonian(RS.H_TFIM)
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)
    eng.launch(R, solver='direct', store_env=True)
    G, one, near = eng.correlator_sums(ops, z, B=R, want_one_site=True, want_site=True)
    A, r = eng.ansatz_probe(_lib.ANSATZ_SHALLOW_CNOT, P), eng.environments(R)
    ref = T2.reference(A, r, ops, z) + (T2.bound(A, r, z),)
    _check(G, one, near, ref, R, 3, 3, D, 'ansatz')
    var = eng.energy_variance(B=R)
    assert var.shape == (R, 1) and np.isfinite(var).all()
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)                  # new states: the environments no longer belong to them
    if D == 4:
        eng.launch(R, solver='direct', store_env=False)                 # (only the direct D = 4 path can solve without storing them)
    with pytest.raises(_lib.QmpsError) as info:
        eng.correlator_sums(ops, z, B=R)
    assert info.value.code == _lib.QMPS_ERR_STATE and 'environment' in str(info.value)


@pytest.mark.parametrize('D', T2.DS)
def test_nothing_else_moves(engine_factory, D):
    eng = engine_factory(D)
    B = 65 if D <= 8 else 5
    RS.solve(eng, K.haar_tensors(D)[:B], D)
    before = (eng.results(B), eng.environments(B), eng.results_status(B), eng.tensors(B))
    eng.correlator_sums(T2.generic_ops(), T2.Z[:2], B=B, want_one_site=True, want_site=True)
    eng.structure_factor(T2.hermitian_ops(), [0.0, 0.3], B=B)
    eng.energy_variance(B=B)
    after = (eng.results(B), eng.environments(B), eng.results_status(B), eng.tensors(B))
    for x, y in zip(before[0] + before[1:], after[0] + after[1:]):
        assert x.tobytes() == y.tobytes()


def test_argument_errors(engine_factory):
    eng = _haar(engine_factory, 4)
    lib, ctx = eng._lib, eng._ctx
    ops = np.ascontiguousarray(T2.generic_ops()).view(np.float64)
    z = np.ascontiguousarray(T2.Z).view(np.float64)
    out = np.full(2 * 17 * 6 * 16, 7.0)
    one = np.full(2 * 17 * 4, 7.0)
    near = np.full(2 * 17 * 16 * 3, 7.0)
    f = lambda a: a.ctypes.data_as(RS.DP)

    def untouched():
        return np.all(out == 7.0) and np.all(one == 7.0) and np.all(near == 7.0)

    def refused(rc, word):
        msg = lib.qmps_last_error().decode()
        assert rc == _lib.QMPS_ERR_ARG and word in msg, (rc, msg)
        assert untouched()

    def valid():
        G, o1, n1 = eng.correlator_sums(T2.generic_ops(), T2.Z, B=17, want_one_site=True, want_site=True)
        _check(G, o1, n1, T2.haar_reference(4), 17, 4, 6, 4, 'after an error')

    call = lib.qmps_correlator_sums_two_site
    refused(call(ctx, 17, 0, f(ops), 6, f(z), f(out), f(one), f(near)), 'n_ops')
    refused(call(ctx, 17, 5, f(ops), 6, f(z), f(out), f(one), f(near)), 'n_ops')
    refused(call(ctx, 17, 4, f(ops), 0, f(z), f(out), f(one), f(near)), 'n_z')
    refused(call(ctx, 17, 4, f(ops), 1025, f(z), f(out), f(one), f(near)), 'n_z')
    valid()
    refused(call(ctx, 17, 4, f(ops), 6, f(z), None, f(one), f(near)), 'G_out')
    refused(call(ctx, 17, 4, None, 6, f(z), f(out), f(one), f(near)), 'ops')
    refused(call(ctx, 17, 4, f(ops), 6, None, f(out), f(one), f(near)), 'null z')
    refused(call(None, 17, 4, f(ops), 6, f(z), f(out), f(one), f(near)), 'null context')
    valid()
    for bad in (1.0 + 1e-6, 0.8 + 0.8j, np.nan, np.inf):
        zb = T2.Z.copy()
        zb[4] = bad
        refused(call(ctx, 17, 4, f(ops), 6, f(np.ascontiguousarray(zb).view(np.float64)), f(out), f(one), f(near)), 'z[4]')
    valid()
    eng.set_window(100)                                         # a window that runs past the buffers
    refused(call(ctx, eng.max_batch - 50, 4, f(ops), 6, f(z), f(out), f(one), f(near)), 'window')
    # ... and one that runs past the resident states: the state of the context is wrong, not the arguments
    assert call(ctx, 40, 4, f(ops), 6, f(z), f(out), f(one), f(near)) == _lib.QMPS_ERR_STATE and b'resident' in lib.qmps_last_error()
    assert untouched()
    eng.set_window(0)
    refused(call(ctx, -1, 4, f(ops), 6, f(z), f(out), f(one), f(near)), 'window')
    valid()
    # 65536 x 1024 x 16 x 16 bytes = 16 GiB: refused by arithmetic, before anything is allocated or written
    zl = np.zeros(2 * 1024)
    refused(call(ctx, eng.max_batch, 4, f(ops), 1024, f(zl), f(out), f(one), f(near)), '1 GiB')
    with pytest.raises(_lib.QmpsError):
        eng.correlator_sums(T2.generic_ops(), np.zeros(1024), B=eng.max_batch)
    valid()
    for shape in ((2, 4, 3), (2, 3, 2), (4, 3)):
        with pytest.raises(ValueError):
            eng.correlator_sums(np.zeros(shape), T2.Z, B=17)
        with pytest.raises(ValueError):
            eng.structure_factor(np.zeros(shape), [0.0], B=17)
    with pytest.raises(ValueError):
        eng.energy_variance(np.zeros((2, 2)), B=17)
    valid()
    # e^(ik) as float64 rounds it is accepted, B = 0 is fine and writes nothing
    assert call(ctx, 0, 4, f(ops), 6, f(z), f(out), f(one), f(near)) == _lib.QMPS_OK and untouched()
    kk = np.linspace(0.0, 2 * np.pi, 1024)
    assert np.isfinite(eng.correlator_sums(T2.ZZ, np.exp(1j * kk), B=3)).all()
    valid()


def test_energy_variance_without_a_hamiltonian():
    """A context that never received a Hamiltonian, and one whose upload failed: ValueError, then a valid call with h given."""
    from qmps_amd import EnergyEngine
    A, r = K.haar_tensors(2)[:3], S.haar_environments(2, 3)
    with EnergyEngine(2, 16) as eng:
        eng.set_tensors(A)
        eng.set_env_guess(r)
        with pytest.raises(ValueError):
            eng.energy_variance(B=3)
        var = eng.energy_variance(RS.H_TFIM, B=3)
        assert var.shape == (3, 1) and np.isfinite(var).all()
        eng.set_hamiltonian(RS.H_TFIM)
        assert eng.energy_variance(B=3).tobytes() == var.tobytes()


@pytest.mark.parametrize('D', T2.DS)
def test_degenerate_fixed_point_and_unusable_environment(engine_factory, D):
    """The pass-through tensor A0 with r = 1 / D in the middle of a batch of five: on the unit circle its resolvent is singular at z = 1
    (NaN in G there, for it alone; one and near finite); at z = 0.5 + 0.25i it is finite, and as b_c vanishes G is exactly 0; the other
    four rows stay within the bound.  Then row 1 with r = 0: NaN in all its outputs, the others bit for bit as before."""
    rows = 4
    Ah, rh = K.haar_tensors(D)[:rows], S.haar_environments(D, rows)
    keep = np.array([0, 1, 3, 4])
    A = np.ascontiguousarray(np.concatenate([Ah[:2], S.passthrough_tensor(D)[None], Ah[2:4]]))
    r = np.ascontiguousarray(np.concatenate([rh[:2], (np.eye(D) / D).astype(np.complex128)[None], rh[2:4]]))
    z = np.array([1.0, 0.5 + 0.25j], dtype=np.complex128)
    ops = T2.generic_ops()
    eng = _given(engine_factory, D, A, r)
    G, one, near = eng.correlator_sums(ops, z, B=5, want_one_site=True, want_site=True)
    assert np.isnan(G[2, 0]).all()
    assert np.isfinite(G[2, 1]).all() and not G[2, 1].any()
    assert np.isfinite(one).all() and np.isfinite(near).all() and np.abs(one[2] - ops[:, 0, 0]).max() == 0.0
    ref = T2.reference(A[keep], r[keep], ops, z) + (T2.bound(A[keep], r[keep], z),)
    _check(G[keep], one[keep], near[keep], ref, 4, 4, 2, D, 'beside the pass-through tensor')
    r0 = r.copy()
    r0[1] = 0.0
    eng.set_env_guess(r0)
    G0, one0, near0 = eng.correlator_sums(ops, z, B=5, want_one_site=True, want_site=True)
    assert np.isnan(G0[1]).all() and np.isnan(one0[1]).all() and np.isnan(near0[1]).all()
    others = np.array([0, 2, 3, 4])
    for x, y in ((G, G0), (one, one0), (near, near0)):
        assert x[others].tobytes() == y[others].tobytes()


@pytest.mark.parametrize('D', (2, 4))
def test_host_helpers(D):
    from qmps_amd.ground_state import Hamiltonian, energy_variance, structure_factor
    from oracle import qmps_oracle as O
    P = K.ansatz_params(D)[:3]
    k = np.array([0.0, 0.3, np.pi])
    var, st = energy_variance(P, Hamiltonian({'ZZ': -1.0, 'X': 1.0}), D=D)
    assert var.shape == (3, 1) and st.shape == (3,) and np.all(st == 0)
    Sq, one, st = structure_factor(P, T2.hermitian_ops(), k, D=D)
    assert Sq.shape == (3, 3, 2, 2) and one.shape == (3, 2)
    A = K.ansatz_tensors(D)[:3]
    r = np.stack([O.env_dense_eig(a)[1] for a in A])
    z = S.k_to_z(k)
    Gr, oner, nearr = T2.reference(A, r, T2.hermitian_ops(), z, dtype=np.complex128)
    # 1e-10 is what the energy tests grant an environment against the dense-eig oracle; the resolvent amplifies it by its norm
    tol = 1e-10 * max(1.0, float(S.kappa(A, r, z).max()))
    assert np.abs(Sq - T2.structure_factor(Gr, oner, nearr, z)).max() < tol and np.abs(one - oner).max() < 1e-10
    h = Hamiltonian({'ZZ': -1.0, 'X': 1.0}).to_matrix()
    Gh, oneh, nearh = T2.reference(A, r, h[None], z[:2], dtype=np.complex128)
    assert np.abs(var[:, 0] - T2.structure_factor(Gh, oneh, nearh, z[:2])[:, 0, 0, 0].real).max() < 16 * tol
