"""GPU: qmps_correlator_sums - the sums over all distances of the connected two-point functions of the resident states - against the
long-double resolvent reference of tests/structure_factor_cases.py evaluated from the tensors and environments read back from the
device (the kernel alone, within the rounding bound), against the truncated series of qmps_correlators on the same resident state,
the host composition of the structure factor, and the contract of the call: window, fused-ansatz batches, untouched state, argument
errors, degenerate fixed points and unusable environments.

Worst err / bound of the kernel-alone comparison measured on an MI355X: see profiles/EXPERIMENTS.md."""
import numpy as np
import pytest

import correlator_cases as K
import resident_cases as RS
import structure_factor_cases as S
from oracle import qmps_oracle as O
from qmps_amd import _lib

pytestmark = pytest.mark.gpu

D16_ROWS = max(S.D16_BATCHES)
D16_Z = S.Z[:max(S.D16_N_Z)]


def _haar(engine_factory, D):
    eng, s = RS.haar(engine_factory, D)
    assert np.all(s['st'] == 0)
    return eng, s


def _cached(D, key, make):
    return RS.cached(D, __name__, key, make)


def _haar_reference(D):
    """(G, one, site, bound) of the generic operators on the rows and points the kernel comparison uses, from the read-back arrays."""
    s = RS.solved(D)
    rows, z = (K.HAAR_B, S.Z) if D <= 8 else (D16_ROWS, D16_Z)
    return _cached(D, 'haar', lambda: S.reference(s['A'][:rows], s['r'][:rows], K.generic_ops(), z) + (S.bound(s['A'][:rows], s['r'][:rows], z),))


def _check(G, one, site, ref, rows, m, n_z, D, what):
    Gr, oner, siter, bnd = ref
    rows = np.arange(rows) if np.isscalar(rows) else rows
    err = np.abs(G - Gr[rows][:, :n_z, :m, :m]).astype(float).max(axis=(2, 3))
    ratio = float((err / bnd[rows][:, :n_z]).max())
    e1 = max(float(np.abs(one - oner[rows][:, :m]).max()), float(np.abs(site - siter[rows][:, :m, :m]).max()))
    assert ratio <= 1.0, (what, D, len(rows), m, n_z, ratio)
    assert e1 <= K.bound(D, 1), (what, D, len(rows), m, n_z, e1)
    return ratio, e1


@pytest.mark.parametrize('D', S.DS)
def test_kernel_alone_within_the_rounding_bound(engine_factory, D):
    """Haar tensors with the environments the device solved, and the small-gap family fed with set_tensors + set_env_guess; tensors and
    environments read back; G elementwise within bound(b, j) of the long-double reference of those arrays, `one` and `site` within
    correlator_cases.bound(D, 1).  D <= 8: B in (1, 17, 65, 130) x n_ops in (1, 2, 3, 4) x n_z in (1, 2, 6); D = 16: B in (1, 5),
    n_ops in (1, 4), n_z in (1, 3)."""
    eng, s = _haar(engine_factory, D)
    ref = _haar_reference(D)
    batches, n_ops, n_zs = (S.BATCHES, S.N_OPS, S.N_Z) if D <= 8 else (S.D16_BATCHES, S.D16_N_OPS, S.D16_N_Z)
    worst, worst_one = 0.0, 0.0
    for B in batches:
        for m in n_ops:
            for n_z in n_zs:
                G, one, site = eng.correlator_sums(K.generic_ops()[:m], S.Z[:n_z], B=B, want_one_site=True, want_site=True)
                assert G.shape == (B, n_z, m, m) and one.shape == (B, m) and site.shape == (B, m, m) and G.dtype == np.complex128
                ratio, e1 = _check(G, one, site, ref, B, m, n_z, D, 'Haar')
                worst, worst_one = max(worst, ratio), max(worst_one, e1)
    print(f'correlator_sums D={D} Haar: worst err / bound {worst:.3f}, worst |one, site - long double| {worst_one:.2e}')
    # the family
    Af, rf, _ = S.family(D)
    zf = S.Z if D <= 8 else D16_Z
    eng.set_tensors(Af)
    eng.set_env_guess(rf)
    R = Af.shape[0]
    A, r = eng.tensors(R), eng.environments(R)
    assert A.tobytes() == Af.tobytes() and r.tobytes() == rf.tobytes()
    fam = _cached(D, 'family', lambda: S.reference(A, r, K.generic_ops(), zf) + (S.bound(A, r, zf),))
    G, one, site = eng.correlator_sums(K.generic_ops(), zf, B=R, want_one_site=True, want_site=True)
    ratio, e1 = _check(G, one, site, fam, R, 4, len(zf), D, 'family')
    print(f'correlator_sums D={D} family (1 - |lambda_2| down to {min(S.gap(a) for a in Af):.1e}, resolvent norm up to '
          f'{fam[3].max() / (S.C_BOUND * S.EPS):.3g}): worst err / bound {ratio:.3f}')


@pytest.mark.parametrize('D', (2, 4, 8))
def test_against_the_series_of_the_correlator_kernel(engine_factory, D):
    """z = 0.5 and 0.5i, B = 17: G = sum_(n <= 64) z^n (C - one one) with C and one of EnergyEngine.correlators on the same resident
    state, within the sum of the two modules' bounds (the remainder of the series, 2^-64 of its terms, is granted too)."""
    eng, s = _haar(engine_factory, D)
    B, N = 17, 64
    ops = K.generic_ops()
    z = np.array([0.5, 0.5j])
    G = eng.correlator_sums(ops, z, B=B)
    C, one = eng.correlators(ops, N, B=B, want_one_site=True)
    conn = C - (one[:, :, None] * one[:, None, :])[..., None]
    n = np.arange(1, N + 1)
    ser = np.einsum('zn,bacn->bzac', z[:, None] ** n[None], conn)
    tol = S.bound(s['A'][:B], s['r'][:B], z) + float((0.5 ** n * (K.bound(D, n) + 2 * K.bound(D, 1))).sum()) + 4 * 0.5 ** N
    err = np.abs(G - ser).max(axis=(2, 3))
    print(f'correlator_sums D={D}: against the 64-term series of qmps_correlators {err.max():.2e} (granted {tol.min():.2e})')
    assert np.all(err <= tol)


@pytest.mark.parametrize('D', S.DS)
def test_structure_factor(engine_factory, D):
    """EnergyEngine.structure_factor with X, Y, Z at k = 0, 0.3, pi: equal to the host composition of the reference G, one and site;
    every S[b, q] Hermitian within twice the bound with smallest eigenvalue >= -3 bound."""
    eng, s = _haar(engine_factory, D)
    B = 17 if D <= 8 else 2
    k = np.array([0.0, 0.3, np.pi])
    z = S.k_to_z(k)
    ops = K.PAULIS[1:]
    Sq = eng.structure_factor(ops, k, B=B)
    assert Sq.shape == (B, 3, 3, 3)
    Gr, oner, siter = _cached(D, 'paulis', lambda: S.reference(s['A'][:B], s['r'][:B], ops, z))
    bnd = S.bound(s['A'][:B], s['r'][:B], z)
    Sr = S.structure_factor(Gr, oner, siter)
    pair = bnd[:, 0::2] + bnd[:, 1::2] + 3 * K.bound(D, 1)
    err = np.abs(Sq - Sr).astype(float).max(axis=(2, 3))
    assert np.all(err <= pair), (D, float((err / pair).max()))
    bq = np.maximum(bnd[:, 0::2], bnd[:, 1::2])
    herm = np.abs(Sq - Sq.conj().swapaxes(-1, -2)).max(axis=(2, 3))
    low = np.linalg.eigvalsh((Sq + Sq.conj().swapaxes(-1, -2)) / 2).min(axis=-1)
    print(f'structure_factor D={D}: |S - reference| / granted {float((err / pair).max()):.3f}, |S - S^H| / bound {float((herm / bq).max()):.3f}, '
          f'smallest eigenvalue / bound {float((low / bq).min()):.3f}')
    assert np.all(herm <= 2 * bq) and np.all(low >= -3 * bq)


@pytest.mark.parametrize('D', S.DS)
def test_window(engine_factory, D):
    eng, s = _haar(engine_factory, D)
    ops = K.generic_ops()[:3]
    z = S.Z[:2]
    full = eng.correlator_sums(ops, z, B=K.HAAR_B, want_one_site=True, want_site=True)
    eng.set_window(64)
    part = eng.correlator_sums(ops, z, B=66, want_one_site=True, want_site=True)
    eng.set_window(0)
    for f, p in zip(full, part):
        assert np.array_equal(p, f[64:130])
    ratio, _ = _check(full[0][:D16_ROWS], full[1][:D16_ROWS], full[2][:D16_ROWS], _haar_reference(D), D16_ROWS, 3, 2, D, 'window')


@pytest.mark.parametrize('D', (2, 4))
def test_fused_ansatz_batch(engine_factory, D):
    """ShallowCNOT parameters: the tensors are built on the device, d_A is materialised by the call; without resident environments
    the call refuses (QMPS_ERR_STATE)."""
    eng = engine_factory(D)
    P = K.ansatz_params(D)
    R = P.shape[0]
    ops = np.stack([K.SIGMA_PLUS, K.Z, K.X])
    z = S.Z[2:5]
    eng.set_hamiltonian(RS.H_TFIM)
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)
    eng.launch(R, solver='direct', store_env=True)
    G, one, site = eng.correlator_sums(ops, z, B=R, want_one_site=True, want_site=True)
    A, r = eng.ansatz_probe(_lib.ANSATZ_SHALLOW_CNOT, P), eng.environments(R)
    assert np.abs(A - K.ansatz_tensors(D)).max() < 1e-13
    ref = S.reference(A, r, ops, z) + (S.bound(A, r, z),)
    ratio, e1 = _check(G, one, site, ref, R, 3, 3, D, 'ansatz')
    print(f'correlator_sums D={D}, fused ShallowCNOT batch: worst err / bound {ratio:.3f}')
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)                  # new states: the environments no longer belong to them
    if D == 4:
        eng.launch(R, solver='direct', store_env=False)                 # (only the direct D = 4 path can solve without storing them)
    with pytest.raises(_lib.QmpsError) as info:
        eng.correlator_sums(ops, z, B=R)
    assert info.value.code == _lib.QMPS_ERR_STATE and 'environment' in str(info.value)


@pytest.mark.parametrize('D', S.DS)
def test_nothing_else_moves(engine_factory, D):
    eng = engine_factory(D)
    B = 65
    RS.solve(eng, K.haar_tensors(D)[:B], D)
    before = (eng.results(B), eng.environments(B), eng.results_status(B), eng.tensors(B))
    eng.correlator_sums(K.generic_ops(), S.Z[:2], B=B, want_one_site=True, want_site=True)
    eng.structure_factor(K.Z, [0.0, 0.3], B=B)
    after = (eng.results(B), eng.environments(B), eng.results_status(B), eng.tensors(B))
    for x, y in zip(before[0] + before[1:], after[0] + after[1:]):
        assert x.tobytes() == y.tobytes()


def test_argument_errors(engine_factory):
    eng, s = _haar(engine_factory, 4)
    lib, ctx = eng._lib, eng._ctx
    ops = np.ascontiguousarray(K.PAULIS).view(np.float64)
    z = np.ascontiguousarray(S.Z).view(np.float64)
    out = np.full(2 * 17 * 6 * 16, 7.0)
    one = np.full(2 * 17 * 4, 7.0)
    site = np.full(2 * 17 * 16, 7.0)
    f = lambda a: a.ctypes.data_as(RS.DP)

    def untouched():
        return np.all(out == 7.0) and np.all(one == 7.0) and np.all(site == 7.0)

    def refused(rc, word):
        msg = lib.qmps_last_error().decode()
        assert rc == _lib.QMPS_ERR_ARG and word in msg, (rc, msg)
        assert untouched()

    call = lib.qmps_correlator_sums
    refused(call(ctx, 17, 0, f(ops), 6, f(z), f(out), f(one), f(site)), 'n_ops')
    refused(call(ctx, 17, 5, f(ops), 6, f(z), f(out), f(one), f(site)), 'n_ops')
    refused(call(ctx, 17, 4, f(ops), 0, f(z), f(out), f(one), f(site)), 'n_z')
    refused(call(ctx, 17, 4, f(ops), 1025, f(z), f(out), f(one), f(site)), 'n_z')
    refused(call(ctx, 17, 4, f(ops), 6, f(z), None, f(one), f(site)), 'G_out')
    refused(call(ctx, 17, 4, None, 6, f(z), f(out), f(one), f(site)), 'ops')
    refused(call(ctx, 17, 4, f(ops), 6, None, f(out), f(one), f(site)), 'null z')
    for bad in (1.0 + 1e-6, 0.8 + 0.8j, np.nan, np.inf):
        zb = S.Z.copy()
        zb[4] = bad
        refused(call(ctx, 17, 4, f(ops), 6, f(np.ascontiguousarray(zb).view(np.float64)), f(out), f(one), f(site)), 'z[4]')
    eng.set_window(100)                                         # a window that runs past the buffers
    refused(call(ctx, eng.max_batch - 50, 4, f(ops), 6, f(z), f(out), f(one), f(site)), 'window')
    # ... and one that runs past the resident states: the state of the context is wrong, not the arguments
    assert call(ctx, 40, 4, f(ops), 6, f(z), f(out), f(one), f(site)) == _lib.QMPS_ERR_STATE and b'resident' in lib.qmps_last_error()
    assert untouched()
    eng.set_window(0)
    refused(call(ctx, -1, 4, f(ops), 6, f(z), f(out), f(one), f(site)), 'window')
    # 65536 x 1024 x 16 x 16 bytes = 16 GiB: refused by arithmetic, before anything is allocated or written
    zl = np.zeros(2 * 1024)
    refused(call(ctx, eng.max_batch, 4, f(ops), 1024, f(zl), f(out), f(one), f(site)), '1 GiB')
    with pytest.raises(_lib.QmpsError):
        eng.correlator_sums(K.PAULIS, np.zeros(1024), B=eng.max_batch)
    with pytest.raises(ValueError):
        eng.correlator_sums(np.zeros((2, 3, 2)), S.Z, B=17)
    # e^(ik) as float64 rounds it is accepted, B = 0 is fine and writes nothing
    assert call(ctx, 0, 4, f(ops), 6, f(z), f(out), f(one), f(site)) == _lib.QMPS_OK and untouched()
    kk = np.linspace(0.0, 2 * np.pi, 1024)
    assert np.isfinite(eng.correlator_sums(K.Z, np.exp(1j * kk), B=3)).all()
    # a following valid call still works
    G, o1, s1 = eng.correlator_sums(K.generic_ops(), S.Z, B=17, want_one_site=True, want_site=True)
    _check(G, o1, s1, _haar_reference(4), 17, 4, 6, 4, 'after errors')


@pytest.mark.parametrize('D', S.DS)
def test_degenerate_fixed_point_and_unusable_environment(engine_factory, D):
    """The pass-through tensor A0 with r = 1 / D in the middle of a batch of five: its resolvent is singular at z = 1 (non-finite G
    there, for it alone) and b_c vanishes, so G is exactly 0 at z = 0.5; the other four rows stay within the bound.  Then row 1 with
    r = 0: NaN in all its outputs, the others bit for bit as before."""
    eng, s = _haar(engine_factory, D)
    keep = np.array([0, 1, 3, 4])
    A = np.ascontiguousarray(np.concatenate([s['A'][:2], S.passthrough_tensor(D)[None], s['A'][2:4]]))
    r = np.ascontiguousarray(np.concatenate([s['r'][:2], (np.eye(D) / D).astype(np.complex128)[None], s['r'][2:4]]))
    z = np.array([1.0, 0.5], dtype=np.complex128)
    ops = K.generic_ops()
    eng.set_tensors(A)
    eng.set_env_guess(r)
    G, one, site = eng.correlator_sums(ops, z, B=5, want_one_site=True, want_site=True)
    assert not np.isfinite(G[2, 0]).any()
    assert not G[2, 1].any()
    assert np.isfinite(one).all() and np.isfinite(site).all() and np.abs(one[2] - ops[:, 0, 0]).max() == 0.0
    ref = S.reference(A[keep], r[keep], ops, z) + (S.bound(A[keep], r[keep], z),)
    _check(G[keep], one[keep], site[keep], ref, 4, 4, 2, D, 'beside the pass-through tensor')
    r0 = r.copy()
    r0[1] = 0.0
    eng.set_env_guess(r0)
    G0, one0, site0 = eng.correlator_sums(ops, z, B=5, want_one_site=True, want_site=True)
    assert np.isnan(G0[1]).all() and np.isnan(one0[1]).all() and np.isnan(site0[1]).all()
    others = np.array([0, 2, 3, 4])
    for x, y in ((G, G0), (one, one0), (site, site0)):
        assert x[others].tobytes() == y[others].tobytes()


@pytest.mark.parametrize('D', (2, 4))
def test_host_helper(D):
    from qmps_amd.ground_state import structure_factor
    P = K.ansatz_params(D)[:3]
    ops = np.stack([K.Z, K.X])
    k = np.array([0.0, 0.3, np.pi])
    Sq, one, st = structure_factor(P, ops, k, D=D)
    assert Sq.shape == (3, 3, 2, 2) and one.shape == (3, 2) and st.shape == (3,) and np.all(st == 0)
    A = K.ansatz_tensors(D)[:3]
    r = np.stack([O.env_dense_eig(a)[1] for a in A])
    Gr, oner, siter = S.reference(A, r, ops, S.k_to_z(k), dtype=np.complex128)
    # 1e-10 is what the energy tests grant an environment against the dense-eig oracle; the resolvent amplifies it by its norm
    tol = 1e-10 * max(1.0, float(S.kappa(A, r, S.k_to_z(k)).max()))
    assert np.abs(Sq - S.structure_factor(Gr, oner, siter)).max() < tol and np.abs(one - oner).max() < 1e-10
