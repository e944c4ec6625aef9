"""GPU: qmps_entanglement - Schmidt spectra, entropies and eigenvectors of the resident environments - against the long-double Jacobi
reference of tests/entanglement_cases.py (the kernels alone: the cases go in verbatim through qmps_set_env_guess), against the
oracle's dense-eig environments after a real solve, and the contract of the call: NaN rows, window, fused-ansatz batches, untouched
state, argument errors, the host helper."""
import numpy as np
import pytest

import entanglement_cases as K
import resident_cases as RS
from oracle import qmps_oracle as O
from qmps_amd import _lib

pytestmark = pytest.mark.gpu

SOLVE_TOL = 1e-13                     # EnergyEngine.launch's default tolerance of the environment solve
_HAAR = {}


def _haar(D, B=max(K.BATCHES)):
    if D not in _HAAR:
        A = np.ascontiguousarray(O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(K.HAAR_SEED[D] + 1), 2 * D, max(K.BATCHES))))
        A.setflags(write=False)
        _HAAR[D] = A
    return _HAAR[D][:B]


def _resident_cases(engine_factory, D, B):
    """Engine with B Haar tensors and, as their environments, the case list cycled (copied verbatim)."""
    eng = engine_factory(D)
    eng.set_tensors(_haar(D, B))
    eng.set_env_guess(K.batch(D, B))
    return eng


@pytest.mark.parametrize('D', K.DS)
def test_kernel_alone_holds_the_three_bounds(engine_factory, D):
    """Every batch size: p within eig_bound, S within entropy_bound, the two eigenvector residuals within eig_bound; NaN rows are exactly
    the all-zero and the NaN case (their neighbours within the bounds like everyone else); the indefinite case returns its negative
    eigenvalue and an S that ignores it; without eigenvectors the same bits."""
    p_ref, V_ref, S_ref = K.case_reference(D)
    kinds = K.kinds(D)
    worst = np.zeros(4)
    for B in K.BATCHES:
        eng = _resident_cases(engine_factory, D, B)
        p, S, V = eng.entanglement(B=B, want_vectors=True)
        assert p.shape == (B, D) and S.shape == (B,) and V.shape == (B, D, D) and V.dtype == np.complex128
        idx = K.batch_index(D, B)
        nan = kinds[idx] == 'nan'
        assert np.array_equal(np.isnan(p).any(axis=1), nan) and np.array_equal(np.isnan(p).all(axis=1), nan)
        assert np.array_equal(np.isnan(S), nan) and np.array_equal(np.isnan(V).all(axis=(1, 2)), nan) and np.array_equal(np.isnan(V).any(axis=(1, 2)), nan)
        ok = ~nan
        e_p = np.abs(p[ok] - p_ref[idx[ok]]).astype(float).max(axis=1)
        e_S = np.abs(S[ok] - S_ref[idx[ok]]).astype(float)
        orth, eq = K.residuals(K.batch(D, B)[ok], p[ok], V[ok])
        now = np.array([e_p.max() / K.eig_bound(D), e_S.max() / K.entropy_bound(D), orth.max() / K.eig_bound(D), eq.max() / K.eig_bound(D)])
        worst = np.maximum(worst, now)
        print(f'entanglement D={D} B={B}: |p - ref| {e_p.max():.2e}, |S - ref| {e_S.max():.2e}, |V^+ V - 1| {orth.max():.2e}, |h V - V p| {eq.max():.2e}'
              f'  (fractions of the bounds {now[0]:.3f} {now[1]:.4f} {now[2]:.3f} {now[3]:.3f})')
        assert np.all(e_p <= K.eig_bound(D)), (D, B, [K.cases(D)[i][0] for i in idx[ok][e_p > K.eig_bound(D)]])
        assert np.all(e_S <= K.entropy_bound(D)), (D, B)
        assert np.all(orth <= K.eig_bound(D)) and np.all(eq <= K.eig_bound(D)), (D, B, orth.max(), eq.max())
        assert np.all(np.diff(p[ok], axis=1) <= 0)
        for b in np.where(kinds[idx] == 'indefinite')[0]:
            pos = p[b][p[b] > 1e-9]
            assert p[b, -1] < -0.1 and abs(S[b] + (pos * np.log(pos)).sum()) <= K.entropy_bound(D)
        p2, S2 = eng.entanglement(B=B)
        assert p2.tobytes() == p.tobytes() and S2.tobytes() == S.tobytes()
    print(f'entanglement D={D}: worst fractions of the bounds: p {worst[0]:.3f}, S {worst[1]:.4f}, |V^+ V - 1| {worst[2]:.3f}, |h V - V p| {worst[3]:.3f}')


@pytest.mark.parametrize('D', K.DS)
def test_after_a_real_solve(engine_factory, D):
    """Haar unitaries, the default solver: p against eigvalsh of the oracle's dense-eig environment within the bound plus ten times the
    tolerance of the solve; a spectrum: positive, of unit sum; where the status is 0 the smallest eigenvalue is positive, as the solve's
    Cholesky test found."""
    B = 12 if D < 16 else 6
    eng = engine_factory(D)
    RS.solve(eng, _haar(D, B), D)
    p, S, V = eng.entanglement(B=B, want_vectors=True)
    st = eng.results_status(B)
    ref = np.stack([np.linalg.eigvalsh(O.env_dense_eig(a)[1])[::-1] for a in _haar(D, B)])
    err = float(np.abs(p - ref).max())
    print(f'entanglement D={D}: after a solve, against eigvalsh of the dense-eig environment {err:.2e}; statuses {np.unique(st).tolist()}')
    assert err <= K.eig_bound(D) + 10 * SOLVE_TOL
    assert np.all(p > 0) and np.abs(p.sum(axis=1) - 1).max() <= 4 * D * K.EPS
    assert np.all(p[st == 0, -1] > 0) and np.mean(st == 0) > 0.9
    assert np.all(S > 0) and np.all(S <= np.log(D) + K.entropy_bound(D))
    orth, eq = K.residuals(eng.environments(B), p, V)
    assert orth.max() <= K.eig_bound(D) and eq.max() <= K.eig_bound(D)


def test_product_state_has_no_entropy(engine_factory):
    """D = 2 ShallowCNOT at (beta_1, gamma_1, beta_2, gamma_2) = (0, pi/2, 0, 0), (0, pi/2, 0, pi/2), (0, 3 pi/2, 0, 3 pi/2): the oracle's
    environment has rank one (a product state across every cut).  S stays below the entropy bound and p = (1, 0) within the
    eigenvalue bound.  Measured on an MI355X: S = 0, -2.2e-16, 0 and p[1] = -1.1e-16 in all three rows.  The status of the solve is 2
    (not positive definite) in all three: the rank-one r has a smallest eigenvalue of -1.1e-16, and the Cholesky test says so."""
    from qmps_amd.ground_state import STATUS_NOT_PD, entanglement_entropy
    prm = np.array([(0, 1, 0, 0), (0, 1, 0, 1), (0, 3, 0, 3)], dtype=float) * np.pi / 2
    ref = np.stack([np.linalg.eigvalsh(O.env_dense_eig(O.unitary_to_tensor(O.shallow_cnot_unitary(2, q)))[1])[::-1] for q in prm])
    assert np.abs(ref[:, 1]).max() < 1e-12 and np.abs(ref[:, 0] - 1).max() < 1e-12
    S, p, st = entanglement_entropy(prm, D=2)
    print(f'entanglement: product states, S {S.tolist()}, p[1] {p[:, 1].tolist()}, status {st.tolist()}')
    assert np.all((st == 0) | (st == STATUS_NOT_PD))
    assert np.all(np.abs(S) <= K.entropy_bound(2))
    assert np.all(np.abs(p[:, 0] - 1) <= K.eig_bound(2)) and np.all(np.abs(p[:, 1]) <= K.eig_bound(2))


def test_embedded_tensor_keeps_the_spectrum(engine_factory):
    """A D = 4 tensor that is the embedding A x 1 of a D = 2 one (`embed_bond_dimension`, eps = 0).  Its transfer map is T x id on the new
    bond index, so every r x X is a fixed point; with the new index in a pure state, r4 = r2 x |0><0|, the first two p are the D = 2
    spectrum and the rest is below the bound."""
    from qmps_amd.ground_state import SU, embed_bond_dimension
    rng = np.random.default_rng(6301)
    B = 5
    v = 0.8 * rng.standard_normal((B, 15))
    A2 = np.ascontiguousarray(np.stack([O.unitary_to_tensor(SU(x, 4)) for x in v]))
    A4 = np.ascontiguousarray(np.stack([O.unitary_to_tensor(SU(embed_bond_dimension(x, eps=0.0), 8)) for x in v]))
    ref = np.einsum('bsij,ac->bsiajc', A2, np.eye(2)).reshape(B, 2, 4, 4)
    ph = np.einsum('bsij,bsij->b', ref.conj(), A4)
    assert np.abs(A4 - (ph / np.abs(ph))[:, None, None, None] * ref).max() < 1e-10
    e2 = engine_factory(2)
    RS.solve(e2, A2, 2)
    assert np.all(e2.results_status(B) == 0)
    r2 = e2.environments(B)
    p2, S2 = e2.entanglement(B=B)
    e4 = engine_factory(4)
    e4.set_tensors(A4)
    r4 = np.stack([np.kron(r, np.diag([1.0, 0.0])) for r in r2])
    # r4 is a fixed point of the embedded map, to the accuracy r2 is one of its own
    T4 = np.einsum('bsij,bjk,bslk->bil', A4, r4, A4.conj())
    assert np.abs(T4 - r4).max() < 1e-12
    e4.set_env_guess(r4)
    p4, S4 = e4.entanglement(B=B)
    # (p2 carries its own rounding: both bounds add)
    assert np.abs(p4[:, :2] - p2).max() <= K.eig_bound(4) + K.eig_bound(2) and np.abs(p4[:, 2:]).max() <= K.eig_bound(4)
    assert np.abs(S4 - S2).max() <= K.entropy_bound(4) + K.entropy_bound(2)


def test_fused_ansatz_batch(engine_factory):
    """D = 4, ShallowCNOT parameters: the direct kernel builds the tensors itself; the spectra are those of the environments it stored.
    Without stored environments the call refuses (QMPS_ERR_STATE)."""
    eng = engine_factory(4)
    P = np.random.default_rng(6204).standard_normal((21, 4))
    R = P.shape[0]
    eng.set_hamiltonian(RS.H_TFIM)
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)
    eng.launch(R, solver='direct', store_env=True)
    p, S, V = eng.entanglement(B=R, want_vectors=True)
    r = eng.environments(R)
    p_ref, V_ref, S_ref = K.reference_spectrum(r)
    orth, eq = K.residuals(r, p, V)
    assert np.abs(p - p_ref).max() <= K.eig_bound(4) and np.abs(S - S_ref).max() <= K.entropy_bound(4)
    assert orth.max() <= K.eig_bound(4) and eq.max() <= K.eig_bound(4)
    # the resident parameters stay as they were: the batch launched again rebuilds its tensors from them, to the same bits
    before = eng.results(R) + (r,)
    eng.launch(R, solver='direct', store_env=True)
    after = eng.results(R) + (eng.environments(R),)
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)
    eng.launch(R, solver='direct', store_env=False)
    with pytest.raises(_lib.QmpsError) as info:
        eng.entanglement(B=R)
    assert info.value.code == _lib.QMPS_ERR_STATE and 'environment' in str(info.value)


@pytest.mark.parametrize('D', K.DS)
def test_window(engine_factory, D):
    """Two batches side by side (64 and 66 evaluations); the window addresses the second."""
    eng = _resident_cases(engine_factory, D, 130)
    p, S, V = eng.entanglement(B=130, want_vectors=True)
    eng.set_window(64)
    p1, S1, V1 = eng.entanglement(B=66, want_vectors=True)
    eng.set_window(0)
    assert p1.tobytes() == p[64:].tobytes() and S1.tobytes() == S[64:].tobytes() and V1.tobytes() == V[64:].tobytes()


@pytest.mark.parametrize('D', K.DS)
def test_nothing_else_moves(engine_factory, D):
    eng = engine_factory(D)
    B = 65
    RS.solve(eng, _haar(D, B), D)
    before = (eng.results(B), eng.environments(B), eng.results_status(B), eng.tensors(B))
    eng.entanglement(B=B, want_vectors=True)
    eng.entanglement(B=B)
    after = (eng.results(B), eng.environments(B), eng.results_status(B), eng.tensors(B))
    for x, y in zip(before[0] + before[1:], after[0] + after[1:]):
        assert np.array_equal(x, y) and x.tobytes() == y.tobytes()


def test_argument_errors(engine_factory):
    eng = _resident_cases(engine_factory, 4, 40)
    lib, ctx = eng._lib, eng._ctx
    out = np.full(4 * 64, 7.0)
    f = lambda a: a.ctypes.data_as(RS.DP)

    def refused(rc, code, word):
        msg = lib.qmps_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        assert np.all(out == 7.0)

    refused(lib.qmps_entanglement(ctx, 17, None, None, None), _lib.QMPS_ERR_ARG, 'p_out')
    refused(lib.qmps_entanglement(ctx, -1, f(out), None, None), _lib.QMPS_ERR_ARG, 'window')
    refused(lib.qmps_entanglement(ctx, eng.max_batch + 1, f(out), None, None), _lib.QMPS_ERR_ARG, 'max_batch')
    refused(lib.qmps_entanglement(ctx, 41, f(out), None, None), _lib.QMPS_ERR_STATE, 'resident')       # beyond the resident states
    assert lib.qmps_entanglement(ctx, 0, f(out), None, None) == _lib.QMPS_OK and np.all(out == 7.0)     # empty batch: nothing written
    eng.set_tensors(_haar(4, 40))                                                                      # new states: no environment
    refused(lib.qmps_entanglement(ctx, 40, f(out), None, None), _lib.QMPS_ERR_STATE, 'environment')
    with pytest.raises(_lib.QmpsError):
        eng.entanglement(B=40)
    # a following valid call still works
    eng.set_env_guess(K.batch(4, 40))
    p, S = eng.entanglement(B=17)
    assert np.abs(p[0] - K.case_reference(4)[0][0]).max() <= K.eig_bound(4)


@pytest.mark.parametrize('D', (2, 4))
def test_host_helper(D):
    from qmps_amd.ground_state import entanglement_entropy
    P = np.random.default_rng(6400 + D).standard_normal((5, 4))
    S, p, st = entanglement_entropy(P, D=D)
    assert S.shape == (5,) and p.shape == (5, D) and st.shape == (5,) and np.all(st == 0)
    ref = np.stack([np.linalg.eigvalsh(O.env_dense_eig(O.unitary_to_tensor(O.shallow_cnot_unitary(D, q)))[1])[::-1] for q in P])
    S_ref = -np.where(ref > 1e-300, ref * np.log(np.where(ref > 1e-300, ref, 1.0)), 0.0).sum(axis=1)
    assert np.abs(p - ref).max() < 1e-10 and np.abs(S - S_ref).max() < 1e-9
