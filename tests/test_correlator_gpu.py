"""GPU: qmps_correlators - the two-point functions of the resident states - against the long-double reference of
tests/correlator_cases.py evaluated from the tensors and environments read back from the device (the kernel alone, within the
rounding bound), against the oracle's own environments and state vectors (1e-10, the tolerance the energy tests hold against the
dense-eig oracle), and the contract of the call: conventions, window, fused-ansatz batches, untouched state, argument errors."""
import numpy as np
import pytest

import correlator_cases as K
import resident_cases as RS
from oracle import qmps_oracle as O
from qmps_amd import _lib

pytestmark = pytest.mark.gpu

def _reference(D, ops_name, rows, n_max):
    """Long-double reference from the read-back arrays, cached per (operators, block of the plan)."""
    s = RS.solved(D)
    ops = {'generic': K.generic_ops(), 'paulis': K.PAULIS}[ops_name]
    return RS.cached(D, __name__, (ops_name, rows, n_max), lambda: K.reference(s['A'][:rows], s['r'][:rows], ops, n_max))


@pytest.mark.parametrize('D', K.DS)
def test_kernel_alone_within_the_rounding_bound(engine_factory, D):
    """Haar tensors, environments stored, tensors and environments read back; `correlators` against the long-double reference of
    those arrays, elementwise within bound(D, n): B in (1, 17, 65, 130) x n_ops in (1, 2, 3, 4) x n_max in (1, 2, 7), n_max = 64 at
    B = 1 and 17, n_max = 512 at D = 2, 4 (B = 17); non-Hermitian complex operators."""
    eng, s = RS.haar(engine_factory, D)
    (rows_s, n_s), (rows_l, n_l) = K.reference_plan(D)
    worst, worst_ratio, worst_one = 0.0, 0.0, 0.0
    for B, m, n_max in K.kernel_cases(D):
        Cr, oner = _reference(D, 'generic', rows_s, n_s) if n_max <= n_s else _reference(D, 'generic', rows_l, n_l)
        C, one = eng.correlators(K.generic_ops()[:m], n_max, B=B, want_one_site=True)
        assert C.shape == (B, m, m, n_max) and one.shape == (B, m) and C.dtype == np.complex128
        err = np.abs(C - Cr[:B, :m, :m, :n_max]).astype(float)
        err_one = float(np.abs(one - oner[:B, :m]).max())
        bnd = K.bound(D, np.arange(1, n_max + 1))
        worst, worst_ratio, worst_one = max(worst, float(err.max())), max(worst_ratio, float((err / bnd).max())), max(worst_one, err_one)
        assert np.all(err <= bnd), (D, B, m, n_max, float(err.max()), float((err / bnd).max()))
        assert err_one <= K.bound(D, 1), (D, B, m, n_max, err_one)
    print(f'correlators D={D}: worst |C - long double| {worst:.2e} (largest err / bound {worst_ratio:.3f}), worst |one - long double| {worst_one:.2e}')


def test_against_the_state_vectors_of_the_oracle(engine_factory):
    """D = 2, B = 8, n <= 5: the oracle's state-vector route with its own get_env_exact - no transfer map, no device environment."""
    eng = engine_factory(2)
    U = O.haar_unitaries(np.random.default_rng(5402), 4, 8)
    RS.solve(eng, O.unitary_to_tensor(U), 2)
    ops = np.concatenate([K.generic_ops()[:2], K.SIGMA_PLUS[None]])
    C, one = eng.correlators(ops, 5, B=8, want_one_site=True)
    assert np.all(eng.results_status(8) == 0)
    for b in range(8):
        Cs, ones = K.statevector_correlators(U[b], ops, 5)
        assert np.abs(C[b] - Cs).max() < 1e-10 and np.abs(one[b] - ones).max() < 1e-10


@pytest.mark.parametrize('D', K.DS)
def test_against_the_dense_eig_environment(engine_factory, D):
    """The reference evaluated with env_dense_eig's r instead of the device's: every Haar item has status 0."""
    eng, s = RS.haar(engine_factory, D)
    assert np.all(s['st'] == 0)
    rows = 12 if D < 16 else 6
    ops = np.concatenate([K.generic_ops()[:3], K.SIGMA_PLUS[None]])
    C, one = eng.correlators(ops, 16, B=rows, want_one_site=True)
    r = np.stack([O.env_dense_eig(a)[1] for a in s['A'][:rows]])
    Cr, oner = K.reference(s['A'][:rows], r, ops, 16, dtype=np.complex128)
    err = max(float(np.abs(C - Cr).max()), float(np.abs(one - oner).max()))
    print(f'correlators D={D}: against the dense-eig environment {err:.2e}')
    assert err < 1e-10


@pytest.mark.parametrize('D', K.DS)
def test_conventions_with_the_paulis(engine_factory, D):
    eng, s = RS.haar(engine_factory, D)
    B = 17
    C, one = eng.correlators(K.PAULIS, 7, B=B, want_one_site=True)
    assert np.abs(C[:, 0, :, :] - one[:, :, None]).max() < 1e-10          # identity on site 0: <O_c>
    assert np.abs(C[:, :, 0, :] - one[:, :, None]).max() < 1e-10          # identity on site n: <O_a>, for every n
    assert np.abs(C[:, 0, 0, :] - 1.0).max() < 1e-10
    rho = eng.rdm(B)
    C1, o1 = K.rdm_correlators(rho, K.PAULIS)
    assert np.abs(C[..., 0] - C1).max() < 1e-10 and np.abs(one - o1).max() < 1e-10
    # one (2, 2) matrix is one operator
    Cz = eng.correlators(K.Z, 7, B=B)
    assert Cz.shape == (B, 1, 1, 7) and np.abs(Cz[:, 0, 0] - C[:, 3, 3]).max() < 1e-14


def test_fused_ansatz_batch(engine_factory):
    """D = 4, ShallowCNOT parameters: the direct kernel builds the tensors itself, d_A is materialised by the call; without stored
    environments the call refuses (QMPS_ERR_STATE)."""
    eng = engine_factory(4)
    P = K.ansatz_params(4)
    R = P.shape[0]
    ops = np.stack([K.SIGMA_PLUS, K.Z, K.X])
    eng.set_hamiltonian(RS.H_TFIM)
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)
    eng.launch(R, solver='direct', store_env=True)
    C, one = eng.correlators(ops, K.N_LONG, B=R, want_one_site=True)
    A, r = eng.ansatz_probe(_lib.ANSATZ_SHALLOW_CNOT, P), eng.environments(R)
    assert np.abs(A - K.ansatz_tensors(4)).max() < 1e-13
    Cr, oner = K.reference(A, r, ops, K.N_LONG)
    err = np.abs(C - Cr).astype(float)
    print(f'correlators D=4, fused ShallowCNOT batch: worst |C - long double| {err.max():.2e}')
    assert np.all(err <= K.bound(4, np.arange(1, K.N_LONG + 1))) and np.abs(one - oner).max() <= K.bound(4, 1)
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)
    eng.launch(R, solver='direct', store_env=False)
    with pytest.raises(_lib.QmpsError) as info:
        eng.correlators(ops, 4, B=R)
    assert info.value.code == _lib.QMPS_ERR_STATE and 'environment' in str(info.value)


@pytest.mark.parametrize('D', K.DS)
def test_window(engine_factory, D):
    eng, s = RS.haar(engine_factory, D)
    ops = K.generic_ops()[:3]
    full, one_full = eng.correlators(ops, 7, B=K.HAAR_B, want_one_site=True)
    eng.set_window(64)
    part, one_part = eng.correlators(ops, 7, B=66, want_one_site=True)
    eng.set_window(0)
    assert np.array_equal(part, full[64:130]) and np.array_equal(one_part, one_full[64:130])


@pytest.mark.parametrize('D', K.DS)
def test_nothing_else_moves(engine_factory, D):
    eng = engine_factory(D)
    B = 65
    RS.solve(eng, K.haar_tensors(D)[:B], D)
    before = (eng.results(B), eng.environments(B), eng.results_status(B), eng.tensors(B))
    eng.correlators(K.generic_ops(), 7, B=B, want_one_site=True)
    after = (eng.results(B), eng.environments(B), eng.results_status(B), eng.tensors(B))
    for x, y in zip(before[0] + before[1:], after[0] + after[1:]):
        assert x.tobytes() == y.tobytes()


def test_argument_errors(engine_factory):
    eng, s = RS.haar(engine_factory, 4)
    lib, ctx = eng._lib, eng._ctx
    ops = np.ascontiguousarray(K.PAULIS).view(np.float64)
    out = np.full(2 * 17 * 16 * 4, 7.0)
    f = lambda a: a.ctypes.data_as(RS.DP)

    def refused(rc, word):
        msg = lib.qmps_last_error().decode()
        assert rc == _lib.QMPS_ERR_ARG and word in msg, (rc, msg)
        assert np.all(out == 7.0)

    refused(lib.qmps_correlators(ctx, 17, 0, f(ops), 4, f(out), None), 'n_ops')
    refused(lib.qmps_correlators(ctx, 17, 5, f(ops), 4, f(out), None), 'n_ops')
    refused(lib.qmps_correlators(ctx, 17, 4, f(ops), 0, f(out), None), 'n_max')
    refused(lib.qmps_correlators(ctx, 17, 4, f(ops), 4097, f(out), None), 'n_max')
    refused(lib.qmps_correlators(ctx, 17, 4, f(ops), 4, None, None), 'C_out')
    refused(lib.qmps_correlators(ctx, 17, 4, None, 4, f(out), None), 'ops')
    eng.set_window(100)                                         # a window that runs past the buffers
    refused(lib.qmps_correlators(ctx, eng.max_batch - 50, 4, f(ops), 4, f(out), None), 'window')
    # ... and one that runs past the resident states: the state of the context is wrong, not the arguments
    assert lib.qmps_correlators(ctx, 40, 4, f(ops), 4, f(out), None) == _lib.QMPS_ERR_STATE and b'resident' in lib.qmps_last_error()
    assert np.all(out == 7.0)
    eng.set_window(0)
    refused(lib.qmps_correlators(ctx, -1, 4, f(ops), 4, f(out), None), 'window')
    # 65536 x 16 x 4096 x 16 bytes = 64 GiB: refused by arithmetic, before anything is allocated or written
    refused(lib.qmps_correlators(ctx, eng.max_batch, 4, f(ops), 4096, f(out), None), '1 GiB')
    with pytest.raises(_lib.QmpsError):
        eng.correlators(K.PAULIS, 4096, B=eng.max_batch)
    with pytest.raises(ValueError):
        eng.correlators(np.zeros((2, 3, 2)), 4, B=17)
    # a following valid call still works
    C = eng.correlators(K.generic_ops(), 7, B=17)
    assert np.all(np.abs(C - _reference(4, 'generic', *K.reference_plan(4)[0])[0][:17]) <= K.bound(4, np.arange(1, 8)))


@pytest.mark.parametrize('D', (2, 4))
def test_host_helper(D):
    from qmps_amd.ground_state import correlation_functions
    P = K.ansatz_params(D)[:3]
    ops = np.stack([K.Z, K.X, K.SIGMA_PLUS])
    C, one, st = correlation_functions(P, ops, 12, D=D)
    assert C.shape == (3, 3, 3, 12) and one.shape == (3, 3) and st.shape == (3,) and np.all(st == 0)
    A = K.ansatz_tensors(D)[:3]
    r = np.stack([O.env_dense_eig(a)[1] for a in A])
    Cr, oner = K.reference(A, r, ops, 12, dtype=np.complex128)
    assert np.abs(C - Cr).max() < 1e-10 and np.abs(one - oner).max() < 1e-10
    Cc, one_c, _ = correlation_functions(P, ops, 12, D=D, connected=True)
    assert np.abs(Cc - (Cr - (oner[:, :, None] * oner[:, None, :])[..., None])).max() < 1e-10 and np.abs(one_c - oner).max() < 1e-10
    assert np.abs(Cc - C).max() > 1e-3
