"""GPU: qmps_string_correlators - two-point functions with a one-site string between their ends, and the string order itself -
against the long-double reference of tests/string_correlator_cases.py evaluated from the tensors and environments read back from the
device (the kernel alone, within the rounding bound of tests/correlator_cases.py), on symmetric tensors whose string order does not
decay, against the plain call and against itself, against the oracle's state vectors (1e-10), and the contract of the call: window,
fused-ansatz batches, untouched state, argument errors."""
import numpy as np
import pytest

import correlator_cases as K
import resident_cases as RS
import string_correlator_cases as SC
from oracle import qmps_oracle as O
from qmps_amd import _lib

pytestmark = pytest.mark.gpu

STRINGS = ('X', 'generic')


def _reference(D, string, rows, n_max):
    """Long-double reference from the read-back arrays, cached per (string, block of the plan)."""
    s = RS.solved(D)
    return RS.cached(D, __name__, (string, rows, n_max),
                     lambda: SC.reference(s['A'][:rows], s['r'][:rows], K.generic_ops(), SC.strings()[string], n_max))


@pytest.mark.parametrize('string', STRINGS)
@pytest.mark.parametrize('D', K.DS)
def test_kernel_alone_within_the_rounding_bound(engine_factory, D, string):
    """Haar tensors, environments stored, tensors and environments read back; C, one and str against the long-double reference of those
    arrays, elementwise within bound(D, n): B in (1, 17, 65, 130) x n_ops in (1, 2, 3, 4) x n_max in (1, 2, 7), n_max = 64 at B = 1 and
    17, n_max = 512 at D = 2, 4 (B = 17); non-Hermitian complex operators, the strings X and a non-normal complex matrix."""
    eng, s = RS.haar(engine_factory, D)
    S = SC.strings()[string]
    (rows_s, n_s), (rows_l, n_l) = K.reference_plan(D)
    worst, worst_ratio, worst_one = 0.0, 0.0, 0.0
    for B, m, n_max in K.kernel_cases(D):
        Cr, oner, strr = _reference(D, string, rows_s, n_s) if n_max <= n_s else _reference(D, string, rows_l, n_l)
        C, one, st = eng.correlators(K.generic_ops()[:m], n_max, B=B, want_one_site=True, string=S, want_string=True)
        assert C.shape == (B, m, m, n_max) and one.shape == (B, m) and st.shape == (B, n_max) and C.dtype == st.dtype == np.complex128
        err = np.abs(C - Cr[:B, :m, :m, :n_max]).astype(float)
        err_str = np.abs(st - strr[:B, :n_max]).astype(float)
        err_one = float(np.abs(one - oner[:B, :m]).max())
        bnd = K.bound(D, np.arange(1, n_max + 1))
        worst = max(worst, float(err.max()), float(err_str.max()))
        worst_ratio, worst_one = max(worst_ratio, float((err / bnd).max()), float((err_str / bnd).max())), max(worst_one, err_one)
        assert np.all(err <= bnd), (D, B, m, n_max, float(err.max()), float((err / bnd).max()))
        assert np.all(err_str <= bnd), (D, B, m, n_max, float(err_str.max()), float((err_str / bnd).max()))
        assert err_one <= K.bound(D, 1), (D, B, m, n_max, err_one)
        # C alone, without the optional outputs: the same numbers
        if m == 2 and n_max == 7:
            assert np.array_equal(eng.correlators(K.generic_ops()[:m], n_max, B=B, string=S), C)
    print(f'string correlators D={D}, string {string}: worst |C, str - long double| {worst:.2e} (largest err / bound {worst_ratio:.3f}), '
          f'worst |one - long double| {worst_one:.2e}')


@pytest.mark.parametrize('D', K.DS)
def test_symmetric_batch_where_the_string_order_does_not_decay(engine_factory, D):
    """Tensors with X.A = u A u^+ and their power-iterated environments, handed over by set_env_guess (no solver takes part): E_X has an
    eigenvalue of modulus 1, str tends to |tr(u r)|^2 and every step's rounding stays in all later values.  Same bound, n_max = 64
    (512 at D = 2, 4); the last |str| is within 1e-3 of the reference's own value, which is not zero."""
    eng = engine_factory(D)
    A, r = SC.symmetric_tensors(D), SC.symmetric_environments(D)
    B, n_max = A.shape[0], SC.SYMMETRIC_N[D]
    eng.set_tensors(A)
    eng.set_hamiltonian(RS.H_TFIM)
    eng.set_env_guess(r)
    Ab, rb = eng.tensors(B), eng.environments(B)
    assert np.array_equal(Ab, A) and np.array_equal(rb, r)
    ops = np.stack([K.X, K.Z])
    C, one, st = eng.correlators(ops, n_max, B=B, want_one_site=True, string=K.X, want_string=True)
    Cr, oner, strr = SC.reference(Ab, rb, ops, K.X, n_max)
    bnd = K.bound(D, np.arange(1, n_max + 1))
    err, err_str = np.abs(C - Cr).astype(float), np.abs(st - strr).astype(float)
    last = np.abs(strr[:, -1]).astype(float)
    print(f'string correlators D={D}, symmetric batch of {B}, n_max={n_max}: worst |C, str - long double| {max(err.max(), err_str.max()):.2e} '
          f'(largest err / bound {max((err / bnd).max(), (err_str / bnd).max()):.3f}), |str[n_max]| between {last.min():.2e} and {last.max():.2e}')
    assert np.all(err <= bnd) and np.all(err_str <= bnd) and np.abs(one - oner).max() <= K.bound(D, 1)
    assert last.min() > 1e-6
    assert np.abs(np.abs(st[:, -1]) - last).max() < 1e-3


@pytest.mark.parametrize('D', K.DS)
def test_identity_string_is_the_plain_call(engine_factory, D):
    eng, s = RS.haar(engine_factory, D)
    B = 17
    for n_max in (7, K.N_LONG):
        Cp, onep = eng.correlators(K.generic_ops(), n_max, B=B, want_one_site=True)
        C, one, st = eng.correlators(K.generic_ops(), n_max, B=B, want_one_site=True, string=K.I2, want_string=True)
        bnd = K.bound(D, np.arange(1, n_max + 1))
        assert np.all(np.abs(C - Cp) <= bnd) and np.abs(one - onep).max() <= K.bound(D, 1)
        assert np.all(np.abs(st - 1.0) <= bnd)
        assert np.array_equal(eng.string_order(K.I2, n_max, B=B), st)


@pytest.mark.parametrize('string', STRINGS)
@pytest.mark.parametrize('D', K.DS)
def test_string_among_the_operators_gives_the_string_order(engine_factory, D, string):
    """C[S][S][n - 1] = <S(0) S(1) .. S(n)> is the string of n + 1 sites, str[n]: two chains of the same launch, read out differently."""
    eng, s = RS.haar(engine_factory, D)
    S = SC.strings()[string]
    B, n_max = 17, K.N_LONG
    C, st = eng.correlators(np.stack([K.Z, S]), n_max, B=B, string=S, want_string=True)
    bnd = K.bound(D, np.arange(2, n_max + 1))
    assert np.all(np.abs(C[:, 1, 1, :-1] - st[:, 1:]) <= bnd)
    assert np.array_equal(eng.string_order(S, n_max, B=B), st)


def test_against_the_state_vectors_of_the_oracle(engine_factory):
    """D = 2, B = 8, n <= 5: the oracle's state-vector route with its own get_env_exact and the string on every inner site - no
    transfer map, no device environment."""
    eng = engine_factory(2)
    U = O.haar_unitaries(np.random.default_rng(5402), 4, 8)
    RS.solve(eng, O.unitary_to_tensor(U), 2)
    ops = np.concatenate([K.generic_ops()[:2], K.SIGMA_PLUS[None]])
    assert np.all(eng.results_status(8) == 0)
    for name in STRINGS:
        S = SC.strings()[name]
        C, one, st = eng.correlators(ops, 5, B=8, want_one_site=True, string=S, want_string=True)
        for b in range(8):
            Cs, ones, sts = SC.statevector_string_correlators(U[b], ops, S, 5)
            assert np.abs(C[b] - Cs).max() < 1e-10 and np.abs(one[b] - ones).max() < 1e-10 and np.abs(st[b] - sts).max() < 1e-10, (name, b)


@pytest.mark.parametrize('D', K.DS)
def test_window(engine_factory, D):
    eng, s = RS.haar(engine_factory, D)
    ops, S = K.generic_ops()[:3], SC.strings()['generic']
    full = eng.correlators(ops, 7, B=K.HAAR_B, want_one_site=True, string=S, want_string=True)
    eng.set_window(64)
    part = eng.correlators(ops, 7, B=66, want_one_site=True, string=S, want_string=True)
    eng.set_window(0)
    for f, p in zip(full, part):
        assert np.array_equal(p, f[64:130])


def test_fused_ansatz_batch(engine_factory):
    """D = 4, ShallowCNOT parameters: the direct kernel builds the tensors itself, d_A is materialised by the call; without stored
    environments the call refuses (QMPS_ERR_STATE) and leaves its outputs alone."""
    eng = engine_factory(4)
    P = K.ansatz_params(4)
    R = P.shape[0]
    ops = np.stack([K.SIGMA_PLUS, K.Z, K.X])
    eng.set_hamiltonian(RS.H_TFIM)
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)
    eng.launch(R, solver='direct', store_env=True)
    C, one, st = eng.correlators(ops, K.N_LONG, B=R, want_one_site=True, string=K.X, want_string=True)
    A, r = eng.ansatz_probe(_lib.ANSATZ_SHALLOW_CNOT, P), eng.environments(R)
    Cr, oner, strr = SC.reference(A, r, ops, K.X, K.N_LONG)
    bnd = K.bound(4, np.arange(1, K.N_LONG + 1))
    err = max(float(np.abs(C - Cr).max()), float(np.abs(st - strr).max()))
    print(f'string correlators D=4, fused ShallowCNOT batch: worst |C, str - long double| {err:.2e}')
    assert np.all(np.abs(C - Cr) <= bnd) and np.all(np.abs(st - strr) <= bnd) and np.abs(one - oner).max() <= K.bound(4, 1)
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)
    eng.launch(R, solver='direct', store_env=False)
    with pytest.raises(_lib.QmpsError) as info:
        eng.correlators(ops, 4, B=R, string=K.X)
    assert info.value.code == _lib.QMPS_ERR_STATE and 'environment' in str(info.value)
    out = np.full(2 * R * 9 * 4, 7.0)
    f = lambda a: a.ctypes.data_as(RS.DP)
    rc = eng._lib.qmps_string_correlators(eng._ctx, R, 3, f(np.ascontiguousarray(ops).view(np.float64)), f(np.ascontiguousarray(K.X).view(np.float64)), 4,
                                          f(out), f(out), f(out))
    assert rc == _lib.QMPS_ERR_STATE and np.all(out == 7.0)


@pytest.mark.parametrize('D', K.DS)
def test_nothing_else_moves(engine_factory, D):
    eng = engine_factory(D)
    B = 65
    RS.solve(eng, K.haar_tensors(D)[:B], D)
    before = (eng.results(B), eng.environments(B), eng.results_status(B), eng.tensors(B))
    eng.correlators(K.generic_ops(), 7, B=B, want_one_site=True, string=K.X, want_string=True)
    after = (eng.results(B), eng.environments(B), eng.results_status(B), eng.tensors(B))
    for x, y in zip(before[0] + before[1:], after[0] + after[1:]):
        assert x.tobytes() == y.tobytes()


def test_argument_errors(engine_factory):
    eng, s = RS.haar(engine_factory, 4)
    lib, ctx = eng._lib, eng._ctx
    ops = np.ascontiguousarray(K.PAULIS).view(np.float64)
    S = np.ascontiguousarray(K.X).view(np.float64)
    out, one, st = np.full(2 * 17 * 16 * 4, 7.0), np.full(2 * 17 * 4, 7.0), np.full(2 * 17 * 4, 7.0)
    f = lambda a: a.ctypes.data_as(RS.DP)
    call = lib.qmps_string_correlators

    def untouched():
        return np.all(out == 7.0) and np.all(one == 7.0) and np.all(st == 7.0)

    def refused(rc, word):
        msg = lib.qmps_last_error().decode()
        assert rc == _lib.QMPS_ERR_ARG and word in msg, (rc, msg)
        assert untouched()

    refused(call(ctx, 17, 4, f(ops), None, 4, f(out), f(one), f(st)), 'string')
    refused(call(ctx, 17, 0, f(ops), f(S), 4, f(out), f(one), f(st)), 'n_ops')
    refused(call(ctx, 17, 5, f(ops), f(S), 4, f(out), f(one), f(st)), 'n_ops')
    refused(call(ctx, 17, 4, f(ops), f(S), 0, f(out), f(one), f(st)), 'n_max')
    refused(call(ctx, 17, 4, f(ops), f(S), 4097, f(out), f(one), f(st)), 'n_max')
    refused(call(ctx, 17, 4, f(ops), f(S), 4, None, f(one), f(st)), 'C_out')
    refused(call(ctx, 17, 4, None, f(S), 4, f(out), f(one), f(st)), 'ops')
    eng.set_window(100)                                         # a window that runs past the buffers
    refused(call(ctx, eng.max_batch - 50, 4, f(ops), f(S), 4, f(out), f(one), f(st)), 'window')
    # ... and one that runs past the resident states: the state of the context is wrong, not the arguments
    assert call(ctx, 40, 4, f(ops), f(S), 4, f(out), f(one), f(st)) == _lib.QMPS_ERR_STATE and b'resident' in lib.qmps_last_error()
    assert untouched()
    eng.set_window(0)
    refused(call(ctx, -1, 4, f(ops), f(S), 4, f(out), f(one), f(st)), 'window')
    # 65536 x 17 x 4096 x 16 bytes = 68 GiB: refused by arithmetic, before anything is allocated or written
    refused(call(ctx, eng.max_batch, 4, f(ops), f(S), 4096, f(out), f(one), f(st)), '1 GiB')
    # the limit counts str: 32769 x (1 + 1) x 1024 x 16 bytes is 32 KiB more than 1 GiB; without str_out it is half of that, and the
    # call goes on to find that so many states are not resident
    assert eng.max_batch >= 32769
    refused(call(ctx, 32769, 1, f(ops), f(S), 1024, f(out), f(one), f(st)), '1 GiB')
    assert call(ctx, 32769, 1, f(ops), f(S), 1024, f(out), f(one), None) == _lib.QMPS_ERR_STATE and b'resident' in lib.qmps_last_error()
    assert untouched()
    with pytest.raises(_lib.QmpsError):
        eng.correlators(K.PAULIS, 4096, B=eng.max_batch, string=K.X, want_string=True)
    with pytest.raises(ValueError):
        eng.correlators(K.PAULIS, 4, B=17, string=np.zeros((2, 3)))
    # B = 0 writes nothing
    assert call(ctx, 0, 4, f(ops), f(S), 4, f(out), f(one), f(st)) == _lib.QMPS_OK and untouched()
    # a following valid call still works
    C, strv = eng.correlators(K.generic_ops(), 7, B=17, string=K.X, want_string=True)
    Cr, _, strr = _reference(4, 'X', *K.reference_plan(4)[0])
    bnd = K.bound(4, np.arange(1, 8))
    assert np.all(np.abs(C - Cr[:17]) <= bnd) and np.all(np.abs(strv - strr[:17]) <= bnd)


@pytest.mark.parametrize('D', (2, 4))
def test_host_helper(D):
    from qmps_amd.ground_state import string_correlators
    P = K.ansatz_params(D)[:3]
    ops = np.stack([K.Z, K.X, K.SIGMA_PLUS])
    C, one, st, status = string_correlators(P, ops, K.X, 12, D=D)
    assert C.shape == (3, 3, 3, 12) and one.shape == (3, 3) and st.shape == (3, 12) and status.shape == (3,) and np.all(status == 0)
    A = K.ansatz_tensors(D)[:3]
    r = np.stack([O.env_dense_eig(a)[1] for a in A])
    Cr, oner, strr = SC.reference(A, r, ops, K.X, 12, dtype=np.complex128)
    assert np.abs(C - Cr).max() < 1e-10 and np.abs(one - oner).max() < 1e-10 and np.abs(st - strr).max() < 1e-10
