"""CPU: tests/string_correlator_cases.py checked without a GPU - the long-double reference of the string correlators against the
oracle's state vectors, against the plain reference (identity string) and against itself (C_SS = str), the symmetric tensors, the
rounding bound of tests/correlator_cases.py against float64 numpy on the very cases the GPU tests use, and the C-ABI checks that need
no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import correlator_cases as K
import string_correlator_cases as SC
from oracle import qmps_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_equals_the_state_vector_route():
    """D = 2, n <= 5: <psi| O_a(0) S(1) .. S(n-1) O_c(n) |psi> and <psi| S(1) .. S(n) |psi> on oracle.state_vector, every string."""
    U = O.haar_unitaries(np.random.default_rng(5750), 4, 1)[0]
    A = O.unitary_to_tensor(U)
    _, r = O.env_dense_eig(A)
    ops = np.concatenate([K.generic_ops()[:2], K.SIGMA_PLUS[None]])
    for name, S in SC.strings().items():
        C, one, st = SC.reference(A, r, ops, S, 5)
        Cs, ones, sts = SC.statevector_string_correlators(U, ops, S, 5)
        err = max(float(np.abs(C - Cs).max()), float(np.abs(one - ones).max()), float(np.abs(st - sts).max()))
        print(f'string {name}: reference vs state vectors {err:.2e}')
        assert err < 1e-10
    # the string matters from n = 2 on, and not before
    C1 = SC.reference(A, r, ops, K.X, 5)[0]
    Cp = K.reference(A, r, ops, 5)[0]
    assert np.abs(C1[..., 0] - Cp[..., 0]).max() < 1e-15 and np.abs(C1[..., 1:] - Cp[..., 1:]).max() > 1e-3


@pytest.mark.parametrize('D', K.DS)
def test_identity_string_reproduces_the_plain_reference(D):
    A = K.haar_tensors(D)[:6]
    r = K.fixed_points(A)
    C, one, st = SC.reference(A, r, K.generic_ops(), K.I2, 9)
    Cp, onep = K.reference(A, r, K.generic_ops(), 9)
    assert np.abs(C - Cp).max() < 1e-17 and np.abs(one - onep).max() < 1e-17
    assert np.abs(st - 1).max() < 1e-13                     # T keeps the trace of an isometry's environment


@pytest.mark.parametrize('D', K.DS)
def test_string_among_the_operators_gives_the_string_order(D):
    """<S(0) S(1) .. S(n-1) S(n)> is the string of n + 1 sites: C[S][S][n - 1] == str[n]."""
    A = K.haar_tensors(D)[:6]
    r = K.fixed_points(A)
    for name, S in SC.strings().items():
        C, _, st = SC.reference(A, r, np.stack([K.Z, S]), S, 9)
        assert np.abs(C[:, 1, 1, :-1] - st[:, 1:]).max() < 1e-17, name


@pytest.mark.parametrize('D', K.DS)
def test_symmetric_tensors(D):
    A = SC.symmetric_tensors(D)
    u = SC.parity(D)
    assert A.shape == (SC.SYMMETRIC_B[D], 2, D, D)
    G = np.einsum('bsji,bsjk->bik', A.conj(), A)
    assert np.abs(G - np.eye(D)).max() < 1e-14
    assert np.abs(np.einsum('ts,bsij->btij', K.X, A) - np.einsum('ij,btjk,kl->btil', u, A, u.conj().T)).max() < 1e-14
    # the string order does not decay: it tends to |tr(u r)|^2
    r = SC.symmetric_environments(D)
    n = SC.SYMMETRIC_N[D]
    _, _, st = SC.reference(A, r, K.X, K.X, n, dtype=np.complex128)
    limit = np.abs(np.einsum('ij,bji->b', u, r)) ** 2
    print(f'D={D}: |str[{n}]| between {np.abs(st[:, -1]).min():.2e} and {np.abs(st[:, -1]).max():.2e}, |tr(u r)|^2 between {limit.min():.2e} and {limit.max():.2e}')
    assert np.abs(st[:, -1]).min() > 1e-6
    if D <= 4:
        assert np.abs(np.abs(st[:, -1]) - limit).max() < 1e-6


def _ratio(A, r, ops, S, n_max):
    Cl, ol, sl = SC.reference(A, r, ops, S, n_max)
    Cd, od, sd = SC.reference(A, r, ops, S, n_max, dtype=np.complex128)
    D = A.shape[-1]
    per_n = np.maximum(np.abs(Cd - Cl).max(axis=(0, 1, 2)), np.abs(sd - sl).max(axis=0)).astype(float)
    bnd = K.bound(D, np.arange(1, n_max + 1))
    return max(float((per_n / bnd).max()), float(np.abs(od - ol).max()) / K.bound(D, 1)), float(per_n.max())


@pytest.mark.parametrize('D', K.DS)
def test_float64_stays_within_a_third_of_the_bound(D):
    """The rule of `correlator_cases.bound`, on the cases of the string tests: every string on the Haar tensors at every (rows, n_max)
    block of the kernel comparison, and X on the symmetric tensors, where the string order does not decay."""
    worst = 0.0
    A = K.haar_tensors(D)
    r = K.fixed_points(A)
    for rows, n_max in K.reference_plan(D):
        for name, S in SC.strings().items():
            ratio, err = _ratio(A[:rows], r[:rows], K.generic_ops(), S, n_max)
            print(f'D={D} rows={rows} n_max={n_max} string {name}: float64 - long double {err:.2e}, largest err / bound {ratio:.3f}')
            worst = max(worst, ratio)
    As, rs = SC.symmetric_tensors(D), SC.symmetric_environments(D)
    ratio, err = _ratio(As, rs, np.stack([K.X, K.Z]), K.X, SC.SYMMETRIC_N[D])
    print(f'D={D} symmetric tensors ({len(As)} rows), (X, Z), string X, n_max={SC.SYMMETRIC_N[D]}: float64 - long double {err:.2e}, largest err / bound {ratio:.3f}')
    worst = max(worst, ratio)
    print(f'D={D}: largest float64 error / bound {worst:.3f}')
    assert worst <= 1.0 / 3.0


def test_symbol_is_declared_bound_and_refuses_without_a_device():
    from qmps_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'qmps_hip.h')).read()
    assert re.search(r'^int qmps_string_correlators\(qmps_ctx\* ctx, int64_t B, int n_ops, const double\* ops', header, flags=re.M)
    assert 'qmps_string_correlators' in header.split('int qmps_abi_minor(void);')[0].split('Added later without a bump')[1]
    assert re.search(r'#define QMPS_ABI_MINOR 7\b', header)
    plain = _lib.SIGNATURES['qmps_correlators']
    # qmps_correlators with the string before n_max and str_out at the end
    assert _lib.SIGNATURES['qmps_string_correlators'] == (plain[0], plain[1][:4] + [_lib._dp] + plain[1][4:] + [_lib._dp])
    lib = _lib.load()
    ops = np.ascontiguousarray(K.PAULIS).view(np.float64)
    S = np.ascontiguousarray(K.X).view(np.float64)
    out = np.zeros(2 * 16 * 3)
    dp = ctypes.POINTER(ctypes.c_double)
    f = lambda a: a.ctypes.data_as(dp)
    rc = lib.qmps_string_correlators(None, 1, 4, f(ops), f(S), 3, f(out), None, None)
    assert rc == _lib.QMPS_ERR_ARG and b'null context' in lib.qmps_last_error()
    assert not out.any()


def test_engine_refuses_a_misshapen_string_before_any_library_call():
    from qmps_amd import engine
    eng = object.__new__(engine.EnergyEngine)
    eng.B = 1
    with pytest.raises(ValueError):
        engine.EnergyEngine.correlators(eng, K.Z, 4, B=1, string=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        engine.EnergyEngine.correlators(eng, K.Z, 4, B=1, want_string=True)
