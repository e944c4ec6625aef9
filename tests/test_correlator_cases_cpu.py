"""CPU: tests/correlator_cases.py checked without a GPU - the long-double reference of the two-point functions against the oracle's
state vectors and its two-site density matrix, the rounding bound against float64 numpy on the very cases the GPU tests use, and the
C-ABI's argument checks that need no device."""
import ctypes

import numpy as np
import pytest

import correlator_cases as K
from oracle import qmps_oracle as O


@pytest.mark.parametrize('D', (2, 4))
def test_reference_equals_the_state_vector_route(D):
    """<psi| O_a(site 0) O_c(site n) |psi> of oracle.state_vector(U, get_env_exact(U), n + 1), n = 1 .. 5, non-Hermitian operators; the
    physical sites are qubits log2 D .. log2 D + n of that register (correlator_cases.site_operator)."""
    U = O.haar_unitaries(np.random.default_rng(5300 + D), 2 * D, 1)[0]
    A = O.unitary_to_tensor(U)
    _, r = O.env_dense_eig(A)
    ops = np.concatenate([K.generic_ops()[:2], K.SIGMA_PLUS[None]])
    C, one = K.reference(A, r, ops, 5)
    Cs, ones = K.statevector_correlators(U, ops, 5)
    err = max(float(np.abs(C - Cs).max()), float(np.abs(one - ones).max()))
    print(f'D={D}: reference vs state vectors {err:.2e}')
    assert err < 1e-12
    # an operator on qubits 0 .. n instead would be a different number: the check can tell the layouts apart
    psi = O.state_vector(U, O.get_env_exact(U), 2)
    wrong = psi.conj() @ (np.kron(np.kron(np.kron(ops[0], ops[1]), np.eye(D)), np.eye(D)) @ psi)
    assert abs(wrong - C[0, 1, 0]) > 1e-3


@pytest.mark.parametrize('D', K.DS)
def test_first_step_equals_the_two_site_density_matrix(D):
    """C[a, c, 0] = sum (O_a x O_c)[sigma, tau] rho[tau, sigma] and one[a] = its partial trace, rho = oracle.two_site_rdm."""
    A = K.haar_tensors(D)[:6]
    r = K.fixed_points(A)
    ops = K.generic_ops()
    C, one = K.reference(A, r, ops, 2)
    rho = np.stack([O.two_site_rdm(a, x) for a, x in zip(A, r)])
    C1, o1 = K.rdm_correlators(rho, ops)
    assert np.abs(C[..., 0] - C1).max() < 1e-13 and np.abs(one - o1).max() < 1e-13
    # transposed operators are a different number (non-Hermitian, non-symmetric operators)
    assert np.abs(K.rdm_correlators(rho, ops.transpose(0, 2, 1))[0] - C1).max() > 1e-3


def _ratio(A, r, ops, n_max):
    Cl, ol = K.reference(A, r, ops, n_max)
    Cd, od = K.reference(A, r, ops, n_max, dtype=np.complex128)
    D = A.shape[-1]
    per_n = np.abs(Cd - Cl).max(axis=(0, 1, 2)).astype(float)
    bnd = K.bound(D, np.arange(1, n_max + 1))
    return max(float((per_n / bnd).max()), float(np.abs(od - ol).max()) / K.bound(D, 1)), float(per_n.max())


@pytest.mark.parametrize('D', K.DS)
def test_float64_stays_within_a_third_of_the_bound(D):
    """The rule `correlator_cases.bound` states for itself, on the very cases of the module: Haar tensors at every (rows, n_max) block of
    the kernel comparison with the generic operators and with (1, X, Y, Z), and the ansatz-built tensors with sigma^+."""
    worst = 0.0
    A = K.haar_tensors(D)
    r = K.fixed_points(A)
    for rows, n_max in K.reference_plan(D):
        for name, ops in (('generic', K.generic_ops()), ('paulis', K.PAULIS)):
            ratio, err = _ratio(A[:rows], r[:rows], ops, n_max)
            print(f'D={D} rows={rows} n_max={n_max} {name}: float64 - long double {err:.2e}, largest err / bound {ratio:.3f}')
            worst = max(worst, ratio)
    if D in K.ANSATZ_PARAMS:
        At = K.ansatz_tensors(D)
        ratio, err = _ratio(At, K.fixed_points(At), np.stack([K.SIGMA_PLUS, K.Z, K.X]), K.N_LONG)
        print(f'D={D} ansatz tensors, (sigma+, Z, X), n_max={K.N_LONG}: float64 - long double {err:.2e}, largest err / bound {ratio:.3f}')
        worst = max(worst, ratio)
    print(f'D={D}: largest float64 error / bound {worst:.3f}')
    assert worst <= 1.0 / 3.0


def test_conventions_of_the_reference():
    """With (1, X, Y, Z): C[0, c, n] = one[c], C[a, 0, n] = one[a], C[0, 0, n] = 1 - an isometry and its fixed point."""
    A = K.haar_tensors(4)[:5]
    C, one = K.reference(A, K.fixed_points(A), K.PAULIS, 9)
    assert np.abs(C[:, 0, :, :] - one[:, :, None]).max() < 1e-13
    assert np.abs(C[:, :, 0, :] - one[:, :, None]).max() < 1e-13
    assert np.abs(C[:, 0, 0, :] - 1).max() < 1e-13


def test_null_context_is_refused_without_a_device():
    from qmps_amd import _lib
    assert 'qmps_correlators' in _lib.SIGNATURES
    lib = _lib.load()
    ops = np.ascontiguousarray(K.PAULIS).view(np.float64)
    out = np.zeros(2 * 16 * 3)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.qmps_correlators(None, 1, 4, ops.ctypes.data_as(dp), 3, out.ctypes.data_as(dp), None)
    assert rc == _lib.QMPS_ERR_ARG and b'null context' in lib.qmps_last_error()
    assert not out.any()
