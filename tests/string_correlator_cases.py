"""String order of the resident states (qmps_string_correlators): the long-double reference, the state-vector route, the strings and
the symmetric tensors of the tests that use them (test infrastructure; tests/test_string_correlator_cases_cpu.py checks all of it
without a GPU).  Shapes, operators, Haar tensors and the rounding bound are those of tests/correlator_cases.py.

Conventions as there (A[s, i, j] a left isometry, r its right fixed point, O[t, s] = <t|O|s>, site 0 the left site), S the string:

    E_O(x) = sum_(t,s) O[t, s] A_s x A_t^+      L_a = sum_(t,s) O_a[t, s] A_t^+ A_s      tau = tr r
    C[a, c, n - 1] = tr(L_a E_S^(n-1)(E_(O_c)(r))) / tau = <O_a(0) S(1) .. S(n-1) O_c(n)>,   n = 1 .. n_max
    str[n - 1]     = tr(E_S^n(r)) / tau                  = <S(1) .. S(n)>,                   n = 1 .. n_max
    one[a]         = tr(L_a r) / tau                     = <O_a>
"""
import functools

import numpy as np

import correlator_cases as K
from oracle import qmps_oracle as O

CLD = K.CLD
SYMMETRIC_SEED = {2: 5702, 4: 5704, 8: 5708, 16: 5716}
SYMMETRIC_B = {2: 17, 4: 17, 8: 17, 16: 6}
SYMMETRIC_N = {2: K.N_VERY_LONG, 4: K.N_VERY_LONG, 8: K.N_LONG, 16: K.N_LONG}
FIXED_POINT_STEPS = 2000


def strings():
    """name -> string: X (the disorder operator of the Ising chain), a non-normal complex matrix of unit norm, the identity."""
    return {'X': K.X, 'generic': K.generic_ops()[3], 'identity': K.I2}


def reference(A, r, ops, string, n_max, dtype=CLD):
    """The three formulas of the module docstring, evaluated as written in `dtype` (np.clongdouble: the reference; np.complex128:
    what float64 numpy gives for them).  A (B, 2, D, D) or (2, D, D), r (B, D, D) or (D, D), ops (m, 2, 2) or (2, 2), string (2, 2)
    -> C (B, m, m, n_max), one (B, m), str (B, n_max) (without the batch axis for a single tensor)."""
    single = np.ndim(A) == 3
    A = np.asarray(A, dtype=dtype).reshape((-1,) + np.shape(A)[-3:])
    r = np.asarray(r, dtype=dtype).reshape((-1,) + np.shape(r)[-2:])
    ops = np.asarray(ops, dtype=dtype).reshape(-1, 2, 2)
    S = np.asarray(string, dtype=dtype).reshape(2, 2)
    B, m = A.shape[0], ops.shape[0]
    Ah = A.conj().swapaxes(-1, -2)                           # A_t^+

    def E(W, x):                                             # E_W(x[b, c]) for W (2, 2) or one W per c (c, 2, 2)
        Y = np.matmul(A[:, None], x[:, :, None])             # (B, c, s, D, D): A_s x
        Z = np.einsum('ts,bcsij->bctij' if W.ndim == 2 else 'cts,bcsij->bctij', W, Y)      # z_t = sum_s W[t, s] A_s x
        return np.matmul(Z, Ah[:, None]).sum(axis=2)

    M = np.matmul(Ah[:, :, None], A[:, None])                # (B, t, s, D, D): A_t^+ A_s
    L = np.einsum('ats,btsij->baij', ops, M)
    tau = np.trace(r, axis1=1, axis2=2)

    def left_traces(x):                                      # tr(L_a x[b, c]) -> (B, a, c)
        return np.einsum('baij,bcji->bac', L, x)

    one = left_traces(r[:, None])[:, :, 0] / tau[:, None]
    C = np.empty((B, m, m, n_max), dtype=dtype)
    st = np.empty((B, n_max), dtype=dtype)
    x = E(ops, np.broadcast_to(r[:, None], (B, m) + r.shape[1:]))
    y = r[:, None]
    for n in range(n_max):
        C[..., n] = left_traces(x) / tau[:, None, None]
        y = E(S, y)
        st[:, n] = np.trace(y[:, 0], axis1=1, axis2=2) / tau
        if n + 1 < n_max:
            x = E(S, x)
    return (C[0], one[0], st[0]) if single else (C, one, st)


def statevector_string_correlators(U, ops, string, n_max):
    """C (m, m, n_max), one (m,) and str (n_max,) from the oracle's state vectors with its own get_env_exact, the string placed on
    every inner site - no transfer map anywhere."""
    D = U.shape[0] // 2
    V = O.get_env_exact(U)
    ops = np.asarray(ops, dtype=np.complex128).reshape(-1, 2, 2)
    S = np.asarray(string, dtype=np.complex128).reshape(2, 2)
    m = ops.shape[0]
    C = np.empty((m, m, n_max), dtype=np.complex128)
    st = np.empty(n_max, dtype=np.complex128)
    for n in range(1, n_max + 1):
        psi = O.state_vector(U, V, n + 1)
        inner = {k: S for k in range(1, n)}
        for a in range(m):
            for c in range(m):
                C[a, c, n - 1] = psi.conj() @ (K.site_operator(D, n + 1, {**inner, 0: ops[a], n: ops[c]}) @ psi)
        st[n - 1] = psi.conj() @ (K.site_operator(D, n + 1, {k: S for k in range(1, n + 1)}) @ psi)
    psi = O.state_vector(U, V, 2)
    one = np.array([psi.conj() @ (K.site_operator(D, 2, {0: o}) @ psi) for o in ops])
    return C, one, st


def parity(D):
    """u = diag(+1, -1, +1, ...): the bond representation of the spin flip on `symmetric_tensors`."""
    return np.diag((-1.0) ** np.arange(D)).astype(np.complex128)


@functools.lru_cache(maxsize=None)
def symmetric_tensors(D, B=None):
    """(B, 2, D, D) left isometries with sum_s X[t, s] A_s = u A_t u^+: Haar tensors averaged with the spin flip,
    A_t <- (A_t + sum_s X[t, s] u^+ A_s u) / 2, then the polar factor of the (2 D, D) matrix (which keeps the symmetry).  On them E_X
    has an eigenvalue of modulus 1 (left eigenvector u), and <X_1 .. X_n> tends to |tr(u r)|^2 instead of decaying: the chain on which
    rounding accumulates under a string."""
    B = SYMMETRIC_B[D] if B is None else B
    A = O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(SYMMETRIC_SEED[D]), 2 * D, B))
    u = parity(D)
    A = (A + np.einsum('ts,ij,bsjk,kl->btil', K.X, u.conj().T, A, u)) / 2
    W, _, Vh = np.linalg.svd(A.reshape(B, 2 * D, D), full_matrices=False)
    out = np.ascontiguousarray(np.matmul(W, Vh).reshape(B, 2, D, D))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def symmetric_environments(D):
    """Right environments of `symmetric_tensors(D)` by plain power iteration (correlator_cases.fixed_points, 2000 steps): what the
    GPU test hands to set_env_guess, so that no solver takes part."""
    r = K.fixed_points(symmetric_tensors(D), FIXED_POINT_STEPS)
    r.setflags(write=False)
    return r
