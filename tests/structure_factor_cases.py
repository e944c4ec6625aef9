"""Correlator sums of the resident states (qmps_correlator_sums): the long-double reference, the inputs of the tests that use it, the
float64 port of the kernels' elimination and the rounding bound (test infrastructure; tests/test_structure_factor_cases_cpu.py checks
all of it without a GPU).

Conventions are those of tests/correlator_cases.py.  For one evaluation, with tau = tr r:

    E_O(x) = sum_(t,s) O[t, s] A_s x A_t^+        T = E_1        L_a = sum_(t,s) O_a[t, s] A_t^+ A_s
    one[a]     = tr(E_(O_a)(r)) / tau
    site[a, c] = tr(E_(O_a O_c)(r)) / tau                       (O_a O_c the 2 x 2 matrix product)
    b_c        = E_(O_c)(r) - one[c] r
    Tt(x)      = T(x) - r tr(x) / tau                           (the deflated map)
    G[j, a, c] = z_j tr(L_a (1 - z_j Tt)^(-1)(b_c)) / tau       ( = sum_(n >= 1) z_j^n (C[a, c, n - 1] - one[a] one[c]) for |z| <= 1)
    S[q, a, c] = site[a, c] - one[a] one[c] + G_ac(e^(-i k_q)) + G_ca(e^(+i k_q))

Matrices are vectorised row-major: x[i, j] sits at i D + j, so T[(i, j), (k, l)] = sum_s A_s[i, k] conj(A_s[j, l]).
"""
import functools

import numpy as np
from scipy.linalg import expm

import correlator_cases as K
from oracle import qmps_oracle as O

LD = np.longdouble
CLD = np.clongdouble
EPS = 2.0 ** -52

DS = K.DS
Z = np.array([1, -1, 1j, np.exp(0.3j), np.exp(-0.3j), 0.5 + 0.25j], dtype=np.complex128)
Z.setflags(write=False)
N_Z = (1, 2, 6)                       # prefixes of Z
BATCHES = K.BATCHES                   # D <= 8: lane, 16-lane-group and workgroup tails
N_OPS = K.N_OPS
D16_BATCHES, D16_N_Z, D16_N_OPS = (1, 5), (1, 3), (1, 4)
FAMILY_T = (0.5, 0.1, 0.02)
GAPS = {2: (1.1e-1, 4.1e-3, 1.6e-4), 4: (2.8e-1, 3.4e-2, 1.5e-3), 8: (2.3e-1, 3.7e-2, 1.6e-3)}    # 1 - |lambda_2| of the first row per t
C_BOUND = 7.0


def family_rows(D):
    return 3 if D <= 8 else 1


def passthrough_tensor(D):
    """A0[0] = 1_D, A0[1] = 0: the transfer map is the identity."""
    A0 = np.zeros((2, D, D), dtype=np.complex128)
    A0[0] = np.eye(D)
    return A0


@functools.lru_cache(maxsize=None)
def family(D):
    """The small-gap family: U = U0 exp(-i t H) around the pass-through tensor, H = (X + X^H) / 2 with X complex standard normal from
    default_rng(40 + D) (one draw per row), t in FAMILY_T.  -> A (len(FAMILY_T) * rows, 2, D, D) ordered t-major, r = env_direct(A) in
    float64, t of every row."""
    rng = np.random.default_rng(40 + D)
    U0 = O.tensor_to_unitary(passthrough_tensor(D))
    Hs = []
    for _ in range(family_rows(D)):
        X = rng.standard_normal((2 * D, 2 * D)) + 1j * rng.standard_normal((2 * D, 2 * D))
        Hs.append((X + X.conj().T) / 2)
    A = np.stack([O.unitary_to_tensor(U0 @ expm(-1j * t * H)) for t in FAMILY_T for H in Hs])
    r = np.stack([O.env_direct(a)[0] for a in A])
    t = np.repeat(np.array(FAMILY_T), family_rows(D))
    for a in (A, r, t):
        a.setflags(write=False)
    return np.ascontiguousarray(A), np.ascontiguousarray(r), t


@functools.lru_cache(maxsize=None)
def haar_environments(D, rows):
    """Float64 environments of the first rows of correlator_cases.haar_tensors(D) by the oracle's direct solve - the CPU stand-in for
    what the device solves (correlator_cases.fixed_points stops after 400 power steps, 3.6e-8 short of the fixed point at the smallest
    gap of the D = 2 batch)."""
    r = np.stack([O.env_direct(a)[0] for a in K.haar_tensors(D)[:rows]])
    r.setflags(write=False)
    return r


def transfer_matrix(A, dtype=np.complex128):
    A = np.asarray(A, dtype=dtype)
    N = A.shape[-1] ** 2
    return np.einsum('sik,sjl->ijkl', A, A.conj()).reshape(N, N)


def gap(A):
    """1 - |lambda_2| of the transfer map."""
    w = np.sort(np.abs(np.linalg.eigvals(transfer_matrix(A))))
    return 1.0 - w[-2]


def deflated(A, r, dtype=np.complex128):
    """Matrix of Tt on row-major vectorised matrices."""
    A = np.asarray(A, dtype=dtype)
    r = np.asarray(r, dtype=dtype)
    D = A.shape[-1]
    return transfer_matrix(A, dtype) - np.outer(r.reshape(-1), np.eye(D, dtype=dtype).reshape(-1)) / np.trace(r)


def solve_gepp(M, R):
    """Gaussian elimination with partial (row) pivoting and back substitution in the dtype of M, batched over the leading axis:
    M (S, N, N), R (S, N, m) -> X (S, N, m).  numpy has no long-double solve."""
    S, N, _ = M.shape
    W = np.concatenate([M, R], axis=2).copy()
    rows = np.arange(S)
    for k in range(N):
        p = k + np.argmax(np.abs(W[:, k:, k]), axis=1)
        top, piv = W[rows, k].copy(), W[rows, p].copy()
        W[rows, p], W[rows, k] = top, piv
        f = W[:, k + 1:, k] / W[:, k, k][:, None]
        W[:, k + 1:, k + 1:] -= f[:, :, None] * W[:, k, None, k + 1:]
    X = np.empty_like(W[:, :, N:])
    for k in range(N - 1, -1, -1):
        X[:, k] = (W[:, k, N:] - np.einsum('sc,scm->sm', W[:, k, k + 1:N], X[:, k + 1:])) / W[:, k, k][:, None]
    return X


def _np_solve(M, R):
    return np.linalg.solve(M, R)


def reference(A, r, ops, z, dtype=CLD, solve=None):
    """The definition of the module docstring, evaluated as written in `dtype` (np.clongdouble with the hand-written elimination: the
    reference; np.complex128 with np.linalg.solve: what float64 numpy gives for it).  A (B, 2, D, D), r (B, D, D), ops (m, 2, 2),
    z (n_z,) -> G (B, n_z, m, m), one (B, m), site (B, m, m)."""
    if solve is None:
        solve = solve_gepp if dtype == CLD else _np_solve
    A = np.asarray(A, dtype=dtype)
    r = np.asarray(r, dtype=dtype)
    ops = np.asarray(ops, dtype=dtype).reshape(-1, 2, 2)
    z = np.asarray(z, dtype=dtype).reshape(-1)
    B, D, m, nz = A.shape[0], A.shape[-1], ops.shape[0], z.shape[0]
    N = D * D
    G = np.empty((B, nz, m, m), dtype=dtype)
    one = np.empty((B, m), dtype=dtype)
    site = np.empty((B, m, m), dtype=dtype)
    prod = np.einsum('atu,cus->acts', ops, ops)
    eye = np.eye(N, dtype=dtype)
    for b in range(B):
        Ab, rb = A[b], r[b]
        tau = np.trace(rb)
        R = np.einsum('sik,kl,tjl->tsij', Ab, rb, Ab.conj())                 # A_s r A_t^+
        W = np.einsum('tsii->ts', R)
        one[b] = np.einsum('ats,ts->a', ops, W) / tau
        site[b] = np.einsum('acts,ts->ac', prod, W) / tau
        rhs = np.einsum('cts,tsij->cij', ops, R) - one[b][:, None, None] * rb  # b_c
        L = np.einsum('ats,tki,skj->aij', ops, Ab.conj(), Ab)
        Tt = deflated(Ab, rb, dtype)
        M = eye[None] - z[:, None, None] * Tt[None]
        Rm = np.broadcast_to(rhs.reshape(m, N).T[None], (nz, N, m))
        X = solve(M, np.ascontiguousarray(Rm))                               # (n_z, N, m)
        G[b] = z[:, None, None] * np.einsum('aji,zijc->zac', L, X.reshape(nz, D, D, m)) / tau   # tr(L_a X_c)
    return G, one, site


def port(A, r, ops, z):
    """Float64 port of what the kernels do for G: the matrix 1 - z Tt built entry by entry from A, r and 1 / tr r, Gauss-Jordan
    elimination with partial pivoting (the row of largest |re| + |im| in the column among the rows not yet used, the lowest such row
    at a tie; rows stay where they are), the pivot row scaled by the reciprocal of the pivot, every other row eliminated, read-out
    z / tau sum_rows L_a[column the row was pivot of] rhs[row, c].  Shapes as `reference`; returns G."""
    A = np.asarray(A, dtype=np.complex128)
    r = np.asarray(r, dtype=np.complex128)
    ops = np.asarray(ops, dtype=np.complex128).reshape(-1, 2, 2)
    z = np.asarray(z, dtype=np.complex128).reshape(-1)
    B, D, m, nz = A.shape[0], A.shape[-1], ops.shape[0], z.shape[0]
    N = D * D
    G = np.empty((B, nz, m, m), dtype=np.complex128)
    for b in range(B):
        Ab, rb = A[b], r[b]
        inv = 1.0 / np.trace(rb)
        R = np.einsum('sik,kl,tjl->tsij', Ab, rb, Ab.conj())
        W = np.einsum('tsii->ts', R)
        one = np.einsum('ats,ts->a', ops, W) * inv
        rhs = (np.einsum('cts,tsij->cij', ops, R) - one[:, None, None] * rb).reshape(m, N).T
        Lv = np.einsum('ats,tki,skj->aji', ops, Ab.conj(), Ab).reshape(m, N)  # Lv[a, (i, j)] = L_a[j, i]
        T = np.einsum('sik,sjl->ijkl', Ab, Ab.conj()) - (rb * inv)[:, :, None, None] * np.eye(D)[None, None]
        for j in range(nz):
            Wm = np.concatenate([np.eye(N) - z[j] * T.reshape(N, N), rhs], axis=1)
            free = np.ones(N, dtype=bool)
            col_of = np.zeros(N, dtype=int)
            for k in range(N):
                v = np.where(free, np.abs(Wm[:, k].real) + np.abs(Wm[:, k].imag), -1.0)
                p = int(np.argmax(v))
                free[p] = False
                col_of[p] = k
                with np.errstate(all='ignore'):
                    Wm[p, k + 1:] *= 1.0 / Wm[p, k]
                    f = Wm[:, k].copy()
                    f[p] = 0.0
                    Wm[:, k + 1:] -= f[:, None] * Wm[p, None, k + 1:]
            G[b, j] = z[j] * inv * np.einsum('an,nc->ac', Lv[:, col_of], Wm[:, N:])
    return G


def kappa(A, r, z):
    """||(1 - z_j Tt)^(-1)||_2 in float64 numpy: (B, n_z)."""
    z = np.asarray(z, dtype=np.complex128).reshape(-1)
    out = np.empty((len(A), len(z)))
    for b in range(len(A)):
        Tt = deflated(A[b], r[b])
        for j, zz in enumerate(z):
            with np.errstate(all='ignore'):
                try:
                    out[b, j] = np.linalg.norm(np.linalg.inv(np.eye(Tt.shape[0]) - zz * Tt), 2)
                except np.linalg.LinAlgError:
                    out[b, j] = np.inf
    return out


def bound(A, r, z):
    """Largest |G - reference| (elementwise, operators of unit spectral norm) granted to a float64 evaluation: (B, n_z),
    C_BOUND 2^-52 ||(1 - z_j Tt)^(-1)||_2.

    The error of a backward-stable solve of (1 - z Tt) X = b is eps kappa |X| with the condition number ||M|| ||M^-1||; here
    ||M|| <= 1 + ||Tt|| is of order one, |b| <= 2 and the read-out with ||L_a|| <= 1 keeps the size, so the resolvent norm alone
    carries the scale and nothing grows with N.  The rule (that of correlator_cases.bound): float64 numpy - np.linalg.solve on the
    same matrix and right-hand sides - stays within a third on every case of the module, C_BOUND being three times its worst
    err / (2^-52 kappa) rounded up to one digit.  Measured (tests/test_structure_factor_cases_cpu.py prints them; all 130 Haar rows at
    D <= 8, 5 at D = 16, with r = env_direct(A); every family row; all six points; the four generic operators), Haar / family:
    D = 2: 2.14 / 0.90, D = 4: 0.38 / 0.77, D = 8: 0.25 / 0.52, D = 16: 0.11 / 0.88.  Worst 2.14, times three 6.4: C_BOUND = 7.
    The worst case is the D = 2 Haar row 120 at z = 1 where |G| = 18.5 at kappa = 36.5: the error follows eps kappa |X| and the sum
    itself is large there; wherever |G| <= 1 the ratio stays below 1 and there is no growth with N.  The float64 port of the
    kernels' Gauss-Jordan elimination: 3.57 / 0.89, 1.21 / 0.77, 0.26 / 0.52, 0.14 / 0.88, i.e. at most 0.51 of the bound.  On the
    family both agree to 1 %: what they share, the rounding of the matrix entries, carries the error, not the elimination.
    `one` and `site` are held to correlator_cases.bound(D, 1)."""
    return C_BOUND * EPS * kappa(A, r, z)


def structure_factor(G, one, site):
    """Host composition: G (B, 2 n_k, m, m) at z = (e^(-i k_0), e^(+i k_0), e^(-i k_1), ...) -> S (B, n_k, m, m)."""
    conn = site - one[:, :, None] * one[:, None, :]
    return conn[:, None] + G[:, 0::2] + np.swapaxes(G[:, 1::2], -1, -2)


def k_to_z(k):
    k = np.asarray(k, dtype=np.float64).reshape(-1)
    z = np.empty(2 * len(k), dtype=np.complex128)
    z[0::2] = np.exp(-1j * k)
    z[1::2] = np.exp(1j * k)
    return z


def power_fixed_point(A, steps):
    """Unrounded long-double fixed point by long-double power iteration (tr r = 1)."""
    A = np.asarray(A, dtype=CLD)
    D = A.shape[-1]
    r = np.eye(D, dtype=CLD) / D
    for _ in range(steps):
        r = np.einsum('sik,kl,sjl->ij', A, r, A.conj())
        r = (r + r.conj().T) / 2
        r = r / np.trace(r).real
    return r


def series(A, r, ops, z, n_terms):
    """sum_(n = 1 .. n_terms) z^n (C[a, c, n - 1] - one[a] one[c]) in long double from correlator_cases.reference: (n_z, m, m)."""
    C, one = K.reference(A, r, ops, n_terms)
    conn = C - (one[:, None] * one[None, :])[..., None]
    z = np.asarray(z, dtype=CLD).reshape(-1)
    pw = z[:, None] ** np.arange(1, n_terms + 1, dtype=LD)[None]
    return np.einsum('zn,acn->zac', pw, conn)
