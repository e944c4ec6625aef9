"""Two-point functions of the resident states (qmps_correlators): the long-double reference, the inputs of the tests that use it
and the rounding bound they hold the kernels to (test infrastructure; tests/test_correlator_cases_cpu.py checks all of it without a GPU).

Conventions (oracle/qmps_oracle.py): A[s, i, j] a left isometry, r the right fixed point of x -> sum_s A_s x A_s^+, site 0 the left
site, an operator O[t, s] = <t|O|s> (the index order of h in two_site_rdm):

    E_O(x) = sum_(t,s) O[t, s] A_s x A_t^+          T = E_1
    C[a, c, n - 1] = tr(E_(O_a)(T^(n-1)(E_(O_c)(r)))) / tr r = <O_a(site 0) O_c(site n)>,   n = 1 .. n_max
    one[a]         = tr(E_(O_a)(r)) / tr r                   = <O_a>
"""
import functools

import numpy as np

from oracle import qmps_oracle as O

LD = np.longdouble
CLD = np.clongdouble

DS = (2, 4, 8, 16)
BATCHES = (1, 17, 65, 130)            # lane, quad and workgroup tails: prefixes of the one Haar batch per D
N_OPS = (1, 2, 3, 4)                  # prefixes of `generic_ops()`
N_SHORT = (1, 2, 7)                   # chain lengths every batch size is taken at ...
N_LONG = 64                           # ... the long chain: B = 1 and 17
N_VERY_LONG = 512                     # D = 2, 4 at B = 17 only
B_LONG = 17
HAAR_B = max(BATCHES)
HAAR_SEED = {2: 5102, 4: 5104, 8: 5108, 16: 5116}
ANSATZ_KIND = 0                       # ShallowCNOT
ANSATZ_PARAMS = {2: 4, 4: 4}
ANSATZ_ROWS = 21

I2 = np.eye(2, dtype=np.complex128)
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)
PAULIS = np.stack([I2, X, Y, Z])
SIGMA_PLUS = np.array([[0, 1], [0, 0]], dtype=np.complex128)       # |0><1|: O[t, s] = <t|O|s>


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def generic_ops():
    """Four complex one-site operators of unit spectral norm, neither Hermitian nor normal: seeded complex Gaussians."""
    rng = np.random.default_rng(5001)
    G = rng.standard_normal((4, 2, 2)) + 1j * rng.standard_normal((4, 2, 2))
    return _frozen(np.ascontiguousarray(G / np.linalg.norm(G, 2, axis=(1, 2))[:, None, None]))


@functools.lru_cache(maxsize=None)
def haar_tensors(D):
    """The Haar batch of bond dimension D, (HAAR_B, 2, D, D) complex128."""
    rng = np.random.default_rng(HAAR_SEED[D])
    return _frozen(np.ascontiguousarray(O.unitary_to_tensor(O.haar_unitaries(rng, 2 * D, HAAR_B))))


@functools.lru_cache(maxsize=None)
def ansatz_params(D):
    return _frozen(np.random.default_rng(5200 + D).standard_normal((ANSATZ_ROWS, ANSATZ_PARAMS[D])))


@functools.lru_cache(maxsize=None)
def ansatz_tensors(D):
    """ShallowCNOT tensors of `ansatz_params(D)` as the oracle builds them."""
    return _frozen(np.ascontiguousarray(np.stack([O.unitary_to_tensor(O.shallow_cnot_unitary(D, p)) for p in ansatz_params(D)])))


def kernel_cases(D):
    """(B, n_ops, n_max) of the kernel-alone comparison at bond dimension D: every batch size with every number of operators at the
    short chains, the long chain at B = 1 and 17, the very long one at D = 2, 4."""
    out = [(B, m, n) for B in BATCHES for m in N_OPS for n in N_SHORT]
    out += [(B, m, N_LONG) for B in (1, B_LONG) for m in N_OPS]
    if D <= 4:
        out.append((B_LONG, 4, N_VERY_LONG))
    return out


def reference_plan(D):
    """(rows, n_max) blocks that cover `kernel_cases(D)` with the least long-double work: all rows at the short chains, the first
    B_LONG rows at the long ones."""
    return ((HAAR_B, max(N_SHORT)), (B_LONG, N_VERY_LONG if D <= 4 else N_LONG))


def fixed_points(A, steps=400):
    """Right environments of a batch by plain power iteration in float64 (Hermitian, tr r = 1) - inputs of the rounding measurement,
    which needs the same r on both sides and no more; the GPU tests use the environments the device solved."""
    A = np.asarray(A)
    D = A.shape[-1]
    r = np.broadcast_to(np.eye(D, dtype=np.complex128) / D, (A.shape[0], D, D)).copy()
    Ah = A.conj().swapaxes(-1, -2)
    for _ in range(steps):
        r = np.matmul(np.matmul(A, r[:, None]), Ah).sum(axis=1)
        r = (r + r.conj().transpose(0, 2, 1)) / 2
        r /= np.trace(r, axis1=1, axis2=2).real[:, None, None]
    return r


def reference(A, r, ops, n_max, dtype=CLD):
    """The formula of the module docstring, evaluated as written in `dtype` (np.clongdouble: the reference; np.complex128: what
    float64 numpy gives for it).  A (B, 2, D, D) or (2, D, D), r (B, D, D) or (D, D), ops (m, 2, 2) or (2, 2)
    -> C (B, m, m, n_max), one (B, m) (without the batch axis for a single tensor)."""
    single = np.ndim(A) == 3
    A = np.asarray(A, dtype=dtype).reshape((-1,) + np.shape(A)[-3:])
    r = np.asarray(r, dtype=dtype).reshape((-1,) + np.shape(r)[-2:])
    ops = np.asarray(ops, dtype=dtype).reshape(-1, 2, 2)
    B, m = A.shape[0], ops.shape[0]
    Al = A[:, None]                                          # (B, 1, 2, D, D)
    Ah = A.conj().swapaxes(-1, -2)[:, None]                  # A_t^+
    Ac = A.conj()

    def left(x):                                             # Y[b, c, s] = A_s x[b, c]
        return np.matmul(Al, x[:, :, None])

    def traces(Yx):                                          # tr(E_(O_a)(x)) = sum_(t,s) O_a[t, s] tr(A_s x A_t^+)
        G = np.einsum('bcsik,btik->bcts', Yx, Ac)
        return np.einsum('ats,bcts->bac', ops, G)

    tr_r = np.trace(r, axis1=1, axis2=2)
    one = traces(left(r[:, None]))[:, :, 0] / tr_r[:, None]
    # x[b, c] = E_(O_c)(r)
    Yr = left(r[:, None])                                    # (B, 1, 2, D, D)
    Zt = np.einsum('cts,bsij->bctij', ops, Yr[:, 0])
    x = np.matmul(Zt, Ah).sum(axis=2)
    C = np.empty((B, m, m, n_max), dtype=dtype)
    for n in range(n_max):
        Yx = left(x)
        C[..., n] = traces(Yx) / tr_r[:, None, None]
        if n + 1 < n_max:
            x = np.matmul(Yx, Ah).sum(axis=2)
    return (C[0], one[0]) if single else (C, one)


def site_operator(D, n_sites, placed):
    """kron(1_D, o_0, ..., o_(n_sites-1), 1_D) with o_k = placed.get(k, 1): an operator on the physical sites of
    oracle.state_vector(U, V, n_sites), which sit on qubits log2 D .. log2 D + n_sites - 1 (the layout of kron(eye(D), h, eye(D)) in
    energy_statevector), not on qubits 0 .. n_sites - 1."""
    M = np.eye(D, dtype=np.complex128)
    for k in range(n_sites):
        M = np.kron(M, placed.get(k, I2))
    return np.kron(M, np.eye(D))


def statevector_correlators(U, ops, n_max):
    """C (m, m, n_max) and one (m,) from the oracle's state vectors with its own get_env_exact - no transfer map anywhere."""
    D = U.shape[0] // 2
    V = O.get_env_exact(U)
    ops = np.asarray(ops, dtype=np.complex128).reshape(-1, 2, 2)
    m = ops.shape[0]
    C = np.empty((m, m, n_max), dtype=np.complex128)
    for n in range(1, n_max + 1):
        psi = O.state_vector(U, V, n + 1)
        for a in range(m):
            for c in range(m):
                C[a, c, n - 1] = psi.conj() @ (site_operator(D, n + 1, {0: ops[a], n: ops[c]}) @ psi)
    psi = O.state_vector(U, V, 2)
    one = np.array([psi.conj() @ (site_operator(D, 2, {0: o}) @ psi) for o in ops])
    return C, one


def rdm_correlators(rho, ops):
    """C[a, c] at n = 1 and one[a] from a two-site density matrix rho[tau, sigma] (index 2 s1 + s2, s1 the left site)."""
    ops = np.asarray(ops, dtype=np.complex128).reshape(-1, 2, 2)
    C1 = np.einsum('aik,cjl,...klij->...ac', ops, ops, np.asarray(rho).reshape(np.shape(rho)[:-2] + (2, 2, 2, 2)))
    one = np.einsum('aik,...kjij->...a', ops, np.asarray(rho).reshape(np.shape(rho)[:-2] + (2, 2, 2, 2)))
    return C1, one


def bound(D, n):
    """Largest |C - reference| (elementwise, operators of unit spectral norm) granted to a float64 evaluation of a chain of n steps.

    Linear in n: the component of x along the fixed point does not decay, so every application of T adds its rounding - a few
    units of eps = 1.1e-16 relative to |x| <= 1 - to all later values.  Constants: 4e-15 + 5e-16 n (36 eps at the start, which
    covers the products of E_(O_c), the read-out and the division by tr r, plus 4.5 eps per step) for every D; the rounding does
    not grow with D because the D-term sums average it.  The rule (that of ansatz_cases.bound): float64 numpy on the very cases of
    this module stays within a third.  Measured worst cases behind the constants (tests/test_correlator_cases_cpu.py prints them;
    the Paulis, whose identity keeps the whole fixed-point component, are worse than the generic operators):
    D = 2: 9.1e-16 at n <= 7, 6.4e-15 at n <= 64, 6.5e-14 at n <= 512 (bound 2.6e-13, ratio 0.25: the margin to a third is for
    another BLAS); D = 4: 5.9e-16, 2.6e-15, 8.9e-15; D = 8: 6.7e-16, 1.5e-15; D = 16: 8.8e-16 at n <= 7 (bound 7.5e-15, ratio 0.15),
    2.1e-15 at n <= 64."""
    return 4e-15 + 5e-16 * n
