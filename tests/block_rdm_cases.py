"""Reduced density matrices of blocks of n = 1 .. 4 sites (qmps_block_entanglement): the long-double reference, the inputs of the tests
that use it, two float64 evaluations of the formula in different orders and the bounds the results are held to (test infrastructure;
tests/test_block_rdm_cases_cpu.py checks all of it without a GPU).

Conventions (include/qmps_hip.h): for a tensor A (2, D, D) and a right environment r (D, D)

    B_t       = A_t1 A_t2 .. A_tn,  t = sum_k t_k 2^(n-k)        (t1 the left site, most significant: repeated oracle `merge`)
    rho[t, s] = tr(B_t r B_s^+) / tr r                            (the complex trace of r, as the kernels divide)
    p, S      = entanglement_cases.reference_spectrum(rho)       (herm(rho) / tr rho, descending; S = - sum_(p > 0) p ln p)

Bounds.  |rho - rho_ref|_max <= RHO_C (n + 1) D 2^-52 max(1, |rho_ref|_max): n products of length D and one contraction with r, each
a sum of D terms per element, then the Gram sum, whose D^2 terms are products of entries of size 1 / D on average.  RHO_C = 1 was set
on the CPU, the way EIG_C of entanglement_cases was: the formula is evaluated in float64 in two different orders - the products
first and then the Gram matrix (`gram_order`), and the site-by-site recursion X -> A_t X A_s^+ from the right end of the block
(`recursion_order`) - and both stay within a third of the bound on every finite case of this module, against the long-double reference.
Measured worst ratios to the bound (tests/test_block_rdm_cases_cpu.py prints them), D = 2 / 4 / 8 / 16, over n = 1 .. 4:
gram_order 0.18 / 0.07 / 0.08 / 0.05, recursion_order 0.18 / 0.06 / 0.05 / 0.02 (RHO_C = 1 is the smallest whole number that keeps a
third; the margin to it is for another BLAS, as with EIG_C).
p is held to eig_bound(2^n) + 2^n (the rho bound) - Weyl: an eigenvalue moves by at most the 2-norm of the perturbation, at most 2^n
times its largest element - and S to the form of entanglement_cases.entropy_bound with that delta.  On the cases of this module the
float64 port of the Jacobi kernels (`entanglement_cases.kernel_port`), fed the float64 rho, stays within 0.054 of the p bound and
0.004 of the S bound and needs at most 1 / 5 / 8 / 10 sweeps at the orders 2 / 4 / 8 / 16 (caps 1 / 10 / 24 / 30), the rank-deficient
blocks included (D = 2, n = 3, 4: rank 4 in order 8 and 16; the product state: rank 1).
"""
import functools

import numpy as np

import entanglement_cases as EC
from oracle import qmps_oracle as O

LD = np.longdouble
CLD = np.clongdouble
EPS = 2.0 ** -52

DS = (2, 4, 8, 16)
NS = (1, 2, 3, 4)
# tails of every partition (16 / 4 / 1 / 1 evaluations per workgroup at D = 2 / 4 / 8 / 16): a last workgroup of 1 (17, 65), 2 (130) and,
# with 31, one that is nearly full: 15 of 16 at D = 2, 3 of 4 at D = 4
BATCHES = (1, 17, 31, 65, 130)
RHO_C = 1.0
HAAR = 5                              # Haar isometries with dense-eig environments per bond dimension
GENERIC = 3                           # tensors that are no isometries, with an r that is not Hermitian
SEED = {2: 7102, 4: 7104, 8: 7108, 16: 7116}


def rho_bound(D, n, scale=1.0):
    """Largest |rho - rho_ref|_max granted to a float64 evaluation; scale = |rho_ref|_max of the evaluation."""
    return RHO_C * (n + 1) * D * EPS * np.maximum(1.0, scale)


def p_bound(D, n, scale=1.0):
    return EC.eig_bound(2 ** n) + 2 ** n * rho_bound(D, n, scale)


def entropy_bound(D, n, scale=1.0):
    """entanglement_cases.entropy_bound with delta = p_bound: T delta (1 + |ln delta|) for the T = 2^n terms, T 2^-52 ln T for the sum."""
    T = 2 ** n
    d = p_bound(D, n, scale)
    return T * d * (1.0 + np.abs(np.log(d))) + T * EPS * np.log(T)


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases(D):
    """Tuple of (name, A (2, D, D), r (D, D), kind), kind in ('isometry', 'product', 'generic', 'nan').  'isometry' and 'product':
    sum_s A_s^+ A_s = 1 and r is a fixed point of the transfer map.  The two NaN cases sit apart, between finite ones; the first case
    is finite."""
    rng = np.random.default_rng(SEED[D])
    out = []
    for k, a in enumerate(O.unitary_to_tensor(O.haar_unitaries(rng, 2 * D, HAAR))):
        a = np.ascontiguousarray(a)
        out.append((f'Haar isometry {k}', a, np.asarray(O.env_dense_eig(a)[1], dtype=np.complex128), 'isometry'))
    for k in range(GENERIC):
        # entries of variance 1 / (2 D): sum_s A_s^+ A_s = 1 on average and no more; r = 1 / D plus a complex matrix of the same size
        a = (rng.standard_normal((2, D, D)) + 1j * rng.standard_normal((2, D, D))) / np.sqrt(4 * D)
        r = np.eye(D) / D + 0.3 * (rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D))) / D
        out.append((f'no isometry {k}, r not Hermitian', a, r, 'generic'))
    # a product state: A_s = c_s W with W unitary; the map is r -> W r W^+, of which 1 / D is a fixed point, rho_n = (|c><c|)^(x n)
    c = rng.standard_normal(2) + 1j * rng.standard_normal(2)
    c /= np.linalg.norm(c)
    W = O.haar_unitaries(rng, D, 1)[0]
    out.append(('product state', c[:, None, None] * W[None], np.eye(D, dtype=np.complex128) / D, 'product'))
    traceless = np.array(out[1][2])
    traceless[np.arange(D), np.arange(D)] = 0.25 * np.where(np.arange(D) % 2 == 0, 1.0, -1.0)      # finite, not zero: the trace is exactly zero
    with_nan = np.array(out[2][2])
    with_nan[D - 1, 0] = np.nan
    out.insert(3, ('tr r = 0', out[1][1], traceless, 'nan'))
    out.insert(7, ('a NaN element in r', out[2][1], with_nan, 'nan'))
    out = [(name, np.ascontiguousarray(a, dtype=np.complex128), np.ascontiguousarray(r, dtype=np.complex128), kind) for name, a, r, kind in out]
    for _, a, r, _ in out:
        a.setflags(write=False)
        r.setflags(write=False)
    return tuple(out)


def kinds(D):
    return np.array([k for _, _, _, k in cases(D)])


@functools.lru_cache(maxsize=None)
def case_tensors(D):
    return _frozen(np.stack([a for _, a, _, _ in cases(D)])), _frozen(np.stack([r for _, _, r, _ in cases(D)]))


def batch_index(D, B):
    """Case of every row of a batch of B: the list cycled, so that the NaN rows sit between finite ones in every workgroup they reach."""
    return np.arange(B) % len(cases(D))


def batch(D, B):
    A, r = case_tensors(D)
    idx = batch_index(D, B)
    return np.ascontiguousarray(A[idx]), np.ascontiguousarray(r[idx])


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def products(A, n):
    """B_t, t = sum_k t_k 2^(n-k): (2^n, D, D) in the dtype of A, by n - 1 calls of the oracle's `merge`."""
    Bt = A
    for _ in range(n - 1):
        Bt = O.merge(Bt, A)
    return Bt


def reference_rho(A, r, n):
    """rho (B, 2^n, 2^n) in np.clongdouble for A (B, 2, D, D), r (B, D, D) (or one of each: (2^n, 2^n)).  Rows whose tr r is zero or not
    finite, or whose r holds a non-finite element, come back as NaN."""
    A, r = np.asarray(A), np.asarray(r)
    single = r.ndim == 2
    A, r = A.reshape((-1,) + A.shape[-3:]).astype(CLD), r.reshape((-1,) + r.shape[-2:]).astype(CLD)
    T = 2 ** n
    out = np.empty((A.shape[0], T, T), dtype=CLD)
    for b in range(A.shape[0]):
        tr = np.trace(r[b])
        if not (np.isfinite(r[b].real).all() and np.isfinite(r[b].imag).all()) or tr == 0:
            out[b] = np.nan
            continue
        Bt = products(A[b], n)
        out[b] = np.einsum('tik,sik->ts', np.einsum('tij,jk->tik', Bt, r[b]), Bt.conj()) / tr
    return out[0] if single else out


@functools.lru_cache(maxsize=None)
def case_reference(D, n):
    """(rho, p, S) of the cases in long double, computed once: rho (cases, 2^n, 2^n), p (cases, 2^n), S (cases,); NaN on the NaN rows."""
    A, r = case_tensors(D)
    rho = reference_rho(A, r, n)
    p, _, S = EC.reference_spectrum(rho)
    return _frozen(rho), _frozen(p), _frozen(S)


def spectrum_of(rho):
    """(p, S) in long double of the rho a caller holds (the device's, or one built from the device's environments)."""
    p, _, S = EC.reference_spectrum(rho)
    return p, S


# ---- two float64 evaluations of the formula, in different orders -------------------------------------------------------------------------
def gram_order(A, r, n):
    """complex128: the 2^n products, M_t = B_t r, then the Gram matrix (the order of the kernels)."""
    A, r = np.asarray(A, dtype=np.complex128), np.asarray(r, dtype=np.complex128)
    Bt = products(A, n)
    with np.errstate(all='ignore'):
        return np.einsum('tik,sik->ts', np.matmul(Bt, r), Bt.conj()) / np.trace(r)


def recursion_order(A, r, n):
    """complex128: X -> A_t X A_s^+ site by site from the right end of the block, 4^k matrices after k sites, then their traces."""
    A, r = np.asarray(A, dtype=np.complex128), np.asarray(r, dtype=np.complex128)
    D = r.shape[0]
    X = r.reshape(1, 1, D, D)
    for _ in range(n):
        # the new site is to the left of those already there: it becomes the most significant bit of both indices
        X = np.einsum('tij,abjk,slk->tasbil', A, X, A.conj())
        X = X.reshape(X.shape[0] * X.shape[1], X.shape[2] * X.shape[3], D, D)
    with np.errstate(all='ignore'):
        return np.einsum('tsii->ts', X) / np.trace(r)


def partial_traces(rho):
    """(trace over the rightmost site, trace over the leftmost site) of rho (.., 2^n, 2^n): two (.., 2^(n-1), 2^(n-1))."""
    T = rho.shape[-1]
    x = rho.reshape(rho.shape[:-2] + (T // 2, 2, T // 2, 2))
    y = rho.reshape(rho.shape[:-2] + (2, T // 2, 2, T // 2))
    return np.einsum('...tasa->...ts', x), np.einsum('...atas->...ts', y)
