"""Accuracy of qmps_overlap_gradient (test infrastructure): pools of iterates per (D, ansatz kind), two references of their gradient
that do not share the kernels' arithmetic, and the bounds the kernels are held to as functions of the row.  Nothing here touches
the GPU; tests/test_gradient_cases_cpu.py checks all of it, tests/test_gradient_accuracy_gpu.py holds the kernels to it.

The gradient.  With M(x) the dense D^2 x D^2 matrix of the mixed map x -> sum_s C_s x Bm_s(x)^+ (C = WW . merge(A, A) of the reference
state, Bm = merge(B, B) of the iterate's tensor B(x)), eta its dominant eigenvalue, r / y its right / left eigenvectors, the device
returns g_k = (f(+h e_k) - f(-h e_k)) / 2h with f(x') = -sqrt|<y, M(x') r> / <y, r>| (include/qmps_hip.h, qmps_overlap_gradient).

Pools, per (D, kind) with D in (4, 8, 16) and kind in ansatz_cases.KINDS[D]; n_params = the largest of ansatz_cases.fd_param_counts
(6 everywhere it is not empty; kind 4 at D = 8 / 16 has none of 4 or 6 parameters: one layer, 8 / 10).
    near    X = ref + 0.03 N against the device-built references of `ref`, WW = expm(-0.05j H_TFIM); Xw = X + 1e-3 N is the warm call.
    far     parameters unrelated to their references, WW = expm(-0.2j (XX + YY + 0.5 ZZ)) (tests/test_overlap_gpu.py), selected by
            the dense spectrum into the bands |eta_2 / eta_1| < 0.9, 0.9 .. 0.99, 0.99 .. 0.998 in equal shares, shuffled with a fixed
            seed so that slow and fast rows share waves.
The operator is state of the context, not of a row, so a pool is one launch and (near, far) of a (D, kind) are two launches of the same
test.  ROWS: 13 at D = 4 (four items per wave: a tail of one), 7 at D = 8, 3 at D = 16 (5 for kind 0).  No row has a dominant pair
closer than MAX_RATIO = 0.998; the tied and Krylov tests cover that regime.  ExactAfter4 (kind 5) at D = 8, 16 crowds its dominant ring
even next to the reference: no near row passes (`pools` raises if one does), so its warm call is the far pool moved by 1e-3 N
(`far_warm`, selected to stay below MAX_RATIO as well).

References, per row and parameter k (`references`).
    g_exact     -Re(conj(eta) <y, dM/dx_k r> / <y, r>) / (2 |eta|^(3/2)): the derivative itself.  dM/dx_k from a Richardson ladder of
                central differences (h0 = 0.02, 5 levels) of Bm(x) - M is linear in Bm and entire in x, no eigenvalue crossing enters.
                A second ladder from h0 / 2 must agree to LADDER_TOL = 1e-11 on every row or the module raises.
    g_formula   the documented formula at the kernels' h beyond float64: tensors in long double from the float64 parameters
                (ansatz_cases.reference_columns; x +- h formed by ONE float64 addition, as the kernels form it), eta, y, r from the
                dense eigen-solve refined in long double by Newton steps on the bordered system until both eigen-residuals are below
                1e-17, the probes and the difference in long double.
    ratio, gap = 1 - ratio, inv_yr = 1 / |<y, r>| for unit vectors, dnorm = ||dM/dx_k||_2, eta, f = -sqrt|eta|, sens (below).

Bounds (`formula_bound`, `exact_bound`).
    device against g_formula(h)   C_R[D] 2^-52 / h + (tol + C_S 2^-52) amp(row, k)
        - the rounding of two probes over 2h, and the acceptance criterion ||x' - x||_F < tol of the two solves amplified into g.
    device against g_exact        the same plus |g_formula(h) - g_exact| of that row and k: the c h^2 of that row, from the references alone.
amp is NOT the norm product dnorm inv_yr / gap (`amp_norms`) but the first-order amplification itself, which is about the same on the fast rows and
smaller by factors of up to several hundred on the slow ones.  A power step from x = r + delta (delta in the complement of r) gives x' - x = (M / eta - 1) delta, so
delta = -S e with e = x' - x, ||e|| < tol, and S the reduced resolvent (1 - M / eta)^-1 on the complement (0 on r): it is large only for
an eigenvalue close to eta ITSELF, not for one of nearly equal modulus and another phase, which a step difference sees at full size.
With y exact, <y, M(x') (r + delta)> / <y, r + delta> moves by <y, (M(x') - M) delta> / <y, r> (y^+ M = eta y^+ and <y, delta> = 0), the
central difference of that is <y, dM_k S e> / <y, r>; an error S^+ e' of y gives <e', S dM_k r> / <y, r> likewise; and |dg| <= |d eta'| /
(2 sqrt|eta|).  Hence
    sens(row, k) = (||y^+ dM_k S||_2 + ||S dM_k r||_2) / (2 sqrt|eta| |<y, r>|),   amp = C_A sens.
C_R = 8 / 16 / 24 at D = 4 / 8 / 16, C_S = 8, C_A = 2.5: chosen on the CPU so that two float64 implementations of the METHOD (not of the
kernels) stay within a third of both bounds on every row, at h = 1e-6, 1e-4, 1e-2: `port` with y, r from numpy's dense eigen-solve
(float64 oracle tensors, one map application per neighbour), judged at tol = 0 - LAPACK's vectors answer to no tolerance - and
`port(power_tol=tol)`, y and r from float64 power iterations stopped at ||x' - x||_F < tol, tol = 1e-13 and 1e-10.  The ports' rounding
reaches 2.2 / 5.0 / 7.0 times 2^-52 / h at D = 4 / 8 / 16 (sums over D^2 terms: hence C_R per D), the power port 0.71 tol sens.
"Within a third of the exact bound" means: the part of |g - g_exact| beyond the references' own distance |g_formula(h) - g_exact| is
within a third of the formula bound (anything that follows the formula sits AT that distance; at h = 1e-2 it is 1e-4 .. 1e-2 and
everything else is noise on it).  `fractions` returns, and both test files print, these two figures.

What the bounds can see (tests/test_gradient_cases_cpu.py::test_the_bounds_bite; h = 1e-2, the dense-eig port, tol = 0).  conj dropped
from y and s1, s2 swapped in the probe contraction leave the bound by factors of 1e8 and more on every row of every pool.  One element
of one G_s moved by 1e-10 relative and one neighbour-tensor element moved by 1e-12 - each the element its entry of g leans on most -
leave it on EVERY row of every pool at D = 4 (5.8 and 2.1 bounds at the least) and at D = 8 (1.6 and 1.2).  At D = 16 they cannot on
every row, whatever the pools: an element is one of 1 024 there and the two mutations move g by as little as 1.0e-13, while the float64
ports themselves are up to 7.0 2^-52 / h = 1.6e-13 off the formula, so a bound that leaves the ports a factor of three is 4.7e-13 at the
least (C_R = 24: 5.3e-13).  A mutated port is off the formula by at most (what the mutation moves it by) + (what the port is off by) <= move + bound / 3,
and by at least move - bound / 3: a row moved by 4/3 bounds or more MUST leave the bound, a row moved by less than 2/3 cannot.  The
test asserts the first set - 33 (G_s) and 46 (neighbour) of the 48 rows - and pins those counts.

Measured on the CPU, worst fraction of the formula bound / beyond the references' distance, over pools, h and tol (the test prints them):
    eig port     D = 4   kind 0 0.227 / 0.179   1 0.277 / 0.277   3 0.235 / 0.235   4 0.189 / 0.189   5 0.257 / 0.257
                 D = 8   kind 0 0.178 / 0.178   1 0.269 / 0.197   3 0.184 / 0.182   4 0.141 / 0.136   5 0.203 / 0.203
                 D = 16  kind 0 0.211 / 0.162   1 0.137 / 0.137   3 0.148 / 0.147   4 0.190 / 0.190   5 0.292 / 0.292
    power port   D = 4   kind 0 0.255 / 0.251   1 0.258 / 0.258   3 0.218 / 0.218   4 0.188 / 0.187   5 0.256 / 0.256
                 D = 8   kind 0 0.142 / 0.142   1 0.171 / 0.165   3 0.142 / 0.142   4 0.181 / 0.179   5 0.312 / 0.312
                 D = 16  kind 0 0.181 / 0.181   1 0.126 / 0.126   3 0.148 / 0.147   4 0.172 / 0.172   5 0.153 / 0.139
References: the two ladders agree to 5.5e-13 / 1.1e-12 / 1.0e-12 at D = 4 / 8 / 16; |g_formula(1e-6) - g_exact| <= 1.9e-10 / 2.6e-10 /
3.5e-10 (far rows; ~1e-11 on the near pools); |g_formula(1e-2) - g_exact| / |g_formula(1e-3) - g_exact| = 94.3 .. 105.6 on the 1 984
entries above 1e-9; eigen-residuals of the refined y, r <= 3.4e-19.
Measured on an MI355X (tests/test_gradient_accuracy_gpu.py prints them), the same two figures, worst over every test of the file - pools,
h, tol = 1e-13 .. 1e-8, routes, warm calls, masks:
    D = 4   kind 0 0.309 / 0.284 (QMPS_OVERLAP_POWER, h = 1e-2)   1 0.223 / 0.223   3 0.190 / 0.190   4 0.095 / 0.094   5 0.125 / 0.125
    D = 8   kind 0 0.161 / 0.161 (tol = 1e-10)   1 0.127 / 0.121   3 0.148 / 0.145   4 0.140 / 0.100   5 0.052 / 0.048
    D = 16  kind 0 0.062 / 0.062   1 0.111 / 0.111   3 0.056 / 0.055   4 0.080 / 0.039   5 0.032 / 0.031
Largest |g - g_formula(h)| at tol = 1e-13: 5.9e-10 (h = 1e-6; 2.7 2^-52 / h), 5.1e-12 (1e-4), 2.0e-12 (1e-2); at tol = 1e-8: 2.0e-8.
"""
import functools

import numpy as np
import scipy.linalg
from scipy.linalg import expm

import ansatz_cases as AC
import evolve_replay as ER
from oracle import qmps_oracle as O

LD, CLD = np.longdouble, np.clongdouble
EPS = 2.0 ** -52
DS = (4, 8, 16)
HS = (1e-6, 1e-4, 1e-2)
H_LAW = 1e-3                       # the extra step of the h^2 law (references only)
MAX_RATIO = 0.998
BANDS = ((0.0, 0.9), (0.9, 0.99), (0.99, MAX_RATIO))
LADDER_H0, LADDER_LEVELS, LADDER_TOL = 0.02, 5, 1e-11
C_R, C_S, C_A = {4: 8.0, 8: 16.0, 16: 24.0}, 8.0, 2.5
WW_NEAR = expm(-0.05j * O.hamiltonian_matrix({'ZZ': -1.0, 'X': 1.0}))
WW_FAR = expm(-0.2j * O.hamiltonian_matrix({'XX': 1, 'YY': 1, 'ZZ': 0.5}))
POOLS = ('near', 'warm', 'far')
# ExactAfter4 at D >= 8 crowds its dominant ring even next to the reference (|eta_2 / eta_1| = 0.9998 .. 1.0000 at ref + 0.03 N): no near row
# passes MAX_RATIO (`pools` raises if one does), so these have a far pool and, for the warm call, the far pool moved by 1e-3 N
NO_NEAR = ((8, 5), (16, 5))
COLD_OF = {'warm': 'near', 'far_warm': 'far'}          # the pool whose call leaves the fixed points a warm pool starts from


def cases():
    return [(D, kind) for D in DS for kind in AC.KINDS[D]]


def pool_names(D, kind):
    return ('far', 'far_warm') if (D, kind) in NO_NEAR else POOLS


def n_params(D, kind):
    counts = AC.fd_param_counts(kind, D)
    return counts[-1] if counts else AC.per_layer(kind, D)


def rows(D, kind):
    return {4: 13, 8: 7, 16: 5 if kind == 0 else 3}[D]


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------
# float64 pieces shared by the pool selection and the ports
# ---------------------------------------------------------------------------------------------
def ratios64(D, kind, ref, X, WW_):
    """|eta_2 / eta_1| of the rows (ref[b], X[b]) by the dense spectrum (float64 of the batched long-double tensors)."""
    A, B = AC.reference_tensors(D, kind, ref), AC.reference_tensors(D, kind, X)
    C = np.einsum('st,btij->bsij', WW_, merge_ld(A))
    M = np.einsum('bsij,bskl->bikjl', C, merge_ld(B).conj()).reshape(len(A), D * D, D * D)
    w = np.sort(np.abs(np.linalg.eigvals(M)), axis=1)
    return w[:, -2] / w[:, -1]


@functools.lru_cache(maxsize=None)
def pools(D, kind):
    """dict(ref_near, X_near, X_warm (rows, P): the warm call's iterates against ref_near; ref_far, X_far, X_far_warm (used by the NO_NEAR
    cases alone: selected there so that it stays below MAX_RATIO too), band_far (rows,) int)."""
    P, n = n_params(D, kind), rows(D, kind)
    rng = np.random.default_rng([20261021, D, kind])
    chunk = {4: 256, 8: 64, 16: 24}[D]
    ref, X, Xw = [], [], []
    for _ in range(3 if (D, kind) in NO_NEAR else 20):
        a = rng.standard_normal((2 * n, P))
        x = a + 0.03 * rng.standard_normal((2 * n, P))
        xw = x + 1e-3 * rng.standard_normal((2 * n, P))
        ok = np.maximum(ratios64(D, kind, a, x, WW_NEAR), ratios64(D, kind, a, xw, WW_NEAR)) < MAX_RATIO - 1e-4
        ref.extend(a[ok]), X.extend(x[ok]), Xw.extend(xw[ok])
        if len(ref) >= n:
            break
    else:
        if (D, kind) not in NO_NEAR:
            raise RuntimeError(f'near pool of D = {D}, kind {kind}: {len(ref)} of {n} rows below ratio {MAX_RATIO}')
    if (D, kind) in NO_NEAR:
        if len(ref):
            raise RuntimeError(f'D = {D}, kind {kind} is listed in NO_NEAR, but {len(ref)} near rows are below ratio {MAX_RATIO}')
        ref, X, Xw = (np.empty((0, P)),) * 3
    want = [n // 3 + (1 if b < n % 3 else 0) for b in range(3)]
    far = [[] for _ in BANDS]
    rng_w = np.random.default_rng([20261024, D, kind])
    for _ in range(60):
        a, x = rng.standard_normal((chunk, P)), rng.standard_normal((chunk, P))
        q = ratios64(D, kind, a, x, WW_FAR)
        xw = x + 1e-3 * rng_w.standard_normal((chunk, P))
        warm_ok = ratios64(D, kind, a, xw, WW_FAR) < MAX_RATIO - 1e-4 if (D, kind) in NO_NEAR else np.ones(chunk, bool)
        for b, (lo, hi) in enumerate(BANDS):
            for i in np.flatnonzero((q >= lo + (1e-4 if b else 0.0)) & (q < hi - 1e-4) & warm_ok)[:want[b] - len(far[b])]:
                far[b].append((a[i], x[i], xw[i]))
        if all(len(f) == w for f, w in zip(far, want)):
            break
    else:
        raise RuntimeError(f'far pool of D = {D}, kind {kind}: bands filled {[len(f) for f in far]} of {want}')
    band = np.concatenate([[b] * w for b, w in enumerate(want)]).astype(int)
    fr = np.array([a for f in far for a, _, _ in f])
    fx = np.array([x for f in far for _, x, _ in f])
    fw = np.array([w for f in far for _, _, w in f])
    perm = np.random.default_rng([20261022, D, kind]).permutation(n)
    perm_n = np.random.default_rng([20261023, D, kind]).permutation(min(n, len(ref)))
    return _frozen({'ref_near': np.array(ref[:n])[perm_n], 'X_near': np.array(X[:n])[perm_n], 'X_warm': np.array(Xw[:n])[perm_n],
                    'ref_far': fr[perm], 'X_far': fx[perm], 'X_far_warm': fw[perm], 'band_far': band[perm]})


def pool(D, kind, name):
    """(ref (rows, P), X (rows, P), WW) of pool `name` in ('near', 'warm', 'far', 'far_warm')."""
    p = pools(D, kind)
    if name in ('far', 'far_warm'):
        return p['ref_far'], p['X_' + name], WW_FAR
    return p['ref_near'], p['X_warm' if name == 'warm' else 'X_near'], WW_NEAR


# ---------------------------------------------------------------------------------------------
# the long-double reference
# ---------------------------------------------------------------------------------------------
def tensors_ld(D, kind, params):
    """(R, 2, D, D) clongdouble, not rounded."""
    S = AC.reference_columns(D, kind, params)
    return np.swapaxes(S.reshape(S.shape[0], D, 2, D), 1, 2)


def merge_ld(A):
    """(..., 2, D, D) -> (..., 4, D, D): merge(A, A)[2 s1 + s2] = A[s1] A[s2]."""
    D = A.shape[-1]
    return np.einsum('...sij,...tjk->...stik', A, A).reshape(A.shape[:-3] + (4, D, D))


def shifted(x, hs):
    """(len(hs), 2, P, P): [a, 0, k] = x + hs[a] e_k, [a, 1, k] = x - hs[a] e_k, each by one float64 addition."""
    P = len(x)
    out = np.broadcast_to(np.asarray(x, dtype=np.float64), (len(hs), 2, P, P)).copy()
    for a, h in enumerate(hs):
        for k in range(P):
            out[a, 0, k, k] = x[k] + h
            out[a, 1, k, k] = x[k] - h
    return out


def _refine(M, lam, v):
    """Newton steps on (M - lam) v = 0, v0^H v = 1 with the residual in long double and the float64 LU of the bordered Jacobian as the
    solver; returns (lam, v / ||v||, residual) in long double."""
    N = len(v)
    v0 = v.astype(np.complex128)
    J = np.zeros((N + 1, N + 1), dtype=np.complex128)
    J[:N, :N] = M.astype(np.complex128) - complex(lam) * np.eye(N)
    J[:N, N] = -v0
    J[N, :N] = v0.conj()
    lu = scipy.linalg.lu_factor(J)
    lam, v = CLD(lam), v.astype(CLD)
    for _ in range(8):
        res = M @ v - lam * v
        size = float(np.sqrt(np.sum(np.abs(res) ** 2)) / np.sqrt(np.sum(np.abs(v) ** 2)))
        if size < 1e-17:
            break
        d = scipy.linalg.lu_solve(lu, np.concatenate([-(res / size).astype(np.complex128), [0.0]]))
        v = v + CLD(size) * d[:N].astype(CLD)
        lam = lam + CLD(size) * CLD(d[N])
    else:
        raise RuntimeError(f'the long-double refinement of an eigenpair stopped at residual {size:.1e}')
    return lam, v / np.sqrt(np.sum(np.abs(v) ** 2)), size


def _richardson(levels):
    """levels[j] = central difference at h0 / 2^j -> the extrapolated value (error O(h^(2 len)))."""
    T = list(levels)
    for m in range(1, len(T)):
        T = [(4.0 ** m * T[j + 1] - T[j]) / (4.0 ** m - 1.0) for j in range(len(T) - 1)]
    return T[0]


def row_reference(D, kind, xref, x, WW_, hs=HS + (H_LAW,)):
    """The references of one row: dict(eta, f, ratio, gap, inv_yr, dnorm (P,), g_exact (P,), ladder (P,): |difference of the two
    ladders|, g_formula (len(hs), P), residual: the larger eigen-residual of the refined y, r)."""
    P, N = len(x), D * D
    A = tensors_ld(D, kind, xref[None])[0]
    C = np.tensordot(WW_.astype(CLD), merge_ld(A), [1, 0])
    ladder_h = [LADDER_H0 / 2 ** j for j in range(LADDER_LEVELS + 1)]
    prm = np.concatenate([np.asarray(x, dtype=np.float64)[None], shifted(x, list(hs)).reshape(-1, P), shifted(x, ladder_h).reshape(-1, P)])
    Bm = merge_ld(tensors_ld(D, kind, prm))
    Bm0, Bm_h, Bm_l = Bm[0], Bm[1:1 + 2 * P * len(hs)].reshape(len(hs), 2, P, 4, D, D), Bm[1 + 2 * P * len(hs):].reshape(len(ladder_h), 2, P, 4, D, D)
    M = np.einsum('sij,skl->ikjl', C, Bm0.conj()).reshape(N, N)
    w, vl, vr = scipy.linalg.eig(M.astype(np.complex128), left=True, right=True)
    order = np.argsort(-np.abs(w))
    k0 = order[0]
    ratio = float(abs(w[order[1]]) / abs(w[k0]))
    eta, r, res_r = _refine(M, w[k0], vr[:, k0])
    etac, y, res_y = _refine(M.conj().T, np.conj(w[k0]), vl[:, k0])
    assert abs(complex(etac) - np.conj(complex(eta))) < 1e-15
    Y, R = y.reshape(D, D), r.reshape(D, D)
    yr = np.sum(y.conj() * r)
    G = np.einsum('ji,sjk,kl->sil', Y.conj(), C, R)                       # G_s = y^+ C_s r
    q = np.einsum('apksij,sij->apk', Bm_h.conj(), G) / yr                   # <y, T'(r)> / <y, r> of every neighbour
    fn = -np.sqrt(np.abs(q))
    h2 = np.array([LD(2.0 * h) for h in hs], dtype=LD)
    g_formula = ((fn[:, 0] - fn[:, 1]) / h2[:, None]).astype(np.float64)
    # the derivative itself: dBm / dx_k by two Richardson ladders (float64 of the long-double tensors), dM = sum_s C_s (x) conj(dBm_s)
    cd = [((Bm_l[j, 0] - Bm_l[j, 1]) / LD(2.0 * ladder_h[j])).astype(np.complex128) for j in range(len(ladder_h))]
    C64, y64, r64, eta64, yr64 = C.astype(np.complex128), y.astype(np.complex128), r.astype(np.complex128), complex(eta), complex(yr)
    g_ladders, dnorm, sens = [], np.empty(P), np.empty(P)
    # reduced resolvent S = (1 - M / eta)^-1 on the complement of r (zero on r): the eigenvector error of a step difference e is S e
    M64 = M.astype(np.complex128)
    P1 = np.outer(r64, y64.conj()) / yr64
    S = np.linalg.solve(np.eye(N) - M64 / eta64 + P1, np.eye(N) - P1)
    for first in (0, 1):
        dBm = _richardson(cd[first:first + LADDER_LEVELS])                  # (P, 4, D, D)
        gk = np.empty(P)
        for k in range(P):
            dM = np.einsum('sij,skl->ikjl', C64, dBm[k].conj()).reshape(N, N)
            deta = np.vdot(y64, dM @ r64) / yr64
            gk[k] = -np.real(np.conj(eta64) * deta) / (2.0 * abs(eta64) ** 1.5)
            if first == 0:
                dnorm[k] = np.linalg.norm(dM, 2)
                sens[k] = (np.linalg.norm(y64.conj() @ dM @ S) + np.linalg.norm(S @ (dM @ r64))) / (abs(yr64) * 2.0 * np.sqrt(abs(eta64)))
        g_ladders.append(gk)
    return {'eta': eta64, 'f': -np.sqrt(abs(eta64)), 'ratio': ratio, 'gap': 1.0 - ratio, 'inv_yr': 1.0 / abs(yr64), 'dnorm': dnorm, 'sens': sens,
            'g_exact': g_ladders[0], 'ladder': np.abs(g_ladders[0] - g_ladders[1]), 'g_formula': g_formula, 'residual': max(res_r, res_y)}


@functools.lru_cache(maxsize=None)
def references(D, kind, name):
    """The references of pool `name` of (D, kind): dict(eta (rows,), f, ratio, gap, inv_yr, residual; dnorm, g_exact, ladder (rows, P);
    g_formula (rows, len(HS) + 1, P) - the steps HS, then H_LAW).  Raises where the two ladders disagree by more than LADDER_TOL."""
    ref, X, WW_ = pool(D, kind, name)
    out = [row_reference(D, kind, a, x, WW_) for a, x in zip(ref, X)]
    got = {k: np.array([o[k] for o in out]) for k in out[0]}
    if not got['ladder'].max() <= LADDER_TOL:
        raise RuntimeError(f'D = {D}, kind {kind}, {name}: the Richardson ladders of dM/dx disagree by {got["ladder"].max():.1e}')
    if not got['ratio'].max() < MAX_RATIO:
        raise RuntimeError(f'D = {D}, kind {kind}, {name}: a row with ratio {got["ratio"].max():.6f}')
    return _frozen(got)


def g_formula(D, kind, name, h):
    hs = HS + (H_LAW,)
    return references(D, kind, name)['g_formula'][:, hs.index(h)]


# ---------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------
def amp(D, kind, name):
    """(rows, P): C_A sens - the first-order amplification of the two solves' step differences into g (module docstring)."""
    return C_A * references(D, kind, name)['sens']


def amp_norms(D, kind, name):
    """(rows, P): ||dM/dx_k||_2 / (|<y, r>| gap), the norm-product estimate `amp` replaces."""
    ref = references(D, kind, name)
    return ref['dnorm'] * (ref['inv_yr'] / ref['gap'])[:, None]


def formula_bound(D, kind, name, h, tol):
    return C_R[D] * EPS / h + (tol + C_S * EPS) * amp(D, kind, name)


def exact_bound(D, kind, name, h, tol):
    return formula_bound(D, kind, name, h, tol) + np.abs(g_formula(D, kind, name, h) - references(D, kind, name)['g_exact'])


def fractions(D, kind, name, h, tol, g, use=None):
    """Worst fractions over the rows in `use` (default all): |g - g_formula(h)| / formula_bound, and - the exact bound being the formula
    bound plus the references' own distance - the part of |g - g_exact| beyond that distance, over the formula bound again (anything
    that follows the formula sits AT the distance; the room it has is the formula bound).  Both <= 1 inside the bounds."""
    use = slice(None) if use is None else use
    fb = formula_bound(D, kind, name, h, tol)
    a = np.abs(g - g_formula(D, kind, name, h)) / fb
    b = (np.abs(g - references(D, kind, name)['g_exact']) - (exact_bound(D, kind, name, h, tol) - fb)) / fb
    return float(a[use].max()), float(max(b[use].max(), 0.0))


# ---------------------------------------------------------------------------------------------
# two float64 ports of the method
# ---------------------------------------------------------------------------------------------
def _power(M, tol, cap=400000):
    """x' = M x / <x, M x>, normalised, until ||x' - x||_F < tol (the documented acceptance criterion)."""
    N = M.shape[0]
    x = (np.ones(N) + 0.3j * np.cos(np.arange(N))).astype(complex)
    x /= np.linalg.norm(x)
    for it in range(cap):
        z = M @ x
        z = z / np.vdot(x, z)
        z /= np.linalg.norm(z)
        d = np.linalg.norm(z - x)
        x = z
        if d < tol:
            return x
    raise RuntimeError(f'the power iteration of the port did not reach {tol:.0e} in {cap} steps')


@functools.lru_cache(maxsize=None)
def _port_vectors(D, kind, name, power_tol):
    """Per row of the pool: (C, M, y, r) in float64 - y, r from the dense eigen-solve (power_tol None) or from power iterations."""
    ref, X, WW_ = pool(D, kind, name)
    out = []
    for a, x in zip(ref, X):
        A, B = ER.tensor(kind, D, a), ER.tensor(kind, D, x)
        C = np.tensordot(WW_, O.merge(A, A), [1, 0])
        M = O.transfer_matrix(C, O.merge(B, B))
        if power_tol is None:
            w, vl, vr = scipy.linalg.eig(M, left=True, right=True)
            k0 = int(np.argmax(np.abs(w)))
            r, y = vr[:, k0], vl[:, k0]
        else:
            r, y = _power(M, power_tol), _power(M.conj().T, power_tol)
        out.append((C, M, y, r))
    return out


@functools.lru_cache(maxsize=None)
def _port_neighbours(D, kind, name, h):
    """(rows, 2, P, 2, D, D): the float64 oracle's tensors at x + h e_k ([:, 0, k]) and x - h e_k ([:, 1, k])."""
    X = pool(D, kind, name)[1]
    Bn = np.array([[[ER.tensor(kind, D, p) for p in side] for side in shifted(x, [h])[0]] for x in X])
    Bn.setflags(write=False)
    return Bn


def port_row(D, kind, Bn, C, M, y, r, h, mutate=None):
    """One row of the documented formula in float64: (f, g (P,)).  mutate: None or one of MUTATIONS - a deliberately wrong variant (the
    bounds must notice)."""
    P = Bn.shape[1]
    eta = np.vdot(y, M @ r) / np.vdot(y, r)
    Y, R = y.reshape(D, D), r.reshape(D, D)
    if mutate == 'conj':
        Y = Y.conj()
    yr = np.sum(Y.conj() * R)
    G = np.einsum('ji,sjk,kl->sil', Y.conj(), C, R)
    if mutate == 'neighbour':                                               # the +h neighbour of every parameter: the element its probe leans on most
        Bn = Bn.copy()
        Gs = G.reshape(2, 2, D, D)
        for k in range(P):
            W = np.einsum('tbl,stal->sab', Bn[0, k].conj(), Gs) + np.einsum('tia,tsib->sab', Bn[0, k].conj(), Gs)
            Bn[0, k][np.unravel_index(np.argmax(np.abs(W)), W.shape)] += 1e-12
    Bm = np.einsum('pksij,pktjl->pkstil', Bn, Bn).reshape(2, P, 4, D, D)
    if mutate == 'swap':
        Bm = Bm.reshape(2, P, 2, 2, D, D).swapaxes(2, 3).reshape(2, P, 4, D, D)
    if mutate == 'G':                                                       # the element of G some entry of the gradient leans on most
        i = np.unravel_index(np.argmax(np.abs(G * (Bm[0] - Bm[1]).conj()).max(axis=0)), G.shape)
        G[i] *= 1.0 + 1e-10
    q = np.einsum('pksij,sij->pk', Bm.conj(), G) / yr
    fn = -np.sqrt(np.abs(q))
    return -np.sqrt(abs(eta)), (fn[0] - fn[1]) / (2.0 * h)


MUTATIONS = ('G', 'conj', 'swap', 'neighbour')
SMALL_MUTATIONS = ('G', 'neighbour')


def port(D, kind, name, h, power_tol=None, mutate=None):
    """(f (rows,), g (rows, P)) of a float64 port on pool `name`.  power_tol None: y, r from numpy's dense eigen-solve; else from float64
    power iterations stopped at ||x' - x||_F < power_tol."""
    out = [port_row(D, kind, Bn, C, M, y, r, h, mutate) for Bn, (C, M, y, r) in zip(_port_neighbours(D, kind, name, h), _port_vectors(D, kind, name, power_tol))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])
