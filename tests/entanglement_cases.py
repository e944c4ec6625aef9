"""Entanglement spectra of the resident states (qmps_entanglement): the long-double reference, the inputs of the tests that use it, a
float64 numpy port of the kernels' own sweep and the bounds they are held to (test infrastructure;
tests/test_entanglement_cases_cpu.py checks all of it without a GPU).

Conventions (include/qmps_hip.h): for a right environment r

    p[k]    = k-th largest eigenvalue of herm(r) / tr r,  herm(r) = (r + r^+) / 2          (descending, signed)
    S       = - sum_(p > 0) p ln p                                                         (nats)
    V[i, k] = component i of the unit eigenvector of p[k]:  herm(r) V = tr(r) V diag(p),  V^+ V = 1

Bounds.  EIG_C = 4: |p - p_ref| <= EIG_C D 2^-52, absolute (the spectrum has unit trace; Jacobi is backward stable in
|r|_F <= tr r).  Set on the CPU so that numpy.linalg.eigvalsh in float64 and the float64 port of the kernels' sweep (`kernel_port`)
both stay within a third of it on every finite case of this module, against the long-double reference.  Measured worst cases
(tests/test_entanglement_cases_cpu.py prints them), in units of D 2^-52 at D = 2 / 4 / 8 / 16:
eigvalsh 0.89 / 0.36 / 0.16 / 0.17 (ratio to the bound 0.22 at most; the margin to a third is for another LAPACK),
the port 0.28 / 0.23 / 0.28 / 0.12.  The port's eigenvector residuals, held to the same bound: |V^+ V - 1|_max 1.00 / 1.91 / 1.73 /
1.66 (every rotation is unitary to a rounding or two and they accumulate), |herm(r) V / tr r - V diag(p)|_max 0.29 / 0.25 / 0.25 /
0.13.  Sweeps the port needed: 1 / 4 / 7 / 11 at most on the cases of this module, 1 / 4 / 12 / 14 on `tied_cluster_batch` with
k = 2 .. D and 300 to 2000 Haar bases per (k, tail) (profiles/EXPERIMENTS.md).  Clusters of tied eigenvalues are what the rule
DROP2 is for: without it they hover just above the termination test for up to 47 sweeps at D = 16.
The entropy bound follows from the eigenvalue bound (modulus of continuity of -p ln p at 0, plus the summation); it is not measured.
"""
import functools

import numpy as np

from oracle import qmps_oracle as O

LD = np.longdouble
CLD = np.clongdouble
EPS = 2.0 ** -52

DS = (2, 4, 8, 16)
BATCHES = (1, 17, 65, 130)            # lane, group and workgroup tails: the case list of a bond dimension, cycled
EIG_C = 4.0
SWEEP_CAP = {2: 1, 4: 10, 8: 24, 16: 30}       # the kernels' compile-time caps (qmps_entanglement.hip): twice the sweeps seen, or more
DROP2 = 2.0 ** -102                   # ... and so is one with |a_pq|^2 <= DROP2 |a_pp a_qq|: rounding noise between tied eigenvalues
TINY2 = 2.0 ** -960                   # a pivot with |a_pq|^2 below this is set to zero without a rotation (qmps_entanglement.hip)
HAAR_ENVS = 6                         # solved environments per bond dimension among the cases
HAAR_SEED = {2: 6102, 4: 6104, 8: 6108, 16: 6116}


def eig_bound(D):
    """Largest |p - p_ref| granted to a float64 eigenvalue of a unit-trace matrix of size D; also the bound of the two eigenvector
    residuals |V^+ V - 1|_max and |herm(r) V / tr r - V diag(p)|_max."""
    return EIG_C * D * EPS


def entropy_bound(D):
    """|S - S_ref| that follows from eig_bound: D delta (1 + |ln delta|) for the D terms -p ln p (modulus of continuity at 0) plus
    D 2^-52 ln D for the summation."""
    d = eig_bound(D)
    return D * d * (1.0 + abs(np.log(d))) + D * EPS * np.log(D)


def _frozen(a):
    a.setflags(write=False)
    return a


def herm(r):
    r = np.asarray(r)
    h = (r + r.conj().swapaxes(-1, -2)) / 2
    return h


# ---- the reference: row-cyclic Jacobi in long double, batched -----------------------------------------------------------------------
def reference_spectrum(r):
    """(p, V, S) of r (D, D) or (B, D, D) in np.longdouble / np.clongdouble: descending eigenvalues of herm(r) / tr r, their unit
    eigenvectors in the columns of V, S = - sum_(p > 0) p ln p.  Row-cyclic Jacobi, every pivot of a sweep one after the other, until
    off(A)^2 <= (2^-63)^2 sum a_ii^2; a pivot with |a_pq| <= 2^-62 sqrt|a_pp a_qq| is zeroed without a rotation (the rule DROP2 at
    this precision: an eigenvalue moves by 2^-62 at most).  Rows whose trace is zero or that hold a non-finite element come back as NaN."""
    r = np.asarray(r)
    single = r.ndim == 2
    a = np.array(r, dtype=CLD).reshape((-1,) + r.shape[-2:])
    B, D, _ = a.shape
    tr = np.trace(a, axis1=1, axis2=2).real
    bad = ~np.isfinite(a.real).all(axis=(1, 2)) | ~np.isfinite(a.imag).all(axis=(1, 2)) | (tr == 0)
    a[bad] = np.eye(D, dtype=CLD)
    tr = np.where(bad, LD(1), tr)
    a = (a + a.conj().transpose(0, 2, 1)) / 2 / tr[:, None, None]
    V = np.broadcast_to(np.eye(D, dtype=CLD), a.shape).copy()
    idx = np.arange(D)
    offdiag = 1 - np.eye(D)
    eps2 = LD(2.0) ** -126
    drop2 = LD(2.0) ** -124            # pivots below 2^-62 sqrt|a_pp a_qq| are zeroed without a rotation (noise between tied eigenvalues)
    for _ in range(60):
        d2 = (a[:, idx, idx].real ** 2).sum(axis=1)
        off2 = ((a.real ** 2 + a.imag ** 2) * offdiag).sum(axis=(1, 2))
        if np.all(off2 <= eps2 * d2):
            break
        for p in range(D - 1):
            for q in range(p + 1, D):
                apq = a[:, p, q].copy()
                ab = np.abs(apq)
                m = ab * ab > drop2 * np.abs(a[:, p, p].real * a[:, q, q].real)       # (false at ab = 0)
                safe = np.where(m, ab, LD(1))
                w = np.where(m, apq / safe, CLD(1))
                tau = (a[:, q, q].real - a[:, p, p].real) / (2 * safe)
                t = np.where(tau >= 0, LD(1), LD(-1)) / (np.abs(tau) + np.sqrt(1 + tau * tau))
                t = np.where(m, t, LD(0))
                c = 1 / np.sqrt(1 + t * t)
                s = t * c
                app, aqq = a[:, p, p].real - t * ab, a[:, q, q].real + t * ab
                wc = w.conj()
                for M in (a, V):                             # columns: M J
                    cp, cq = M[:, :, p].copy(), M[:, :, q].copy()
                    M[:, :, p] = c[:, None] * cp - (s * wc)[:, None] * cq
                    M[:, :, q] = s[:, None] * cp + (c * wc)[:, None] * cq
                rp, rq = a[:, p, :].copy(), a[:, q, :].copy()   # rows: J^+ A
                a[:, p, :] = c[:, None] * rp - (s * w)[:, None] * rq
                a[:, q, :] = s[:, None] * rp + (c * w)[:, None] * rq
                a[:, p, q] = 0
                a[:, q, p] = 0
                a[:, p, p] = np.where(m, app, a[:, p, p].real)
                a[:, q, q] = np.where(m, aqq, a[:, q, q].real)
    else:
        raise RuntimeError('the long-double Jacobi did not converge')
    p = a[:, idx, idx].real
    order = np.argsort(-p, axis=1, kind='stable')
    p = np.take_along_axis(p, order, axis=1)
    V = np.take_along_axis(V, order[:, None, :], axis=2)
    S = entropy(p)
    p[bad], V[bad], S[bad] = np.nan, np.nan, np.nan
    return (p[0], V[0], S[0]) if single else (p, V, S)


def entropy(p):
    """- sum_(p > 0) p ln p over the last axis, smallest eigenvalues first, in the dtype of p."""
    p = np.sort(np.asarray(p), axis=-1)
    q = np.where(p > 0, p, 1)
    return -_ascending_sum(q * np.log(q))


def _ascending_sum(terms):
    """Sum over the last axis in the order of the eigenvalues ascending (what the kernels do), in the dtype of `terms`."""
    s = np.zeros(terms.shape[:-1], dtype=terms.dtype)
    for k in range(terms.shape[-1]):
        s = s + terms[..., k]
    return s


# ---- the float64 port of the kernels' sweep ------------------------------------------------------------------------------------------
def round_robin(D):
    """The D - 1 rounds of D / 2 disjoint pivots (p < q) of one sweep, in the kernels' order: the circle method with D - 1 fixed."""
    rounds = []
    for m in range(D - 1):
        pairs = [(m, D - 1)]
        for k in range(1, D // 2):
            a, b = (m + k) % (D - 1), (m - k) % (D - 1)
            pairs.append((min(a, b), max(a, b)))
        rounds.append(pairs)
    return rounds


def kernel_port(r, want_sweeps=False):
    """What qmps_entanglement.hip computes, in float64 numpy: herm and division by tr r on load, the D / 2 rotations of a round-robin
    round taken from the matrix before the round and applied together, termination after a sweep by off(A)^2 <= 2^-104 sum a_ii^2 (or
    a sweep without a rotation), the cap on sweeps (NaN beyond it), descending sort, S summed ascending.  (p, V, S[, sweeps])."""
    r = np.asarray(r, dtype=np.complex128)
    a = r.reshape((-1,) + r.shape[-2:]).copy()
    B, D, _ = a.shape
    tr = np.trace(a, axis1=1, axis2=2).real
    with np.errstate(all='ignore'):
        scale = 1.0 / tr
    bad = ~np.isfinite(a.real).all(axis=(1, 2)) | ~np.isfinite(a.imag).all(axis=(1, 2)) | ~np.isfinite(tr) | (tr == 0) | ~np.isfinite(scale)
    a[bad] = np.eye(D)
    scale = np.where(bad, 1.0, scale)
    a = (a + a.conj().transpose(0, 2, 1)) * 0.5 * scale[:, None, None]
    V = np.broadcast_to(np.eye(D, dtype=np.complex128), a.shape).copy()
    idx = np.arange(D)
    offdiag = 1 - np.eye(D)
    done = bad.copy()
    sweeps = np.zeros(B, dtype=int)
    rounds = round_robin(D)
    for _ in range(SWEEP_CAP[D]):
        live = ~done
        if not live.any():
            break
        sweeps[live] += 1
        rotated = np.zeros(B, dtype=bool)
        for pairs in rounds:
            J = np.broadcast_to(np.eye(D, dtype=np.complex128), a.shape).copy()
            new_diag = {}
            for p, q in pairs:
                apq = a[:, p, q]
                n2 = apq.real ** 2 + apq.imag ** 2
                m = (n2 >= TINY2) & (n2 > DROP2 * np.abs(a[:, p, p].real * a[:, q, q].real)) & live
                rotated |= m
                inv = 1.0 / np.sqrt(np.where(m, n2, 1.0))
                ab = n2 * inv
                w = apq * inv
                tau = 0.5 * (a[:, q, q].real - a[:, p, p].real) * inv
                ta = np.minimum(np.abs(tau), 1e150)
                t = np.copysign(1.0, tau) / (ta + np.sqrt(1 + ta * ta))
                c = 1 / np.sqrt(1 + t * t)
                s = t * c
                c, s, w = np.where(m, c, 1.0), np.where(m, s, 0.0), np.where(m, w, 1.0)
                J[:, p, p], J[:, q, p], J[:, p, q], J[:, q, q] = c, -s * w.conj(), s, c * w.conj()
                new_diag[(p, q)] = (m, a[:, p, p].real - t * ab, a[:, q, q].real + t * ab)
            Jh = J.conj().transpose(0, 2, 1)
            a_new = np.matmul(Jh, np.matmul(a, J))
            V = np.where(live[:, None, None], np.matmul(V, J), V)
            for (p, q), (m, app, aqq) in new_diag.items():
                z = live & ~m                                   # below TINY2: zeroed without a rotation
                a_new[:, p, q] = np.where(m | z, 0.0, a_new[:, p, q])
                a_new[:, q, p] = np.where(m | z, 0.0, a_new[:, q, p])
                a_new[:, p, p] = np.where(m, app, a[:, p, p].real)
                a_new[:, q, q] = np.where(m, aqq, a[:, q, q].real)
            a_new = (a_new + a_new.conj().transpose(0, 2, 1)) / 2   # the kernels store one triangle (D <= 4) or mirror it (D >= 8)
            a = np.where(live[:, None, None], a_new, a)
        d2 = (a[:, idx, idx].real ** 2).sum(axis=1)
        off2 = ((a.real ** 2 + a.imag ** 2) * offdiag).sum(axis=(1, 2))
        done |= live & ((off2 <= 2.0 ** -104 * d2) | ~rotated)
    p = a[:, idx, idx].real.copy()
    order = np.argsort(-p, axis=1, kind='stable')
    p = np.take_along_axis(p, order, axis=1)
    V = np.take_along_axis(V, order[:, None, :], axis=2)
    S = entropy(p)
    fail = bad | ~done
    p[fail], V[fail], S[fail] = np.nan, np.nan, np.nan
    return (p, V, S, sweeps) if want_sweeps else (p, V, S)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def spectra(D):
    rng = np.random.default_rng(6000 + D)
    k = np.arange(D)
    half = np.zeros(D)
    half[:2] = 0.5
    return {'mixed': np.full(D, 1.0 / D), 'product': np.eye(D)[0], 'half': half, 'steep': 10.0 ** (-2 * k), 'gentle': 10.0 ** (-k / 2),
            'uniform': rng.uniform(size=D)}


TAILS = ('zero', 'tiny', 'graded')


def tied_cluster_spectrum(D, k, tail, rng):
    """k tied eigenvalues 1 and D - k others: zero, 1e-12 x uniform, or 10^-1, 10^-2, ... (not normalised)."""
    p = np.zeros(D)
    p[:k] = 1.0
    if tail == 'tiny':
        p[k:] = 1e-12 * rng.uniform(size=D - k)
    elif tail == 'graded':
        p[k:] = 10.0 ** -np.arange(1, D - k + 1)
    return p


def tied_cluster_batch(D, k, tail, n, seed):
    """n Haar-rotated matrices with the spectrum `tied_cluster_spectrum(D, k, tail)`, and that spectrum descending with unit sum."""
    rng = np.random.default_rng(seed)
    p = tied_cluster_spectrum(D, k, tail, rng)
    U = O.haar_unitaries(rng, D, n)
    return herm(np.einsum('bij,j,bkj->bik', U, p, U.conj())), np.sort(p)[::-1] / p.sum()


def cluster_sizes(D):
    """Cluster sizes among the cases: two tied, half, all but two, all but one."""
    return sorted({k for k in (2, D // 2, D - 2, D - 1) if 2 <= k < D})


@functools.lru_cache(maxsize=None)
def cases(D):
    """Tuple of (name, r (D, D) complex128, kind), kind in ('finite', 'nan', 'indefinite').  The two NaN cases sit apart, between
    finite ones; the first case is finite."""
    rng = np.random.default_rng(6200 + D)
    U = O.haar_unitaries(rng, D, 8)
    out = []

    def rotated(p, u):
        return herm((u * p[None, :]) @ u.conj().T)

    for name, p in spectra(D).items():
        out.append((f'{name}, Haar basis', rotated(p, U[0]), 'finite'))
        out.append((f'{name}, diagonal', np.diag(p).astype(np.complex128), 'finite'))
    K = rng.standard_normal((D, D)) * 0.1
    out.append(('imaginary off-diagonal', np.diag(rng.uniform(size=D) + 1.0) + 1j * (K - K.T), 'finite'))
    G = rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D))
    out.append(('not exactly Hermitian', rotated(spectra(D)['uniform'], U[1]) + 1e-9 * (G - G.conj().T) / 2, 'finite'))
    base = rotated(rng.uniform(size=D), U[2])
    base = base / np.trace(base).real
    for tr in (1.0, 3.7, 1e-3):
        out.append((f'trace {tr}', base * tr, 'finite'))
    A = O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(HAAR_SEED[D]), 2 * D, HAAR_ENVS))
    for b, a in enumerate(A):
        out.append((f'Haar environment {b}', np.asarray(O.env_dense_eig(a)[1], dtype=np.complex128), 'finite'))
    for n, k in enumerate(cluster_sizes(D)):
        for tail in TAILS:
            out.append((f'{k} tied, {tail} tail', tied_cluster_batch(D, k, tail, 1, 6500 + 37 * D + 3 * n + TAILS.index(tail))[0][0], 'finite'))
    ind = np.zeros(D)
    ind[:min(D, 3)] = (0.8, 0.4, -0.2) if D > 2 else (0.8, -0.2)
    out.append(('indefinite', rotated(ind, U[3]), 'indefinite'))
    with_nan = rotated(spectra(D)['uniform'], U[4])
    with_nan[D - 1, 0] = np.nan
    out.insert(3, ('all zero', np.zeros((D, D), dtype=np.complex128), 'nan'))
    out.insert(9, ('a NaN element', with_nan, 'nan'))
    for _, r, _ in out:
        r.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case_matrices(D):
    return _frozen(np.stack([r for _, r, _ in cases(D)]))


def kinds(D):
    return np.array([k for _, _, k in cases(D)])


def batch_index(D, B):
    """Case of every row of a batch of B: the list cycled, so that every wave mixes matrices that are done at once with slow ones and
    the NaN cases sit between healthy ones."""
    return np.arange(B) % len(cases(D))


def batch(D, B):
    return np.ascontiguousarray(case_matrices(D)[batch_index(D, B)])


@functools.lru_cache(maxsize=None)
def case_reference(D):
    """Long-double (p, V, S) of `case_matrices(D)`, computed once."""
    p, V, S = reference_spectrum(case_matrices(D))
    return _frozen(p), _frozen(V), _frozen(S)


def residuals(r, p, V):
    """(|p - p_ref| is the caller's) the two gauge-free eigenvector residuals of a result, in long double:
    |V^+ V - 1|_max and |herm(r) V / tr r - V diag(p)|_max per row."""
    r = np.asarray(r, dtype=CLD)
    V = np.asarray(V, dtype=CLD)
    p = np.asarray(p, dtype=LD)
    h = (r + r.conj().swapaxes(-1, -2)) / 2 / np.trace(r, axis1=-2, axis2=-1).real[..., None, None]
    D = r.shape[-1]
    orth = np.abs(np.matmul(V.conj().swapaxes(-1, -2), V) - np.eye(D)).max(axis=(-2, -1))
    eq = np.abs(np.matmul(h, V) - V * p[..., None, :]).max(axis=(-2, -1))
    return orth.astype(float), eq.astype(float)
