"""Closing transfer gaps (test infrastructure): state tensors whose transfer map T has a second eigenvalue of modulus 1 - gap, gap
from ~1e-2 down to ~1e-9, at three places of the unit circle, the mpmath reference of their environment r, two-site density matrix
rho and energies E, and the bounds the solvers are held to as functions of the row (tests/test_gap_cases_cpu.py checks all of it
without a GPU; tests/test_gap_gpu.py holds the kernels to it).

The families.  `sector_tensor`: k sectors of bond dimension D / k, sector j feeding sector (j + shift) % k, behind a Haar gauge, the
unitary of the tensor then kicked by exp(t K): at t = 0 the map has k eigenvalues of modulus 1, the kick couples the sectors and
moves all but one inside the circle by O(t^2).
    slow    k 2, shift 0   lambda_2 -> +1: two nearly invariant sectors (overlap_cases.slow_environment_tensor).  The fixed point itself
                           is ill conditioned, kappa ~ 1 / gap.
    flip    k 2, shift 1   lambda_2 -> -1: period two.  The fixed point is perfectly conditioned (kappa 3 .. 7), every iteration is slow.
    cycle4  k 4, shift 1   three eigenvalues near -1, +i, -i of almost equal modulus: period four.  D >= 4.
Strengths t = 0.3 .. 1e-4 (D = 16: 0.3 .. 3e-4), ROWS[D] rows per (family, t), N_HAAR[D] Haar tensors added, everything shuffled once
with a fixed seed: slow and fast rows share quads, waves and work-counter draws.  Batches: 113 / 161 / 81 / 15 rows at D = 2 / 4 / 8 /
16 - no multiple of 16 (one Haar row more than a round number at D <= 8 sees to that).

Per row: r_ref from conditioning_cases.reference_mp (mpmath, 60 digits), rho_ref = oracle.two_site_rdm of the rounded r_ref, E_ref
for conditioning_cases.hamiltonian_terms(), lambda_2 (the subdominant eigenvalue of largest modulus), gap = 1 - |lambda_2|,
kappa = 1 / sigma_min(1 - Tt) with Tt = structure_factor_cases.deflated(A, r_ref) - the amplification of the residual of any
fixed-point solve - and lam_min, the smallest eigenvalue of r_ref.

The bounds.
    direct      max(C 2^-52 kappa, FLOOR 2^-52 D) on max |dr| and max |drho|, the same times ||h_n||_F on |dE_n|: a backward-stable solve
                of the pinned system.  C = 3, FLOOR = 4: chosen on the CPU so that oracle.env_direct on every row and
                direct_emu.energies_d4 (the D = 4 kernel's own arithmetic) on every D = 4 row stay within a third of it.
    iterative   (tol + C 2^-52) max(kappa, 1 / gap): the documented acceptance criterion ||r' - r||_F < tol times its worst
                amplification - 1 / gap for a single slow mode, kappa for the non-normal rest.
    status      of an iterative solve, from the reference spectrum alone: n* = ln(tol) / ln|lambda_2| power steps are needed;
                n* <= max_iter / 4 must be status 0, n* >= 4 max_iter may be status 1, in between either.  With a Krylov hand-over
                armed, a gap >= 3e-6 must be status 0.

Measured on the CPU over the final family, worst row of max |dr| / max |drho| / |dE| / ||h|| in units of 2^-52 kappa
(tests/test_gap_cases_cpu.py prints them, per family):
    oracle.env_direct        D = 2  0.44 / 0.44 / 0.27   D = 4  0.74 / 0.29 / 0.25   D = 8  0.71 / 0.25 / 0.21   D = 16  0.72 / 0.21 / 0.18
    direct_emu.energies_d4   D = 4  0.37 / 0.32 / 0.34 (both energy routes)
As fractions of the direct bound: env_direct 0.126 at most (D = 2, slow, r), the emulation 0.063; both accepted every row in one step
with status 0.  oracle.env_dense_eig reaches 0.85 (D = 2, slow, r) and leaves the bound at D = 8: 1.21 on E of a slow row - it is no
reference here.  The smallest lam_min is 1.0e-3 (D = 4), 4.5e-3 at D = 8, 4.7e-3 at D = 16: no row may be status 2.
D = 2 has sectors of bond dimension one: two rows at t = 0.3 carry their lambda_2 0.12 / 0.31 off the real axis, and a flip row whose
third eigenvalue is +0.9955 has kappa 223.
"""
import functools

import numpy as np
from scipy.linalg import expm

import structure_factor_cases as SF
from oracle import qmps_oracle as O
from tests import conditioning_cases as CC

EPS = 2.0 ** -52
DS = (2, 4, 8, 16)
FAMILIES = {'slow': (2, 0), 'flip': (2, 1), 'cycle4': (4, 1)}          # name: (sectors, shift)
STRENGTHS = {2: (0.3, 0.1, 0.03, 0.01, 3e-3, 1e-3, 3e-4, 1e-4), 16: (0.3, 0.03, 3e-3, 3e-4)}
STRENGTHS[4] = STRENGTHS[8] = STRENGTHS[2]
ROWS = {2: 6, 4: 6, 8: 3, 16: 1}                                       # per (family, t)
N_HAAR = {2: 17, 4: 17, 8: 9, 16: 3}                                   # (16 / 16 / 8 would make the batches 112 / 160 / 80 = multiples of 16)
SEED = {2: 7302, 4: 7304, 8: 7308, 16: 7316}
C_BOUND = 3.0
FLOOR = 4.0
KRYLOV_GAP = 3e-6            # the smallest gap tests/test_energy_gpu.py holds the Krylov hand-over to
LAM_MIN_FLOOR = 1e-3         # every row is positive definite by this margin: no status 2 is legitimate


def families(D):
    """cycle4 needs four sectors: D >= 4"""
    return tuple(f for f, (k, _) in FAMILIES.items() if D >= k and (k < 4 or D >= 4))


def sector_tensor(rng, D, t, k, shift):
    """k sectors of bond dimension D/k; sector j feeds sector (j + shift) % k; Haar gauge; unitary kicked by exp(t K)"""
    d = D // k
    Us = O.haar_unitaries(rng, 2 * d, k)
    A = np.zeros((2, D, D), dtype=complex)
    for j in range(k):
        i = (j + shift) % k
        A[:, i * d:(i + 1) * d, j * d:(j + 1) * d] = O.unitary_to_tensor(Us[j])
    G = O.haar_unitaries(rng, D, 1)[0]
    A = np.einsum('ij,sjk,lk->sil', G, A, G.conj())
    K = rng.standard_normal((2 * D, 2 * D)) + 1j * rng.standard_normal((2 * D, 2 * D))
    K = K - K.conj().T
    return O.unitary_to_tensor((expm(t * K / np.linalg.norm(K)) @ O.tensor_to_unitary(A))[None])[0]


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def family(D):
    """The rows of bond dimension D in their shuffled order: dict(A (B, 2, D, D), family (B,) of str - 'haar' for the Haar rows -, t (B,),
    0 for the Haar rows)."""
    rng = np.random.default_rng(SEED[D])
    A, fam, t = [], [], []
    for name in families(D):
        k, shift = FAMILIES[name]
        for tt in STRENGTHS[D]:
            for _ in range(ROWS[D]):
                A.append(sector_tensor(rng, D, tt, k, shift))
                fam.append(name)
                t.append(tt)
    A += list(O.unitary_to_tensor(O.haar_unitaries(rng, 2 * D, N_HAAR[D])))
    fam += ['haar'] * N_HAAR[D]
    t += [0.0] * N_HAAR[D]
    B = len(A)
    assert B % 16 != 0 and B % 64 != 0, B
    perm = np.random.default_rng(SEED[D] + 1).permutation(B)
    return _frozen({'A': np.ascontiguousarray(np.stack(A)[perm]), 'family': np.array(fam)[perm], 't': np.array(t)[perm]})


def subdominant(A):
    """Eigenvalues of the transfer map by modulus, descending, without the dominant one."""
    w = np.linalg.eigvals(O.transfer_matrix(A))
    return w[np.argsort(-np.abs(w))][1:]


def kappa_of(A, r):
    """||(1 - Tt)^-1||_2, Tt the transfer map with its fixed point projected out."""
    N = A.shape[1] ** 2
    return 1.0 / np.linalg.svd(np.eye(N) - SF.deflated(A, r), compute_uv=False)[-1]


@functools.lru_cache(maxsize=None)
def references(D):
    """dict(r, rho, E (B, terms), lam2 (complex), lam3 (B, 3) complex: the three subdominant eigenvalues, gap, kappa, lam_min) for the
    rows of family(D).  reference_mp raises where its refinement does not converge."""
    fam = family(D)
    h = CC.hamiltonian_terms()
    r, lam_min, lam3, kappa = [], [], [], []
    for a in fam['A']:
        rr, lm = CC.reference_mp(a)
        r.append(rr)
        lam_min.append(lm)
        lam3.append(subdominant(a)[:3])
        kappa.append(kappa_of(a, rr))
    r = np.stack(r)
    rho = np.stack([O.two_site_rdm(a, rr) for a, rr in zip(fam['A'], r)])
    lam3 = np.stack(lam3)
    return _frozen({'r': r, 'rho': rho, 'E': np.real(np.einsum('nst,bts->bn', h, rho)), 'lam2': lam3[:, 0].copy(), 'lam3': lam3,
                    'gap': 1.0 - np.abs(lam3[:, 0]), 'kappa': np.array(kappa), 'lam_min': np.array(lam_min)})


def h_norms():
    return np.linalg.norm(CC.hamiltonian_terms().reshape(-1, 16), axis=1)


def direct_bound(D):
    """(B,) bound on max |dr| and max |drho| of a direct solve; the bound on |dE[:, n]| is this times h_norms()[n]."""
    return np.maximum(C_BOUND * EPS * references(D)['kappa'], FLOOR * EPS * D)


def iterative_bound(D, tol):
    ref = references(D)
    return (tol + C_BOUND * EPS) * np.maximum(ref['kappa'], 1.0 / ref['gap'])


def power_steps_needed(D, tol):
    """n* = ln(tol) / ln|lambda_2|"""
    return np.log(tol) / np.log(np.abs(references(D)['lam2']))


def must_converge(D, tol, max_iter, krylov=False):
    """(B,) bool: rows an iterative solve must end with status 0 on."""
    must = power_steps_needed(D, tol) <= max_iter / 4
    if krylov:
        must |= references(D)['gap'] >= KRYLOV_GAP
    return must


def may_fail(D, tol, max_iter, krylov=False):
    """(B,) bool: rows on which status 1 is certainly right (no assertion rests on it: between the two bands either status is)."""
    may = power_steps_needed(D, tol) >= 4 * max_iter
    if krylov:
        may &= references(D)['gap'] < KRYLOV_GAP
    return may


def errors(D, out, rows=None):
    """max |dr|, max |drho| (B,) and |dE| (B, terms) of dict(E, r, rho) against the reference, for rows `rows` of the family (default
    all, in order)."""
    ref = references(D)
    g = np.arange(len(ref['r'])) if rows is None else np.asarray(rows)
    return (np.abs(out['r'] - ref['r'][g]).reshape(len(g), -1).max(1), np.abs(out['rho'] - ref['rho'][g]).reshape(len(g), -1).max(1),
            np.abs(out['E'] - ref['E'][g]))


def worst_fraction(D, out, bound, use=None):
    """Largest error of `out` over the rows in `use` (bool mask, default all) as a fraction of bound (B,), per quantity and per family:
    dict(family: (r, rho, E)).  E is measured against bound x ||h_n||_F."""
    dr, drho, dE = errors(D, out)
    fam = family(D)['family']
    use = np.ones(len(fam), bool) if use is None else use
    fig = {}
    for name in families(D) + ('haar',):
        m = use & (fam == name)
        if m.any():
            fig[name] = (float((dr[m] / bound[m]).max()), float((drho[m] / bound[m]).max()),
                         float((dE[m] / (bound[m, None] * h_norms())).max()))
    return fig


def show(label, fig):
    print(label + ': ' + '; '.join(f'{k} r {v[0]:.3f} rho {v[1]:.3f} E {v[2]:.3f}' for k, v in fig.items()))


def cpu_direct(D):
    """oracle.env_direct on every row: dict(E, r, rho, iters, status)."""
    fam = family(D)
    h = CC.hamiltonian_terms()
    sol = [O.env_direct(a) for a in fam['A']]
    r = np.stack([s[0] for s in sol])
    rho = np.stack([O.two_site_rdm(a, rr) for a, rr in zip(fam['A'], r)])
    return {'r': r, 'rho': rho, 'E': np.real(np.einsum('nst,bts->bn', h, rho)), 'iters': np.array([s[1] for s in sol]),
            'status': np.array([s[2] for s in sol])}


def cpu_dense_eig(D):
    fam = family(D)
    h = CC.hamiltonian_terms()
    r = np.stack([O.env_dense_eig(a)[1] for a in fam['A']])
    rho = np.stack([O.two_site_rdm(a, rr) for a, rr in zip(fam['A'], r)])
    return {'r': r, 'rho': rho, 'E': np.real(np.einsum('nst,bts->bn', h, rho))}
