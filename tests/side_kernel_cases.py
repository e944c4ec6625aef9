"""Inputs and references for the kernels behind the secondary optimisers (test infrastructure; tests/test_side_kernel_cases_cpu.py proves
every condition stated here without a GPU, tests/test_side_kernels_gpu.py holds the kernels to it):

  qmps_cell2.hip      two-site unit cell, D = 2           NonSparseFullTwoSiteEnergyOptimizer
  qmps_brickwall.hip  bw_env / bw_expval / bw_manifold    new_tdvp
  qmps_su.hip         SU(N) parameters -> unitary/tensor  NonSparseFullEnergyOptimizer, examples/bond_dimension.py

1. Two-site cells.  conditioning_cases.near_product_tensors at D = 2, two independent draws per cell, as UNITARIES (the kernel applies
unitary_to_tensor on load): ungauged U = exp(-i t H); gauged U' = (G x 1_2) U blockdiag(G^H, 1_D), which is A_s -> G A_s G^H under
unitary_to_tensor.  12 gauged strengths and 4 ungauged ones, 8 cells each, and 41 Haar cells: 169 rows (not a multiple of 64), shuffled once.
(Gauged t = 1e-8, 1e-10 and 1e-11 were added to the nine strengths first chosen: at D = 2 the kernel still resolves lam_min ~ 1e-15 at
t = 1e-7, and only the 8 gauged rows at t = 1e-9 came back status 2 - a seventh of the rows with t <= 1e-5, where a fifth is asked for.)
The transfer gap of T_A1 T_A2 stays at or above 0.17; the first pivot of the unpivoted 4 x 4 elimination, |T[0][0] - 1|, falls below the
acceptance threshold 1e-10 on the ungauged cells from t = 1e-6 down and nowhere else, so exactly those rows take the power loop.
Reference: conditioning_cases.reference_mp on oracle.merge(A1, A2) (physical dimension 4) gives r12 and its smallest eigenvalue;
r21 = T_A2(r12) / tr is formed in mpmath from the rounded r12 (its rounding, 1e-16, is a thousandth of the status band) and goes through
mpmath's eigh as well.  Energies: oracle.two_site_cell_energy_closed with the rounded environments, per term of
conditioning_cases.hamiltonian_terms().

2. Brick-wall environments.  leading_eigenpair(M) is the kernel's documented rule restated on LAPACK's eigenvalues: largest
Re(lambda) + 1e-6 Im(lambda), all eigenvalues within 1e-9 of the best under that order; a matrix whose imaginary part is exactly zero goes
through the REAL eigen-solver, so that conjugate pairs are exact (the complex solver returns the pair with real parts that differ in
the last bit, and oracle.brickwall_oracle.dominant - numpy's argmax - then picks either sign).  Rows, two sides each: (a) 150 Haar-orthogonal
quadruples (real matrices: a leading conjugate pair is an exact tie in the real part, the tilt alone decides; the seed is one of the
four among nine tried that keep every leading pair out of the second status-1 class below, which begins at |Im| < 5e-3: its smallest
|Im| is 1.28e-2), (b) 150 Haar-unitary
quadruples, (c) 150 state-like ones (primed gates = daggers, eta = 1), (d) 600 quadruples drawn from an 11-gate grid of special gates and
the 12 rows of the existing regression.  Status 1 is explained by the reference in two classes only: M nilpotent (||M^4||_F < 1e-12), or
the two leading eigenvalues closer than 1e-8 under the tilted order without being equal (|difference| > 1e-12: LAPACK returns a semi-simple
eigenvalue to a few ulps, a defective one split by ~1e-8).  The bound: the power exp(c M)^(2^40) is rank one to the kernel's 1e-11 only if
the tilted gap exceeds ln(1e11) / 2^40 = 2.3e-11, reached after the Taylor start; 1e-8 leaves a margin of ~50 on the 2e-10 that the three
rank-one rounds the relaxed acceptance asks for would need.

3. SU(N).  Eight standard-normal parameter rows interleaved with rows scaled by 6, 300 and 1e5 (at N = 4 every workgroup of four mixes all
sizes); mpmath expm of the host mirror's generator at N = 4, 8.  Pools for the tensor output (13 rows: 4 k + 1) and the two-site cell (41)."""
import functools

import mpmath as mp
import numpy as np

from oracle import brickwall_oracle as BW
from oracle import qmps_oracle as O
from qmps_amd import ground_state as G
from tests import conditioning_cases as CC

POOL = 41                        # prime, as in batch_edge_cases: the copies of a member land in every lane and workgroup slot


def tile(pool, B):
    """The pool repeated cyclically to B rows: row b is pool member b % len(pool)."""
    pool = np.asarray(pool)
    return np.ascontiguousarray(pool[np.arange(B) % len(pool)])


def differing_copies(a, n=POOL):
    """Rows of a tiled result that are not byte-identical to the first copy of their pool member."""
    a = np.ascontiguousarray(a)
    B = a.shape[0]
    raw = a.reshape(B, -1).view(np.uint8)
    return np.flatnonzero(np.any(raw != raw[np.arange(B) % n], axis=1))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# 1. two-site unit cell
# ---------------------------------------------------------------------------------------------------------------------------
CELL_T_GAUGED = (1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10, 1e-11)
CELL_T_UNGAUGED = (1e-4, 1e-6, 1e-7, 1e-9)
CELL_PER_T = 8
CELL_HAAR = 41
CELL_GAP = 0.17                  # 1 - |lambda_2| of T_A1 T_A2 over the whole family
CELL_PIVOT = 1e-10               # direct_fixed_point_d2 is accepted while the largest |1 / pivot| stays below 1e10
CELL_POWER_T = 1e-6              # ungauged cells from here down leave the direct solve
CELL_SMALL_T = 1e-5              # rows with 0 < t <= this: lam_min is rounding noise of either sign, both statuses occur
CELL_BATCHES = (1, 63, 64, 65, 4141)


def near_product_unitaries(rng, D, t, n, gauge=True):
    """The unitaries whose tensors are conditioning_cases.near_product_tensors(rng, D, t, n, gauge): the same draws in the same order."""
    N = 2 * D
    X = rng.standard_normal((n, N, N)) + 1j * rng.standard_normal((n, N, N))
    w, V = np.linalg.eigh((X + X.conj().transpose(0, 2, 1)) / 2)
    U = np.einsum('bij,bj,bkj->bik', V, np.exp(-1j * t * w), V.conj())
    if gauge:
        Gd = O.haar_unitaries(rng, D, n)
        left = np.einsum('bij,st->bisjt', Gd, np.eye(2)).reshape(n, N, N)                    # G x 1_2: row 2 i + s
        right = np.tile(np.eye(N, dtype=complex), (n, 1, 1))
        right[:, :D, :D] = Gd.conj().transpose(0, 2, 1)                                      # blockdiag(G^H, 1_D)
        U = left @ U @ right
    return np.ascontiguousarray(U)


@functools.lru_cache(maxsize=None)
def cell_family():
    """dict(U1, U2 (169, 4, 4), t (0: Haar), gauged), in generation order: the gauged strengths, the ungauged ones, Haar."""
    rng = np.random.default_rng(9200)
    U1, U2, t, gauged = [], [], [], []
    for gauge, ts in ((True, CELL_T_GAUGED), (False, CELL_T_UNGAUGED)):
        for tt in ts:
            U1.append(near_product_unitaries(rng, 2, tt, CELL_PER_T, gauge))
            U2.append(near_product_unitaries(rng, 2, tt, CELL_PER_T, gauge))
            t += [tt] * CELL_PER_T
            gauged += [gauge] * CELL_PER_T
    U1.append(O.haar_unitaries(rng, 4, CELL_HAAR))
    U2.append(O.haar_unitaries(rng, 4, CELL_HAAR))
    t += [0.0] * CELL_HAAR
    gauged += [True] * CELL_HAAR
    out = {'U1': np.ascontiguousarray(np.concatenate(U1)), 'U2': np.ascontiguousarray(np.concatenate(U2)), 't': np.array(t),
           'gauged': np.array(gauged)}
    assert len(out['t']) % 64 != 0
    return _frozen(out)


def cell_reference_mp(A1, A2):
    """(r12, r21, lam_min(r12), lam_min(r21)) of one cell; the environments rounded to complex128."""
    r12, lam12 = CC.reference_mp(O.merge(A1, A2))
    D = A2.shape[1]
    with mp.workdps(CC.MP_DIGITS):
        Amp = [[[mp.mpc(A2[s, i, j]) for j in range(D)] for i in range(D)] for s in range(A2.shape[0])]
        q = CC._mp_apply(Amp, [[mp.mpc(r12[i, j]) for j in range(D)] for i in range(D)], D)
        tr = mp.fsum(q[i][i].real for i in range(D))
        Q = mp.matrix(D, D)
        for i in range(D):
            for j in range(D):
                Q[i, j] = (q[i][j] + q[j][i].conjugate()) / (2 * tr)
        lam = mp.eigh(Q, eigvals_only=True)
        lam21 = float(min(lam[k] for k in range(D)))
        r21 = np.array([[complex(Q[i, j]) for j in range(D)] for i in range(D)])
    return r12, r21, lam12, lam21


@functools.lru_cache(maxsize=None)
def cell_references():
    """dict(r12, r21, lam12, lam21, lam_min = the smaller of the two, E (169, 3), gap, pivot) for the rows of cell_family()."""
    fam = cell_family()
    h = CC.hamiltonian_terms()
    A1s, A2s = O.unitary_to_tensor(fam['U1']), O.unitary_to_tensor(fam['U2'])
    rows = [cell_reference_mp(a1, a2) for a1, a2 in zip(A1s, A2s)]
    E = np.array([[O.two_site_cell_energy_closed(a1, a2, hq, r[0], r[1]) for hq in h] for a1, a2, r in zip(A1s, A2s, rows)])
    gap, pivot = [], []
    for a1, a2 in zip(A1s, A2s):
        T = O.transfer_matrix(O.merge(a1, a2))
        w = np.sort(np.abs(np.linalg.eigvals(T)))
        gap.append(1.0 - w[-2])
        pivot.append(abs(T[0, 0] - 1.0))
    out = {'r12': np.stack([r[0] for r in rows]), 'r21': np.stack([r[1] for r in rows]), 'lam12': np.array([r[2] for r in rows]),
           'lam21': np.array([r[3] for r in rows]), 'E': E, 'gap': np.array(gap), 'pivot': np.array(pivot)}
    out['lam_min'] = np.minimum(out['lam12'], out['lam21'])
    return _frozen(out)


def cell_shuffle():
    return np.random.default_rng(9201).permutation(len(cell_family()['t']))


def cell_pool():
    """41 rows of the family for the batch edges: the first 41 of the shuffle (every kind of row is among them)."""
    return cell_shuffle()[:POOL]


@functools.lru_cache(maxsize=None)
def cell_su_pool():
    """41 rows of the optimiser's 30 parameters (ground_state.py:245: standard normal) -> dict(P, U1, U2 built by the host mirror)."""
    P = np.random.default_rng(9202).standard_normal((POOL, 30))
    return _frozen({'P': P, 'U1': np.stack([G.SU(p[:15], 4) for p in P]), 'U2': np.stack([G.SU(p[15:], 4) for p in P])})


# ---------------------------------------------------------------------------------------------------------------------------
# 2. brick-wall environments
# ---------------------------------------------------------------------------------------------------------------------------
TILT = 1e-6                      # bw_env_kernel: exp((1 - i eps) M), eps = 1e-6
LEAD_SET = 1e-9
PAIR_IM = 1e-3                   # a leading conjugate pair at least this far from the real axis: Im(eta) > 0 is asserted
NILPOTENT = 1e-12
CLOSE = 1e-8
EQUAL = 1e-12
BW_N = 150
BW_GRID_N = 600
BW_BATCHES = (1, 63, 64, 65, 130)


def tilted(w):
    return w.real + TILT * w.imag


def eigenvalues(M):
    """LAPACK's eigenvalues of M; through the real solver if M.imag is exactly zero: conjugate pairs are then exact."""
    M = np.asarray(M)
    return np.linalg.eigvals(M.real) if not np.any(M.imag) else np.linalg.eigvals(M)


def leading_eigenpair(M):
    """The reference's eta[np.argmax(eta)] with the kernel's tie-break: all eigenvalues within 1e-9 of the best under
    Re(lambda) + 1e-6 Im(lambda), best first (the eigenvector is checked by its residual against M, not against LAPACK's)."""
    w = eigenvalues(M)
    key = tilted(w)
    order = np.argsort(-key)
    return w[order][key[order] >= key[order[0]] - LEAD_SET]



def leading_pair_imag(M):
    """|Im| of the leading conjugate pair of a REAL matrix, 0.0 if its leading eigenvalue (largest real part) is real."""
    w = eigenvalues(M)
    k = int(np.argmax(tilted(w)))
    return float(abs(w[k].imag))


def status1_class(M):
    """'nilpotent', 'close' or None: the two situations in which the reference explains a status 1 of bw_env_kernel."""
    M = np.asarray(M)
    if np.linalg.norm(np.linalg.matrix_power(M, 4)) < NILPOTENT:
        return 'nilpotent'
    w = eigenvalues(M)
    order = np.argsort(-tilted(w))
    a, b = w[order[0]], w[order[1]]
    if abs(tilted(a) - tilted(b)) < CLOSE and abs(a - b) > EQUAL:
        return 'close'
    return None


def special_gates():
    """The grid of (d): 1, SWAP, CNOT, reversed CNOT, CZ, H x H, H x 1, X x X, Z x X, iSWAP, sqrt(SWAP)."""
    I, X, Z = np.eye(2), np.array([[0, 1.0], [1.0, 0]]), np.diag([1.0, -1.0])
    H = np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt(2)
    SWAP = np.eye(4)[[0, 2, 1, 3]]
    CNOT = np.eye(4)[[0, 1, 3, 2]]
    RCNOT = np.eye(4)[[0, 3, 2, 1]]
    ISWAP = np.array([[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]])
    SQSWAP = np.array([[1, 0, 0, 0], [0, (1 + 1j) / 2, (1 - 1j) / 2, 0], [0, (1 - 1j) / 2, (1 + 1j) / 2, 0], [0, 0, 0, 1]])
    gates = [np.eye(4), SWAP, CNOT, RCNOT, np.diag([1.0, 1.0, 1.0, -1.0]), np.kron(H, H), np.kron(H, I), np.kron(X, X), np.kron(Z, X), ISWAP,
             SQSWAP]
    return np.stack([np.asarray(g, dtype=complex) for g in gates])


def _dag(U):
    return np.ascontiguousarray(U.conj().transpose(0, 2, 1))


@functools.lru_cache(maxsize=None)
def bw_rows():
    """dict(U1, U2, U1p, U2p (1 062, 4, 4), kind ('a' .. 'd' per row))."""
    from scipy.stats import ortho_group, unitary_group
    n = BW_N
    Oq = ortho_group.rvs(4, size=4 * n, random_state=9308).astype(complex)
    Uq = unitary_group.rvs(4, size=4 * n, random_state=9301)
    Us = unitary_group.rvs(4, size=2 * n, random_state=9302)
    gates = special_gates()
    pick = np.random.default_rng(9303).integers(0, len(gates), size=(BW_GRID_N, 4))
    # the 12 rows of test_brickwall_gpu.test_environment_eigenpair_at_special_unitaries_found_by_the_stress
    Z, X, I = np.diag([1.0, -1.0]), np.array([[0, 1.0], [1.0, 0]]), np.eye(2)
    r1 = np.stack([unitary_group.rvs(4, random_state=100 + s) for s in range(12)])
    r2 = np.stack([unitary_group.rvs(4, random_state=200 + s) for s in range(12)])
    r1p = np.stack([np.kron(Z, X).astype(complex)] * 12)
    r2p = np.stack([np.kron(X, I).astype(complex)] * 12)
    quads = [(Oq[:n], Oq[n:2 * n], Oq[2 * n:3 * n], Oq[3 * n:]), (Uq[:n], Uq[n:2 * n], Uq[2 * n:3 * n], Uq[3 * n:]),
             (Us[:n], Us[n:], _dag(Us[:n]), _dag(Us[n:])), tuple(gates[pick[:, k]] for k in range(4)), (r1, r2, r1p, r2p)]
    kind = np.array(['a'] * n + ['b'] * n + ['c'] * n + ['d'] * (BW_GRID_N + 12))
    out = {name: np.ascontiguousarray(np.concatenate([q[k] for q in quads])) for k, name in enumerate(('U1', 'U2', 'U1p', 'U2p'))}
    out['kind'] = kind
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def bw_matrices(side):
    """The oracle's environment matrices (1 062, 4, 4) of bw_rows(); side 0: right, 1: left.  Real rows come out exactly real."""
    rows = bw_rows()
    fn = BW.left_env_matrix if side else BW.right_env_matrix
    M = np.stack([fn(a, b, c, d) for a, b, c, d in zip(rows['U1'], rows['U2'], rows['U1p'], rows['U2p'])])
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def bw_classes(side):
    """Per row of bw_matrices(side): dict(cls (None / 'nilpotent' / 'close'), pair_im (rows of kind 'a': |Im| of a leading pair))."""
    M, kind = bw_matrices(side), bw_rows()['kind']
    cls = np.array([status1_class(m) for m in M], dtype=object)
    pair = np.array([leading_pair_imag(m) if k == 'a' else 0.0 for m, k in zip(M, kind)])
    return {'cls': cls, 'pair_im': pair}


@functools.lru_cache(maxsize=None)
def bw_pool():
    """41 items for bw_expval and bw_manifold with an operator of their own each: dict(U1, U2, U1p, U2p, O2, O4, Mr, Ml, W) and the oracle's
    values: e2, e4 (per-item operator), ov[(m_shared, w_shared)] (shared: item 0's)."""
    from scipy.stats import unitary_group
    rng = np.random.default_rng(9310)
    U = unitary_group.rvs(4, size=4 * POOL, random_state=9311)

    def cn(*shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    p = {'U1': U[:POOL], 'U2': U[POOL:2 * POOL], 'U1p': U[2 * POOL:3 * POOL], 'U2p': U[3 * POOL:], 'O2': cn(POOL, 4, 4), 'O4': cn(POOL, 16, 16),
         'Mr': cn(POOL, 2, 2), 'Ml': cn(POOL, 2, 2), 'W': unitary_group.rvs(16, size=POOL, random_state=9312)}
    p = {k: np.ascontiguousarray(v) for k, v in p.items()}
    p['e2'] = np.array([BW.exp_val_2(a, b, o) for a, b, o in zip(p['U1'], p['U2'], p['O2'])])
    p['e4'] = np.array([BW.exp_val_4(a, b, o) for a, b, o in zip(p['U1'], p['U2'], p['O4'])])
    for ms in (0, 1):
        for ws in (0, 1):
            p['ov', ms, ws] = np.array([BW.manifold_overlap(p['U1'][k], p['U2'][k], p['U1p'][k], p['U2p'][k], p['Mr'][0 if ms else k],
                                                            p['Ml'][0 if ms else k], p['W'][0 if ws else k]) for k in range(POOL)])
    return _frozen(p)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. SU(N)
# ---------------------------------------------------------------------------------------------------------------------------
SU_N = (4, 8, 16, 32)
SU_SCALES = (1.0, 6.0, 300.0, 1e5)
SU_ROWS = 8
SU_MP_N = (4, 8)
SU_TOL = 1e-12
SU_TENSOR_POOL = 13
SU_TENSOR_BATCHES = (41, 42, 43)         # 4 k + 1, 4 k + 2, 4 k + 3 with k = 10


@functools.lru_cache(maxsize=None)
def su_params(N):
    """dict(P (32, N^2 - 1): row 4 g + k = a standard-normal row times SU_SCALES[k], scale (32,))."""
    rng = np.random.default_rng(9400 + N)
    P = rng.standard_normal((SU_ROWS, len(SU_SCALES), N * N - 1)) * np.array(SU_SCALES)[None, :, None]
    return _frozen({'P': np.ascontiguousarray(P.reshape(-1, N * N - 1)), 'scale': np.tile(SU_SCALES, SU_ROWS)})


def su_reference_mp(p, N):
    """mpmath's expm of the host mirror's generator -i/2 sum_k p_k G_k (its doubles are exact inputs), rounded to complex128."""
    X = -0.5j * np.tensordot(np.asarray(p, dtype=float), G._su_basis(N), axes=1)
    with mp.workdps(CC.MP_DIGITS):
        E = mp.expm(mp.matrix(X.tolist()))
        return np.array([[complex(E[i, j]) for j in range(N)] for i in range(N)])


@functools.lru_cache(maxsize=None)
def su_references(N):
    """Reference unitaries of the rows of su_params(N) with scale 1 and 6 -> (rows, U): mpmath at N = 4, 8, the host mirror (scipy) above."""
    sp = su_params(N)
    rows = np.flatnonzero(sp['scale'] <= 6.0)
    U = np.stack([su_reference_mp(sp['P'][r], N) if N in SU_MP_N else G.SU(sp['P'][r], N) for r in rows])
    U.setflags(write=False)
    return rows, U


@functools.lru_cache(maxsize=None)
def su_tensor_pool(D):
    """13 standard-normal rows of SU(2 D) parameters and the oracle's energies of unitary_to_tensor(SU(p)) per term -> dict(P, E (13, 3))."""
    N = 2 * D
    P = np.random.default_rng(9500 + D).standard_normal((SU_TENSOR_POOL, N * N - 1))
    h = CC.hamiltonian_terms()
    E = []
    for p in P:
        A = np.ascontiguousarray(O.unitary_to_tensor(G.SU(p, N)))
        _, r = O.env_dense_eig(A)
        E.append([O.energy_closed_form(A, hq, r) for hq in h])
    return _frozen({'P': P, 'E': np.array(E)})


@functools.lru_cache(maxsize=None)
def cell_su_mixed():
    """30-parameter rows for cell2_energies_su: dict(P (16, 30), big (rows scaled by 1e5: one in every workgroup of four, at a different slot))."""
    P = np.random.default_rng(9203).standard_normal((16, 30))
    big = np.array([0, 5, 10, 15])
    P[big] *= 1e5
    return _frozen({'P': P, 'big': big})
