"""Two-site operators without the symmetries of TFIM / XXZ, and the inputs of the tests that use them (test infrastructure).

Every other `WW` of the suite is the identity or exp(-i dt H) of a real symmetric, exchange-invariant Hamiltonian: it equals
its transpose and itself with the two sites exchanged, so a kernel that read W[t][s], merged the sites as t = t1 + 2 t2 or
conjugated the wrong factor would pass.  `generic_ww` has none of these symmetries; `wrong_variants` are the operators such a
kernel would effectively apply.  tests/test_operator_cases_cpu.py measures, with the oracle alone, how far every variant moves
the quantity a GPU test compares, on exactly the inputs built here; tests/test_generic_operator_gpu.py and the generic-term
rotosolve tests of tests/test_rotosolve_gpu.py then hold the kernels to the oracle on them.

D = 2 says nothing about site order: the dominant eigenvalue of the mixed transfer map - and the two-site energy - of D = 2
tensors is unchanged to rounding by WW -> S WW S (h -> S h S).  The cases at D >= 4 carry that check."""
import functools

import numpy as np
from scipy.linalg import expm

from oracle import qmps_oracle as O

SWAP = np.eye(4)[[0, 2, 1, 3]]
DTS = (0.05, 0.3)                       # a time step, and a larger move
ANSATZ = 0                              # ShallowCNOT, the family of every parameter case
PARAMS = {2: 8, 4: 4, 8: 6, 16: 8}
PLAIN_B = {2: 12, 4: 12, 8: 12, 16: 8}
WW_SEED = {2: 2002, 4: 2004, 8: 2008, 16: 2016}
ROTO_H_SEED = {2: 3002, 8: 3008}
GRADIENT_SEED = {4: 1424, 8: 1408, 16: 1416}      # (1404 at D = 4: an iterate with |eta_2 / eta_1| = 0.984)


def generic_h(seed):
    """A complex Hermitian 4 x 4 matrix of unit spectral norm: (G + G^H) / 2 of a seeded complex Gaussian G."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
    H = (G + G.conj().T) / 2
    return H / np.linalg.norm(H, 2)


def generic_ww(seed, dt):
    return expm(-1j * dt * generic_h(seed))


def wrong_variants(WW):
    """What a kernel with a transposed read, a wrong conjugation or exchanged sites applies instead of WW (or h)."""
    return {'transpose': WW.T.copy(), 'conj': WW.conj(), 'dagger': WW.conj().T.copy(), 'swap': SWAP @ WW @ SWAP}


def spectrum(A, B, WW):
    """(eta, r, |eta_2 / eta_1|) of the map oracle.overlap_eta diagonalises: one dense eigen-solve for all three."""
    C = np.tensordot(WW, O.merge(A, A), [1, 0])
    w, v = np.linalg.eig(O.transfer_matrix(C, O.merge(B, B)))
    order = np.argsort(-np.abs(w))
    D = A.shape[1]
    r = v[:, order[0]].reshape(D, D)
    return w[order[0]], r / np.linalg.norm(r), abs(w[order[1]]) / abs(w[order[0]])


def spectral_ratio(A, B, WW):
    """|eta_2 / eta_1| of a well-separated spectrum: the dense eigen-solve, at D = 16 ARPACK in operator form (k = 2)."""
    D = A.shape[1]
    if D < 16:
        return spectrum(A, B, WW)[2]
    from scipy.sparse.linalg import LinearOperator, eigs
    C = np.tensordot(WW, O.merge(A, A), [1, 0])
    Bh = O.merge(B, B).conj().transpose(0, 2, 1)
    op = LinearOperator((D * D, D * D), matvec=lambda x: np.matmul(np.matmul(C, x.reshape(D, D)), Bh).sum(axis=0).reshape(-1), dtype=complex)
    w = np.sort(np.abs(eigs(op, k=2, which='LM', v0=np.eye(D, dtype=complex).reshape(-1), tol=1e-10, ncv=32, return_eigenvectors=False)))
    return w[0] / w[1]


def tensor(D, p):
    return O.unitary_to_tensor(O.shallow_cnot_unitary(D, p))


@functools.lru_cache(maxsize=None)
def plain_case(D, dt):
    """One Haar reference tensor, PLAIN_B[D] candidates U exp(i eps K) with eps <= 0.12 -> (A, candidates, WW)."""
    rng = np.random.default_rng(1100 + D)
    n = 2 * D
    U = O.haar_unitaries(rng, n, 1)[0]
    cands = []
    for eps in rng.uniform(0.0, 0.12, PLAIN_B[D]):
        G = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        cands.append(O.unitary_to_tensor(U @ expm(1j * eps * (G + G.conj().T) / 2)))
    return O.unitary_to_tensor(U), np.stack(cands), generic_ww(WW_SEED[D], dt)


@functools.lru_cache(maxsize=None)
def refs_case(D):
    """One reference per candidate, both as ansatz parameters -> (reference parameters (8, P), candidate parameters, WW)."""
    rng = np.random.default_rng(1200 + D)
    ref = rng.standard_normal((8, PARAMS[D]))
    return ref, ref + 0.05 * rng.standard_normal(ref.shape), generic_ww(WW_SEED[D] + 1, DTS[0])


@functools.lru_cache(maxsize=None)
def far_case(D):
    """12 Haar candidates unrelated to the reference (crowded spectra: the Krylov fall-back's inputs) -> (A, candidates, WW)."""
    rng = np.random.default_rng(1300 + D)
    A = O.unitary_to_tensor(O.haar_unitaries(rng, 2 * D, 1)[0])
    return A, O.unitary_to_tensor(O.haar_unitaries(rng, 2 * D, 12)), generic_ww(WW_SEED[D] + 2, DTS[1])


@functools.lru_cache(maxsize=None)
def gradient_case(D):
    """T = 6 iterates within 0.05 of their references -> (reference parameters, iterates, WW, three (t, k) components)."""
    rng = np.random.default_rng(GRADIENT_SEED[D])
    P = PARAMS[D]
    ref = rng.standard_normal((6, P))
    X = ref + rng.uniform(-0.05, 0.05, ref.shape)
    return ref, X, generic_ww(WW_SEED[D] + 3, DTS[0]), ((0, 0), (2, P // 2), (5, P - 1))


# the evolve drivers: (D, trajectories, seed); ShallowCNOT with PARAMS[D] angles, WW = generic_ww(., 0.05).  At the start of a time step
# the candidate IS the reference and dt is small: the variants move the objective by 1e-6 .. 1e-5 only - the seeds are the best of
# 24 (D = 16: 10) for the smallest separation over trajectories, points and variants (tests/test_operator_cases_cpu.py)
DRIVER_CASES = {'bfgs_device_d2': (2, 5, 1504), 'bfgs_device_d4': (4, 5, 1514), 'bfgs_device_d16': (16, 4, 1508), 'rotosolve_d4': (4, 3, 1517),
                'lockstep_d8': (8, 4, 1502)}


@functools.lru_cache(maxsize=None)
def driver_case(name):
    """-> (D, start parameters (T, P), WW)"""
    D, T, seed = DRIVER_CASES[name]
    return D, np.random.default_rng(seed).standard_normal((T, PARAMS[D])), generic_ww(WW_SEED[D] + 4, DTS[0])


def roto_hamiltonian(D):
    """The stacked terms of the whole-run rotosolve tests: TFIM and a complex Hermitian term that is neither symmetric nor
    exchange-invariant (D = 8: scaled like the second term of the TFIM / XXZ stack it replaces)."""
    tfim = O.hamiltonian_matrix({'ZZ': -1, 'X': 1})
    g = generic_h(ROTO_H_SEED[D])
    return np.stack([tfim, g]) if D == 2 else np.stack([g, 0.3 * tfim])


# (kind, angles) of the whole-run rotosolve runs; builders of the families the oracle can restate
ROTO_RUNS = {2: ((0, 8), (1, 4), (2, 15)), 8: ((0, 6), (3, 9), (0, 8))}
ROTO_BUILDERS = {0: O.shallow_cnot_unitary, 1: O.shallow_qaoa_unitary, 2: lambda D, p: O.shallow_full_unitary(p), 3: O.shallow_cnot3_unitary}


def roto_start(D, kind, P, R):
    """Start vectors (R, P) of a whole-run rotosolve case (the first rows of a larger R are those of a smaller one)."""
    return np.random.default_rng(3100 + 100 * D + 10 * kind + P).standard_normal((R, P))
