"""Batches past every grid cap and batch-size switch of the launch code (test infrastructure; tests/test_batch_edges_cpu.py checks all of
it without a GPU, tests/test_batch_edges_gpu.py holds the kernels to it).

The launch code strides (`b += gridDim.x * WAVES`), draws work from counters and changes kernels above a batch size.  Each case here
takes a small POOL of distinct inputs, repeats it cyclically to a batch just past the threshold and lets the oracle evaluate the pool
once: every copy is compared with the reference of its original, and all copies of one pool member with each other, byte for byte -
an evaluation is computed by one wave or one workgroup with the same instruction sequence wherever it sits.  POOL = 41 is prime: the
copies of one member land in every wave slot, every workgroup slot and every pass.  MARGIN = 45 > POOL leaves a ragged last workgroup
and puts at least one copy of every member beyond the threshold.

THRESHOLDS names each threshold by the literal text that sets it in qmps_amd/csrc: a retuned cap fails the CPU test instead of
quietly leaving its loop untested again."""
import functools

import numpy as np
from scipy.linalg import expm

import operator_cases as OP
import overlap_cases as OC
from oracle import qmps_oracle as O

POOL = 41
MARGIN = 45

# row of the table: (source file, literal text, threshold in units of the batch, what it gates)
THRESHOLDS = {
    'energy_d16': ('qmps_energy_d16.hip', 'grid > 4096', 4 * 4096,
                   'energy_mfma_d16_kernel<true> / <false>: 4 096 workgroups x 4 waves, then b += gridDim.x * WAVES'),
    'pending_d16': ('qmps_energy_d16.hip', 'B < 64 ? a.B : 64', 64,
                    'finishing pass energy_mfma_d16x2_kernel<true> (only_pending): 64 workgroups look through the batch'),
    'pending_krylov': ('qmps_overlap_krylov.hip', 'a.env_mode && grid > 32', 32,
                       'environment-mode Krylov launch: 32 workgroups draw the pending evaluations'),
    'two_wave_d16': ('qmps_energy_d16.hip', 'atoll(tuning_knob("QMPS_D16_SPLIT_BELOW")) : 512;', 512,
                     'two-wave main kernel up to 512 evaluations, the one-wave kernel beyond'),
    'direct_d8': ('qmps_capi_energy.hip', 'atoll(tuning_knob("QMPS_D8_FUSE_BELOW")) : 4096;', 4096,
                  'D = 8 direct solve: fused up to 4 096 evaluations, launch_env_direct_d8 + block kernel started from r_in beyond'),
    'corrsum_d16': ('qmps_kernels.h', 'kCorrSumMaxSlabs = 252', 252,
                    'corrsum_global_kernel: at most 252 workgroups, each rebuilding its tiles and its global slab per item'),
    'one_wave_d16': ('qmps_overlap_d16.hip', 'grid > 4096', 4 * 4096,
                     'overlap_mfma_d16_kernel (QMPS_D16_ONE_WAVE): 4 096 workgroups x 4 waves, then a stride'),
    'square_d4': ('qmps_overlap_square.hip', 'grid > 8192', 4 * 8192,
                  'overlap_square_d4_kernel: 8 192 workgroups x 4 evaluations, then a stride'),
    'krylov_chunk': ('qmps_overlap_krylov.hip', 'B <= 4096 ? 1 : 8', 4096,
                     'Krylov fall-back: one candidate per ticket up to 4 096, eight beyond (one LDS basis reused per draw)'),
    'gradient_neighbours': ('qmps_overlap_d16.hip', '< 4096 ? (n_neigh + 3) / 4 : 4096', 4 * 4096,
                            'pair launch: neighbour tensors by 4 096 surplus workgroups x 4 waves, a stride beyond 16 384 neighbours'),
    'gradient_pair': ('qmps_overlap_d16.hip', '< 2048 ? right.B : 2048', 2048,
                      'pair launch: 2 048 workgroups per side, the iterates drawn from two queues beyond'),
}

# the batch of every case that sits MARGIN past its threshold
BATCH = {row: THRESHOLDS[row][2] + MARGIN for row in ('energy_d16', 'direct_d8', 'one_wave_d16', 'square_d4', 'krylov_chunk')}
PENDING_COPIES = (9, 13)                 # B = 369 (two-wave main kernel) and 533 (one-wave main kernel): 72 and 104 pending evaluations
N_SLOW = 8
SLOW_T = (0.3, 0.3, 0.1, 0.1, 0.03, 0.03, 0.01, 0.01)
CORRSUM_ROWS, CORRSUM_N_Z = 5, 3
CORRSUM_BATCHES = (90, 85)               # x 3 points: 270 items, and 255 (exactly three workgroups take a second item)
GRADIENT_T = (1030, 2053)
GRADIENT_P = 8
GRADIENT_MEMBERS = (0, 20, 40)
KRYLOV_FAR = {8: 12, 16: 4}

H2 = np.stack([O.hamiltonian_matrix({'ZZ': -1, 'X': 1}), O.hamiltonian_matrix({'XX': 1, 'YY': 1, 'ZZ': 0.5})])
H2.setflags(write=False)


def tile(pool, B):
    """The pool repeated cyclically to B rows: row b is pool member b % len(pool)."""
    pool = np.asarray(pool)
    return np.ascontiguousarray(pool[np.arange(B) % len(pool)])


def copies(k, B, n=POOL):
    """The rows of a tiled batch of B that hold pool member k."""
    return np.arange(k, B, n)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def haar_pool(D):
    """41 Haar state tensors from default_rng(7100 + D).  The C oracle reports status 0 for every one; the smallest gap 1 - |lambda_2|
    is 0.128 (D = 4), 0.131 (D = 8), 0.220 (D = 16), the most plain power steps 200, 185, 104: none of them meets a fall-back."""
    A = np.ascontiguousarray(O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(7100 + D), 2 * D, POOL)))
    return _frozen(A)


HAAR_GAP = {4: 0.128, 8: 0.131, 16: 0.220}
HAAR_STEPS = {4: 200, 8: 185, 16: 104}


@functools.lru_cache(maxsize=None)
def pending_pool():
    """The eight slow D = 16 tensors of test_energy_gpu.test_d16_environment_krylov_fallback (same generator, same order: every one
    is handed to the Krylov fall-back and comes back through the finishing pass) and the first 33 of haar_pool(16)."""
    rng = np.random.default_rng(160)
    slow = [OC.slow_environment_tensor(rng, 16, t) for t in SLOW_T]
    return _frozen(np.ascontiguousarray(np.stack(slow + list(haar_pool(16)[:POOL - N_SLOW]))))


def near_candidates(A, rng, n):
    """n candidates the way operator_cases.plain_case draws them: U exp(i eps K) with eps <= 0.12 around the unitary of A."""
    D = A.shape[1]
    U = O.tensor_to_unitary(A)
    out = []
    for eps in rng.uniform(0.0, 0.12, n):
        G = rng.standard_normal((2 * D, 2 * D)) + 1j * rng.standard_normal((2 * D, 2 * D))
        out.append(O.unitary_to_tensor(U @ expm(1j * eps * (G + G.conj().T) / 2)))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _plain_padding(D):
    A = OP.plain_case(D, OP.DTS[0])[0]
    return near_candidates(A, np.random.default_rng(7200 + D), POOL - OP.PLAIN_B[D])


@functools.lru_cache(maxsize=None)
def overlap_pool(D, dt):
    """The candidates of operator_cases.plain_case(D, dt) padded to 41 -> (A, candidates, WW); the candidates do not depend on dt."""
    A, cands, WW = OP.plain_case(D, dt)
    return A, _frozen(np.ascontiguousarray(np.concatenate([cands, _plain_padding(D)]))), WW


def overlap_pool_references(D, dt):
    """One reference per candidate: pool member k is compared with candidate k + 1 (all of them near the same Haar tensor)."""
    _, cands, _ = overlap_pool(D, dt)
    return np.ascontiguousarray(np.roll(cands, -1, axis=0))


@functools.lru_cache(maxsize=None)
def krylov_pool(D):
    """KRYLOV_FAR[D] of the Haar-far candidates of operator_cases.far_case(D) - the fall-back's inputs - then plain candidates near its
    reference -> (A, candidates, WW).  D = 8: 12 + 29; D = 16: 4 + 37, a tenth of the batch."""
    A, far, WW = OP.far_case(D)
    n = KRYLOV_FAR[D]
    near = near_candidates(A, np.random.default_rng(7300 + D), POOL - n)
    return A, _frozen(np.ascontiguousarray(np.concatenate([far[:n], near]))), WW


@functools.lru_cache(maxsize=None)
def gradient_pool():
    """41 ShallowCNOT parameter rows at D = 16 -> (references, iterates within 0.03, noise of the warm call, WW of the TFIM step)."""
    rng = np.random.default_rng(7416)
    ref = rng.standard_normal((POOL, GRADIENT_P))
    X = ref + 0.03 * rng.standard_normal(ref.shape)
    noise = rng.standard_normal(ref.shape)
    return _frozen(ref, X, noise) + (expm(-0.05j * O.hamiltonian_matrix({'ZZ': -1.0, 'X': 1.0})),)


def differing_copies(a, n=POOL):
    """Rows of a tiled result that are not byte-identical to the first copy of their pool member (NaN payloads and signed zeros count)."""
    a = np.ascontiguousarray(a)
    B = a.shape[0]
    raw = a.reshape(B, -1).view(np.uint8)
    return np.flatnonzero(np.any(raw != raw[np.arange(B) % n], axis=1))
