"""CPU: the inputs of tests/test_batch_edges_gpu.py (tests/batch_edge_cases.py) - the oracle alone accepts every pool member, the
batches sit where the docstrings say, and every threshold still stands in the source as THRESHOLDS quotes it."""
import os

import numpy as np
import pytest

import batch_edge_cases as BE
import operator_cases as OP
import overlap_cases as OC
import structure_factor_cases as S
from oracle import qmps_oracle as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'qmps_amd', 'csrc')


@pytest.mark.parametrize('D', [4, 8, 16])
def test_haar_pools_meet_no_fall_back(D, c_oracle):
    """41 distinct tensors; the C oracle reports status 0 for every one; smallest gap and most plain power steps as documented."""
    A = BE.haar_pool(D)
    assert A.shape == (BE.POOL, 2, D, D) and len({a.tobytes() for a in A}) == BE.POOL
    ref = c_oracle.energy_batch(A, BE.H2, want_r=True, want_rho=True)
    assert np.all(ref['status'] == 0)
    gap = min(S.gap(a) for a in A)
    print(f'Haar pool D = {D}: smallest gap {gap:.4f}, most plain steps {ref["iters"].max()}')
    assert abs(gap - BE.HAAR_GAP[D]) < 5e-4
    assert abs(int(ref['iters'].max()) - BE.HAAR_STEPS[D]) <= 1


def test_pending_pool_holds_the_slow_tensors_of_the_existing_test():
    """The generator, seed and order of test_energy_gpu.test_d16_environment_krylov_fallback; gaps 3e-3 .. 3e-6: at 30 / gap steps the
    power iteration alone exhausts max_iter = 3 000 on every one of the eight, so all their copies are handed over."""
    pool = BE.pending_pool()
    rng = np.random.default_rng(160)
    slow = np.stack([OC.slow_environment_tensor(rng, 16, t) for t in (0.3, 0.3, 0.1, 0.1, 0.03, 0.03, 0.01, 0.01)])
    assert np.array_equal(pool[:BE.N_SLOW], slow) and np.array_equal(pool[BE.N_SLOW:], BE.haar_pool(16)[:BE.POOL - BE.N_SLOW])
    gaps = np.array([S.gap(a) for a in slow])
    assert np.all(gaps < 4e-3) and np.all(gaps > 2e-6) and np.all(30 / gaps > 3000)
    for a in pool:                                                  # left isometries: the closed form's reference applies
        assert np.abs(np.einsum('sij,sik->jk', a.conj(), a) - np.eye(16)).max() < 1e-12
    for n in BE.PENDING_COPIES:
        assert BE.N_SLOW * n > BE.THRESHOLDS['pending_d16'][2] > BE.THRESHOLDS['pending_krylov'][2]
    two_wave = BE.THRESHOLDS['two_wave_d16'][2]
    assert BE.POOL * BE.PENDING_COPIES[0] <= two_wave < BE.POOL * BE.PENDING_COPIES[1]


@pytest.mark.parametrize('D', [4, 16])
def test_overlap_pools_have_separated_spectra(D):
    """The plain case's candidates first, 41 distinct ones in all, |eta_2 / eta_1| < 0.995 for both operators (D = 4, also with one
    reference per candidate: < 0.96, thirty squarings are far more than 1e-13 needs)."""
    for dt in OP.DTS:
        A, cands, WW = BE.overlap_pool(D, dt)
        A0, c0, WW0 = OP.plain_case(D, dt)
        assert np.array_equal(A, A0) and np.array_equal(cands[:len(c0)], c0) and np.array_equal(WW, WW0)
        assert cands.shape == (BE.POOL, 2, D, D) and len({c.tobytes() for c in cands}) == BE.POOL
        worst = max(OP.spectral_ratio(A, c, WW) for c in cands)
        assert worst < 0.995, worst
        if D == 4:
            R = BE.overlap_pool_references(D, dt)
            assert all(np.array_equal(R[k], cands[(k + 1) % BE.POOL]) for k in range(BE.POOL))
            worst_r = max(OP.spectrum(a, c, WW)[2] for a, c in zip(R, cands))
            assert worst_r < 0.96, worst_r
            # a kernel that took another candidate's reference on its second pass would move eta by far more than the tolerance
            shift = min(abs(O.overlap_eta(R[k], cands[k], WW)[0] - O.overlap_eta(R[(k + 1) % BE.POOL], cands[k], WW)[0]) for k in range(BE.POOL))
            assert shift > 1e-6, shift


@pytest.mark.parametrize('D', [8, 16])
def test_krylov_pools(D):
    """The far candidates of operator_cases.far_case first (crowded spectra), plain ones behind them (|eta_2 / eta_1| < 0.95)."""
    A, cands, WW = BE.krylov_pool(D)
    A0, far, WW0 = OP.far_case(D)
    n = BE.KRYLOV_FAR[D]
    assert np.array_equal(A, A0) and np.array_equal(WW, WW0) and np.array_equal(cands[:n], far[:n])
    assert cands.shape == (BE.POOL, 2, D, D) and len({c.tobytes() for c in cands}) == BE.POOL
    ratios = np.array([OP.spectral_ratio(A, c, WW) for c in cands])
    assert ratios[:n].max() > 0.985 and ratios[n:].max() < 0.95, (ratios[:n], ratios[n:].max())
    assert n + len(cands[n:]) == BE.POOL and (D != 16 or abs(n / BE.POOL - 0.1) < 0.01)       # D = 16: a tenth of the batch


def test_gradient_pool():
    ref, X, noise, WW = BE.gradient_pool()
    assert ref.shape == X.shape == noise.shape == (BE.POOL, BE.GRADIENT_P) and np.abs(X - ref).max() < 0.15
    assert np.abs(WW @ WW.conj().T - np.eye(4)).max() < 1e-14
    assert max(BE.GRADIENT_MEMBERS) < BE.POOL
    P = BE.GRADIENT_P
    small, large = BE.GRADIENT_T
    assert 2 * P * small > BE.THRESHOLDS['gradient_neighbours'][2] and small <= BE.THRESHOLDS['gradient_pair'][2] < large
    assert large * (2 * P + 1) <= 1 << 16                           # the default capacity of engine_factory


def test_every_batch_puts_every_pool_member_past_its_threshold():
    assert BE.POOL == 41 and all(BE.POOL % q for q in range(2, 7)) and BE.MARGIN > BE.POOL
    for row, B in BE.BATCH.items():
        threshold = BE.THRESHOLDS[row][2]
        assert B == threshold + BE.MARGIN and B <= 1 << 16
        assert B % 4 != 0 and B % 8 != 0 and B % 16 != 0                # a ragged last workgroup
        big = BE.tile(np.arange(BE.POOL), B)
        assert big.shape == (B,) and np.array_equal(big[:BE.POOL], np.arange(BE.POOL))
        seen = np.zeros(B, dtype=bool)
        for k in range(BE.POOL):
            rows = BE.copies(k, B)
            assert np.all(big[rows] == k) and rows[-1] >= threshold and rows[0] == k
            seen[rows] = True
        assert seen.all()                                               # no copy is left out of a comparison
    for B in BE.CORRSUM_BATCHES:
        assert B * BE.CORRSUM_N_Z > BE.THRESHOLDS['corrsum_d16'][2]
    assert BE.CORRSUM_BATCHES[1] * BE.CORRSUM_N_Z - BE.THRESHOLDS['corrsum_d16'][2] == 3


def test_differing_copies_sees_one_bit():
    a = BE.tile(np.linspace(0.1, 0.9, BE.POOL), 200).reshape(200, 1) * np.ones((1, 3))
    assert BE.differing_copies(a).size == 0
    a[137, 2] = np.nextafter(a[137, 2], 1.0)
    assert BE.differing_copies(a).tolist() == [137]
    z = np.zeros(100)
    z[50] = -0.0
    assert BE.differing_copies(z).tolist() == [50]


@pytest.mark.parametrize('row', sorted(BE.THRESHOLDS))
def test_threshold_literals_still_stand_in_the_source(row):
    """A retuned cap or switch must fail here rather than quietly leave its loop untested again."""
    name, literal, value, what = BE.THRESHOLDS[row]
    text = open(os.path.join(CSRC, name)).read()
    assert text.count(literal) == 1, f'{name}: "{literal}" ({what}) appears {text.count(literal)} times'
    numbers = [int(x) for x in literal.replace('(', ' ').replace(')', ' ').replace(';', ' ').split() if x.isdigit()]
    assert value in numbers or value in [4 * x for x in numbers], (row, value, numbers)      # (x 4: waves or evaluations per workgroup)
