"""GPU: the two launch lanes of the fused D = 4 energy kernel (qmps_amd/csrc/qmps_hazard.h, QMPS_LAUNCH_LANES) are invisible in results.
The call sequences of tests/launch_lane_cases.py - windows cycled with a cost per step, the same window twice in a row, a cold launch
that stores its environments then a warm start on them, set_tensors / set_hamiltonian between launches, read-backs with no
synchronisation, a change of the exchange period in mid-sequence, an energy-only launch right behind a fused one, a D = 8 launch
between two D = 4 launches - run here under two lanes and once, in a fresh child process, under one lane: every array they hand back
must be the same, bit for bit.  D = 4, B = 17 and 33 (two and three workgroups, a partial last tile), R = 3 windows."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import launch_lane_cases as LC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def one_lane(path):
    """every sequence at every batch size under QMPS_LAUNCH_LANES=1, in one fresh process: computed once, shared by the tests"""
    done = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'launch_lane_cases.py'), path] + [str(B) for B in LC.BATCHES],
                          env=dict(os.environ, QMPS_LAUNCH_LANES='1'), capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    return dict(np.load(path))


@pytest.fixture(scope='module')
def serial(tmp_path_factory):
    return one_lane(str(tmp_path_factory.mktemp('lanes') / 'one_lane.npz'))


@pytest.mark.parametrize('B', LC.BATCHES)
@pytest.mark.parametrize('name', list(LC.CASES))
def test_two_lanes_return_the_bits_of_one(name, B, serial, monkeypatch):
    monkeypatch.setenv('QMPS_LAUNCH_LANES', '2')
    got = LC.CASES[name](B)
    want = {k[len(f'{name}.B{B}.'):]: v for k, v in serial.items() if k.startswith(f'{name}.B{B}.')}
    assert sorted(got) == sorted(want) and len(got) > 0
    for k in sorted(got):
        assert np.array_equal(np.asarray(got[k]), want[k]), (name, B, k)
    # the sequences computed something: every solve was accepted
    for k in got:
        if '_st' in k or k.startswith('st'):
            assert np.all(np.asarray(got[k]) == 0), (name, B, k)


@pytest.mark.parametrize('B', LC.BATCHES)
def test_every_cost_of_the_cycle_is_the_sum_of_its_window(B, serial):
    """the serial run's costs themselves: step k's summed cost against numpy's sum of the energies of window k mod 3.  |E| <= ||h||_2
    <= 2.5, so numpy's sum of B of them is off by at most B u (2.5 B), u = 2^-53, twice that with the wave's own sum of 16; the
    accumulator adds one fixed-point word per wave of 16 evaluations, of resolution 16 ||h||_F 2^-51 with ||h||_F <= 5."""
    waves = (B + 15) // 16
    tol = (2 * 2.5 * B * B + waves * 16 * 5 * 4) * 2.0 ** -53
    cost = serial[f'cycle.B{B}.cost']
    for k in range(LC.STEPS):
        E = serial[f'cycle.B{B}.read_E{k % LC.R}']
        assert np.abs(cost[k] - E.sum(axis=0)).max() < tol, (B, k, tol)
