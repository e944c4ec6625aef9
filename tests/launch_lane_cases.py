"""The call sequences of tests/test_launch_lanes_gpu.py: every one on a fresh D = 4 context over R = 3 windows of B evaluations, each
returning what the calls handed back.  The launch lanes (QMPS_LAUNCH_LANES, read when a context is created) must not show in any of it,
so the test runs run_all() under two lanes and, through the command line below, in a fresh process under one, and compares the bits.

    python tests/launch_lane_cases.py OUT.npz B [B ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import qmps_oracle as O  # noqa: E402

R = 3
BATCHES = (17, 33)          # two and three workgroups of 16 evaluations, the last tile partial
STEPS = 12
H_TFIM = O.hamiltonian_matrix({'ZZ': -1, 'X': 1})
H_TWO = np.stack([H_TFIM, O.hamiltonian_matrix({'XX': 1, 'YY': 1, 'ZZ': 0.5})])


def tensors(seed, n, D=4):
    return O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(seed), 2 * D, n))


def engine(B, D=4):
    from qmps_amd import EnergyEngine
    return EnergyEngine(D, R * B)


def windows(eng, B, out, tag, env=False):
    """E, iterations, statuses (and environments) of the three windows, read with no synchronisation in front"""
    for w in reversed(range(R)):
        eng.set_window(w * B)
        out[f'{tag}_E{w}'], out[f'{tag}_it{w}'], out[f'{tag}_st{w}'] = eng.results(B)
        if env:
            out[f'{tag}_r{w}'] = eng.environments(B)
    eng.set_window(0)


def step(eng, B, k, **kw):
    eng.set_window((k % R) * B)
    eng.launch(B, solver='direct', store_env=kw.pop('store_env', False), accumulate_cost=True, **kw)
    eng.cost_launch(B)


def cycle(B):
    """windows 0, 1, 2, 0, .. for 12 steps with cost_launch each: first with nothing read in between, then with every step's cost read"""
    out = {}
    with engine(B) as eng:
        eng.set_tensors(tensors(100 + B, R * B))
        eng.set_hamiltonian(H_TWO)
        for k in range(STEPS):
            step(eng, B, k)
        out['free_cost'] = eng.get_cost()
        windows(eng, B, out, 'free')
        costs = []
        for k in range(STEPS):
            step(eng, B, k)
            costs.append(eng.get_cost())
        out['cost'] = np.stack(costs)
        windows(eng, B, out, 'read')
    return out


def same_window_twice(B):
    out = {}
    with engine(B) as eng:
        A = tensors(200 + B, R * B)
        eng.set_tensors(A)
        eng.set_hamiltonian(H_TFIM)
        eng.set_window(B)
        eng.launch(B, solver='direct', store_env=True)
        eng.launch(B, solver='direct', store_env=True)
        out['E'], out['it'], out['st'] = eng.results(B)
        out['r'] = eng.environments(B)
        step(eng, B, 1)
        step(eng, B, 1)
        out['cost'] = eng.get_cost()
        eng.set_window(B)
        out['E_acc'], out['it_acc'], out['st_acc'] = eng.results(B)
    return out


def cold_then_warm(B):
    """a cold launch that stores its environments, then a warm start on the same window, which reads them"""
    out = {}
    with engine(B) as eng:
        eng.set_tensors(tensors(300 + B, R * B))
        eng.set_hamiltonian(H_TFIM)
        for w in range(R):
            eng.set_window(w * B)
            eng.launch(B, solver='direct', store_env=True)
            eng.launch(B, solver='direct', store_env=(w == 1), warm_start=True)
        windows(eng, B, out, 'warm', env=True)
    return out


def setters_between(B):
    """set_tensors and set_hamiltonian between launches of the same window: each launch sees what was resident when it was issued"""
    out = {}
    with engine(B) as eng:
        A1, A2 = tensors(400 + B, R * B), tensors(401 + B, R * B)
        eng.set_tensors(A1)
        eng.set_hamiltonian(H_TFIM)
        for w in range(R):
            eng.set_window(w * B)
            eng.launch(B, solver='direct', store_env=False)
        eng.set_tensors(A2)
        for w in range(R):
            eng.set_window(w * B)
            eng.launch(B, solver='direct', store_env=False)
        windows(eng, B, out, 'tensors')
        step(eng, B, 0)
        step(eng, B, 1)
        eng.set_hamiltonian(H_TWO)
        step(eng, B, 2)
        step(eng, B, 0)
        out['cost'] = eng.get_cost()
        eng.set_window(2 * B)
        out['E_h'], _, _ = eng.results(B)
        eng.set_window(0)
        out['E_h0'], _, _ = eng.results(B)
    return out


def exchange_period(B):
    """the exchange period changed in mid-sequence: costs of several steps share a group of the ring, positions are cleared out of turn"""
    out = {}
    with engine(B) as eng:
        eng.set_tensors(tensors(500 + B, R * B))
        eng.set_hamiltonian(H_TWO)
        k = 0
        for period, n in ((1, 3), (4, 6), (1, 3), (16, 5), (2, 4)):
            eng.set_exchange_period(period)
            for _ in range(n):
                step(eng, B, k)
                k += 1
            out[f'cost_p{period}_k{k}'] = eng.get_cost()
        windows(eng, B, out, 'end')
    return out


def energy_only_behind(B):
    """launch_energy_only right behind a fused launch of the same window, which stores the environments it reads"""
    out = {}
    with engine(B) as eng:
        eng.set_tensors(tensors(600 + B, R * B))
        eng.set_hamiltonian(H_TWO)
        for w in range(R):
            eng.set_window(w * B)
            eng.launch(B, solver='direct', store_env=True)
            if w != 1:
                eng.launch_energy_only(B)
        windows(eng, B, out, 'only', env=True)
    return out


def other_bond_dimension_between(B):
    """a D = 8 launch, on its own context, between two D = 4 launches"""
    out = {}
    with engine(B) as eng, engine(8, D=8) as eng8:
        eng.set_tensors(tensors(700 + B, R * B))
        eng.set_hamiltonian(H_TFIM)
        eng8.set_tensors(tensors(701 + B, 8, D=8))
        eng8.set_hamiltonian(H_TFIM)
        step(eng, B, 0)
        eng8.launch(8, solver='direct', store_env=True)
        step(eng, B, 1)
        eng8.launch(8, solver='direct', store_env=True, accumulate_cost=True)
        eng8.cost_launch(8)
        step(eng, B, 0)
        out['cost'], out['cost8'] = eng.get_cost(), eng8.get_cost()
        out['E8'], out['it8'], out['st8'] = eng8.results(8)
        for w in range(2):
            eng.set_window(w * B)
            out[f'E{w}'], out[f'it{w}'], out[f'st{w}'] = eng.results(B)
    return out


CASES = {'cycle': cycle, 'same_window_twice': same_window_twice, 'cold_then_warm': cold_then_warm, 'setters_between': setters_between,
         'exchange_period': exchange_period, 'energy_only_behind': energy_only_behind, 'other_bond_dimension_between': other_bond_dimension_between}


def run_all(batches=BATCHES):
    out = {}
    for B in batches:
        for name, case in CASES.items():
            for k, v in case(B).items():
                out[f'{name}.B{B}.{k}'] = np.asarray(v)
    return out


if __name__ == '__main__':
    np.savez(sys.argv[1], **run_all(tuple(int(b) for b in sys.argv[2:]) or BATCHES))
