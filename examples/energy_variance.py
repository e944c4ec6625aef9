#!/usr/bin/env python3
"""Energy variance per site against bond dimension - how good a variational state is as an eigenstate, which the energy alone does
not say.  The transverse-field Ising chain H = sum -ZZ + g X at one coupling, optimised in the manner of examples/bond_dimension.py
(full SU(2D) parameterisation at D = 2, 4, 8, every optimum embedded as the starting point of the next bond dimension):

    python examples/energy_variance.py [--g 1.0] [--Ds 2 4 8] [--maxiter 150] [--quick] [--json]

For every D it prints the energy per site E, its error against the exact value -(1/pi) int_0^pi sqrt(1 + g^2 - 2 g cos k) dk, and

    sigma^2 = lim (<H^2> - <H>^2) / N = sum_n <dh(0,1) dh(n,n+1)> = S_hh(k = 0),

the structure factor of the energy density at zero momentum, from ONE resolvent solve on the device (`EnergyEngine.energy_variance`,
qmps_correlator_sums_two_site): nothing is truncated, and sigma^2 = 0 exactly on eigenstates.  The error of E is second order in the
distance to the ground state, sigma^2 is the measure of that distance itself: it is the stopping and extrapolation variable of a sweep
over D.  --quick: D = 2, 4, each run to convergence (at most 1000 iterations; a second on one device - what the test runs: an optimiser
stopped early at D = 4 has the lower energy but not yet the lower variance); --json: one JSON line with the table at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qmps_amd import EnergyEngine  # noqa: E402
from qmps_amd.ground_state import SU, Hamiltonian, NonSparseFullEnergyOptimizer, embed_bond_dimension  # noqa: E402


def exact_energy(g, n=20001):
    k = np.linspace(0.0, np.pi, n)
    f = np.sqrt(1 + g * g - 2 * g * np.cos(k))
    return -float(np.sum((f[1:] + f[:-1]) / 2) * (k[1] - k[0])) / np.pi


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--g', type=float, default=1.0)
    ap.add_argument('--Ds', type=int, nargs='+', default=[2, 4, 8])
    ap.add_argument('--maxiter', type=int, default=150)
    ap.add_argument('--seed', type=int, default=2)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--json', action='store_true')
    args = ap.parse_args(argv)
    if args.quick:
        args.Ds, args.maxiter = [2, 4], 1000
    h = Hamiltonian({'ZZ': -1.0, 'X': args.g}).to_matrix()
    e0 = exact_energy(args.g)
    rng = np.random.default_rng(args.seed)
    guess, rows = None, []
    for D in args.Ds:
        x0 = rng.standard_normal((2 * D) ** 2 - 1) if guess is None else guess
        opt = NonSparseFullEnergyOptimizer(h, D, initial_guess=x0)
        opt.change_settings({'verbose': False, 'store_values': False, 'maxiter': args.maxiter, 'tol': 1e-7})
        t0 = time.perf_counter()
        res = opt.optimize_restarts(x0[None], method='BFGS')[0]
        # the optimum made resident once more: its energy from the stored environment, and the variance from the same state
        with EnergyEngine(D, 1) as eng:
            E, _, st = eng.energies(SU(res.x, 2 * D)[None], h, kind='unitary')
            var = eng.energy_variance(B=1)
        rows.append({'D': D, 'E': float(E[0].sum()), 'E_optimiser': float(res.fun), 'error': float(E[0].sum() - e0), 'variance': float(var[0, 0]),
                     'status': int(st[0]), 'nit': int(res.nit), 'seconds': time.perf_counter() - t0})
        print(f'D = {D:2d}: E = {rows[-1]["E"]:+.8f}  E - exact = {rows[-1]["error"]:.2e}  sigma^2 per site = {rows[-1]["variance"]:.3e}  '
              f'({res.nit} BFGS iterations, {rows[-1]["seconds"]:.1f} s)')
        guess = embed_bond_dimension(res.x)
    out = {'g': args.g, 'exact': e0, 'rows': rows}
    if args.json:
        print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
