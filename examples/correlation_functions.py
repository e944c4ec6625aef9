#!/usr/bin/env python3
"""Two-point functions of variational ground states of the transverse-field Ising chain  H = -sum ZZ + lambda sum X:

    python examples/correlation_functions.py [--couplings 0.5 1.0 1.5] [--n-max 16] [--restarts 8] [--D 2] [--depth 2]

`ground_state_sweep` minimises every coupling from several restarts in one lock-step BFGS; `correlation_functions` then rebuilds the
best states on the device, solves their environments once and walks all chains  <O_a(site 0) O_c(site n)>, n = 1 .. n_max, in ONE
kernel launch.  Prints, per coupling, <X>, <Z>, the order-parameter correlator <Z_0 Z_n> with its connected part, and the identity
E = -<Z_0 Z_1> + lambda <X> beside the variational energy."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qmps_amd.ground_state import Hamiltonian, Sx, Sz, correlation_functions, ground_state_sweep  # noqa: E402
from qmps_amd.represent import ShallowCNOTStateTensor  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--couplings', type=float, nargs='+', default=[0.5, 1.0, 1.5])
    ap.add_argument('--n-max', type=int, default=16)
    ap.add_argument('--restarts', type=int, default=8)
    ap.add_argument('--D', type=int, default=2)
    ap.add_argument('--depth', type=int, default=2)
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args(argv)
    lams = np.asarray(args.couplings, dtype=float)
    terms = [Hamiltonian({'ZZ': -1.0}).to_matrix(), Hamiltonian({'X': 1.0}).to_matrix()]
    sweep = ground_state_sweep(terms, np.stack([np.ones_like(lams), lams], axis=1), D=args.D, depth=args.depth, state_tensor=ShallowCNOTStateTensor,
                               restarts=args.restarts, rng=np.random.default_rng(args.seed), maxiter=300)
    ops = np.stack([Sx, Sz])
    C, one, status = correlation_functions(sweep['params'], ops, args.n_max, D=args.D, state_tensor=ShallowCNOTStateTensor)
    zz = C[:, 1, 1, :].real                                     # <Z_0 Z_n>
    zz_connected = zz - (one[:, 1] * one[:, 1]).real[:, None]
    energy_from_correlators = -zz[:, 0] + lams * one[:, 0].real
    for k, lam in enumerate(lams):
        print(f'lambda {lam:5.2f}   status {status[k]}   <X> {one[k, 0].real:+.8f}   <Z> {one[k, 1].real:+.8f}')
        print(f'   E_var {sweep["energy"][k]:+.10f}   -<Z_0 Z_1> + lambda <X> {energy_from_correlators[k]:+.10f}   difference {sweep["energy"][k] - energy_from_correlators[k]:+.1e}')
        print('   n    <Z_0 Z_n>     connected')
        for n in range(1, args.n_max + 1):
            print(f'   {n:<3d}  {zz[k, n - 1]:+.8f}   {zz_connected[k, n - 1]:+.3e}')
    return {'couplings': lams, 'energy': sweep['energy'], 'params': sweep['params'], 'C': C, 'one': one, 'status': status, 'zz': zz,
            'zz_connected': zz_connected, 'energy_from_correlators': energy_from_correlators}


if __name__ == '__main__':
    main()
