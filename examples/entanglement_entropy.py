#!/usr/bin/env python3
"""Entanglement entropy of variational ground states of the transverse-field Ising chain  H = -sum ZZ + lambda sum X:

    python examples/entanglement_entropy.py [--couplings 0.6 0.9 1.0 1.1 1.4] [--Ds 2 4] [--restarts 8] [--depth 2]

`ground_state_sweep` minimises every coupling from several restarts in one lock-step BFGS per bond dimension; `entanglement_entropy`
then rebuilds the best states on the device, solves their environments once and diagonalises them where they are in ONE launch of
the Jacobi kernel.  Prints S(lambda) of the half-chain cut per bond dimension (a matrix-product state of bond dimension D holds at
most ln D; the entropy peaks near the critical point lambda = 1) and the Schmidt spectrum at the coupling nearest to it.

--depth counts layers PER BOND QUBIT: the circuit of bond dimension D gets depth * log2(D) layers (2 angles each).  At equal depth the
three-qubit circuit of D = 4 has fewer angles per qubit than the two-qubit one of D = 2 and is the poorer family: its optimum at the
critical point lies higher in energy and holds less entanglement (figures in profiles/EXPERIMENTS.md)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qmps_amd.ground_state import Hamiltonian, entanglement_entropy, ground_state_sweep  # noqa: E402
from qmps_amd.represent import ShallowCNOTStateTensor  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--couplings', type=float, nargs='+', default=[0.6, 0.9, 1.0, 1.1, 1.4])
    ap.add_argument('--Ds', type=int, nargs='+', default=[2, 4])
    ap.add_argument('--restarts', type=int, default=8)
    ap.add_argument('--depth', type=int, default=2, help='layers per bond qubit: depth * log2(D) layers at bond dimension D')
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args(argv)
    lams = np.asarray(args.couplings, dtype=float)
    terms = [Hamiltonian({'ZZ': -1.0}).to_matrix(), Hamiltonian({'X': 1.0}).to_matrix()]
    critical = int(np.abs(lams - 1.0).argmin())
    out = {'couplings': lams, 'critical': critical, 'Ds': list(args.Ds), 'energy': {}, 'S': {}, 'p': {}, 'status': {}}
    for D in args.Ds:
        layers = args.depth * max(1, int(round(np.log2(D))))
        sweep = ground_state_sweep(terms, np.stack([np.ones_like(lams), lams], axis=1), D=D, depth=layers, state_tensor=ShallowCNOTStateTensor,
                                   restarts=args.restarts, rng=np.random.default_rng(args.seed), maxiter=300)
        S, p, status = entanglement_entropy(sweep['params'], D=D, state_tensor=ShallowCNOTStateTensor)
        out['energy'][D], out['S'][D], out['p'][D], out['status'][D] = sweep['energy'], S, p, status
    print('lambda   ' + '   '.join(f'E (D={D})      S (D={D})' for D in args.Ds))
    for k, lam in enumerate(lams):
        print(f'{lam:6.3f}   ' + '   '.join(f'{out["energy"][D][k]:+.8f}  {out["S"][D][k]:.8f}' for D in args.Ds))
    for D in args.Ds:
        print(f'D = {D}: Schmidt spectrum at lambda = {lams[critical]:.3f}: ' + ' '.join(f'{x:.3e}' for x in out['p'][D][critical])
              + f'   (S = {out["S"][D][critical]:.6f} of at most ln D = {np.log(D):.6f})')
    return out


if __name__ == '__main__':
    main()
