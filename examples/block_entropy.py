#!/usr/bin/env python3
"""Block entropies, mutual information and a three-site expectation of variational ground states of the transverse-field Ising chain
H = -sum ZZ + lambda sum X:

    python examples/block_entropy.py [--couplings 0.6 0.9 1.1 1.4] [--Ds 2 4] [--restarts 8] [--depth 2]

`ground_state_sweep` minimises every coupling from several restarts in one lock-step BFGS per bond dimension.  `block_entropy` then
rebuilds the best states on the device, solves their environments once, contracts the reduced density matrix of n = 1 .. 4 contiguous
sites in ONE launch and diagonalises it with the Jacobi kernel of `entanglement_entropy`.  Prints, per coupling and bond dimension,

    S(n), n = 1 .. 4     the entropy of a block of n sites; a block has two ends, so S(n) approaches TWICE the half-chain entropy of
                         `entanglement_entropy` (printed beside it) as the block outgrows the correlation length - quickly away from
                         lambda = 1, slowly near it
    I = 2 S(1) - S(2)    the mutual information of neighbouring sites
    <Z X Z>              a three-site expectation from `local_expectation` (the cluster term that goes with the string order of
                         examples/string_order.py)

--depth counts layers PER BOND QUBIT, as in examples/entanglement_entropy.py."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qmps_amd.ground_state import Hamiltonian, block_entropy, entanglement_entropy, ground_state_sweep, local_expectation  # noqa: E402
from qmps_amd.represent import ShallowCNOTStateTensor  # noqa: E402

X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)
ZXZ = np.kron(Z, np.kron(X, Z))          # the left site is the most significant index


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--couplings', type=float, nargs='+', default=[0.6, 0.9, 1.1, 1.4])
    ap.add_argument('--Ds', type=int, nargs='+', default=[2, 4])
    ap.add_argument('--restarts', type=int, default=8)
    ap.add_argument('--depth', type=int, default=2, help='layers per bond qubit: depth * log2(D) layers at bond dimension D')
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args(argv)
    lams = np.asarray(args.couplings, dtype=float)
    terms = [Hamiltonian({'ZZ': -1.0}).to_matrix(), Hamiltonian({'X': 1.0}).to_matrix()]
    out = {'couplings': lams, 'Ds': list(args.Ds), 'params': {}, 'energy': {}, 'S_block': {}, 'S_half': {}, 'mutual': {}, 'zxz': {}, 'status': {}}
    for D in args.Ds:
        layers = args.depth * max(1, int(round(np.log2(D))))
        sweep = ground_state_sweep(terms, np.stack([np.ones_like(lams), lams], axis=1), D=D, depth=layers, state_tensor=ShallowCNOTStateTensor,
                                   restarts=args.restarts, rng=np.random.default_rng(args.seed), maxiter=300)
        prm = sweep['params']
        S_half, _, status = entanglement_entropy(prm, D=D, state_tensor=ShallowCNOTStateTensor)
        S_block = np.stack([block_entropy(prm, n, D=D, state_tensor=ShallowCNOTStateTensor)[0] for n in (1, 2, 3, 4)], axis=1)
        zxz, _ = local_expectation(prm, ZXZ, D=D, state_tensor=ShallowCNOTStateTensor)
        out['params'][D], out['energy'][D], out['status'][D] = prm, sweep['energy'], status
        out['S_block'][D], out['S_half'][D], out['mutual'][D], out['zxz'][D] = S_block, S_half, 2 * S_block[:, 0] - S_block[:, 1], zxz[:, 0].real
    for D in args.Ds:
        print(f'D = {D}   (S(n) <= min(n ln 2, 2 ln D) = ' + ' '.join(f'{min(n * np.log(2), 2 * np.log(D)):.4f}' for n in (1, 2, 3, 4)) + ')')
        print('lambda   E              S(1)        S(2)        S(3)        S(4)        2 S(half)   I(1:1)      <Z X Z>')
        for k, lam in enumerate(lams):
            print(f'{lam:6.3f}   {out["energy"][D][k]:+.8f}   ' + '  '.join(f'{s:.8f}' for s in out['S_block'][D][k])
                  + f'  {2 * out["S_half"][D][k]:.8f}  {out["mutual"][D][k]:.8f}  {out["zxz"][D][k]:+.8f}')
    return out


if __name__ == '__main__':
    main()
