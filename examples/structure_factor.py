#!/usr/bin/env python3
"""Static structure factor of variational ground states of the transverse-field Ising chain  H = -sum ZZ + lambda sum X:

    python examples/structure_factor.py [--couplings 0.6 1.0 1.4] [--n-k 9] [--n-max 128] [--restarts 8] [--D 2] [--depth 2]

`ground_state_sweep` minimises every coupling from several restarts in one lock-step BFGS; `structure_factor` then rebuilds the best
states on the device, solves their environments once and obtains  S_zz(k) = sum_n e^(-ikn) (<Z_0 Z_n> - <Z>^2)  for every k from ONE
launch of linear solves - the resolvent of the transfer map with its fixed point projected out, nothing truncated, at a cost that does
not depend on the correlation length.  Prints S_zz(k) on a grid of k in [0, pi] and the susceptibility chi = S_zz(0) per coupling,
beside the same sum truncated at n_max terms of `correlation_functions(..., connected=True)` - the only route without the solve - with
an estimate of what the truncation leaves out."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qmps_amd.ground_state import Hamiltonian, Sz, correlation_functions, ground_state_sweep, structure_factor  # noqa: E402
from qmps_amd.represent import ShallowCNOTStateTensor  # noqa: E402


def truncation_slack(c):
    """What the two-sided sum loses beyond the last term of c (K, n_max): the largest of the last eight terms continued as a geometric
    series with the decay rate of those eight."""
    a = np.abs(c)
    last, first = a[:, -8:].max(axis=1), a[:, -9]
    with np.errstate(all='ignore'):
        rho = np.where(first > 0, (a[:, -1] / first) ** 0.125, 0.0)
    rho = np.clip(np.nan_to_num(rho), 0.0, 0.999)
    return 2.0 * last * rho / (1.0 - rho)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--couplings', type=float, nargs='+', default=[0.6, 1.0, 1.4])
    ap.add_argument('--n-k', type=int, default=9)
    ap.add_argument('--n-max', type=int, default=128)
    ap.add_argument('--restarts', type=int, default=8)
    ap.add_argument('--D', type=int, default=2)
    ap.add_argument('--depth', type=int, default=2)
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args(argv)
    if args.n_max < 9:
        ap.error('--n-max must be at least 9')
    lams = np.asarray(args.couplings, dtype=float)
    k = np.linspace(0.0, np.pi, args.n_k)
    terms = [Hamiltonian({'ZZ': -1.0}).to_matrix(), Hamiltonian({'X': 1.0}).to_matrix()]
    sweep = ground_state_sweep(terms, np.stack([np.ones_like(lams), lams], axis=1), D=args.D, depth=args.depth, state_tensor=ShallowCNOTStateTensor,
                               restarts=args.restarts, rng=np.random.default_rng(args.seed), maxiter=300)
    S, one, status = structure_factor(sweep['params'], Sz, k, D=args.D, state_tensor=ShallowCNOTStateTensor)
    S_zz = S[:, :, 0, 0]
    chi = S_zz[:, 0]
    # the truncated sum: Z^2 = 1 on one site, and c(-n) = c(n) for one operator
    c, _, _ = correlation_functions(sweep['params'], Sz, args.n_max, D=args.D, state_tensor=ShallowCNOTStateTensor, connected=True)
    c = c[:, 0, 0, :]
    n = np.arange(1, args.n_max + 1)
    S_zz_truncated = (1.0 - one[:, 0] ** 2)[:, None] + 2.0 * np.einsum('qn,bn->bq', np.cos(np.outer(k, n)), c)
    slack = truncation_slack(c)
    for b, lam in enumerate(lams):
        print(f'lambda {lam:5.2f}   status {status[b]}   <Z> {one[b, 0].real:+.8f}   chi = S_zz(0) = {chi[b].real:.10f}')
        print(f'   k/pi    S_zz(k)         sum to n = {args.n_max:<5d}  difference (truncation leaves at most {slack[b]:.1e})')
        for q in range(args.n_k):
            print(f'   {k[q] / np.pi:5.3f}   {S_zz[b, q].real:.10f}   {S_zz_truncated[b, q].real:.10f}   {abs(S_zz[b, q] - S_zz_truncated[b, q]):.1e}')
    return {'couplings': lams, 'k': k, 'energy': sweep['energy'], 'params': sweep['params'], 'S': S, 'one': one, 'status': status,
            'S_zz': S_zz, 'chi': chi, 'S_zz_truncated': S_zz_truncated, 'slack': slack}


if __name__ == '__main__':
    main()
