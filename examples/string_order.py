#!/usr/bin/env python3
"""String order of variational ground states of the transverse-field Ising chain  H = -sum ZZ + lambda sum X:

    python examples/string_order.py [--couplings 0.5 0.8 1.25 2.0] [--n-max 16] [--restarts 8] [--D 2] [--depth 2]

`ground_state_sweep` minimises every coupling from several restarts in one lock-step BFGS; `string_correlators` then rebuilds the best
states on the device, solves their environments once and walks, in ONE kernel launch, every chain with the string X on the sites
between its ends.  Printed per coupling:

  the disorder parameter <X_1 .. X_n> at growing n, beside the exact value of the infinite chain, (1 - lambda^-2)^(1/4) in the
  paramagnetic phase lambda > 1 and 0 in the ordered phase lambda < 1 (it is the order parameter of the paramagnet, dual to <Z_0 Z_n>).
  With the field term +lambda X the spins point along -X, so the string of n sites carries (-1)^n: the column is (-1)^n <X_1 .. X_n>;
  the order-parameter correlator <Z_0 Z_n> (`correlation_functions`, no string);
  the two-point function <c^+_0 c_n> of the Jordan-Wigner fermions  c_j = (prod_(l<j) X_l) (Z_j - iY_j) / 2.

The sign of the site-0 factor: c^+_0 c_n = [(Z_0 + iY_0) / 2] (prod_(l<0) X_l) (prod_(l<n) X_l) [(Z_n - iY_n) / 2]; the two strings
cancel left of site 0 and leave X_0 X_1 .. X_(n-1), so site 0 carries (Z + iY) X / 2.  With Z X = iY and Y X = -iZ this is
(iY + Z) / 2 = +(Z + iY) / 2: the raising operator of the X basis acts only on X = +1, where X is +1.  Hence, with no sign,

    <c^+_0 c_n> = <sigma^+_0 X_1 .. X_(n-1) sigma^-_n>,    sigma^+- = (Z +- iY) / 2,

which is C[sigma^+, sigma^-, n - 1] of `string_correlators` with the string X (at n = 1 there is no string site)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qmps_amd.ground_state import Hamiltonian, Sx, Sy, Sz, correlation_functions, ground_state_sweep, string_correlators  # noqa: E402
from qmps_amd.represent import ShallowCNOTStateTensor  # noqa: E402

SIGMA_UP = (Sz + 1j * Sy) / 2          # sigma^+ of the X basis: c^+ without its string
SIGMA_DOWN = (Sz - 1j * Sy) / 2


def exact_disorder(lam):
    """lim <X_1 .. X_n> of the infinite chain: (1 - lambda^-2)^(1/4) for lambda > 1, 0 for lambda <= 1."""
    lam = np.asarray(lam, dtype=float)
    return np.where(lam > 1, np.abs(1 - 1 / np.maximum(lam, 1e-300) ** 2) ** 0.25, 0.0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--couplings', type=float, nargs='+', default=[0.5, 0.8, 1.25, 2.0])
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
    ops = np.stack([SIGMA_UP, SIGMA_DOWN])
    C, one, disorder, status = string_correlators(sweep['params'], ops, Sx, args.n_max, D=args.D, state_tensor=ShallowCNOTStateTensor)
    fermion = C[:, 0, 1, :]                                     # <c^+_0 c_n>
    Cz, _, status_z = correlation_functions(sweep['params'], Sz, args.n_max, D=args.D, state_tensor=ShallowCNOTStateTensor)
    zz = Cz[:, 0, 0, :].real                                    # <Z_0 Z_n>
    exact = exact_disorder(lams)
    for k, lam in enumerate(lams):
        print(f'lambda {lam:5.2f}   status {status[k]}   E_var {sweep["energy"][k]:+.10f}   exact disorder parameter (n -> inf) {exact[k]:.8f}')
        print('   n    (-1)^n <X_1 .. X_n>   <Z_0 Z_n>     <c+_0 c_n>')
        for n in range(1, args.n_max + 1):
            f = fermion[k, n - 1]
            print(f'   {n:<3d}  {(-1) ** n * disorder[k, n - 1].real:+.8f}           {zz[k, n - 1]:+.8f}   {f.real:+.8f}{f.imag:+.1e}i')
    return {'couplings': lams, 'energy': sweep['energy'], 'params': sweep['params'], 'ops': ops, 'C': C, 'one': one, 'str': disorder, 'fermion': fermion,
            'zz': zz, 'status': np.maximum(status, status_z), 'disorder_exact': exact}


if __name__ == '__main__':
    main()
