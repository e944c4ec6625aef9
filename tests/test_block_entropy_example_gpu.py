"""GPU: examples/block_entropy.py end to end (its `main`, in this process: the test needs the parameters it found, not only its table) -
block entropies that grow with the block and respect both ceilings, and a three-site expectation that matches the host reference."""
import importlib.util
import os
import re

import numpy as np
import pytest

import block_rdm_cases as K
from oracle import qmps_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the device's environment is a fixed point to the tolerance of its solve, 1e-13, which a transfer gap of 1e-3 or more (these states are
# no critical ones: D <= 4) turns into 1e-10 in r; <Z X Z> sums the 64 elements of rho_3 with weights of modulus 1 or 0
SOLVE_SLACK = 1e-9


def test_example_prints_the_block_entropy_table(capsys):
    spec = importlib.util.spec_from_file_location('block_entropy_example', os.path.join(ROOT, 'examples', 'block_entropy.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(['--couplings', '0.7', '1.3', '--restarts', '4'])
    text = capsys.readouterr().out
    print(text)
    rows = [ln.split() for ln in text.splitlines() if re.match(r'^\s*\d+\.\d{3}\s', ln)]
    assert [r[0] for r in rows] == ['0.700', '1.300'] * 2, text                       # both sides of lambda = 1, D = 2 then D = 4
    table = np.array([[float(x) for x in r] for r in rows])                            # lambda, E, S(1..4), 2 S(half), I, <ZXZ>
    assert table.shape == (4, 9) and np.all(np.isfinite(table))
    for D in (2, 4):
        S, S_half, zxz, prm = out['S_block'][D], out['S_half'][D], out['zxz'][D], out['params'][D]
        assert S.shape == (2, 4) and S_half.shape == (2,)
        slack = np.array([K.entropy_bound(D, n) for n in K.NS])
        assert np.all(np.diff(S, axis=1) >= -slack[1:]), (D, S)                        # S(n) does not decrease with n here
        ceiling = np.array([min(n * np.log(2.0), 2 * np.log(D)) for n in K.NS])
        assert np.all(S >= -slack) and np.all(S <= ceiling + slack), (D, S)
        assert np.all(out['mutual'][D] >= -2 * slack[0] - slack[1])                    # subadditivity: S(2) <= 2 S(1)
        assert np.all(S[:, 3] <= 2 * S_half + SOLVE_SLACK + slack[3])                  # and S(n) stays below the two cuts it makes
        for k in range(2):
            A = np.ascontiguousarray(O.unitary_to_tensor(O.shallow_cnot_unitary(D, prm[k])))
            r = O.env_dense_eig(A)[1]
            want = complex(np.einsum('ts,st->', mod.ZXZ.astype(K.CLD), K.reference_rho(A, r, 3)))
            assert abs(zxz[k] - want.real) <= np.abs(mod.ZXZ).sum() * K.rho_bound(D, 3) + SOLVE_SLACK, (D, k, zxz[k], want)
            # the same value through the two-site table row: printed to eight digits
            assert abs(table[(0 if D == 2 else 2) + k, 8] - zxz[k]) < 1e-8
