"""GPU: examples/energy_variance.py end to end, its quick setting (D = 2, 4) in a child process: the variance per site is non-negative,
falls with the bond dimension, and belongs to the energy the optimiser of examples/bond_dimension.py reached."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import two_site_sum_cases as T2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quick_setting_in_a_child_process():
    done = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'energy_variance.py'), '--quick', '--json'], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    print(done.stdout)
    out = json.loads(done.stdout.strip().splitlines()[-1])
    rows = out['rows']
    assert [r['D'] for r in rows] == [2, 4] and all(r['status'] == 0 for r in rows)
    assert abs(out['exact'] + 4 / np.pi) < 1e-8                                   # g = 1
    # sigma^2 >= 0 up to the bound: two sums and nine near values for an operator of norm |h| = 2 (the bounds are for unit norm); the
    # resolvent norm at an optimum is far below 1e6 (a gap of 1e-6 would not have converged in the solve)
    granted = 4 * (2 * T2.C_G * T2.EPS * 1e6 + 9 * T2.bound_near())
    assert all(r['variance'] >= -granted for r in rows)
    assert rows[1]['variance'] < rows[0]['variance']                             # strictly better as an eigenstate at D = 4
    for r in rows:
        # the energy of the resident state is the value the bond-dimension optimiser reached, and is variational
        assert abs(r['E'] - r['E_optimiser']) < 1e-9 and r['E'] > out['exact'] - 1e-10 and abs(r['error'] - (r['E'] - out['exact'])) < 1e-12
    assert rows[1]['E'] <= rows[0]['E'] + 1e-9
