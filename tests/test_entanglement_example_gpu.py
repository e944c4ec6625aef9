"""GPU: examples/entanglement_entropy.py end to end in a fresh child process - finite entropies within [0, ln D], and the larger bond
dimension holds at least the entanglement of the smaller one at the coupling nearest to the critical point."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import entanglement_cases as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_prints_the_entropy_table():
    lams = ['0.7', '1.0', '1.3']
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'entanglement_entropy.py'), '--couplings', *lams, '--restarts', '8'],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [ln.split() for ln in run.stdout.splitlines() if re.match(r'^\s*\d+\.\d{3}\s', ln)]
    assert [r[0] for r in rows] == ['0.700', '1.000', '1.300'], run.stdout
    table = np.array([[float(x) for x in r] for r in rows])              # lambda, E (D=2), S (D=2), E (D=4), S (D=4)
    assert table.shape == (3, 5) and np.all(np.isfinite(table))
    S2, S4 = table[:, 2], table[:, 4]
    assert np.all(S2 >= 0) and np.all(S2 <= np.log(2) + 1e-8) and np.all(S4 >= 0) and np.all(S4 <= np.log(4) + 1e-8)
    assert S4[1] >= S2[1] - K.entropy_bound(4) - 1e-8                    # (the table is printed to eight digits)
    spectra = [ln for ln in run.stdout.splitlines() if 'Schmidt spectrum at lambda = 1.000' in ln]
    assert len(spectra) == 2 and spectra[0].startswith('D = 2') and spectra[1].startswith('D = 4')
