"""GPU: examples/correlation_functions.py end to end - the sweep's variational energies against the energy rebuilt from the
correlators, E = -<Z_0 Z_1> + lambda <X>."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_reproduces_the_variational_energy(capsys):
    spec = importlib.util.spec_from_file_location('example_correlation_functions', os.path.join(ROOT, 'examples', 'correlation_functions.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(['--couplings', '0.5', '1.0', '1.5', '--restarts', '4', '--D', '2', '--n-max', '16'])
    assert out['C'].shape == (3, 2, 2, 16) and out['one'].shape == (3, 2) and out['status'].shape == (3,)
    assert out['zz'].shape == (3, 16) and out['zz_connected'].shape == (3, 16) and out['energy_from_correlators'].shape == (3,)
    assert np.all(out['status'] == 0)
    for k in ('C', 'one', 'zz', 'zz_connected', 'energy', 'energy_from_correlators'):
        assert np.all(np.isfinite(out[k])), k
    assert np.abs(out['energy_from_correlators'] - out['energy']).max() < 1e-9
    assert 'lambda' in capsys.readouterr().out
