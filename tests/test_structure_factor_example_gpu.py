"""GPU: examples/structure_factor.py end to end - S_zz(k) from the resolvent solve against the example's own truncated sum of
connected correlators."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_agrees_with_its_truncated_sum(capsys):
    spec = importlib.util.spec_from_file_location('example_structure_factor', os.path.join(ROOT, 'examples', 'structure_factor.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(['--couplings', '0.6', '1.0', '1.4', '--restarts', '4', '--D', '2', '--n-k', '5', '--n-max', '128'])
    assert out['S'].shape == (3, 5, 1, 1) and out['one'].shape == (3, 1) and out['status'].shape == (3,) and out['k'].shape == (5,)
    assert out['S_zz'].shape == (3, 5) and out['S_zz_truncated'].shape == (3, 5) and out['chi'].shape == (3,) and out['slack'].shape == (3,)
    assert np.all(out['status'] == 0)
    for key in ('S', 'one', 'S_zz', 'S_zz_truncated', 'chi', 'slack', 'energy'):
        assert np.all(np.isfinite(out[key])), key
    assert np.abs(out['chi'].imag).max() < 1e-12 and np.all(out['chi'].real > 0)
    diff = np.abs(out['S_zz'] - out['S_zz_truncated'])
    print('S_zz - truncated sum:', diff.max(axis=1), 'slack', out['slack'])
    assert np.all(diff <= 1e-9 + out['slack'][:, None])
    assert 'chi' in capsys.readouterr().out
