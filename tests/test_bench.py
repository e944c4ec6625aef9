"""bench.py's plain run and --dump-outputs: a plain run times exactly --steps steps and carries none of the --full legs; the dump holds
what the last timed step computed, the same for every run with the same arguments (the oracle's energies of the seeded inputs)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_float64_and_seeded_sample(tmp_path, monkeypatch):
    """Every array lands as <name>.npy in float64; beyond the byte cap the per-evaluation arrays are cut to the same fixed sample of rows."""
    bench = _bench_module()
    E = np.arange(3000, dtype=np.float64).reshape(1000, 3)
    it = np.arange(1000, dtype=np.int32)
    bench.dump_outputs(str(tmp_path / 'all'), {'energies': E, 'iterations': it}, {'summed_cost': np.array([1.5])})
    got = {f[:-4]: np.load(tmp_path / 'all' / f) for f in os.listdir(tmp_path / 'all')}
    assert set(got) == {'energies', 'iterations', 'summed_cost'} and all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got['energies'], E) and np.array_equal(got['iterations'], it) and got['summed_cost'][0] == 1.5
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 8 * 1024)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'energies': E, 'iterations': it}, {'summed_cost': np.array([1.5])})
    sizes = sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a'))
    idx = np.load(tmp_path / 'a' / 'sample_index.npy').astype(np.int64)
    assert 0 < len(idx) < 1000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / 'a' / 'energies.npy'), E[idx]) and np.array_equal(np.load(tmp_path / 'a' / 'iterations.npy'), it[idx])
    assert np.array_equal(idx, np.load(tmp_path / 'b' / 'sample_index.npy').astype(np.int64))
    assert sizes < 8 * 1024 + 5 * 128                  # (+ the .npy headers)


def test_dump_outputs_energy_workload_only():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--workload', 'evolve', '--dump-outputs', 'x'],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and 'energy workload only' in out.stderr


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(tmp_path, c_oracle):
    """A plain run: --steps timed steps, the headline fields, none of the --full legs; its dump is the last timed step's window
    (warm-up + timed steps cycle the resident batches) and matches the oracle on the seeded inputs."""
    bench = _bench_module()
    B, R, steps, warmup, seed = 4096, 2, 7, 2, 20241022
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup), '--batch', str(B),
           '--rotate', str(R), '--dump-outputs', str(tmp_path / 'out')]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['steps'] == steps and d['warmup'] == warmup and d['ms_per_step'] > 0 and d['dtype'] == 'f64' and d['higher_is_better'] is True
    assert abs(d['value'] - B * steps / (d['ms_per_step'] * 1e-3 * steps)) < 1e-6 * d['value']
    assert d['repeats']['blocks'] == 1
    for k in ('cpu_baseline', 'other_configs', 'warm_start', 'power_iteration', 'contraction_only', 'pcie_inclusive_evals_per_s'):
        assert k not in d, k
    got = {f[:-4]: np.load(tmp_path / 'out' / f) for f in os.listdir(tmp_path / 'out')}
    assert set(got) == {'energies', 'iterations', 'status', 'summed_cost'} and all(v.dtype == np.float64 for v in got.values())
    last = (warmup + steps - 1) % R
    A = bench.haar_tensors(seed + 1000 * last, 4, B)
    ref = c_oracle.energy_batch(A, bench.tfim_h(1.0))
    E = got['energies'].reshape(B, -1)[:, 0]
    ok = (got['status'] == 0) & (ref['status'] == 0)
    assert ok.mean() > 0.9 and np.abs(E - np.asarray(ref['E']).reshape(B, -1)[:, 0])[ok].max() < 1e-10
    assert abs(got['summed_cost'][0] - E.sum()) < 1e-8 * B
