#!/usr/bin/env python3
"""Wave timeline of the fused D = 4 direct-solve energy kernel: where a SIMD's time goes between its waves.

usage: python tools/wave_timeline.py run [--batch B] [--rotate R] [--reps N] [--out PREFIX]     (needs a GPU)
       python tools/wave_timeline.py reduce DUMP.npy [--tick-ns 10]

`run` needs a library built with the stamps (make -C qmps_amd/csrc EXTRA=-DQMPS_WAVE_TIMELINE in a build directory of its own, passed
in QMPS_HIP_LIB): it sets up the benchmark's headline step (Haar tensors, TFIM, cold start, R rotating windows so that the tensors come from
HBM), asks qmps_wave_timeline for the record of one launch per window and reduces the last one; PREFIX.npy keeps the dump,
PREFIX.json the summary.  Next to the stamped launches it times the same launches unstamped (the buffer pointer null: the stamps'
branches stay) - and, run once more with a plain library (`--plain`), the launches of that library - between HIP events: how much
the stamps perturb the step.

The record (qmps_amd/csrc/qmps_timeline.hip; the words: kTl* in qmps_kernels.h): per wave its workgroup, HW_ID, XCC_ID, the constant-rate clock (100 MHz) at
entry, behind the tile's barrier, behind build, solve, acceptance, density and at the end, and the core clock at entry and end.
HW_ID (gfx9 layout): wave slot [3:0], SIMD [5:4], CU [11:8], shader array [12], shader engine [15:13]; a SIMD is (XCC, SE, SA, CU,
SIMD).  `reduce` gives, per SIMD and over the chip:
  time to first compute      first barrier passed on the SIMD, from the first entry of the launch
  residency                  time the SIMD spends with 0 / 1 / 2 (or more) waves past their barrier, up to its own finish
  lone tail                  the last stretch of the SIMD with one wave left
  phases                     duration of every phase of a wave while it is the older / the younger of a pair / alone (the role that
                             covers most of the phase), medians
  finish spread              how long before the end of the launch the SIMDs finish
  clock                      core-clock ticks per constant-rate tick: the frequency under this kernel
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK, HW_ID, XCC_ID, ENTRY, TILE, BUILD, SOLVE, ACCEPT, DENSITY, END, CYC0, CYC1, RAISED = range(13)
PHASES = [('load', ENTRY, TILE), ('build', TILE, BUILD), ('solve', BUILD, SOLVE), ('accept', SOLVE, ACCEPT),
          ('density', ACCEPT, DENSITY), ('energy+store', DENSITY, END)]


def simd_key(rec):
    hw = rec[:, HW_ID].astype(np.int64)
    return (rec[:, XCC_ID].astype(np.int64) & 0xF) << 16 | (hw & 0xFF00) | (hw & 0x30)


def stats(v, scale=1.0):
    v = np.asarray(v, dtype=float) * scale
    if v.size == 0:
        return None
    return {'median': round(float(np.median(v)), 3), 'p10': round(float(np.percentile(v, 10)), 3), 'p90': round(float(np.percentile(v, 90)), 3),
            'min': round(float(v.min()), 3), 'max': round(float(v.max()), 3), 'mean': round(float(v.mean()), 3)}


def overlap(a0, a1, b0, b1):
    return max(0, min(a1, b1) - max(a0, b0))


def reduce(rec, tick_ns=10.0):
    rec = np.asarray(rec, dtype=np.uint64).astype(np.int64)
    us = tick_ns * 1e-3
    t0, t_end = int(rec[:, ENTRY].min()), int(rec[:, END].max())
    keys = simd_key(rec)
    order = np.argsort(keys, kind='stable')
    bounds = np.flatnonzero(np.diff(keys[order])) + 1
    groups = np.split(order, bounds)
    first, lone, finish, res = [], [], [], {0: [], 1: [], 2: []}
    role_phase = {r: {n: [] for n, _, _ in PHASES} for r in ('older', 'younger', 'alone')}
    whole = {r: [] for r in ('older', 'younger', 'alone')}
    for g in groups:
        w = rec[g]
        w = w[np.argsort(w[:, ENTRY], kind='stable')]
        first.append(int(w[:, TILE].min()) - t0)
        fin = int(w[:, END].max())
        finish.append(t_end - fin)
        # residency: sweep over the barrier-passed intervals [TILE, END)
        ev = sorted([(int(x[TILE]), 1) for x in w] + [(int(x[END]), -1) for x in w])
        level, at, spent = 0, t0, {0: 0, 1: 0, 2: 0}
        for t, d in ev:
            spent[min(level, 2)] += t - at
            level, at = level + d, t
        for k in spent:
            res[k].append(spent[k])
        ends = np.sort(w[:, END])
        last = w[np.argmax(w[:, END])]
        lone.append(fin - max(int(ends[-2]), int(last[TILE])) if len(w) > 1 else fin - int(last[TILE]))
        for i, x in enumerate(w):
            def share(a, b):
                older = younger = 0       # time of [a, b) this wave shares with a partner that entered later / earlier
                for j, y in enumerate(w):
                    if j != i:
                        o = overlap(a, b, int(y[TILE]), int(y[END]))
                        if j > i:
                            older += o
                        else:
                            younger += o
                alone = max(0, (b - a) - older - younger)
                return max((older, 'older'), (younger, 'younger'), (alone, 'alone'))[1]
            for n, a, b in PHASES:
                if x[a] and x[b]:
                    role_phase[share(int(x[a]), int(x[b]))][n].append(int(x[b]) - int(x[a]))
            whole[share(int(x[TILE]), int(x[END]))].append(int(x[END]) - int(x[TILE]))
    dt = (rec[:, END] - rec[:, ENTRY]).astype(float)
    mhz = (rec[:, CYC1] - rec[:, CYC0]) / np.maximum(dt, 1.0) / tick_ns * 1e3
    per_simd = np.array([len(g) for g in groups])
    span = (t_end - t0) * us
    tot = {k: float(np.sum(res[k])) for k in res}
    out = {
        'waves': int(len(rec)), 'simds': int(len(groups)),
        'waves_per_simd': {str(k): int((per_simd == k).sum()) for k in np.unique(per_simd)},
        'raised_waves': int(rec[:, RAISED].sum()),
        'tick_ns': tick_ns,
        'launch_span_us': round(span, 3),
        'entry_spread_us': stats(rec[:, ENTRY] - t0, us),
        'first_entry_per_xcc_us': {str(int(x)): round(float((rec[rec[:, XCC_ID] == x, ENTRY].min() - t0) * us), 3) for x in np.unique(rec[:, XCC_ID])},
        'time_to_first_compute_us': stats(first, us),
        'residency_per_simd_us': {f'{k}_waves_past_barrier': stats(res[k], us) for k in res},
        'residency_share_of_simd_time': {f'{k}_waves_past_barrier': round(tot[k] / max(sum(tot.values()), 1.0), 4) for k in tot},
        'lone_tail_us': stats(lone, us),
        'simd_finish_before_launch_end_us': stats(finish, us),
        'wave_barrier_to_end_us': {r: stats(whole[r], us) for r in whole},
        'waves_by_role': {r: len(whole[r]) for r in whole},
        'phase_us_median': {r: {n: (round(float(np.median(v)) * us, 3) if v else None) for n, v in role_phase[r].items()} for r in role_phase},
        'phase_counts': {r: {n: len(v) for n, v in role_phase[r].items()} for r in role_phase},
        'core_clock_mhz': stats(mhz),
    }
    return out


def stamped_launches(eng, B, reps, max_iter=10000, tol=1e-13):
    """qmps_wave_timeline of a library built with -DQMPS_WAVE_TIMELINE (qmps_amd/csrc/qmps_timeline.hip; bound here by name - it is no part of
    the C-ABI): (record (waves, 16) uint64 of the last of `reps` launches over the window, microseconds per launch between HIP events).
    The launches are the benchmark's: direct solve, no environments stored, cost accumulated in the kernel."""
    import ctypes
    from qmps_amd import _lib as L
    lib = L.load()
    if not hasattr(lib, 'qmps_wave_timeline'):
        sys.exit('wave_timeline.py: the library has no stamps - build it with make -C qmps_amd/csrc EXTRA=-DQMPS_WAVE_TIMELINE (a build directory of its own) and pass it in QMPS_HIP_LIB')
    fn = lib.qmps_wave_timeline
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    words = np.zeros(((B + 15) // 16, 16), dtype=np.uint64)
    us = ctypes.c_double(0)
    L.check(fn(eng._ctx, B, int(max_iter), float(tol), L.ENV_DIRECT | L.FLAG_NO_ENV_OUT | L.FLAG_ACCUMULATE_COST, int(reps),
               words.ctypes.data_as(ctypes.c_void_p), ctypes.byref(us)))
    return words, us.value


def run(a):
    from benchlib.common import haar_tensors, tfim_h
    from qmps_amd import EnergyEngine
    B, R = a.batch, a.rotate
    A = np.concatenate([haar_tensors(a.seed + 1000 * k, 4, B) for k in range(R)])
    eng = EnergyEngine(4, R * B)
    eng.set_tensors(A)
    eng.set_hamiltonian(tfim_h(1.0))

    def plain(n, rotate):
        eng.sync()
        eng.timer_begin()
        for k in range(n):
            eng.set_window((k % R) * B if rotate else 0)
            eng.launch(B, store_env=False, accumulate_cost=True)
            eng.cost_launch(B)
        return 1e3 * eng.timer_end() / n

    t = eng.probe_fp64_tflops()       # (settles the clocks, as bench.py does)
    plain(450, True)
    out = {'batch': B, 'rotate': R, 'reps': a.reps, 'fp64_probe_tflops': round(t, 2)}
    out['us_per_launch_rotating_windows'] = [round(plain(a.reps * R, True), 3) for _ in range(3)]
    # stamped against unstamped: `reps` launches back to back over ONE window, timed the same way on both sides, alternating
    out['us_per_launch_one_window_unstamped'], out['us_per_launch_one_window_stamped'] = [], []
    eng.set_window(0)
    for _ in range(5):
        out['us_per_launch_one_window_unstamped'].append(round(plain(a.reps * R, False), 3))
        if not a.plain:
            out['us_per_launch_one_window_stamped'].append(round(stamped_launches(eng, B, a.reps * R)[1], 3))
    if not a.plain:
        # the record: one stamped launch per window, in turn (the tensors of a window have left the caches when its turn comes again)
        rec = None
        for k in range(2 * R):
            eng.set_window((k % R) * B)
            rec, _ = stamped_launches(eng, B, 1)
        eng.set_window(0)
        out['summary'] = reduce(rec, a.tick_ns)
        if a.out:
            np.save(a.out + '.npy', rec)
    eng.close()
    if a.out:
        with open(a.out + '.json', 'w') as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    r = sub.add_parser('run')
    r.add_argument('--batch', type=int, default=65536)
    r.add_argument('--rotate', type=int, default=9)
    r.add_argument('--reps', type=int, default=20, help='launches per window and timing block')
    r.add_argument('--seed', type=int, default=20241022)
    r.add_argument('--tick-ns', type=float, default=10.0)
    r.add_argument('--plain', action='store_true', help='time the launches only (a library without the stamps)')
    r.add_argument('--out', default=None)
    d = sub.add_parser('reduce')
    d.add_argument('dump')
    d.add_argument('--tick-ns', type=float, default=10.0)
    a = ap.parse_args()
    if a.cmd == 'run':
        return run(a)
    print(json.dumps(reduce(np.load(a.dump), a.tick_ns), indent=1))
    return 0


if __name__ == '__main__':
    sys.exit(main())
