#!/usr/bin/env python3
"""Static instruction mix of the fused D = 4 direct-solve energy kernel, phase by phase.

usage: python tools/isa_mix.py [--asm FILE.s] [--kernel MANGLED_NAME] [--all]

Without --asm, qmps_amd/csrc/qmps_direct.hip is cross-compiled for gfx950 with -save-temps (the Makefile's flags) into a
temporary directory and its device assembly is read.  The kernel body (default energy_direct_d4_kernel<-1, false>, the
benchmark's) is cut into phases at the sched_barrier fences of qmps_direct_core.h / qmps_direct.hip and, per phase, the
f64 VALU, DPP moves, v_cndmask, ds_read and s_nop instructions are counted, with every VALU instruction as the total.
Counts are static (one pass over the text); the rare phases (the fall-back with its hand-over of the site factors; in older
sources the density of an r that is not positive definite) are code that the common path branches over, and "common path" is
the total without them.  The compiler moves arithmetic whose result is read late (the LDL^H pivots: only the status reads them)
down to its reader, across the fences: compare totals rather than single phases.
The staging fences inside a phase (QMPS_STAGE_FENCE: a sched_barrier behind a mark in the text) are no phase boundaries; tools/lds_cover.py
reads the same phases for the LDS waits.
--all lists the register and scratch use of every energy_direct_d4_kernel / energy_only_d4_kernel instantiation.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'qmps_amd', 'csrc')
DEFAULT_KERNEL = '_ZN4qmps23energy_direct_d4_kernelILin1ELb0EEEvNS_8LaneArgsE'
# the fences of the cold-start kernel, in order (qmps_direct.hip: energy_direct_d4_kernel)
PHASES = ['load+build', 'solve', 'accept', 'fallback', 'density', 'energy']
# sources whose density went through the LDL^H factors, with a branch of its own for an r that is not positive definite
PHASES_LDL = ['load+build', 'solve', 'accept', 'fallback', 'density', 'density not-PD', 'energy']
# sources before the density route had its own fences: density and energy in one phase
PHASES_OLD = ['load+build', 'solve', 'accept', 'fallback', 'density+energy']
RARE = ['fallback', 'density not-PD']     # branches the common path skips
FENCE = re.compile(r';\s*sched_barrier mask\(0x0+\)')
STAGE_MARK = 'qmps_stage_fence'
COLS = ['f64', 'dpp', 'cndmask', 'ds_read', 's_nop', 'valu']


def compile_asm(tmp):
    cmd = ['/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else 'hipcc', '--offload-arch=gfx950', '-O3',
           '-std=c++17', '-fPIC', '-I' + CSRC, '-I' + os.path.join(ROOT, 'include'), '-Wno-unused-function',
           '-save-temps', '-c', os.path.join(CSRC, 'qmps_direct.hip'), '-o', os.path.join(tmp, 'qmps_direct.o')]
    subprocess.check_call(cmd, cwd=tmp)
    return os.path.join(tmp, 'qmps_direct-hip-amdgcn-amd-amdhsa-gfx950.s')


def body(lines, name):
    """the kernel's instruction lines (label to .Lfunc_end) and its resource comments"""
    start = next(i for i, ln in enumerate(lines) if ln.split(';')[0].strip() == name + ':')
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    res = {}
    for ln in lines[end:end + 60]:
        m = re.match(r';\s*(NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy):\s*(\d+)', ln)
        if m:
            res[m.group(1)] = int(m.group(2))
    return lines[start + 1:end], res


def classify(op):
    """the columns an instruction counts in"""
    out = []
    if op.startswith('v_'):
        out.append('valu')
        if '_f64' in op:
            out.append('f64')
        if op.startswith('v_mov_b32_dpp') or op.startswith('v_mov_b64_dpp'):
            out.append('dpp')
        if op.startswith('v_cndmask'):
            out.append('cndmask')
    elif op.startswith('ds_read'):
        out.append('ds_read')
    elif op == 's_nop':
        out.append('s_nop')
    return out


def is_phase_fence(text, n):
    """line n is a fence between two phases: a sched_barrier that is not a staging fence (QMPS_STAGE_FENCE of qmps_direct_core.h, which
    writes STAGE_MARK into the text in front of its sched_barrier: a fence inside a phase, between a block's requests and arithmetic)"""
    if not FENCE.match(text[n].strip()):
        return False
    # (the mark and its sched_barrier keep their order - both have side effects - but other instructions may stand between them: the
    # nearest fence or mark above decides)
    for back in range(n - 1, -1, -1):
        s = text[back].strip()
        if STAGE_MARK in s:
            return False
        if FENCE.match(s):
            break
    return True


def phase_names(n_phases):
    return next((n for n in (PHASES, PHASES_LDL, PHASES_OLD) if len(n) == n_phases), [f'phase {i}' for i in range(n_phases)])


def mix(text):
    phases = [collections.Counter()]
    for n, ln in enumerate(text):
        s = ln.strip()
        if is_phase_fence(text, n):
            phases.append(collections.Counter())
            continue
        if not s or s.startswith((';', '.')) or s.endswith(':'):
            continue
        for c in classify(s.split()[0]):
            phases[-1][c] += 1
    return phases


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--asm', help='device assembly (.s) of qmps_direct.hip; compiled afresh when omitted')
    ap.add_argument('--kernel', default=DEFAULT_KERNEL)
    ap.add_argument('--all', action='store_true', help='register / scratch use of every D = 4 direct / energy-only kernel')
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.asm or compile_asm(tmp)
        lines = open(path).read().split('\n')
    text, res = body(lines, a.kernel)
    phases = mix(text)
    names = phase_names(len(phases))
    print(f'{a.kernel}')
    print(f'{"phase":<16}' + ''.join(f'{c:>9}' for c in COLS))
    tot = collections.Counter()
    for n, p in zip(names, phases):
        tot.update(p)
        print(f'{n:<16}' + ''.join(f'{p[c]:>9}' for c in COLS))
    print(f'{"total":<16}' + ''.join(f'{tot[c]:>9}' for c in COLS))
    if names in (PHASES, PHASES_LDL, PHASES_OLD):
        common = tot.copy()
        for n in RARE:
            if n in names:
                common.subtract(phases[names.index(n)])
        print(f'{"common path":<16}' + ''.join(f'{common[c]:>9}' for c in COLS))
    print('VGPRs {} AGPRs {} SGPRs {} scratch {} B occupancy {}'.format(
        res.get('NumVgprs'), res.get('NumAgprs'), res.get('TotalNumSgprs'), res.get('ScratchSize'), res.get('Occupancy')))
    if a.all:
        for ln in lines:
            m = re.match(r'(_ZN4qmps(23energy_direct|21energy_only)_d4_kernel\w*):', ln)
            if m:
                _, r = body(lines, m.group(1))
                print(f'  {m.group(1):<64} VGPRs {r.get("NumVgprs"):>4} scratch {r.get("ScratchSize")}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
