#!/usr/bin/env python3
"""How far ahead of their readers the LDS operands of the fused D = 4 direct-solve energy kernel are requested.

usage: python tools/lds_cover.py [--asm FILE.s] [--kernel MANGLED_NAME] [--min-cover N] [--quiet]

The kernel text (tools/isa_mix.py: cross-compiled for gfx950, or --asm) is cut into the phases of isa_mix and walked in text order.  Every
ds_read / ds_write / scalar load enters the wave's lgkmcnt queue; at every `s_waitcnt lgkmcnt(k)` the queue keeps its k youngest entries,
and the YOUNGEST entry the wait retires is the one it really waits for (LDS returns in order).  Printed per wait of the common path:
    phase, line, k, what is retired (reads / writes / scalar loads), and the COVER: the VALU instructions - f64 apart - issued between that
    youngest retired request and the wait, i.e. the arithmetic that hides its latency.
A wait that retires nothing (the queue was already empty behind an earlier wait) is not listed.  Totals per phase: ds_read_b128, waits,
waits whose cover is below --min-cover f64 instructions (default 56: the smallest block of the staged source, ~224 issue cycles), and the
smallest cover.  The text order is the common path's order except inside the mask tests of the density phase (wave-uniform branches over
single parts of rho): a read requested before such a branch and awaited behind it is charged the instructions of the skipped part too -
compare totals of two builds of the same mask logic, as with isa_mix.  The fall-back phase is the rare path and is left out.
"""
import argparse
import collections
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_mix  # noqa: E402

LGKM = re.compile(r'lgkmcnt\((\d+)\)')
Wait = collections.namedtuple('Wait', 'phase line k reads writes smem valu f64 what')


def queue_kind(op):
    """the lgkmcnt queue an instruction enters: 'read' / 'write' (LDS), 'smem' (scalar memory), or None"""
    if op.startswith('ds_read') or op.startswith('ds_load'):
        return 'read'
    if op.startswith('ds_'):
        return 'write'
    if op.startswith('s_load') or op.startswith('s_buffer_load'):
        return 'smem'
    return None


def waits(text, names):
    """-> (list of Wait, Counter of ds_read_b128 per phase)"""
    out, reads = [], collections.Counter()
    phase = 0
    queue = []          # (kind, valu so far, f64 so far) of the outstanding requests, oldest first
    valu = f64 = 0
    for n, ln in enumerate(text):
        s = ln.strip()
        if isa_mix.is_phase_fence(text, n):
            phase += 1
            continue
        if not s or s.startswith((';', '.')) or s.endswith(':'):
            continue
        op = s.split()[0]
        name = names[phase] if phase < len(names) else f'phase {phase}'
        if op.startswith('v_'):
            valu += 1
            f64 += '_f64' in op
        kind = queue_kind(op)
        if kind is not None:
            queue.append((kind, valu, f64))
            if op.startswith('ds_read_b128'):
                reads[name] += 1
        elif op == 's_waitcnt':
            m = LGKM.search(s)
            if m is None:
                continue
            k = int(m.group(1))
            gone = queue[:len(queue) - k] if k < len(queue) else []
            if gone:
                queue = queue[len(queue) - k:] if k > 0 else []
                kinds = collections.Counter(g[0] for g in gone)
                last = gone[-1]
                out.append(Wait(name, n + 1, k, kinds['read'], kinds['write'], kinds['smem'], valu - last[1], f64 - last[2], last[0]))
    return out, reads


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--asm', help='device assembly (.s) of qmps_direct.hip; compiled afresh when omitted')
    ap.add_argument('--kernel', default=isa_mix.DEFAULT_KERNEL)
    ap.add_argument('--min-cover', type=int, default=56, help='f64 instructions that count as a whole block of cover')
    ap.add_argument('--quiet', action='store_true', help='totals only')
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.asm or isa_mix.compile_asm(tmp)
        lines = open(path).read().split('\n')
    text, res = isa_mix.body(lines, a.kernel)
    names = isa_mix.phase_names(len(isa_mix.mix(text)))
    ws, reads = waits(text, names)
    ws = [w for w in ws if w.phase not in isa_mix.RARE]
    print(a.kernel)
    if not a.quiet:
        print(f'{"phase":<12}{"line":>7}{"lgkmcnt":>9}{"reads":>7}{"writes":>8}{"smem":>6}{"valu":>7}{"f64":>6}  waits for')
        for w in ws:
            print(f'{w.phase:<12}{w.line:>7}{w.k:>9}{w.reads:>7}{w.writes:>8}{w.smem:>6}{w.valu:>7}{w.f64:>6}  {w.what}')
    print(f'{"phase":<12}{"b128 reads":>11}{"waits":>7}{"on LDS":>8}{f"f64 < {a.min_cover}":>10}{"min f64":>9}{"min valu":>10}')
    tot = collections.Counter()
    for name in names:
        if name in isa_mix.RARE:
            continue
        mine = [w for w in ws if w.phase == name]
        lds = [w for w in mine if w.what != 'smem']
        short = [w for w in lds if w.f64 < a.min_cover]
        tot.update(reads=reads[name], waits=len(mine), lds=len(lds), short=len(short))
        print(f'{name:<12}{reads[name]:>11}{len(mine):>7}{len(lds):>8}{len(short):>10}'
              f'{(min(w.f64 for w in lds) if lds else "-"):>9}{(min(w.valu for w in lds) if lds else "-"):>10}')
    print(f'{"common path":<12}{tot["reads"]:>11}{tot["waits"]:>7}{tot["lds"]:>8}{tot["short"]:>10}')
    print('VGPRs {} scratch {} B occupancy {}'.format(res.get('NumVgprs'), res.get('ScratchSize'), res.get('Occupancy')))
    return 0


if __name__ == '__main__':
    sys.exit(main())
