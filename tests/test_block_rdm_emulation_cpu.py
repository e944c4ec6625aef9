"""CPU: block_rdm_kernel (qmps_amd/csrc/qmps_block_rdm.hip) thread by thread in numpy, with the kernel's own index formulas - the LDS
layout of one evaluation, the levels of the doubling that overwrite their predecessors, the Gram operands laid over the dead levels,
the element a thread sums and stores.  A phase is the code between two barriers, run for every thread before the next phase starts;
the region the levels and the Gram operands share is poisoned with NaN at the barrier before it is rewritten, so a read of what nobody
has written yet shows in the result.  Checked: every element of the output is written exactly once, tails included, and equals the
long-double reference to the rho bound of tests/block_rdm_cases.py.  (The arithmetic is numpy's, not the device's: this is a test of
the indexing, and the GPU tests hold the device to the same bound.)"""
import numpy as np
import pytest

import block_rdm_cases as K

NCH = {2: 1, 4: 1, 8: 4, 16: 4}           # parts of the Gram product (launch_block_rdm)


def region(D, NCH, n):
    levels = (1 << (n - 1)) * D * (D + 1) if n >= 3 else 0
    gram = 2 * (1 << n) * (D * D // NCH + 1)
    return max(levels, gram)


def run_block(D, NCH, n, Aall, rall, B, block):
    N = D * D; NT = max(64, N); EV = NT // N; P = D + 1; MS = D * P; CH = N // NCH; CS = CH + 1
    ACC = 1 if NCH == 1 else (256 + NT - 1) // NT
    T = 1 << n; TT = T * T; ES = 5 * MS + region(D, NCH, n)
    smem = np.full(EV + EV * ES, np.nan + 1j * np.nan, dtype=np.complex128)      # poison: reading what nobody wrote shows
    b0 = block * EV; nb = min(EV, B - b0)
    out = {}
    th = []
    for tid in range(NT):
        e, tl = divmod(tid, N); i, j = divmod(tl, D)
        b = b0 + e if e < nb else B - 1
        mine = EV + e * ES
        th.append(dict(tid=tid, e=e, tl=tl, i=i, j=j, b=b, sA=mine, sAr=mine + 2 * MS, sR=mine + 4 * MS, sU=mine + 5 * MS))
    Af = Aall.reshape(B, -1); rf = rall.reshape(B, -1)
    for t in th:
        smem[t['sA'] + t['i'] * P + t['j']] = Af[t['b'], t['tl']]
        smem[t['sA'] + MS + t['i'] * P + t['j']] = Af[t['b'], N + t['tl']]
        smem[t['sR'] + t['i'] * P + t['j']] = rf[t['b'], t['tl']]
    # barrier
    for t in th:
        if t['tl'] == 0:
            tr = sum(smem[t['sR'] + l * P + l] for l in range(D))
            smem[t['e']] = 1 / tr if (tr != 0 and np.isfinite(tr)) else np.nan
        for s in range(2):
            v = 0
            for l in range(D):
                v += smem[t['sA'] + s * MS + t['i'] * P + l] * smem[t['sR'] + l * P + t['j']]
            smem[t['sAr'] + s * MS + t['i'] * P + t['j']] = v
    # barrier
    for t in th:
        t['lev'] = t['sA']
    k = 1
    while k + 1 < n:
        cnt = 1 << k
        for t in th:
            nx = {}
            for tt in range(4):
                if tt < cnt:
                    for s in range(2):
                        v = 0
                        for l in range(D):
                            v += smem[t['lev'] + tt * MS + t['i'] * P + l] * smem[t['sA'] + s * MS + l * P + t['j']]
                        nx[2 * tt + s] = v
            t['nx'] = nx
        for t in th:
            for tt in range(8):
                if tt < 2 * cnt:
                    assert 5 * MS + tt * MS + t['i'] * P + t['j'] < ES
                    smem[t['sU'] + tt * MS + t['i'] * P + t['j']] = t['nx'][tt]
            t['lev'] = t['sU']
        k += 1
    for t in th:
        Bf, Mf = {}, {}
        if n == 1:
            for s in range(2):
                Bf[s] = smem[t['sA'] + s * MS + t['i'] * P + t['j']]
                Mf[s] = smem[t['sAr'] + s * MS + t['i'] * P + t['j']]
        else:
            half = T >> 1
            for tt in range(8):
                if tt < half:
                    for s in range(2):
                        vb = vm = 0
                        for l in range(D):
                            x = smem[t['lev'] + tt * MS + t['i'] * P + l]
                            vb += x * smem[t['sA'] + s * MS + l * P + t['j']]
                            vm += x * smem[t['sAr'] + s * MS + l * P + t['j']]
                        Bf[2 * tt + s] = vb; Mf[2 * tt + s] = vm
        t['Bf'], t['Mf'] = Bf, Mf
        t['acc'] = [0] * ACC
    for c in range(NCH):
        # barrier; poison the union to show stale reads
        for t in th:
            if t['tl'] == 0:
                smem[t['sU']:t['sU'] + region(D, NCH, n)] = np.nan
        for t in th:
            if t['tl'] // CH == c:
                cc = t['tl'] % CH
                for tt in range(16):
                    if tt < T:
                        assert tt * CS + cc < T * CS and T * CS + tt * CS + cc < region(D, NCH, n)
                        smem[t['sU'] + tt * CS + cc] = t['Bf'][tt]
                        smem[t['sU'] + T * CS + tt * CS + cc] = t['Mf'][tt]
        # barrier
        for t in th:
            tid = t['tid']
            if NCH == 1:
                total = nb * TT
                g = tid
                while g < total:
                    ge = g >> (2 * n); idx = g & (TT - 1); tt = idx >> n; s = idx & (T - 1)
                    uB = EV + ge * ES + 5 * MS; uM = uB + T * CS
                    v = 0
                    for cc in range(CH):
                        v += smem[uM + tt * CS + cc] * np.conj(smem[uB + s * CS + cc])
                    out[b0 * TT + g] = v * smem[ge]
                    g += NT
            else:
                for m in range(ACC):
                    g = tid + m * NT
                    if g < TT:
                        tt = g >> n; s = g & (T - 1)
                        v = t['acc'][m]
                        for cc in range(CH):
                            v += smem[t['sU'] + T * CS + tt * CS + cc] * np.conj(smem[t['sU'] + s * CS + cc])
                        t['acc'][m] = v
    if NCH > 1:
        for t in th:
            for m in range(ACC):
                g = t['tid'] + m * NT
                if g < TT:
                    out[b0 * TT + g] = t['acc'][m] * smem[0]
    return out


# (D, n, B): every n where a workgroup holds several evaluations, with full workgroups and tails of 1 (D = 2: 17) and 3 (D = 4: 7); the
# levels and the four parts of the Gram product at D = 8, 16
@pytest.mark.parametrize('D,n,B', [(2, 1, 17), (2, 2, 17), (2, 3, 17), (2, 4, 17), (2, 4, 15), (4, 1, 7), (4, 2, 7), (4, 3, 7), (4, 4, 7),
                                   (8, 1, 2), (8, 3, 2), (8, 4, 2), (16, 1, 1), (16, 2, 1), (16, 3, 1), (16, 4, 1)])
def test_emulated_kernel_writes_every_element_once_and_meets_the_bound(D, n, B):
    EV = max(64, D * D) // (D * D)
    A, r = K.batch(D, B)
    T = 1 << n
    res = np.full(B * T * T, np.nan + 0j)
    seen = set()
    for blk in range((B + EV - 1) // EV):
        o = run_block(D, NCH[D], n, A, r, B, blk)
        assert not (seen & set(o)), 'an element written twice'
        seen |= set(o)
        for kx, v in o.items():
            res[kx] = v
    assert seen == set(range(B * T * T)), (D, n, len(seen))
    res = res.reshape(B, T, T)
    idx = K.batch_index(D, B)
    ref = K.case_reference(D, n)[0][idx]
    nan = K.kinds(D)[idx] == 'nan'
    assert np.isnan(res[nan]).all() and np.isfinite(res[~nan]).all()
    scale = np.abs(ref[~nan]).max(axis=(1, 2)).astype(float)
    err = np.abs(res[~nan] - ref[~nan]).max(axis=(1, 2)).astype(float) / K.rho_bound(D, n, scale)
    print(f'block rdm emulation D={D} n={n} B={B}: worst fraction of the rho bound {err.max():.3f}')
    assert np.all(err <= 1)
