"""Inputs, bounds and the ctypes loader of tests/csrc/libsite_factor_emu.so (test infrastructure) for the site-factor route of the two-site
density matrix (DirectD4::power_step_sites / update_sites / density_sites, qmps_amd/csrc/qmps_direct_core.h):

    rho[(t1 t2)][(s1 s2)] = tr(N_{s1 t1} W_{t2 s2}),   N_{s1 t1} = A_s1^+ A_t1,   W_{t2 s2} = A_t2 r A_s2^+

for any tensor and any r.  The masks and Hamiltonians are those of tests/rho_need_cases.py."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np

from oracle import qmps_oracle as O
from tests import rho_need_cases as RN

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')
_LIB = None
EPS = 2.0 ** -52

# factor bits of qmps::rho_site_factors
N00, N10, N11, W01, W10 = 1, 2, 4, 8, 16
FULL_UPPER = 0x08CE8CEF       # every real and imaginary part of the upper triangle


def lib():
    """Compiles tests/csrc/site_factor_emu.cpp with the flags of tests/csrc/Makefile (read from it) and loads it."""
    global _LIB
    if _LIB is None:
        make = open(os.path.join(_HERE, 'Makefile')).read()
        cxx = os.environ.get('CXX', 'g++')
        flags = re.search(r'^CXXFLAGS\s*\?=\s*(.*)$', make, flags=re.M).group(1).split()
        src, so = os.path.join(_HERE, 'site_factor_emu.cpp'), os.path.join(_HERE, 'libsite_factor_emu.so')
        deps = [src, os.path.join(_HERE, 'direct_emu.cpp'), os.path.join(_HERE, '..', '..', 'qmps_amd', 'csrc', 'qmps_direct_core.h')]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call([cxx] + flags + ['-shared', '-o', so + '.tmp', src], cwd=_HERE)
            os.replace(so + '.tmp', so)
        L = ctypes.CDLL(so)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        L.site_factors_emu.argtypes = [ctypes.c_uint32]
        L.site_factors_emu.restype = ctypes.c_uint32
        L.site_factor_emu_d4.argtypes = [ctypes.c_long, dp, dp, dp, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, dp, dp, dp, ip, dp, dp]
        L.site_factor_emu_d4.restype = ctypes.c_int
        L.site_factor_direct_d4.argtypes = [ctypes.c_long, dp, dp, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, dp, dp, dp, ip, ip]
        L.site_factor_direct_d4.restype = ctypes.c_int
        _LIB = L
    return _LIB


def factors(need):
    return int(lib().site_factors_emu(int(need)))


def _terms(h):
    return np.ascontiguousarray(np.asarray(h, dtype=np.complex128).reshape(-1, 4, 4))


def density_energy(A, r, h, need, via_update=0):
    """power_step_sites + density_sites + energy of the emulation from tensors A (B, 2, 4, 4) and environments r (B, 4, 4) under the mask
    `need` -> dict(E (B, terms), pre, pim (B, 4, 4, 4): the lanes' shares of rho[t][s], pd (B,), y (B, 4, 4), d2 (B,))."""
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    A = np.ascontiguousarray(A, dtype=np.complex128)
    r = np.ascontiguousarray(r, dtype=np.complex128)
    h = _terms(h)
    B, nt = len(A), len(h)
    E = np.empty((B, nt))
    pre, pim = np.empty((B, 4, 4, 4)), np.empty((B, 4, 4, 4))
    pd = np.empty(B, dtype=np.int32)
    y, d2 = np.empty((B, 4, 4)), np.empty(B)
    lib().site_factor_emu_d4(B, A.ctypes.data_as(dp), r.ctypes.data_as(dp), h.ctypes.data_as(dp), nt, int(need), int(via_update),
                             E.ctypes.data_as(dp), pre.ctypes.data_as(dp), pim.ctypes.data_as(dp), pd.ctypes.data_as(ip),
                             y.ctypes.data_as(dp), d2.ctypes.data_as(dp))
    return {'E': E, 'pre': pre, 'pim': pim, 'pd': pd, 'y': y, 'd2': d2}


def energies_d4(A, h, need=None, max_iter=10000, tol=1e-13):
    """The whole cold-start kernel with the site-factor route: tests.direct_emu.energies_d4's arguments and outputs (without resid / E_lean).
    need: the launch's mask (default: the Hamiltonian's)."""
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    A = np.ascontiguousarray(A, dtype=np.complex128)
    h = _terms(h)
    need = RN.mask(h) if need is None else need
    B, nt = len(A), len(h)
    E = np.empty((B, nt))
    r = np.empty((B, 4, 4), dtype=np.complex128)
    rho = np.empty((B, 4, 4), dtype=np.complex128)
    it, st = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
    lib().site_factor_direct_d4(B, A.ctypes.data_as(dp), h.ctypes.data_as(dp), nt, int(need), int(max_iter), float(tol), E.ctypes.data_as(dp),
                                r.ctypes.data_as(dp), rho.ctypes.data_as(dp), it.ctypes.data_as(ip), st.ctypes.data_as(ip))
    return {'E': E, 'r': r, 'rho': rho, 'iters': it, 'status': st}


def quad(shares):
    """the quad sum of the lanes' shares in the order of the DPP butterfly"""
    return (shares[..., 0] + shares[..., 1]) + (shares[..., 2] + shares[..., 3])


def rho_of(out):
    """the upper triangle of rho (B, 4, 4) complex from the lanes' shares (the lower triangle 0)"""
    return quad(out['pre']) + 1j * quad(out['pim'])


def rho_numpy(A, r):
    """rho[b, t, s] = tr(B_t r B_s^+), B_(2 t1 + t2) = A_t1 A_t2 - no normalisation, any tensor, any r"""
    Bm = np.einsum('bsij,btjk->bstik', A, A).reshape(len(A), 4, 4, 4)
    return np.einsum('btij,bjk,bsik->bts', Bm, r, Bm.conj())


def rho_scale(A, r):
    """S[b] = max over (t, s) of tr(|B|_t |r| |B|_s^T) with |B|_(t1 t2) = |A_t1| |A_t2| entry-wise moduli: the sum of the moduli of ALL
    the products any route to rho[t][s] adds up - every rounding error of a route is a relative one of a partial sum of these."""
    a = np.abs(A)
    Bm = np.einsum('bsij,btjk->bstik', a, a).reshape(len(A), 4, 4, 4)
    return np.einsum('btij,bjk,bsik->bts', Bm, np.abs(r), Bm).max(axis=(1, 2))


# A part of rho through the site factors: X = A r (7 multiply-adds deep), W = X A^+ (8), N = A^+ A (8), the part (8), the quad sum (2): no
# partial sum has seen more than 33 roundings, each at most eps (complex products: their real and imaginary parts are sums of two products
# of the moduli bound).  The references (B_tau r B_sigma^+ in the kernel's older route or in numpy) are no deeper.  Both errors: 2 x 40 eps S.
def rho_tol(A, r):
    return 80 * EPS * rho_scale(A, r)


def energy_tol(A, r, h):
    """E = Re sum h rho: the rho bound times sum |h|, and the 28 multiply-adds of the energy sum on either side"""
    return (80 + 56) * EPS * rho_scale(A, r) * max(1.0, float(np.abs(np.asarray(h)).sum()))


def single_part_masks():
    """(mask, t, s, imaginary) of each of the 16 parts of the upper triangle alone"""
    out = []
    for t in range(4):
        for s in range(t, 4):
            out.append((1 << (4 * t + s), t, s, False))
            if s > t:
                out.append((1 << (16 + 4 * t + s), t, s, True))
    return out


def masks():
    """name -> mask: the Hamiltonians of the issue, the full mask, every single part"""
    out = {'tfim': RN.mask(RN.TFIM), 'xxz': RN.mask(RN.XXZ), 'complex_hermitian': RN.mask(RN.COMPLEX_HERMITIAN),
           'three_terms': RN.mask(RN.THREE_TERMS), 'full': 0xFFFFFFFF, 'full_upper': FULL_UPPER, 'none': 0}
    for m, t, s, im in single_part_masks():
        out[f'part_{t}{s}_{"im" if im else "re"}'] = m
    return out


def random_hermitian(rng, n, kind):
    """n Hermitian 4 x 4 matrices of trace 1: 'indefinite' (eigenvalues of both signs), 'singular' (rank 1 and rank 2), 'negative' (r[0][0] < 0)"""
    G = O.haar_unitaries(rng, 4, n)
    if kind == 'indefinite':
        w = rng.standard_normal((n, 4))
        w[:, 0], w[:, 1] = np.abs(w[:, 0]) + 1.5, -np.abs(w[:, 1])
    elif kind == 'singular':
        w = np.zeros((n, 4))
        w[:, 0] = 1.0
        w[n // 2:, 1] = 0.5
    else:
        w = rng.standard_normal((n, 4)) + 0.5
    w = w / w.sum(axis=1, keepdims=True)
    r = np.einsum('bij,bj,bkj->bik', G, w, G.conj())
    r = (r + r.conj().transpose(0, 2, 1)) / 2
    if kind == 'negative':
        r[:, 0, 0] = -np.abs(r[:, 0, 0]) - 0.1
        r /= np.trace(r, axis1=1, axis2=2).real[:, None, None]
    return r


@functools.lru_cache(maxsize=None)
def inputs():
    """(A, r, kind) in a fixed order, read-only:
      haar          64 Haar isometries with the environments of the kernel emulation
      conditioning  every row of tests/conditioning_cases.py at D = 4 that the solve finishes (status 0 or 2): near-singular environments
      general       96 complex Gaussian tensors (no isometry; entries up to ~3) with indefinite, singular and r[0][0] < 0 environments"""
    from tests import conditioning_cases as CC
    from tests import direct_emu as EMU
    haar = O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(77), 8, 64))
    A = np.concatenate([haar, CC.family(4)['A']])
    out = EMU.energies_d4(A, RN.TFIM)
    keep = (out['status'] == 0) | (out['status'] == 2)
    assert keep[:64].all() and (out['status'][64:] == 2).sum() > 100
    A, r = A[keep], out['r'][keep]
    kind = np.array(['haar'] * 64 + ['conditioning'] * (len(A) - 64))
    rng = np.random.default_rng(5150)
    G = (rng.standard_normal((96, 2, 4, 4)) + 1j * rng.standard_normal((96, 2, 4, 4))) * rng.uniform(0.2, 1.0, (96, 1, 1, 1))
    rg = np.concatenate([random_hermitian(rng, 32, k) for k in ('indefinite', 'singular', 'negative')])
    A, r, kind = np.concatenate([A, G]), np.concatenate([r, rg]), np.concatenate([kind, ['general'] * 96])
    for v in (A, r, kind):
        v.setflags(write=False)
    return A, r, kind
