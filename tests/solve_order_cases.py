"""Inputs and the ctypes loader of tests/csrc/libsolve_order_emu.so (test infrastructure): the 16 x 16 solve of the D = 4 kernel
(DirectD4::solve_gathered / normalise_gathered, qmps_amd/csrc/qmps_direct_core.h: LU elimination with the pivots taken round the quad, back
substitution by columns), the route solve -> normalise -> gather of the older emulations, and a test-only Gauss-Jordan elimination in the
natural pivot order as the reference."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np

from oracle import qmps_oracle as O

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')
_LIB = None
ROUTES = ('solve', 'gathered', 'natural')
TOL = 1e-13                   # the solvers' acceptance tolerance
MAX_INVERSE_PIVOT = 1e10      # DirectD4::kMaxInversePivot
N_HAAR = 512


def lib():
    """Compiles tests/csrc/solve_order_emu.cpp with the flags of tests/csrc/Makefile (read from it) and loads it."""
    global _LIB
    if _LIB is None:
        make = open(os.path.join(_HERE, 'Makefile')).read()
        cxx = os.environ.get('CXX', 'g++')
        flags = re.search(r'^CXXFLAGS\s*\?=\s*(.*)$', make, flags=re.M).group(1).split()
        src, so = os.path.join(_HERE, 'solve_order_emu.cpp'), os.path.join(_HERE, 'libsolve_order_emu.so')
        deps = [src, os.path.join(_HERE, 'direct_emu.cpp'), os.path.join(_HERE, '..', '..', 'qmps_amd', 'csrc', 'qmps_direct_core.h')]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call([cxx] + flags + ['-shared', '-o', so + '.tmp', src], cwd=_HERE)
            os.replace(so + '.tmp', so)
        L = ctypes.CDLL(so)
        dp = ctypes.POINTER(ctypes.c_double)
        L.solve_order_emu_d4.argtypes = [ctypes.c_long, dp, dp, dp, dp, dp]
        L.solve_order_emu_d4.restype = ctypes.c_int
        _LIB = L
    return _LIB


def environment(us):
    """r (..., 4, 4) complex from the coordinates us (..., 16): u[(i,i)] = r_ii, u[(i,i')] = Re r_ii' (i < i'), u[(i',i)] = Im r_ii'"""
    r = np.zeros(us.shape[:-1] + (4, 4), dtype=np.complex128)
    for i in range(4):
        r[..., i, i] = us[..., 5 * i]
        for j in range(i + 1, 4):
            r[..., i, j] = us[..., 4 * i + j] + 1j * us[..., 4 * j + i]
            r[..., j, i] = us[..., 4 * i + j] - 1j * us[..., 4 * j + i]
    return r


def solve(A):
    """A (B, 2, 4, 4) -> {route: dict(x (B, 4 lanes, 4), us (B, 16, 4 lanes), pivmax (B,), d2 (B,), r (B, 4, 4) from lane 0's copy,
    accepted (B,): the kernel's criterion at tol 1e-13)} for the routes 'solve' (solve -> normalise -> gather), 'gathered' (solve_gathered ->
    normalise_gathered) and 'natural' (the reference elimination)."""
    dp = ctypes.POINTER(ctypes.c_double)
    A = np.ascontiguousarray(A, dtype=np.complex128)
    B = len(A)
    x, us = np.empty((3, B, 4, 4)), np.empty((3, B, 16, 4))
    piv, d2 = np.empty((3, B)), np.empty((3, B))
    lib().solve_order_emu_d4(B, A.ctypes.data_as(dp), x.ctypes.data_as(dp), us.ctypes.data_as(dp), piv.ctypes.data_as(dp), d2.ctypes.data_as(dp))
    out = {}
    for k, name in enumerate(ROUTES):
        with np.errstate(invalid='ignore'):
            acc = (d2[k] < TOL * TOL) & (piv[k] < MAX_INVERSE_PIVOT)
        out[name] = {'x': x[k], 'us': us[k], 'pivmax': piv[k], 'd2': d2[k], 'r': environment(us[k][:, :, 0]), 'accepted': acc}
    return out


@functools.lru_cache(maxsize=None)
def haar_rows():
    """512 Haar isometries of their own (the family of tests/conditioning_cases.py holds 512 others)"""
    A = O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(7300), 8, N_HAAR))
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def results():
    """(haar, family): solve() of the 512 Haar rows and of every D = 4 row of tests/conditioning_cases.py, computed once"""
    from tests import conditioning_cases as CC
    return solve(haar_rows()), solve(CC.family(4)['A'])
