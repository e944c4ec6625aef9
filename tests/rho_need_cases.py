"""The Hamiltonians of the "needed entries of rho" tests and the ctypes loader of tests/csrc/librho_need_emu.so (test infrastructure).

The D = 4 energy kernels compute only the parts of the two-site density matrix that some term of h reads (qmps::rho_need_mask,
qmps_amd/csrc/qmps_direct_core.h): bit 4 t + s (t <= s) stands for Re rho[t][s], bit 16 + 4 t + s (t < s) for Im rho[t][s]."""
import ctypes
import os
import re
import subprocess

import numpy as np

from oracle import qmps_oracle as O

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')
_LIB = None

Y1 = np.kron(np.array([[0, -1j], [1j, 0]]), np.eye(2))

TFIM = O.hamiltonian_matrix({'ZZ': -1, 'X': 1})
XXZ = O.hamiltonian_matrix({'XX': 1, 'YY': 1, 'ZZ': 0.5})
COMPLEX_HERMITIAN = TFIM + 0.7 * Y1
ZERO = np.zeros((4, 4), dtype=complex)
THREE_TERMS = np.stack([TFIM, COMPLEX_HERMITIAN, XXZ])
TFIM_BITS = {0, 5, 10, 15, 1, 2, 7, 11}


def bit(s, t, imag):
    """the bit entry h[s][t] sets: its real part (imag = False) or its imaginary part"""
    lo, hi = min(s, t), max(s, t)
    return (16 if imag else 0) + 4 * lo + hi


def single_entry(s, t, imag, value=0.37):
    h = ZERO.copy()
    h[s, t] = complex(0.0, value) if imag else complex(value, 0.0)
    return h


def single_entry_cases():
    """(h, expected mask) of one non-zero entry at each of the 16 positions, once real and once imaginary.  An imaginary entry on the
    diagonal multiplies no part of rho (Im rho[t][t] = 0): no bit."""
    out = []
    for s in range(4):
        for t in range(4):
            out.append((single_entry(s, t, False), 1 << bit(s, t, False)))
            out.append((single_entry(s, t, True), 0 if s == t else 1 << bit(s, t, True)))
    return out


def table():
    """name -> h (4, 4): every one-term Hamiltonian of the tests"""
    out = {'tfim': TFIM, 'xxz': XXZ, 'complex_hermitian': COMPLEX_HERMITIAN, 'zero': ZERO, 'minus_zero': np.full((4, 4), complex(-0.0, -0.0)),
           'nan_entry': single_entry(1, 2, False, np.nan)}
    for k, (h, _) in enumerate(single_entry_cases()):        # k = 8 s + 2 t + (imaginary)
        out[f'single_{k // 8}{(k // 2) % 4}_{"im" if k % 2 else "re"}'] = h
    return out


def full_mask_twin(h):
    """h with 1e-300 (1 + i) added to every entry: every bit of the mask is set, and no energy moves by more than 1e-298"""
    return np.asarray(h, dtype=complex) + 1e-300 * (1 + 1j)


def lib():
    """Compiles tests/csrc/rho_need_emu.cpp with the flags of tests/csrc/Makefile (read from it) and loads it."""
    global _LIB
    if _LIB is None:
        make = open(os.path.join(_HERE, 'Makefile')).read()
        cxx = os.environ.get('CXX', 'g++')
        flags = re.search(r'^CXXFLAGS\s*\?=\s*(.*)$', make, flags=re.M).group(1).split()
        src, so = os.path.join(_HERE, 'rho_need_emu.cpp'), os.path.join(_HERE, 'librho_need_emu.so')
        deps = [src, os.path.join(_HERE, 'direct_emu.cpp'), os.path.join(_HERE, 'rho_reference.h'), os.path.join(_HERE, '..', '..', 'qmps_amd', 'csrc', 'qmps_direct_core.h')]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call([cxx] + flags + ['-shared', '-o', so + '.tmp', src], cwd=_HERE)
            os.replace(so + '.tmp', so)
        L = ctypes.CDLL(so)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        L.rho_need_mask_emu.argtypes = [dp, ctypes.c_int]
        L.rho_need_mask_emu.restype = ctypes.c_uint32
        L.rho_need_emu_d4.argtypes = [ctypes.c_long, dp, dp, dp, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, dp, dp, dp, ip]
        L.rho_need_emu_d4.restype = ctypes.c_int
        _LIB = L
    return _LIB


def _terms(h):
    return np.ascontiguousarray(np.asarray(h, dtype=np.complex128).reshape(-1, 4, 4))


def mask(h):
    h = _terms(h)
    return int(lib().rho_need_mask_emu(h.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(h)))


def density_energy(A, r, h, need=None, reference=False):
    """The density matrix and the energies of the emulation from tensors A (B, 2, 4, 4) and environments r (B, 4, 4): without a mask
    (need None), with one, or (reference=True) from the functions as they stood before there was a mask, tests/csrc/rho_reference.h
    -> dict(E (B, terms), pre, pim (B, 4, 4, 4): the lanes' shares of rho[t][s], pd (B,))."""
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    A = np.ascontiguousarray(A, dtype=np.complex128)
    r = np.ascontiguousarray(r, dtype=np.complex128)
    h = _terms(h)
    B, nt = len(A), len(h)
    E = np.empty((B, nt))
    pre, pim = np.empty((B, 4, 4, 4)), np.empty((B, 4, 4, 4))
    pd = np.empty(B, dtype=np.int32)
    lib().rho_need_emu_d4(B, A.ctypes.data_as(dp), r.ctypes.data_as(dp), h.ctypes.data_as(dp), nt, -1 if reference else (0 if need is None else 1),
                          0 if need is None else int(need), E.ctypes.data_as(dp), pre.ctypes.data_as(dp), pim.ctypes.data_as(dp),
                          pd.ctypes.data_as(ip))
    return {'E': E, 'pre': pre, 'pim': pim, 'pd': pd}
