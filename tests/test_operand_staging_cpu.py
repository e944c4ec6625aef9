"""CPU: staging the LDS operands of the D = 4 direct-solve kernel a block ahead of their arithmetic (QMPS_STAGE_FENCE, the operand sets
of qmps_amd/csrc/qmps_direct_core.h) moves reads and nothing else: every operation on data is the same operation in the same order.  The
lock-step emulation tests/csrc/site_factor_emu.cpp is compiled twice - against the header as it is and against the frozen copy of the
header from before the staging, tests/csrc/operand_staging_parent/qmps_direct_core.h (test infrastructure; never loaded by the product) -
and the two must agree BIT FOR BIT (NaN payloads and signed zeros included: the arrays are compared as 64-bit integers):
  * the whole cold-start sequence of core calls (build, solve, acceptance step with its site factors, fall-back with its hand-over,
    density_sites, energies) on 512 Haar isometries, the near-singular family of tests/conditioning_cases.py (which sends rows through the
    fall-back and through the not-positive-definite status) and complex Gaussian tensors that are no isometries: r, rho, E, iterations,
    status;
  * acceptance step + density + energies from PRESCRIBED environments - the Gaussian tensors with indefinite, singular and r[0][0] < 0
    environments of tests/site_factor_cases.py among them - with W as the step leaves it and through update_sites both ways;
under each of the 23 masks of tests/test_site_factors_cpu.py."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import qmps_oracle as O
from tests import rho_need_cases as RN
from tests import site_factor_cases as SF

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')
_FROZEN = os.path.join(_HERE, 'operand_staging_parent')


@functools.lru_cache(maxsize=None)
def frozen_lib():
    """site_factor_emu.cpp against the frozen header: the flags of tests/csrc/Makefile with the frozen copy's directory in front"""
    make = open(os.path.join(_HERE, 'Makefile')).read()
    cxx = os.environ.get('CXX', 'g++')
    flags = re.search(r'^CXXFLAGS\s*\?=\s*(.*)$', make, flags=re.M).group(1).split()
    src, so = os.path.join(_HERE, 'site_factor_emu.cpp'), os.path.join(_FROZEN, 'libsite_factor_emu_parent.so')
    deps = [src, os.path.join(_HERE, 'direct_emu.cpp'), os.path.join(_FROZEN, 'qmps_direct_core.h')]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([cxx, '-I', _FROZEN] + flags + ['-shared', '-o', so + '.tmp', src], cwd=_HERE)
        os.replace(so + '.tmp', so)
    L = ctypes.CDLL(so)
    live = SF.lib()
    for name in ('site_factor_emu_d4', 'site_factor_direct_d4'):
        getattr(L, name).argtypes = getattr(live, name).argtypes
        getattr(L, name).restype = ctypes.c_int
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32 if a.dtype == np.int32 else ctypes.c_double))


def cold_start(L, A, h, need):
    h = np.ascontiguousarray(np.asarray(h, dtype=np.complex128).reshape(-1, 4, 4))
    B, nt = len(A), len(h)
    out = {'E': np.empty((B, nt)), 'r': np.empty((B, 4, 4), dtype=np.complex128), 'rho': np.empty((B, 4, 4), dtype=np.complex128),
           'iters': np.empty(B, dtype=np.int32), 'status': np.empty(B, dtype=np.int32)}
    L.site_factor_direct_d4(B, _ptr(A.view(np.float64)), _ptr(h.view(np.float64)), nt, int(need), 10000, 1e-13, _ptr(out['E']),
                            _ptr(out['r'].view(np.float64)), _ptr(out['rho'].view(np.float64)), _ptr(out['iters']), _ptr(out['status']))
    return out


def from_environment(L, A, r, h, need, via_update):
    h = np.ascontiguousarray(np.asarray(h, dtype=np.complex128).reshape(-1, 4, 4))
    B, nt = len(A), len(h)
    out = {'E': np.empty((B, nt)), 'pre': np.empty((B, 4, 4, 4)), 'pim': np.empty((B, 4, 4, 4)), 'pd': np.empty(B, dtype=np.int32),
           'y': np.empty((B, 4, 4)), 'd2': np.empty(B)}
    L.site_factor_emu_d4(B, _ptr(A.view(np.float64)), _ptr(r.view(np.float64)), _ptr(h.view(np.float64)), nt, int(need), int(via_update),
                         _ptr(out['E']), _ptr(out['pre']), _ptr(out['pim']), _ptr(out['pd']), _ptr(out['y']), _ptr(out['d2']))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize % 8 == 0 else a


def assert_same_bits(got, want, what):
    for key in want:
        assert np.array_equal(bits(got[key]), bits(want[key])), (what, key)


@functools.lru_cache(maxsize=None)
def tensors():
    """(A, kind), read-only: 512 Haar isometries, the conditioning family at D = 4, the 96 complex Gaussian tensors of SF.inputs()"""
    from tests import conditioning_cases as CC
    haar = O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(950), 8, 512))
    cond = CC.family(4)['A']
    A_sf, _, kind_sf = SF.inputs()
    gauss = A_sf[kind_sf == 'general']
    A = np.ascontiguousarray(np.concatenate([haar, cond, gauss]), dtype=np.complex128)
    kind = np.array(['haar'] * len(haar) + ['conditioning'] * len(cond) + ['general'] * len(gauss))
    A.setflags(write=False)
    return A, kind


def test_the_frozen_copy_is_a_header_from_before_the_staging():
    text = open(os.path.join(_FROZEN, 'qmps_direct_core.h')).read()
    live = open(os.path.join(_HERE, '..', '..', 'qmps_amd', 'csrc', 'qmps_direct_core.h')).read()
    assert 'QMPS_STAGE_FENCE' not in text and 'QMPS_STAGE_FENCE' in live


@pytest.mark.parametrize('name', sorted(SF.masks()))
def test_cold_start_bit_for_bit(name):
    need = SF.masks()[name]
    A, kind = tensors()
    h = RN.THREE_TERMS
    new, old = cold_start(SF.lib(), A, h, need), cold_start(frozen_lib(), A, h, need)
    assert_same_bits(new, old, name)
    if name == 'full':
        # the families do what they are there for: the fall-back and every status are met
        assert (old['iters'] > 1).sum() > 50 and (old['status'] == 2).sum() > 100 and (old['status'][kind == 'haar'] == 0).all()
        # (no isometries: the direct solve is not accepted and the power fall-back hands its environment to update_sites)
        assert (old['iters'][kind == 'general'] > 1).mean() > 0.9


@pytest.mark.parametrize('name', sorted(SF.masks()))
def test_prescribed_environments_bit_for_bit(name):
    need = SF.masks()[name]
    A, r, kind = SF.inputs()
    A, r = np.ascontiguousarray(A), np.ascontiguousarray(r)
    for via_update in (0, 1, 2):
        new = from_environment(SF.lib(), A, r, RN.THREE_TERMS, need, via_update)
        old = from_environment(frozen_lib(), A, r, RN.THREE_TERMS, need, via_update)
        assert_same_bits(new, old, (name, via_update))
    if name == 'full':
        assert (old['pd'][kind == 'general'] == 0).sum() >= 64
