"""What the GPU tests of the observables of the resident states share: the Hamiltonian of their solves, the solve step, and the Haar
batch of tests/correlator_cases.py with the environments the device solved for it - solved once per bond dimension, read back, write
protected and from then on put back verbatim, so one reference per module serves every test.  (Plain module: no fixtures, no tests.)"""
import ctypes

import numpy as np

import correlator_cases as K
from oracle import qmps_oracle as O

H_TFIM = O.hamiltonian_matrix({'ZZ': -1, 'X': 1})
DP = ctypes.POINTER(ctypes.c_double)
_SOLVED = {}


def solve(eng, A, D):
    eng.set_tensors(A)
    eng.set_hamiltonian(H_TFIM)
    eng.launch(A.shape[0], solver='direct', store_env=True, krylov_fallback=(D == 8))


def haar(engine_factory, D):
    """Engine with the Haar batch and its solved environments resident, and the cache entry {'A', 'r', 'st', 'ref'} of the arrays as
    read back.  Later calls put the very same arrays back (qmps_set_env_guess copies verbatim)."""
    eng = engine_factory(D)
    if D not in _SOLVED:
        solve(eng, K.haar_tensors(D), D)
        st = eng.results(K.HAAR_B)[2]
        A, r = eng.tensors(K.HAAR_B), eng.environments(K.HAAR_B)
        assert np.array_equal(A, K.haar_tensors(D))
        for a in (A, r, st):
            a.setflags(write=False)
        _SOLVED[D] = {'A': A, 'r': r, 'st': st, 'ref': {}}
    else:
        eng.set_tensors(_SOLVED[D]['A'])
        eng.set_hamiltonian(H_TFIM)
        eng.set_env_guess(_SOLVED[D]['r'])
    return eng, _SOLVED[D]


def solved(D):
    """The cache entry of `haar` (which must have run for this D)."""
    return _SOLVED[D]


def cached(D, module, key, make):
    """A reference computed from the read-back arrays of `haar`, kept per test module; computed once, never changed."""
    ref = _SOLVED[D]['ref'].setdefault(module, {})
    if key not in ref:
        ref[key] = make()
    return ref[key]
