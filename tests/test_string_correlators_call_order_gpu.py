"""GPU: qmps_string_correlators in the call-order suite's terms, without touching its tables (tests/call_order_cases.py holds the
families, the readers and the inputs): after every family the call - fixed batch uploaded again, one launch, the call - returns the
bytes it returns alone on a fresh context; and no reader notices that the call ran.

Contexts of capacity call_order_cases.CAPACITY, created and closed here; at most one is open at a time."""
import time

import numpy as np
import pytest

import call_order_cases as C
import string_correlator_cases as SC
from qmps_amd import EnergyEngine

pytestmark = pytest.mark.gpu

STRING = SC.strings()['generic']


def fresh(D):
    return EnergyEngine(D, C.CAPACITY)


def _call(eng, D):
    return eng.correlators(C.inputs(D)['ops'], C.N_MAX, C.B, want_one_site=True, string=STRING, want_string=True)


def string_family(eng, D):
    """the new call as a self-contained family: it uploads what it reads"""
    I = C.inputs(D)
    C.canon(eng)
    C._solve_for_observables(eng, I)
    Cs, one, st = _call(eng, D)
    order = eng.string_order(STRING, C.N_MAX, C.B)
    E, it, status = eng.results(C.B)
    return {'C': Cs.copy(), 'one': one.copy(), 'str': st.copy(), 'order': order.copy(), 'E': E.copy(), 'iters': it.copy(), 'status': status.copy(),
            'r': eng.environments(C.B).copy()}


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize('D', C.DS)
def test_the_call_after_every_family_equals_alone(D):
    t0 = time.perf_counter()
    with fresh(D) as eng:
        alone = string_family(eng, D)
    assert np.isfinite(alone['C']).all() and alone['C'].shape == (C.B, 3, 3, C.N_MAX) and alone['str'].shape == (C.B, C.N_MAX)
    assert same(alone['str'], alone['order'])
    failures = []
    for X in C.legal(D):
        with fresh(D) as eng:
            C.canon(eng)
            C.FAMILIES[X].run(eng, D, C.inputs(D))
            got = string_family(eng, D)
        bad = sorted(k for k in alone if not same(alone[k], got[k]))
        if bad:
            failures.append((X, bad))
    print(f'string correlators D = {D}: after each of {len(C.legal(D))} families, {time.perf_counter() - t0:.2f} s')
    assert not failures, failures


def _same_outcome(a, b):
    if len(a) != len(b):
        return False
    if a and isinstance(a[0], str):
        return tuple(a) == tuple(b)
    if b and isinstance(b[0], str):
        return False
    return all(x is y or (x is not None and y is not None and same(np.asarray(x), np.asarray(y))) for x, y in zip(a, b))


@pytest.mark.parametrize('D', C.DS)
def test_no_reader_notices_the_call(D):
    """Every reader returns the same bytes, or the same refusal, before and after the call - on the energy preparation (where the call
    succeeds) and on the overlap preparation (where it refuses: no environments)."""
    t0 = time.perf_counter()
    failures = []
    for prepare, readers, succeeds in ((C.prepare_energy, C.ENERGY_READERS, True), (C.prepare_overlap, C.OVERLAP_READERS, False)):
        legal = [r for r in readers if C.reader_legal(r, D)]
        with fresh(D) as eng:
            prepare(eng, D)
            before = {r: C.read(eng, r, C.B) for r in legal}
        with fresh(D) as eng:
            prepare(eng, D)
            got = C._refusal(lambda: _call(eng, D))
            assert isinstance(got[0], str) != succeeds, got[:2]
            after = {r: C.read(eng, r, C.B) for r in legal}
        failures += [r for r in legal if not _same_outcome(before[r], after[r])]
    print(f'string correlators D = {D}: {len(C.READERS)} readers, {time.perf_counter() - t0:.2f} s')
    assert not failures, failures
