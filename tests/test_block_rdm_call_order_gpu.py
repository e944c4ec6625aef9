"""GPU: qmps_block_entanglement in the call-order suite's terms, without touching its tables (tests/call_order_cases.py holds the
families, the readers and the inputs): after every family the call - fixed batch uploaded again, one launch, the call at every n -
returns the bytes it returns alone on a fresh context, between two other observables as well as after them; and no reader notices
that the call ran.

Contexts of capacity call_order_cases.CAPACITY, created and closed here; at most one is open at a time."""
import time

import numpy as np
import pytest

import call_order_cases as C
from qmps_amd import EnergyEngine

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 4)


def fresh(D):
    return EnergyEngine(D, C.CAPACITY)


def _call(eng, D):
    out = {}
    for n in NS:
        p, S, rho = eng.block_entanglement(n, C.B, want_rdm=True)
        out.update({f'rho{n}': rho.copy(), f'p{n}': p.copy(), f'S{n}': S.copy()})
    return out


def block_family(eng, D):
    """the new call as a self-contained family: it uploads what it reads; the call runs before, between and after the other observables
    of the resident states and must return the same bytes each time"""
    I = C.inputs(D)
    C.canon(eng)
    C._solve_for_observables(eng, I)
    first = _call(eng, D)
    eng.correlators(I['ops'], C.N_MAX, C.B)
    between = _call(eng, D)
    eng.entanglement(C.B)
    eng.correlator_sums(I['ops'], C.Z, C.B)
    last = _call(eng, D)
    assert all(same(first[k], between[k]) and same(first[k], last[k]) for k in first), sorted(k for k in first if not (same(first[k], between[k]) and same(first[k], last[k])))
    E, it, status = eng.results(C.B)
    return dict(first, E=E.copy(), iters=it.copy(), status=status.copy(), r=eng.environments(C.B).copy(), A=eng.tensors(C.B).copy())


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize('D', C.DS)
def test_the_call_after_every_family_equals_alone(D):
    t0 = time.perf_counter()
    with fresh(D) as eng:
        alone = block_family(eng, D)
    for n in NS:
        assert np.isfinite(alone[f'rho{n}']).all() and alone[f'rho{n}'].shape == (C.B, 2 ** n, 2 ** n) and alone[f'p{n}'].shape == (C.B, 2 ** n)
        assert np.isfinite(alone[f'p{n}']).all() and np.isfinite(alone[f'S{n}']).all()
    failures = []
    for X in C.legal(D):
        with fresh(D) as eng:
            C.canon(eng)
            C.FAMILIES[X].run(eng, D, C.inputs(D))
            got = block_family(eng, D)
        bad = sorted(k for k in alone if not same(alone[k], got[k]))
        if bad:
            failures.append((X, bad))
    print(f'block entanglement D = {D}: after each of {len(C.legal(D))} families, {time.perf_counter() - t0:.2f} s')
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
            got = C._refusal(lambda: tuple(_call(eng, D).values()))
            assert isinstance(got[0], str) != succeeds, got[:2]
            after = {r: C.read(eng, r, C.B) for r in legal}
        failures += [r for r in legal if not _same_outcome(before[r], after[r])]
    print(f'block entanglement D = {D}: {len(C.READERS)} readers, {time.perf_counter() - t0:.2f} s')
    assert not failures, failures
