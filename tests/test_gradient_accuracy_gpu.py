"""GPU: qmps_overlap_gradient against the references and bounds of tests/gradient_cases.py - the documented formula in long double at
the kernels' own h (the h^2 term is common and cancels: at h = 1e-2 only rounding and the residual term are left) and the exact
derivative - on every ansatz kind, every neighbour build (in the pair launch, beside the solves, inline), every solver route, warm
starts, loose tolerances and a mask inside a wave.  Every call asserts status 0 on every row; no row is left out."""
import numpy as np
import pytest

import batch_edge_cases as BE
import gradient_cases as GC

pytestmark = pytest.mark.gpu

F_TOL = 1e-10          # f of a gradient call against the dense eigen-solve (tests/test_batch_edges_gpu.py)
TOL = 1e-13
CASES = GC.cases()


def check(D, kind, name, h, tol, f, g, st, label, f_too=True):
    """Statuses, both bounds elementwise, f; prints the worst fractions (gradient_cases.fractions) and returns them."""
    ref = GC.references(D, kind, name)
    assert np.all(st == 0), (label, D, kind, name, h, tol, st)
    df = float(np.abs(f - ref['f']).max())
    ef, ex = np.abs(g - GC.g_formula(D, kind, name, h)), np.abs(g - ref['g_exact'])
    bf, bx = GC.formula_bound(D, kind, name, h, tol), GC.exact_bound(D, kind, name, h, tol)
    fa, fb = GC.fractions(D, kind, name, h, tol, g)
    print(f'gradient accuracy D={D} kind={kind} {name} {label} h={h:.0e} tol={tol:.0e}: formula {fa:.3f}, beyond the references\' distance {fb:.3f} of the formula bound, '
          f'max |dg| {ef.max():.2e} (exact {ex.max():.2e}), |df| {df:.1e}')
    assert np.all(ef <= bf), (label, D, kind, name, h, tol, float((ef / bf).max()), np.argwhere(ef > bf)[:4].tolist())
    assert np.all(ex <= bx), (label, D, kind, name, h, tol, float((ex / bx).max()), np.argwhere(ex > bx)[:4].tolist())
    if f_too:
        assert df < F_TOL, (label, D, kind, name, h, tol, df)
    return fa, fb


def run(eng, D, kind, name, h, tol=TOL, label='default', **kw):
    ref, X, WW = GC.pool(D, kind, name)
    eng.overlap_set_refs_params(kind, ref, WW)
    f, g, st = eng.overlap_gradient(kind, X, h=h, tol=tol, **kw)
    return check(D, kind, name, h, tol, f, g, st, label, f_too=tol <= 1e-12 or kw.get('two_sided_f', False))


@pytest.mark.parametrize('D,kind', CASES)
def test_gradient_of_every_kind_against_formula_and_exact_derivative(D, kind, engine_factory):
    """Near and far pools (one launch each: the operator differs), h = 1e-6, 1e-4, 1e-2, tol = 1e-13: D = 4 by squaring, D = 8 in the pair
    launch with neighbours built beside it, D = 16 in the pair launch with the in-pair build (kinds 0, 3) or beside it (1, 4, 5)."""
    eng = engine_factory(D, 4096)
    for name in ('near', 'far'):
        if name in GC.pool_names(D, kind):
            for h in GC.HS:
                run(eng, D, kind, name, h)


@pytest.mark.parametrize('D,kind', [c for c in CASES if c[0] >= 8])
def test_gradient_bounds_grow_with_the_tolerance_of_the_solves(D, kind, engine_factory):
    """tol = 1e-10, 1e-8 (what the BFGS drivers run with): the same bounds, whose residual term grows with tol; with the two-sided
    objective f stays within F_TOL all the same."""
    eng = engine_factory(D, 4096)
    for name in ('near', 'far'):
        if name not in GC.pool_names(D, kind):
            continue
        for tol in (1e-10, 1e-8):
            for two_sided_f in (False, True):
                for h in GC.HS:
                    run(eng, D, kind, name, h, tol=tol, label=f'two_sided_f={two_sided_f}', two_sided_f=two_sided_f)


@pytest.mark.parametrize('D,kind', CASES)
def test_warm_gradient_against_its_own_references(D, kind, engine_factory):
    """Cold at X, warm at X + 1e-3 N from the resident fixed points: the warm call meets the bounds of ITS iterates (the near pool; the
    far pool for ExactAfter4 at D = 8, 16, which has no near rows)."""
    eng = engine_factory(D, 4096)
    warm = [name for name in GC.pool_names(D, kind) if name in GC.COLD_OF][0]
    for h in GC.HS:
        run(eng, D, kind, GC.COLD_OF[warm], h, label='cold')
        run(eng, D, kind, warm, h, label='warm', warm=True)


@pytest.mark.parametrize('D,switch,kind', [(4, 'QMPS_OVERLAP_POWER', 0), (4, 'QMPS_OVERLAP_POWER', 1), (16, 'QMPS_D16_BLOCK', 0), (16, 'QMPS_D16_BLOCK', 4),
                                           (16, 'QMPS_D16_ONE_WAVE', 0), (16, 'QMPS_D16_ONE_WAVE', 5)])
def test_gradient_on_the_separate_solve_routes(D, switch, kind, engine_factory, monkeypatch):
    """The routes off the default: the block kernel's power method at D = 4 (max_rounds is its power-step cap) and D = 16, one wave per
    evaluation at D = 16 - two separate solves, neighbours beside them whatever the kind.  Cold and warm."""
    eng = engine_factory(D, 4096)
    monkeypatch.setenv(switch, '1')
    for name in GC.pool_names(D, kind):
        for h in GC.HS:
            if name in GC.COLD_OF:
                run(eng, D, kind, GC.COLD_OF[name], h, label=switch, max_rounds=100000)
            run(eng, D, kind, name, h, label=switch + (' warm' if name in GC.COLD_OF else ''), max_rounds=100000, warm=name in GC.COLD_OF)


@pytest.mark.parametrize('D,kind', [(4, 0), (4, 1), (8, 0), (8, 4)])
def test_gradient_with_the_inline_neighbour_build(D, kind, engine_factory):
    """More than 1 024 iterates: the neighbour tensors are built on the solves' own stream.  The pools tiled to 1 025 + a tail: the
    members meet the bounds, the copies are byte-identical."""
    eng = engine_factory(D)
    n = GC.rows(D, kind)
    T = 1025 + n + 1
    for name in ('near', 'far'):
        ref, X, WW = GC.pool(D, kind, name)
        eng.overlap_set_refs_params(kind, BE.tile(ref, T), WW)
        for h in GC.HS:
            f, g, st = eng.overlap_gradient(kind, BE.tile(X, T), h=h, tol=TOL)
            check(D, kind, name, h, TOL, f[:n], g[:n], st[:n], f'inline T={T}')
            idx = np.arange(T) % n
            assert np.all(st == 0) and np.array_equal(f, f[idx]) and np.array_equal(g, g[idx]), (D, kind, name, h, np.flatnonzero(np.any(g != g[idx], axis=1))[:8])


@pytest.mark.parametrize('kind', [0, 5])
def test_mask_inside_a_wave_keeps_skipped_rows_and_meets_the_bounds_on_the_rest(kind, engine_factory):
    """D = 4, four iterates per wave: masks that cut through waves after a full call at other parameters.  A skipped row keeps f of the
    earlier call bit for bit and its g is what that call's neighbours give - the same bits at the same h, the earlier differences over
    the new 2h otherwise; the active rows meet the bounds of their new iterates."""
    D, h = 4, 1e-2
    eng = engine_factory(D, 4096)
    ref, X, WW = GC.pool(D, kind, 'near')
    Xw = GC.pool(D, kind, 'warm')[1]
    n = len(X)
    eng.overlap_set_refs_params(kind, ref, WW)
    for pattern, h2 in (([1, 0, 1, 1, 0], h), ([0, 0, 0, 1], h), ([1, 1, 0, 1, 0, 0, 1], 1e-4)):
        f0, g0, st0 = eng.overlap_gradient(kind, X, h=h, tol=TOL)
        check(D, kind, 'near', h, TOL, f0, g0, st0, 'before the mask')
        active = np.array([pattern[t % len(pattern)] for t in range(n)], dtype=bool)
        eng.overlap_set_active(active)
        f1, g1, st1 = eng.overlap_gradient(kind, Xw, h=h2, tol=TOL)
        assert np.all(st1 == 0)
        assert np.array_equal(f1[~active], f0[~active])
        if h2 == h:
            assert np.array_equal(g1[~active], g0[~active])
        else:
            assert np.allclose(g1[~active], g0[~active] * (h / h2), rtol=1e-14, atol=0.0)
        merged_f, merged_g = np.where(active, f1, GC.references(D, kind, 'warm')['f']), np.where(active[:, None], g1, GC.g_formula(D, kind, 'warm', h2))
        check(D, kind, 'warm', h2, TOL, merged_f, merged_g, st1, f'mask {pattern}')
