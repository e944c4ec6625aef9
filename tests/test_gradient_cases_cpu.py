"""CPU: the references and bounds of tests/gradient_cases.py are checked before any kernel is held to them - the two Richardson ladders
of the exact derivative agree, the documented formula in long double is within 1e-9 of it at h = 1e-6 and follows its h^2 law, two float64
ports of the method stay within a third of both bounds, and four deliberately wrong ports leave the bound on every row they touch."""
import numpy as np
import pytest

import gradient_cases as GC

TOLS = (1e-13, 1e-10)


def _each(D):
    return [(kind, name) for DD, kind in GC.cases() if DD == D for name in GC.pool_names(D, kind)]


@pytest.mark.parametrize('D', GC.DS)
def test_pools_have_their_rows_bands_and_tails(D):
    for DD, kind in GC.cases():
        if DD != D:
            continue
        p, n = GC.pools(D, kind), GC.rows(D, kind)
        assert n % (64 // (D * D) if D == 4 else 2) != 0                     # a lane tail at D = 4, an odd batch above
        assert GC.n_params(D, kind) <= 64 and GC.n_params(D, kind) % GC.AC.per_layer(kind, D) == 0
        assert p['X_far'].shape == (n, GC.n_params(D, kind)) and sorted(np.bincount(p['band_far'], minlength=3)) == sorted(n // 3 + (b < n % 3) for b in range(3))
        far = GC.references(D, kind, 'far')
        for b, (lo, hi) in enumerate(GC.BANDS):
            q = far['ratio'][p['band_far'] == b]
            assert np.all((q >= lo) & (q < hi)), (D, kind, b, q)
        if (D, kind) in GC.NO_NEAR:
            assert len(p['X_near']) == 0 and 1e-4 < np.abs(p['X_far_warm'] - p['X_far']).max() < 1e-2
            continue
        assert p['X_near'].shape == p['X_warm'].shape == (n, GC.n_params(D, kind))
        assert 1e-4 < np.abs(p['X_warm'] - p['X_near']).max() < 1e-2 and 1e-3 < np.abs(p['X_near'] - p['ref_near']).max() < 0.2


@pytest.mark.parametrize('D', GC.DS)
def test_ladders_agree_and_the_formula_is_the_derivative_to_second_order(D):
    """The two ladders agree to 1e-11 on every row (references() raises otherwise; asserted again); g_formula(1e-6) is within 1e-9 of
    g_exact - the claim of include/qmps_hip.h; where |g_formula(1e-2) - g_exact| > 1e-9 its ratio to the same at h = 1e-3 lies in [50, 200]."""
    worst_l = worst_6 = 0.0
    lo, hi, n_law = np.inf, 0.0, 0
    for kind, name in _each(D):
        ref = GC.references(D, kind, name)
        worst_l = max(worst_l, ref['ladder'].max())
        assert ref['residual'].max() < 1e-17
        d6 = np.abs(GC.g_formula(D, kind, name, 1e-6) - ref['g_exact'])
        worst_6 = max(worst_6, d6.max())
        assert d6.max() < 1e-9, (D, kind, name, d6.max())
        d2, d3 = np.abs(GC.g_formula(D, kind, name, 1e-2) - ref['g_exact']), np.abs(GC.g_formula(D, kind, name, 1e-3) - ref['g_exact'])
        law = d2 > 1e-9
        if law.any():
            q = d2[law] / d3[law]
            lo, hi, n_law = min(lo, q.min()), max(hi, q.max()), n_law + int(law.sum())
            assert np.all((q >= 50) & (q <= 200)), (D, kind, name, q.min(), q.max())
    print(f'gradient references D={D}: ladders {worst_l:.1e}, |g_formula(1e-6) - g_exact| {worst_6:.1e}, h^2 law on {n_law} entries: ratio {lo:.1f} .. {hi:.1f}')
    assert worst_l <= GC.LADDER_TOL and n_law > 0


@pytest.mark.parametrize('D', GC.DS)
def test_two_float64_ports_stay_within_a_third_of_both_bounds(D):
    worst = {}
    for kind, name in _each(D):
        f_ref = GC.references(D, kind, name)['f']
        for h in GC.HS:
            for label, tol in (('eig', 0.0),) + tuple(('power', tol) for tol in TOLS):      # (LAPACK's vectors answer to no tolerance)
                f, g = GC.port(D, kind, name, h, tol or None)
                fa, fb = GC.fractions(D, kind, name, h, tol, g)
                key = (kind, label)
                worst[key] = (max(worst.get(key, (0, 0))[0], fa), max(worst.get(key, (0, 0))[1], fb))
                assert np.abs(f - f_ref).max() < 1e-13 + tol * tol * 1e4
                assert fa <= 1 / 3 and fb <= 1 / 3, (D, kind, name, h, tol, label, fa, fb)
    for (kind, label), (fa, fb) in sorted(worst.items()):
        print(f'gradient ports D={D} kind={kind} {label}: worst fraction of the formula bound {fa:.3f}, of the exact bound {fb:.3f}')


@pytest.mark.parametrize('mutation', GC.MUTATIONS)
@pytest.mark.parametrize('D', GC.DS)
def test_the_bounds_bite(D, mutation):
    """A wrong element of G_s (1e-10 relative), conj dropped from y, s1 and s2 swapped in the probe contraction, one element of a
    neighbour tensor off by 1e-12: each leaves the device-against-formula bound at h = 1e-2 on EVERY row of every pool - but for the two
    small ones at D = 16, where that is not possible on every row (gradient_cases, "What the bounds can see"): there every row the
    mutation moves by 4/3 bounds or more must leave the bound, and these are 33 (G_s) and 46 (neighbour) of the 48 rows."""
    h, tol = 1e-2, 0.0          # (the mutated port takes y, r from LAPACK: its solves answer to no tolerance)
    least, n_rows, n_all = np.inf, 0, 0
    for kind, name in _each(D):
        _, g0 = GC.port(D, kind, name, h, None)
        _, g = GC.port(D, kind, name, h, None, mutate=mutation)
        bound = GC.formula_bound(D, kind, name, h, tol)
        per_row = (np.abs(g - GC.g_formula(D, kind, name, h)) / bound).max(axis=1)
        touched = np.ones(len(per_row), bool)
        if D == 16 and mutation in GC.SMALL_MUTATIONS:
            touched = (np.abs(g - g0) / bound).max(axis=1) >= 4 / 3
        least, n_rows, n_all = min([least] + list(per_row[touched])), n_rows + int(touched.sum()), n_all + len(touched)
        assert np.all(per_row[touched] > 1.0), (D, kind, name, mutation, per_row, touched)
    print(f'gradient bounds bite D={D} {mutation}: {n_rows} of {n_all} rows, the least affected at {least:.2f} bounds')
    assert n_rows == n_all or (D == 16 and n_rows >= {'G': 33, 'neighbour': 46}.get(mutation, n_all)), (D, mutation, n_rows, n_all)
