"""CPU: tests/two_site_sum_cases.py checked without a GPU - the bound rule against float64 numpy on every case of the module, the
resolvent reference against the long-double series over n >= 2, the embedded one-site operators against the one-site structure
factor, the product states against the closed form, the symmetries of the near terms, and the C-ABI checks that need no device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import correlator_cases as K
import structure_factor_cases as S
import two_site_sum_cases as T2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = np.array([0.0, 0.7, np.pi])


@pytest.mark.parametrize('D', T2.DS)
def test_float64_stays_within_a_third_of_both_bounds(D):
    """The rule the bounds state for themselves: float64 numpy (np.linalg.solve on the same matrix and right-hand sides) within a third
    of C_G 2^-52 kappa for G and of C_NEAR 2^-52 for one and near, on every case of the module: all Haar rows, the small-gap family,
    the product rows; all eight operators; all six points."""
    ops = T2.all_ops()
    rows = T2.haar_rows(D)
    Af, rf, _ = S.family(D)
    Ap, rp, _ = T2.product_rows(D)
    worst_g, worst_n = 0.0, 0.0
    for name, A, r in (('Haar', K.haar_tensors(D)[:rows], S.haar_environments(D, rows)), ('family', Af, rf), ('product', Ap, rp)):
        Gl, onel, nearl = T2.reference(A, r, ops, T2.Z)
        Gd, oned, neard = T2.reference(A, r, ops, T2.Z, dtype=np.complex128)
        scale = T2.EPS * S.kappa(A, r, T2.Z)
        r_g = float((np.abs(Gd - Gl).max(axis=(2, 3)).astype(float) / scale).max())
        r_n = max(float(np.abs(oned - onel).max()), float(np.abs(neard - nearl).max())) / T2.EPS
        print(f'D={D} {name} ({len(A)} rows): G err / (2^-52 kappa) {r_g:.3f}, kappa up to {scale.max() / T2.EPS:.3g}; one, near {r_n:.2f} x 2^-52')
        worst_g, worst_n = max(worst_g, r_g), max(worst_n, r_n)
    print(f'D={D}: C_G = {T2.C_G:g} (worst x 3 = {3 * worst_g:.2f}), C_NEAR = {T2.C_NEAR:g} (worst x 3 = {3 * worst_n:.1f})')
    assert worst_g <= T2.C_G / 3
    assert worst_n <= T2.C_NEAR / 3
    assert T2.C_G <= 5 and T2.C_NEAR <= 40


def _series_rows(D):
    A, _, t = S.family(D)
    return [('Haar', a) for a in K.haar_tensors(D)[:3]] + [('t=0.5', a) for a in A[t == 0.5]]


@pytest.mark.parametrize('D', (2, 4, 8))
def test_resolvent_reference_equals_the_series(D):
    """G of the reference against sum_(n = 2 .. N) z^n (<O_a(0,1) O_c(n,n+1)> - one one), both in long double on an unrounded
    long-double fixed point, N with |lambda_2|^N < 1e-22 as in tests/test_structure_factor_cases_cpu.py; at all six points."""
    ops = T2.generic_ops()[:3]
    for name, A in _series_rows(D):
        lam2 = 1.0 - S.gap(A)
        n_terms = int(math.ceil(math.log(1e-22) / math.log(lam2))) + 1
        r = S.power_fixed_point(A, n_terms + 50)
        G, _, _ = T2.reference(A[None], r[None], ops, T2.Z)
        ser = T2.series(A, r, ops, T2.Z, n_terms + 1)
        err = float(np.abs(G[0] - ser).max())
        print(f'D={D} {name}: |lambda_2| = {lam2:.4f}, n <= {n_terms + 1}, resolvent - series {err:.2e}')
        assert err < 1e-10
    # a sum that started at n = 1, or a wrong power of z, is not a rounding matter
    assert float(np.abs(G[0, 5] - ser[5] / T2.Z[5]).max()) > 1e-3


@pytest.mark.parametrize('D', (2, 4))
def test_embedded_one_site_operators_reproduce_the_one_site_structure_factor(D):
    """h = O (x) 1 and h = 1 (x) O: S_hh(k) = S_OO(k) of structure_factor_cases.reference at k = 0, 0.7, pi, and the mixed entries
    carry the phase of the shifted support, S_(O1, 1O)(k) = e^(+ik) S_OO(k).  Long double on both sides."""
    A, r = K.haar_tensors(D)[:5], S.haar_environments(D, 5)
    z = S.k_to_z(KS)
    for O1 in K.generic_ops()[:2]:
        G, one, near = T2.reference(A, r, T2.embedded_ops(O1), z)
        S2 = T2.structure_factor(G, one, near, z)
        S1 = S.structure_factor(*S.reference(A, r, O1[None], z))[:, :, 0, 0]
        ph = np.exp(1j * KS)[None]
        err = max(float(np.abs(S2[:, :, 0, 0] - S1).max()), float(np.abs(S2[:, :, 1, 1] - S1).max()),
                  float(np.abs(S2[:, :, 0, 1] - ph * S1).max()), float(np.abs(S2[:, :, 1, 0] - S1 / ph).max()))
        print(f'D={D}: two-site S of the embedded operator - one-site S {err:.2e}')
        # (r is the fixed point to float64 only, and A^+ A = 1 likewise: the two supports differ by that much, not by long-double rounding)
        assert err < 1e-15 * max(1.0, float(np.abs(S1).max()))


@pytest.mark.parametrize('D', T2.DS)
def test_product_rows_give_the_closed_form(D):
    """H = sum ZZ on the product state with <Z> = c: 1 + 2 c^2 - 3 c^4 per site; th = 0 is an eigenstate (0)."""
    A, r, c = T2.product_rows(D)
    z = S.k_to_z([0.0])
    for dtype in (T2.CLD, np.complex128):
        G, one, near = T2.reference(A, r, T2.ZZ[None], z, dtype=dtype)
        var = T2.structure_factor(G, one, near, z)[:, 0, 0, 0]
        assert np.abs(var - T2.zz_variance(c)).max() <= T2.bound_S(A, r, [0.0]).max()
        assert not G.any() and var[0] == 0
        assert np.abs(one[:, 0] - c ** 2).max() <= T2.bound_near()


@pytest.mark.parametrize('D', (2, 4, 8))
def test_hermitian_operators_real_nonnegative_and_mirrored(D):
    """S_hh(k) of Hermitian h is real and >= 0 up to the bound; the left neighbour is the mirror image of the right one,
    near[a, c, 2] = conj(near[c, a, 1]), for Hermitian operators - and not for the generic ones."""
    rows = 17
    A, r = K.haar_tensors(D)[:rows], S.haar_environments(D, rows)
    z = S.k_to_z(KS)
    G, one, near = T2.reference(A, r, T2.hermitian_ops(), z, dtype=np.complex128)
    Sq = T2.structure_factor(G, one, near, z)
    bnd = T2.bound_S(A, r, KS)
    for a in range(2):
        assert np.all(np.abs(Sq[:, :, a, a].imag) <= bnd) and np.all(Sq[:, :, a, a].real >= -bnd)
    assert np.linalg.eigvalsh((Sq + Sq.conj().swapaxes(-1, -2)) / 2).min() >= -3 * bnd.max()
    assert np.abs(near[..., 2] - near[..., 1].conj().swapaxes(-1, -2)).max() <= 2 * T2.bound_near()
    assert np.abs(one.imag).max() <= T2.bound_near()
    _, _, near_g = T2.reference(A, r, T2.generic_ops(), z[:1], dtype=np.complex128)
    assert np.abs(near_g[..., 2] - near_g[..., 1].conj().swapaxes(-1, -2)).max() > 1e-2


def test_symbol_is_declared_bound_and_refuses_a_null_context():
    from qmps_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'qmps_hip.h')).read()
    assert re.search(r'^int qmps_correlator_sums_two_site\(qmps_ctx\* ctx, int64_t B, int n_ops, const double\* ops', header, flags=re.M)
    assert 'qmps_correlator_sums_two_site' in header.split('int qmps_abi_minor(void);')[0].split('Added later without a bump')[1]
    assert re.search(r'#define QMPS_ABI_MINOR 7\b', header)
    assert _lib.SIGNATURES['qmps_correlator_sums_two_site'] == _lib.SIGNATURES['qmps_correlator_sums']
    lib = _lib.load()
    ops = np.ascontiguousarray(T2.generic_ops()).view(np.float64)
    z = np.ascontiguousarray(T2.Z).view(np.float64)
    out = np.zeros(2 * 16 * 6)
    dp = ctypes.POINTER(ctypes.c_double)
    f = lambda a: a.ctypes.data_as(dp)
    rc = lib.qmps_correlator_sums_two_site(None, 1, 4, f(ops), 6, f(z), f(out), None, None)
    assert rc == _lib.QMPS_ERR_ARG and b'null context' in lib.qmps_last_error()
    assert not out.any()


def test_engine_tells_the_operator_shapes_apart():
    """(m, 4, 4) and (4, 4) are two-site, (m, 2, 2) and (2, 2) one-site, everything else a ValueError - decided before any library call."""
    from qmps_amd import engine
    assert engine._two_site_ops(np.zeros((4, 4))).shape == (1, 4, 4) and engine._two_site_ops(np.zeros((3, 4, 4))).shape == (3, 4, 4)
    assert engine._two_site_ops(np.zeros((4, 2, 2))) is None and engine._two_site_ops(np.zeros((2, 2))) is None
    for shape in ((2, 4, 3), (4, 3), (2, 3, 2), (16,)):
        assert engine._two_site_ops(np.zeros(shape)) is None
        with pytest.raises(ValueError):
            engine._one_site_ops(np.zeros(shape))
