"""CPU: tests/structure_factor_cases.py checked without a GPU - the bound rule against float64 numpy and the float64 port of the
kernels' elimination on the very cases the GPU tests use, the gaps of the small-gap family, the resolvent reference against the
long-double series of correlator_cases.reference, the host composition of the structure factor, and the C-ABI check that needs no
device."""
import ctypes
import math

import numpy as np
import pytest

import correlator_cases as K
import structure_factor_cases as S


def _haar_rows(D):
    return K.HAAR_B if D <= 8 else max(S.D16_BATCHES)


@pytest.mark.parametrize('D', S.DS)
def test_float64_stays_within_a_third_and_the_port_within_the_bound(D):
    """The rule `structure_factor_cases.bound` states for itself: np.linalg.solve in float64 within a third on every case of the module;
    the float64 port of the kernels' Gauss-Jordan elimination within the bound; `one` and `site` within a third of theirs."""
    ops = K.generic_ops()
    rows = _haar_rows(D)
    Af, rf, _ = S.family(D)
    worst_np, worst_port = 0.0, 0.0
    for name, A, r in (('Haar', K.haar_tensors(D)[:rows], S.haar_environments(D, rows)), ('family', Af, rf)):
        Gl, onel, sitel = S.reference(A, r, ops, S.Z)
        Gd, oned, sited = S.reference(A, r, ops, S.Z, dtype=np.complex128)
        Gp = S.port(A, r, ops, S.Z)
        scale = S.EPS * S.kappa(A, r, S.Z)
        r_np = float((np.abs(Gd - Gl).max(axis=(2, 3)).astype(float) / scale).max())
        r_port = float((np.abs(Gp - Gl).max(axis=(2, 3)).astype(float) / scale).max())
        e_one = max(float(np.abs(oned - onel).max()), float(np.abs(sited - sitel).max()))
        print(f'D={D} {name} ({len(A)} rows): err / (2^-52 kappa) of np.linalg.solve {r_np:.3f}, of the port {r_port:.3f}; kappa up to '
              f'{scale.max() / S.EPS:.3g}; one, site {e_one:.2e}')
        worst_np, worst_port = max(worst_np, r_np), max(worst_port, r_port)
        assert e_one <= K.bound(D, 1) / 3
    print(f'D={D}: np.linalg.solve at {worst_np / S.C_BOUND:.3f} of the bound, the port at {worst_port / S.C_BOUND:.3f}')
    assert worst_np <= S.C_BOUND / 3
    assert worst_port <= S.C_BOUND
    assert S.C_BOUND <= 8


@pytest.mark.parametrize('D', (2, 4, 8))
def test_gaps_of_the_family(D):
    """1 - |lambda_2| of the first row of every t within a factor 3 of the table; ~0.4 t^2."""
    A, r, t = S.family(D)
    rows = S.family_rows(D)
    for n, want in enumerate(S.GAPS[D]):
        g = S.gap(A[n * rows])
        print(f'D={D} t={t[n * rows]}: 1 - |lambda_2| = {g:.3g} (table {want:.2g})')
        assert want / 3 <= g <= want * 3
    assert np.all(np.linalg.eigvalsh(r).min(axis=1) >= 1.5e-2)


def _series_rows(D):
    A, _, t = S.family(D)
    return [('Haar', a) for a in K.haar_tensors(D)[:3]] + [('t=0.5', a) for a in A[t == 0.5]]


@pytest.mark.parametrize('D', (2, 4, 8))
def test_resolvent_reference_equals_the_series(D):
    """G of the reference against sum_n z^n (C - one one) of correlator_cases.reference, both in long double on an unrounded long-double
    fixed point, with enough terms for |lambda_2|^n < 1e-22; and the composed structure factor against the two-sided sum."""
    ops = K.generic_ops()[:3]
    worst = 0.0
    for name, A in _series_rows(D):
        lam2 = 1.0 - S.gap(A)
        n_terms = int(math.ceil(math.log(1e-22) / math.log(lam2))) + 1
        r = S.power_fixed_point(A, n_terms + 50)
        G, one, site = S.reference(A[None], r[None], ops, S.Z)
        ser = S.series(A, r, ops, S.Z, n_terms)
        err = float(np.abs(G[0] - ser).max())
        worst = max(worst, err)
        print(f'D={D} {name}: |lambda_2| = {lam2:.4f}, {n_terms} terms, resolvent - series {err:.2e}')
        assert err < 1e-10
        # two-sided sum at k = 0.3: conn(0) = site - one one, conn(-n)[a, c] = conn(n)[c, a]
        kz = S.k_to_z([0.3])
        Gk, _, _ = S.reference(A[None], r[None], ops, kz)
        Sk = S.structure_factor(Gk, one, site)[0, 0]
        sk = S.series(A, r, ops, kz, n_terms)
        two_sided = site[0] - one[0][:, None] * one[0][None, :] + sk[0] + sk[1].T
        assert float(np.abs(Sk - two_sided).max()) < 1e-10
    # a wrong power of z, index or projector is not a rounding matter
    assert float(np.abs(G[0, 5] - ser[5] / S.Z[5]).max()) > 1e-3


def test_structure_factor_of_the_paulis_is_hermitian_and_positive():
    A = K.haar_tensors(4)[:4]
    r = S.haar_environments(4, 4)
    G, one, site = S.reference(A, r, K.PAULIS[1:], S.k_to_z([0.0, 0.3, np.pi]), dtype=np.complex128)
    Sq = S.structure_factor(G, one, site)
    assert Sq.shape == (4, 3, 3, 3)
    assert np.abs(Sq - Sq.conj().swapaxes(-1, -2)).max() < 1e-13
    assert np.linalg.eigvalsh((Sq + Sq.conj().swapaxes(-1, -2)) / 2).min() > -1e-13


@pytest.mark.parametrize('D', (2, 4))
def test_port_on_the_pass_through_tensor(D):
    """A0 with r = 1 / D: b_c vanishes exactly, so G is exactly zero wherever the resolvent exists (z = 0.5) and the elimination meets an
    exact zero pivot at z = 1, where it does not."""
    A0 = S.passthrough_tensor(D)[None]
    r = (np.eye(D) / D).astype(np.complex128)[None]
    G = S.port(A0, r, K.generic_ops(), [1.0, 0.5])
    assert not np.isfinite(G[0, 0]).any()
    assert not G[0, 1].any()


def test_null_context_is_refused_without_a_device():
    from qmps_amd import _lib
    assert 'qmps_correlator_sums' in _lib.SIGNATURES
    lib = _lib.load()
    ops = np.ascontiguousarray(K.PAULIS).view(np.float64)
    z = np.ascontiguousarray(S.Z).view(np.float64)
    out = np.zeros(2 * 16 * 6)
    dp = ctypes.POINTER(ctypes.c_double)
    f = lambda a: a.ctypes.data_as(dp)
    rc = lib.qmps_correlator_sums(None, 1, 4, f(ops), 6, f(z), f(out), None, None)
    assert rc == _lib.QMPS_ERR_ARG and b'null context' in lib.qmps_last_error()
    assert not out.any()
