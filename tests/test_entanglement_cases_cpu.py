"""CPU: tests/entanglement_cases.py checked without a GPU - the long-double Jacobi reference against numpy.linalg.eigvalsh and analytic
spectra, the bounds against float64 numpy (LAPACK and the port of the kernels' own sweep) on the very cases the GPU tests use, and the
declaration of the C-ABI symbol."""
import ctypes
import os
import re

import numpy as np
import pytest

import entanglement_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _finite(D):
    return K.kinds(D) != 'nan'


@pytest.mark.parametrize('D', K.DS)
def test_reference_against_eigvalsh_and_analytic_spectra(D):
    M, (p, V, S) = K.case_matrices(D), K.case_reference(D)
    fin = _finite(D)
    assert p.dtype == np.longdouble and np.isnan(p[~fin]).all() and np.isnan(S[~fin]).all() and np.isnan(V[~fin].real).all()
    lap = np.stack([np.linalg.eigvalsh(K.herm(m) / np.trace(m).real)[::-1] for m in M[fin]])
    err = float(np.abs(lap - p[fin]).max())
    print(f'D={D}: reference vs eigvalsh {err:.2e} = {err / (D * K.EPS):.2f} D 2^-52')
    assert err <= K.eig_bound(D) / 3
    assert np.all(np.diff(p[fin].astype(float), axis=1) <= 0)
    assert np.abs(p[fin].sum(axis=1) - 1).max() < 1e-17
    # matrices built diagonal: the spectrum is the diagonal over its sum, to the last long-double digit
    for k, (name, r, _) in enumerate(K.cases(D)):
        if name.endswith(', diagonal'):
            q = np.sort(np.diag(r).real.astype(np.longdouble))[::-1]
            assert np.abs(p[k] - q / q.sum()).max() < 1e-18, name
    # the same spectrum in a Haar basis: the rotation is a float64 one, so only to float64 rounding
    for name, q in K.spectra(D).items():
        k = [n for n, _, _ in K.cases(D)].index(f'{name}, Haar basis')
        assert np.abs(p[k] - np.sort(q)[::-1] / q.sum()).max() < 20 * D * K.EPS, name


@pytest.mark.parametrize('D', K.DS)
def test_reference_meets_the_eigenvector_checks(D):
    M, (p, V, S) = K.case_matrices(D), K.case_reference(D)
    fin = _finite(D)
    orth, eq = K.residuals(M[fin], p[fin], V[fin])
    print(f'D={D}: reference |V^+ V - 1| {orth.max():.2e}, |h V - V p| {eq.max():.2e}')
    assert orth.max() <= K.eig_bound(D) / 100 and eq.max() <= K.eig_bound(D) / 100


@pytest.mark.parametrize('D', K.DS)
def test_float64_stays_within_a_third_of_the_bound(D):
    """The rule EIG_C states for itself: eigvalsh and the port of the kernels' sweep, every finite case; the port also meets the entropy
    bound and the two eigenvector bounds, and is done within half of the kernels' cap on sweeps (D = 2: the one rotation)."""
    M, (p, V, S) = K.case_matrices(D), K.case_reference(D)
    fin = _finite(D)
    u = D * K.EPS
    lap = np.stack([np.linalg.eigvalsh(K.herm(m) / np.trace(m).real)[::-1] for m in M[fin]])
    e_lap = float(np.abs(lap - p[fin]).max())
    pk, Vk, Sk, sweeps = K.kernel_port(M, want_sweeps=True)
    assert np.isnan(pk[~fin]).all() and np.isnan(Sk[~fin]).all() and np.isfinite(pk[fin]).all()
    e_port = float(np.abs(pk[fin] - p[fin]).max())
    e_S = float(np.abs(Sk[fin] - S[fin]).max())
    orth, eq = K.residuals(M[fin], pk[fin], Vk[fin])
    print(f'D={D}: eigvalsh {e_lap / u:.2f}, port {e_port / u:.2f} (D 2^-52; bound {K.EIG_C:.0f}); port S {e_S:.2e} ({e_S / K.entropy_bound(D):.4f} of its bound), '
          f'|V^+ V - 1| {orth.max() / u:.2f}, |h V - V p| {eq.max() / u:.2f} (D 2^-52); sweeps at most {sweeps.max()} (cap {K.SWEEP_CAP[D]})')
    assert e_lap <= K.eig_bound(D) / 3 and e_port <= K.eig_bound(D) / 3
    assert e_S <= K.entropy_bound(D)
    assert orth.max() <= K.eig_bound(D) and eq.max() <= K.eig_bound(D)
    assert 2 * sweeps.max() <= max(K.SWEEP_CAP[D], 2)


@pytest.mark.parametrize('D', K.DS)
def test_entropies_of_the_analytic_cases(D):
    names = [n for n, _, _ in K.cases(D)]
    p, V, S = K.case_reference(D)
    pk, Vk, Sk = K.kernel_port(K.case_matrices(D))
    for basis in ('Haar basis', 'diagonal'):
        for name, want in (('mixed', np.log(D)), ('product', 0.0), ('half', np.log(2.0))):
            k = names.index(f'{name}, {basis}')
            assert abs(float(S[k]) - want) <= K.entropy_bound(D), (name, basis)
            assert abs(Sk[k] - want) <= K.entropy_bound(D), (name, basis)
    k = names.index('indefinite')
    assert K.kinds(D)[k] == 'indefinite' and p[k, -1] < -0.1 and abs(float(p[k].sum()) - 1) < 1e-15
    pos = p[k][p[k] > 1e-12].astype(float)
    assert abs(float(S[k]) + (pos * np.log(pos)).sum()) < 1e-13          # the negative eigenvalue contributes nothing


@pytest.mark.parametrize('D', (4, 8, 16))
def test_tied_clusters_end_within_half_the_cap(D):
    """Haar-rotated clusters of k tied eigenvalues with zero, tiny and graded tails - the spectra on which a Jacobi sweep without the
    rule DROP2 hovers above its termination test: the port is done within half the cap, no NaN, eigenvalues within a third of the bound."""
    worst_sweeps, worst = 0, 0.0
    for k in sorted({2, 3, D // 2, D // 2 + 1, D - 2, D - 1} & set(range(2, D))):
        for t, tail in enumerate(K.TAILS):
            M, want = K.tied_cluster_batch(D, k, tail, 48, 6600 + 100 * D + 3 * k + t)
            p, V, S, sweeps = K.kernel_port(M, want_sweeps=True)
            assert np.isfinite(p).all(), (D, k, tail)
            worst_sweeps, worst = max(worst_sweeps, int(sweeps.max())), max(worst, float(np.abs(p - want).max()))
    print(f'D={D}: tied clusters, sweeps at most {worst_sweeps} (cap {K.SWEEP_CAP[D]}), |p - spectrum| {worst / (D * K.EPS):.2f} D 2^-52')
    assert 2 * worst_sweeps <= K.SWEEP_CAP[D]
    # (the spectrum is exact only up to the float64 rotation that built the matrix: a few roundings of entries of size 1 / k)
    assert worst <= K.eig_bound(D) / 3


def test_batches_cycle_the_cases():
    for D in K.DS:
        n = len(K.cases(D))
        kinds = K.kinds(D)
        assert n < 65 and kinds[0] == 'finite' and (kinds == 'nan').sum() == 2 and (kinds == 'indefinite').sum() == 1
        for k in np.where(kinds == 'nan')[0]:
            assert kinds[k - 1] != 'nan' and kinds[(k + 1) % n] != 'nan'
        idx = K.batch_index(D, 130)
        assert idx.max() == n - 1 and np.array_equal(K.batch(D, 130)[n:2 * n], K.case_matrices(D), equal_nan=True)
        assert K.round_robin(D)[0][0] == (0, D - 1)
        for pairs in K.round_robin(D):
            assert sorted(i for pq in pairs for i in pq) == list(range(D))
        assert len({pq for pairs in K.round_robin(D) for pq in pairs}) == D * (D - 1) // 2


def test_symbol_is_declared_and_bound():
    from qmps_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'qmps_hip.h')).read()
    assert re.search(r'^int qmps_entanglement\(qmps_ctx\* ctx, int64_t B, double\* p_out', header, flags=re.M)
    assert 'qmps_entanglement' in header.split('int qmps_abi_minor(void);')[0].split('Added later without a bump')[1]
    assert 'qmps_entanglement' in _lib.SIGNATURES
    lib = _lib.load()
    out = np.zeros(4)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.qmps_entanglement(None, 1, out.ctypes.data_as(dp), None, None)
    assert rc == _lib.QMPS_ERR_ARG and b'null context' in lib.qmps_last_error()
    assert not out.any()
    assert lib.qmps_abi_minor() == 7
