"""CPU: tests/block_rdm_cases.py checked without a GPU - the two float64 orders and the port of the Jacobi kernels against the long-double
reference within the bounds the GPU tests use, the sweeps the cases need, the identities a block density matrix of an isometry with a
fixed-point environment obeys, and the declaration of the C-ABI symbol."""
import ctypes
import os
import re

import numpy as np
import pytest

import block_rdm_cases as K
import entanglement_cases as EC
from oracle import qmps_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('D', K.DS)
def test_float64_orders_stay_within_a_third_of_the_bound(D):
    """The rule RHO_C states for itself, every finite case and every n: both float64 orders within a third of the rho bound; the port of
    the Jacobi kernels on the float64 rho within the p and S bounds, without NaN and within the kernels' cap on sweeps."""
    worst = np.zeros(4)
    sweeps_at = {}
    for n in K.NS:
        rho_ref, p_ref, S_ref = K.case_reference(D, n)
        for k, (name, A, r, kind) in enumerate(K.cases(D)):
            if kind == 'nan':
                assert np.isnan(rho_ref[k].real).all() and np.isnan(p_ref[k]).all() and np.isnan(S_ref[k]), name
                continue
            scale = float(np.abs(rho_ref[k]).max())
            rho = K.gram_order(A, r, n)
            e_g = float(np.abs(rho - rho_ref[k]).max()) / K.rho_bound(D, n, scale)
            e_r = float(np.abs(K.recursion_order(A, r, n) - rho_ref[k]).max()) / K.rho_bound(D, n, scale)
            assert e_g <= 1 / 3 and e_r <= 1 / 3, (D, n, name, e_g, e_r)
            p, _, S, sweeps = EC.kernel_port(rho[None], want_sweeps=True)
            assert np.isfinite(p).all() and np.isfinite(S).all(), (D, n, name)
            assert sweeps[0] <= EC.SWEEP_CAP[2 ** n], (D, n, name, sweeps[0])
            e_p = float(np.abs(p[0] - p_ref[k]).max()) / K.p_bound(D, n, scale)
            e_S = float(abs(S[0] - S_ref[k])) / K.entropy_bound(D, n, scale)
            assert e_p <= 1 and e_S <= 1, (D, n, name, e_p, e_S)
            worst = np.maximum(worst, [e_g, e_r, e_p, e_S])
            sweeps_at[n] = max(sweeps_at.get(n, 0), int(sweeps[0]))
    print(f'block rdm D={D}: worst ratios to the bounds: gram_order {worst[0]:.2f}, recursion_order {worst[1]:.2f}, port p {worst[2]:.3f}, '
          f'port S {worst[3]:.4f}; sweeps at the orders 2 / 4 / 8 / 16: {" / ".join(str(sweeps_at[n]) for n in K.NS)}')


@pytest.mark.parametrize('D', K.DS)
def test_identities_of_isometries_with_fixed_point_environments(D):
    """To 1e-12 (the environment is a dense-eig fixed point: the tolerance rests on its residual, not on a solver setting): both partial
    traces of rho_n are rho_(n-1), tr rho = 1, rank at most min(2^n, D^2), rho_2 is the oracle's two-site density matrix; the product
    state has rank one and the spectrum (1, 0, ..)."""
    fixed = [(name, A, r, kind) for name, A, r, kind in K.cases(D) if kind in ('isometry', 'product')]
    assert len(fixed) == K.HAAR + 1
    for name, A, r, kind in fixed:
        assert np.abs(np.einsum('sji,sjk->ik', A.conj(), A) - np.eye(D)).max() < 1e-13, name
        assert np.abs(O.apply_transfer(A, r) - r).max() < 1e-13, name
        rhos = {n: K.reference_rho(A, r, n).astype(np.complex128) for n in K.NS}
        for n in K.NS:
            rho = rhos[n]
            assert abs(np.trace(rho) - 1) < 1e-12 and np.abs(rho - rho.conj().T).max() < 1e-12, (name, n)
            w = np.linalg.eigvalsh(EC.herm(rho))
            assert w.min() > -1e-12 and (w > 1e-12).sum() <= min(2 ** n, D * D), (name, n)
            if kind == 'product':
                assert abs(w[-1] - 1) < 1e-12 and np.abs(w[:-1]).max() < 1e-12, n
            if n > 1:
                right, left = K.partial_traces(rho)
                assert np.abs(right - rhos[n - 1]).max() < 1e-12 and np.abs(left - rhos[n - 1]).max() < 1e-12, (name, n)
        assert np.abs(rhos[2] - O.two_site_rdm(A, r)).max() < 1e-12, name


def test_index_order_is_that_of_merge_and_of_h():
    """t1 is the left site and the most significant bit: rho_2 contracted with a two-site h is the oracle's energy, and a one-site
    operator on the left site of three is np.kron(O, 1, 1)."""
    D = 4
    name, A, r, kind = K.cases(D)[0]
    h = O.hamiltonian_matrix({'ZZ': -1, 'X': 1}) + 0.3 * O.hamiltonian_matrix({'ZY': 1})
    rho2 = K.gram_order(A, r, 2)
    assert abs(np.einsum('st,ts->', h, rho2).real - O.energy_closed_form(A, h, r)) < 1e-13
    rho1, rho3 = K.gram_order(A, r, 1), K.gram_order(A, r, 3)
    Z, X, one = O.PAULI['Z'], O.PAULI['X'], np.eye(2)
    assert abs(np.trace(np.kron(Z, np.kron(one, one)) @ rho3) - np.trace(Z @ rho1)) < 1e-13
    # <Z X 1> on three sites is <Z X> on two
    assert abs(np.trace(np.kron(np.kron(Z, X), one) @ rho3) - np.trace(np.kron(Z, X) @ rho2)) < 1e-13
    assert np.abs(K.recursion_order(A, r, 3) - rho3).max() < 1e-14


def test_batches_cycle_the_cases():
    for D in K.DS:
        n = len(K.cases(D))
        kinds = K.kinds(D)
        assert n < 17 and kinds[0] != 'nan' and (kinds == 'nan').sum() == 2 and (kinds == 'generic').sum() == K.GENERIC and (kinds == 'product').sum() == 1
        for k in np.where(kinds == 'nan')[0]:
            assert kinds[k - 1] != 'nan' and kinds[(k + 1) % n] != 'nan'
        names = [c[0] for c in K.cases(D)]
        r0 = K.cases(D)[names.index('tr r = 0')][2]
        assert np.trace(r0) == 0 and np.isfinite(r0.real).all() and np.abs(r0).max() > 0.1
        A, r = K.batch(D, 130)
        assert np.array_equal(A[n:2 * n], K.case_tensors(D)[0]) and np.array_equal(r[n:2 * n], K.case_tensors(D)[1], equal_nan=True)
        # the r of a generic case is far from Hermitian, its tensor far from an isometry
        for name, a, rr, kind in K.cases(D):
            if kind == 'generic':
                assert np.abs(rr - rr.conj().T).max() > 0.05 / D and np.abs(np.einsum('sji,sjk->ik', a.conj(), a) - np.eye(D)).max() > 0.05


def test_symbol_is_declared_and_bound():
    from qmps_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'qmps_hip.h')).read()
    assert re.search(r'^int qmps_block_entanglement\(qmps_ctx\* ctx, int64_t B, int n_sites,', header, flags=re.M)
    assert 'qmps_block_entanglement' in header.split('int qmps_abi_minor(void);')[0].split('Added later without a bump')[1]
    dp = ctypes.POINTER(ctypes.c_double)
    assert _lib.SIGNATURES['qmps_block_entanglement'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, dp, dp, dp])
    lib = _lib.load()
    out = np.zeros(8)
    # the checks of the call's own arguments come before the context is looked at, and write nothing
    for n_sites in (0, 5, -1):
        assert lib.qmps_block_entanglement(None, 1, n_sites, out.ctypes.data_as(dp), None, None) == _lib.QMPS_ERR_ARG
        assert b'n_sites' in lib.qmps_last_error()
    assert lib.qmps_block_entanglement(None, 1, 2, None, None, None) == _lib.QMPS_ERR_ARG and b'nothing to return' in lib.qmps_last_error()
    assert lib.qmps_block_entanglement(None, 1, 2, out.ctypes.data_as(dp), None, None) == _lib.QMPS_ERR_ARG and b'null context' in lib.qmps_last_error()
    assert not out.any()
    assert lib.qmps_abi_minor() == 7
