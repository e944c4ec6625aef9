"""GPU: the cold-start D = 4 energy kernels take the two-site density matrix from the site factors of the acceptance step
(DirectD4::power_step_sites / update_sites / density_sites, qmps_direct_core.h; CPU: test_site_factors_cpu.py).  Energies against the C
oracle and against the density matrices of the energy-only kernel (eng.rdm(): the route from the tensor) at the batch sizes where a wave
is a lone quad, partial, full, and one past a tile boundary; waves that mix accepted evaluations with the power fall-back, and status 0
with status 2: no row depends on its wave-mates; the ansatz instantiations against the tensor route.

Measured on one MI355X: E against the oracle at most 5.5e-13 and against E(rho) 1.0e-15 (0.002 of the bound); 54 of 436 structured rows
fall back, 24 of 27 waves mixed, fall-back rows 3.6e-15 from the closed form and 3.3e-16 from their own environment; 15 of 49 rows
status 2 in 3 mixed waves; ansatz kernel 1.1e-15 and rotosolve 2.7e-15 from the tensor kernel; every bit-for-bit comparison holds."""
import itertools

import numpy as np
import pytest

from oracle import qmps_oracle as O
from qmps_amd import _lib
from tests import rho_need_cases as RN
from tests import site_factor_cases as SF

pytestmark = pytest.mark.gpu

E_TOL = 1e-10          # tests/test_energy_gpu.py: energies against the oracle
SHAPES = [1, 15, 16, 17, 33]
HAMS = {'tfim': RN.TFIM, 'xxz': RN.XXZ, 'complex_hermitian': RN.COMPLEX_HERMITIAN, 'three_terms': RN.THREE_TERMS}


@pytest.mark.parametrize('B', SHAPES)
def test_energies_against_the_oracle_and_the_density_matrix(B, c_oracle, engine_factory):
    eng = engine_factory(4, 64)
    eng.set_solver('direct')
    A = O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(6000 + B), 8, B))
    for name, h in HAMS.items():
        h = np.asarray(h).reshape(-1, 4, 4)
        E, it, st = eng.energies(A, h)
        assert np.all(st == 0) and np.all(it == 1), name
        r, rho = eng.environments(), eng.rdm()
        from_rho = np.real(np.einsum('nst,bts->bn', h, rho))
        tol = SF.energy_tol(A, r, h)
        ref = c_oracle.energy_batch(A, h)
        err_o = np.abs(E - np.asarray(ref['E']).reshape(E.shape)).max()
        err_r = np.abs(E - from_rho).max(axis=1)
        print(f'{name} B={B}: |E - oracle| {err_o:.2e}, |E - E(rho)| {err_r.max():.2e} (x tol {(err_r / tol).max():.3f})')
        assert np.all(ref['status'] == 0) and err_o < E_TOL, name
        assert np.all(err_r <= tol), name


def structured_batch():
    """ShallowCNOT depth-2 tensors on the grid of multiples of pi / 4 (product states, degenerate transfer spectra: the direct solve is
    refused), 1e-9 beside them, and random angles, shuffled: 436 rows = 27 waves and a quarter, most of them mixed."""
    grid = np.array([0, np.pi / 4, np.pi / 2, np.pi, -np.pi / 2, 3 * np.pi / 4])
    base = np.array(list(itertools.product(grid, repeat=4)))[::7]
    rng = np.random.default_rng(6060)
    prm = np.concatenate([base, base + 1e-9 * rng.standard_normal(base.shape), 2 * rng.standard_normal((64, 4))])
    prm = prm[rng.permutation(len(prm))]
    return np.stack([O.unitary_to_tensor(O.shallow_cnot_unitary(4, p)[None])[0] for p in prm])


def test_fall_back_rows_beside_accepted_rows(engine_factory):
    """One batch whose waves mix accepted evaluations with evaluations that take the power fall-back (they take the W of their final
    environment in a wave-uniform branch, with a select per evaluation).  Fall-back rows with a separated spectrum: the closed-form oracle;
    accepted rows: bit for bit what they give in a batch without any fall-back row."""
    A = structured_batch()
    B = len(A)
    h = np.stack([RN.TFIM, RN.XXZ])
    eng = engine_factory(4, 8192)
    eng.set_solver('direct')
    E, it, st = eng.energies(A, h, max_iter=100000)
    r = eng.environments()
    fb = it > 1
    mixed = sum(1 for g in range(B // 16) if 0 < fb[16 * g:16 * g + 16].sum() < 16)
    print(f'rows {B}, fall-back {fb.sum()}, status 0 / 1 / 2: {[(st == k).sum() for k in range(3)]}, mixed waves {mixed} of {B // 16}')
    assert fb.sum() >= 30 and (~fb).sum() >= 300 and mixed >= 10
    assert np.all(np.log2(it[fb] - 1) % 1 == 0)
    T = np.einsum('bsij,bskl->bikjl', A, A.conj()).reshape(B, 16, 16)
    w = np.sort(np.abs(np.linalg.eigvals(T)), axis=1)[:, ::-1]
    gap = w[:, 0] - w[:, 1]
    sel = np.flatnonzero(fb & (st != 1) & (gap > 1e-6))
    assert len(sel) >= 10
    worst = 0.0
    for b in sel:
        for t in range(2):
            err = abs(E[b, t] - O.energy_closed_form(A[b], h[t]))
            worst = max(worst, err)
            assert err < 1e-9 * max(1.0, 1e-6 / gap[b]), (b, t)        # (tests/test_direct_gpu.py::test_structured_angles_stress)
    # every fall-back row that converged, whatever its spectrum: E from the kernel's own environment in numpy
    conv = np.flatnonzero(fb & (st != 1))
    E_own = np.real(np.einsum('nst,bts->bn', h, SF.rho_numpy(A[conv], r[conv])))
    err_own = np.abs(E[conv] - E_own).max(axis=1)
    tol = SF.energy_tol(A[conv], r[conv], h)
    print(f'fall-back rows: {len(sel)} against the closed form, worst {worst:.2e}; {len(conv)} against their own environment, '
          f'worst {err_own.max():.2e} (x tol {(err_own / tol).max():.3f})')
    assert np.all(err_own <= tol)
    keep = np.flatnonzero(~fb)
    E2, it2, st2 = eng.energies(A[keep], h, max_iter=100000)
    r2 = eng.environments()
    assert np.all(it2 == 1)
    assert np.array_equal(E2, E[keep]) and np.array_equal(st2, st[keep]) and np.array_equal(r2, r[keep])


def test_status_2_rows_beside_status_0_rows(engine_factory):
    """Near-singular environments (tests/conditioning_cases.py, t <= 3e-5 behind the gauge: the pivot test splits them) and Haar rows in
    the same waves: each status launched on its own gives the same bits."""
    from tests import conditioning_cases as CC
    fam = CC.family(4)
    rows = np.flatnonzero(fam['gauged'] & (fam['t'] > 0) & (fam['t'] <= 3e-5))[::13][:40]
    A = np.concatenate([fam['A'][rows], O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(6100), 8, 9))])
    A = np.ascontiguousarray(A[np.random.default_rng(6101).permutation(len(A))])
    h = RN.THREE_TERMS
    eng = engine_factory(4, 64)
    eng.set_solver('direct')
    E, it, st = eng.energies(A, h)
    r = eng.environments()
    B = len(A)
    mixed = sum(1 for g in range((B + 15) // 16) if len(set(st[16 * g:16 * g + 16])) > 1)
    print(f'rows {B}, status 0 / 1 / 2: {[(st == k).sum() for k in range(3)]}, mixed waves {mixed}')
    assert np.all(it == 1) and (st == 2).sum() >= 8 and (st == 0).sum() >= 8 and not np.any(st == 1) and mixed >= 2
    E_own = np.real(np.einsum('nst,bts->bn', h, SF.rho_numpy(A, r)))
    assert np.all(np.abs(E - E_own).max(axis=1) <= SF.energy_tol(A, r, h))
    for status in (0, 2):
        k = np.flatnonzero(st == status)
        Ek, itk, stk = eng.energies(A[k], h)
        assert np.array_equal(Ek, E[k]) and np.array_equal(stk, st[k]) and np.array_equal(eng.environments(), r[k]), status


def test_ansatz_kernels_against_the_tensor_route(engine_factory):
    """The kernels that build the tensor in LDS from ShallowCNOT depth-2 angles (33 rows: two tiles and a lone quad) and the shift batches
    of a rotosolve sweep, against the tensor kernel on host-built tensors of the same angles.  The device's tensors are the host's to
    1e-13 (tests/test_api_gpu.py); the fixed-point solve amplifies that by at most 1 / gap: 1e-13 / gap on E (|h| ~ 1), 1e-11 at the least."""
    rng = np.random.default_rng(6200)
    prm = rng.standard_normal((33, 4))
    h = np.stack([RN.TFIM, RN.COMPLEX_HERMITIAN])
    eng = engine_factory(4, 256)
    eng.set_solver('direct')

    def by_tensors(p):
        A = np.stack([O.unitary_to_tensor(O.shallow_cnot_unitary(4, x)[None])[0] for x in p])
        T = np.einsum('bsij,bskl->bikjl', A, A.conj()).reshape(len(A), 16, 16)
        w = np.sort(np.abs(np.linalg.eigvals(T)), axis=1)[:, ::-1]
        return eng.energies(A, h), (w[:, 0] - w[:, 1]).min()

    eng.set_hamiltonian(h)
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, prm)
    eng.launch(33)
    E, it, st = eng.results(33)
    (Et, itt, stt), gap = by_tensors(prm)
    print(f'ansatz kernel against the tensor kernel: {np.abs(E - Et).max():.2e}, smallest gap {gap:.2e}')
    assert np.all(st == 0) and np.array_equal(it, itt) and np.array_equal(st, stt)
    assert np.abs(E - Et).max() < max(1e-11, 1e-13 / gap)
    # two rotosolve sweeps (three shifts per angle: the kernel adds them to the resident angles), then the energies at the final angles
    eng.set_hamiltonian(RN.TFIM)
    hist, pfin = eng.rotosolve(_lib.ANSATZ_SHALLOW_CNOT, prm[:12], 2)
    eng.set_hamiltonian(h)
    (Ef, _, stf), gap = by_tensors(pfin)
    print(f'rotosolve final energies against the tensor kernel: {np.nanmax(np.abs(hist[-1] - Ef[:, 0])):.2e}, smallest gap {gap:.2e}')
    assert np.all(stf == 0)
    assert np.abs(hist[-1] - Ef[:, 0]).max() < max(1e-11, 1e-13 / gap)
