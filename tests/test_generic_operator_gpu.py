"""GPU: every site that applies the two-site operator, C_s = sum_t WW[s][t] A_t1 A_t2 with t = 2 t1 + t2, against the oracle with
operators that are neither symmetric nor invariant under exchanging the sites (tests/operator_cases.py): WW = exp(-i dt H), H a
random complex Hermitian matrix.  Every other test of the suite uses the identity, TFIM or XXZ - operators a kernel could read
transposed, or with the sites exchanged, without anyone noticing.  tests/test_operator_cases_cpu.py shows that on the inputs used
here each such mistake moves the compared number by 1e-6 at least (eta: 1e-5 .. 1e-1), against tolerances of 1e-10 (eta) and 1e-8
(recorded objectives).  D = 2 is blind to the exchange of sites by a symmetry of its map; D >= 4 carries that check.

One test per site:
  overlap_lane_kernel (qmps_overlap_d2.h)                 test_plain_solves[2-*], test_one_reference_per_candidate[2]
  overlap_square_d4_kernel (qmps_overlap_d4.h)            test_plain_solves[4-*], test_one_reference_per_candidate[4]
  overlap_block_kernel<4> (qmps_overlap_block.hip)        test_d4_power_method_in_a_child_process
  overlap_block_kernel<8> (qmps_overlap_block.hip)        test_plain_solves[8-*], test_one_reference_per_candidate[8]
  overlap_mfma_d16x4_kernel (four waves; qmps_overlap_d16.hip) test_plain_solves[16-*], test_one_reference_per_candidate[16]
  overlap_mfma_d16_kernel (one wave; qmps_overlap_d16.hip) test_d16_one_wave_kernel
  overlap_block_kernel<16> (qmps_overlap_block.hip)       test_d16_tile_kernel_in_a_child_process
  qmps_overlap_krylov.hip, D = 8 and D = 16               test_krylov_fallback
  overlap_g_kernel, overlap_g_d16_kernel, pair kernel     test_gradient_path (qmps_overlap_grad.hip; adjoint solves, probes)
  qmps_evolve_d2.hip (build_reference, lane solves)       test_device_resident_bfgs[2] (also QMPS_EVOLVE_D2_SQUARING)
  qmps_evolve_d4.hip (through qmps_overlap_d4.h)          test_device_resident_bfgs[4], test_device_rotosolve_d4
  qmps_evolve_d16.hip                                     test_device_resident_bfgs[16]
  lock-step driver, D = 8                                 test_lockstep_driver_d8
qmps_overlap_amp.hip has had a Haar operator since test_circuit_amplitude_for_given_environments.  Every test prints its worst
deviation from the oracle (pytest -s)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import evolve_replay as ER
import operator_cases as OP
from oracle import qmps_oracle as O
from qmps_amd import _lib as L

pytestmark = pytest.mark.gpu

ETA_TOL = 1e-10
F_TOL = 1e-8           # test_evolve_gpu.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def plain_reference(D, dt):
    """the oracle's (eta, r) of every candidate of a plain case: computed once, shared by the tests of one bond dimension"""
    A, cands, WW = OP.plain_case(D, dt)
    return [O.overlap_eta(A, c, WW) for c in cands]


def check(what, eta, st, r, refs):
    """every candidate: status 0, eta the oracle's, the fixed point the dense eigenvector's ray with unit Frobenius norm"""
    assert np.all(st == 0) and len(eta) == len(refs), (what, st)
    worst, worst_r = 0.0, 0.0
    for k, (ref, r_ref) in enumerate(refs):
        worst = max(worst, abs(eta[k] - ref))
        if r is not None:
            worst_r = max(worst_r, abs(abs(np.vdot(r_ref, r[k])) - 1.0), abs(np.linalg.norm(r[k]) - 1.0))
    print(f'{what}: max |eta - oracle| = {worst:.2e}, fixed point off the ray by {worst_r:.2e}')
    assert worst < ETA_TOL and worst_r < 1e-9, (what, worst, worst_r)


@pytest.mark.parametrize('dt', OP.DTS)
@pytest.mark.parametrize('D', [2, 4, 8, 16])
def test_plain_solves(D, dt, engine_factory):
    """qmps_overlap_batch with a shared reference and tensors as candidates: the lane kernel (D = 2), the squaring kernel (D = 4),
    overlap_block_kernel<8>, the four-wave matrix-core kernel (D = 16: a batch of 8)."""
    A, cands, WW = OP.plain_case(D, dt)
    eng = engine_factory(D, 4096)
    eta, rounds, st, r = eng.overlaps(A, cands, WW, want_r=True)
    check(f'plain solves D = {D} dt = {dt}', eta, st, r, plain_reference(D, dt))


@pytest.mark.parametrize('D', [2, 4, 8, 16])
def test_one_reference_per_candidate(D, engine_factory):
    """References and candidates as ansatz parameters, one reference per candidate (qmps_overlap_set_refs_ansatz): the kernels
    address their reference through overlap_ref_index."""
    ref, cand, WW = OP.refs_case(D)
    eng = engine_factory(D, 4096)
    eng.overlap_set_refs_params(OP.ANSATZ, ref, WW)
    eng.set_ansatz_params(OP.ANSATZ, cand)
    eng.overlap_launch(len(cand), tol=1e-13, want_r=True)
    eta, rounds, st, r = eng.overlap_results(len(cand), want_r=True)
    f = eng.overlap_objective(len(cand))
    check(f'one reference per candidate D = {D}', eta, st, r, [O.overlap_eta(OP.tensor(D, p), OP.tensor(D, q), WW) for p, q in zip(ref, cand)])
    assert np.abs(f + np.sqrt(np.abs(eta))).max() < 1e-14


CHILD = ("import sys; sys.path[:0] = [%r, %r]\n"
         "import numpy as np, operator_cases as OP\nfrom qmps_amd import EnergyEngine\n"
         "D, out = int(sys.argv[1]), {}\n"
         "eng = EnergyEngine(D, 64)\n"
         "for i, dt in enumerate(OP.DTS):\n"
         "    A, C, WW = OP.plain_case(D, dt)\n"
         "    out['eta%%d' %% i], out['rounds%%d' %% i], out['st%%d' %% i], out['r%%d' %% i] = eng.overlaps(A, C, WW, max_rounds=100000, want_r=True)\n"
         "eng.close()\nnp.savez(sys.argv[2], **out)\n" % (ROOT, os.path.join(ROOT, 'tests')))


def plain_solves_in_a_child(D, switch, tmp_path):
    """the plain solves of both dt in a fresh process with `switch` set"""
    path = str(tmp_path / 'child.npz')
    done = subprocess.run([sys.executable, '-c', CHILD, str(D), path], env=dict(os.environ, **{switch: '1'}), capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.load(path)
    for i, dt in enumerate(OP.DTS):
        check(f'{switch} D = {D} dt = {dt}', got[f'eta{i}'], got[f'st{i}'], got[f'r{i}'], plain_reference(D, dt))
    return got


def test_d4_power_method_in_a_child_process(tmp_path):
    """QMPS_OVERLAP_POWER: overlap_block_kernel<4>, the operator-form power method (power steps, not squarings)."""
    got = plain_solves_in_a_child(4, 'QMPS_OVERLAP_POWER', tmp_path)
    assert got['rounds0'].max() > 30


def test_d16_tile_kernel_in_a_child_process(tmp_path):
    """QMPS_D16_BLOCK: overlap_block_kernel<16>, the LDS-tile kernel."""
    plain_solves_in_a_child(16, 'QMPS_D16_BLOCK', tmp_path)


def test_d16_one_wave_kernel(engine_factory, monkeypatch):
    """QMPS_D16_ONE_WAVE: overlap_mfma_d16_kernel serves batches above 2 048 - the candidates of the plain solves, 300 times over;
    every copy is compared with the oracle's value of its original."""
    eng = engine_factory(16, 4096)
    for dt in OP.DTS:
        A, cands, WW = OP.plain_case(16, dt)
        n = len(cands)
        big = np.concatenate([cands] * 300)
        monkeypatch.setenv('QMPS_D16_ONE_WAVE', '1')
        eta, rounds, st, r = eng.overlaps(A, big, WW, want_r=True)
        monkeypatch.delenv('QMPS_D16_ONE_WAVE')
        assert len(big) > 2048 and np.all(st == 0)
        ref = plain_reference(16, dt)
        worst = max(np.abs(eta[k::n] - ref[k][0]).max() for k in range(n))
        worst_r = max(np.abs(np.abs(r[k::n].reshape(300, -1).conj() @ ref[k][1].reshape(-1)) - 1.0).max() for k in range(n))
        print(f'one-wave kernel D = 16 dt = {dt}: max |eta - oracle| = {worst:.2e}, fixed point off the ray by {worst_r:.2e}')
        assert worst < ETA_TOL and worst_r < 1e-9
        assert np.abs(np.linalg.norm(r.reshape(len(big), -1), axis=1) - 1.0).max() < 1e-12


@pytest.mark.parametrize('D', [8, 16])
def test_krylov_fallback(D, engine_factory, monkeypatch):
    """12 Haar-far candidates, max_rounds = 3 000, tol = 1e-12.  That the fall-back took candidates shows against the same launch
    with QMPS_NO_KRYLOV: the power kernel is the same code until it hands a candidate over, so a different count of map applications
    is a candidate that went through qmps_overlap_krylov.hip (seeds 1308 / 1316 of operator_cases.far_case: |eta_2 / eta_1| up to
    0.989 / 0.9985, the plain power method needs more than 1 000 steps there)."""
    A, cands, WW = OP.far_case(D)
    eng = engine_factory(D, 4096)
    eta, rounds, st, r = eng.overlaps(A, cands, WW, max_rounds=3000, tol=1e-12, want_r=True)
    monkeypatch.setenv('QMPS_NO_KRYLOV', '1')
    eta_p, rounds_p, st_p = eng.overlaps(A, cands, WW, max_rounds=3000, tol=1e-12)
    monkeypatch.delenv('QMPS_NO_KRYLOV')
    taken = rounds != rounds_p
    print(f'Krylov fall-back D = {D}: took {int(taken.sum())} of {len(cands)} candidates; map applications {rounds.tolist()} / plain power {rounds_p.tolist()}')
    assert taken.any()
    check(f'Krylov fall-back D = {D}', eta, st, r, [O.overlap_eta(A, c, WW) for c in cands])


@pytest.mark.parametrize('D', [4, 8, 16])
def test_gradient_path(D, engine_factory):
    """qmps_overlap_gradient with the two-sided objective: right and left (adjoint) solves, overlap_g_kernel / overlap_g_d16_kernel and
    their probes, at D = 16 the pair kernel that builds its neighbours.  f at every iterate, three gradient components by the
    oracle's central differences."""
    ref, X, WW, components = OP.gradient_case(D)
    h = 1e-6
    eng = engine_factory(D, 4096)
    eng.overlap_set_refs_params(OP.ANSATZ, ref, WW)
    f, g, st = eng.overlap_gradient(OP.ANSATZ, X, h=h, tol=1e-13, two_sided_f=True)
    assert np.all(st == 0), st
    worst_f = max(abs(f[t] - ER.objective(OP.ANSATZ, D, OP.tensor(D, ref[t]), X[t], WW)) for t in range(len(X)))
    worst_g = 0.0
    for t, k in components:
        e = np.zeros(X.shape[1])
        e[k] = h
        A = OP.tensor(D, ref[t])
        g_ref = (ER.objective(OP.ANSATZ, D, A, X[t] + e, WW) - ER.objective(OP.ANSATZ, D, A, X[t] - e, WW)) / (2 * h)
        worst_g = max(worst_g, abs(g[t, k] - g_ref))
    print(f'gradient path D = {D}: max |f - oracle| = {worst_f:.2e}, max |g - central difference| = {worst_g:.2e}')
    assert worst_f < ETA_TOL and worst_g < 1e-6


def recorded_objectives_are_the_oracles(D, X0, run, WW):
    """fun[step, t] = the oracle's objective of params_hist[step, t] against the previous step's parameters, every t"""
    prev, worst = X0, 0.0
    for step in range(len(run['params_hist'])):
        for t in range(len(X0)):
            f_t = ER.objective(OP.ANSATZ, D, OP.tensor(D, prev[t]), run['params_hist'][step, t], WW, arpack=D >= 16)
            worst = max(worst, abs(f_t - run['fun'][step, t]))
        prev = run['params_hist'][step]
    return worst


@pytest.mark.parametrize('D', [2, 4, 16])
def test_device_resident_bfgs(D, engine_factory, monkeypatch):
    """qmps_evolve_bfgs_device against qmps_evolve_bfgs (bounds of the D = 2 / 4 / 16 tests of test_evolve_gpu.py) and the oracle at
    the recorded parameters.  No claim that the objective reaches -1: a generic operator need not keep the state inside the family."""
    _, X0, WW = OP.driver_case(f'bfgs_device_d{D}')
    T, P = X0.shape
    tol = 1e-12 if D == 16 else 1e-13
    eng = engine_factory(D, T * (2 * P + 1))
    host = eng.evolve_bfgs(OP.ANSATZ, X0, WW, n_steps=2, maxiter=40, tol=tol)
    runs = {'device': eng.evolve_bfgs_device(OP.ANSATZ, X0, WW, n_steps=2, maxiter=40, tol=tol)}
    if D == 2:
        monkeypatch.setenv('QMPS_EVOLVE_D2_SQUARING', '1')
        runs['device, squaring solves'] = eng.evolve_bfgs_device(OP.ANSATZ, X0, WW, n_steps=2, maxiter=40, tol=tol)
        monkeypatch.delenv('QMPS_EVOLVE_D2_SQUARING')
    for name, dev in runs.items():
        d_host, worst = np.abs(dev['fun'] - host['fun']).max(), recorded_objectives_are_the_oracles(D, X0, dev, WW)
        print(f'{name} D = {D}: max |f_dev - f_host| = {d_host:.2e}, max |f - oracle| = {worst:.2e}, iterations {dev["nit"].max(axis=1).tolist()} / host {host["nit"].tolist()}')
        assert dev['failed_evaluations'] == 0
        assert d_host < (1e-8 if D == 16 else 1e-7)
        assert np.abs(dev['fun_start'][0] - host['fun_start'][0]).max() < (1e-12 if D == 2 else 1e-10)
        assert worst < F_TOL
        assert np.all(dev['fun'] <= dev['fun_start'] + 1e-12)


def test_device_rotosolve_d4(engine_factory):
    """qmps_evolve_rotosolve at D = 4 (T = 3, one step, one sweep, three shifts) against the oracle-driven replay."""
    D, X0, WW = OP.driver_case('rotosolve_d4')
    T, P = X0.shape
    eng = engine_factory(D, 4096)
    eng.overlap_stats(reset=True)
    Xf, ph, fh = eng.evolve_rotosolve(OP.ANSATZ, X0, WW, n_steps=1, n_sweeps=1, double_frequency=False, max_rounds=60, tol=1e-12, rule=L.ROTO_GLOBAL_ARGMIN)
    stats = eng.overlap_stats()
    assert stats['not_converged'] == 0 and stats['evaluations'] == (3 * P + 1) * T, stats
    ph_ref, fh_ref = ER.replay_rotosolve(OP.ANSATZ, D, X0, WW, 1, 1, 3, global_argmin=True)
    worst = 0.0
    for t in range(T):
        worst = max(worst, abs(ER.objective(OP.ANSATZ, D, OP.tensor(D, X0[t]), ph[0, t], WW) - fh[0, -1, t]))
        o = abs(O.overlap_eta(OP.tensor(D, ph[0, t]), OP.tensor(D, ph_ref[0, t]), np.eye(4))[0])
        assert abs(o - 1.0) < 1e-6, (t, o)
    print(f'device rotosolve D = 4: max |f - replay| = {np.abs(fh - fh_ref).max():.2e}, max |f - oracle at the device parameters| = {worst:.2e}')
    assert np.abs(fh - fh_ref).max() < F_TOL and worst < F_TOL
    assert np.array_equal(Xf, ph[-1]) and np.all(fh < 0) and np.all(fh >= -1 - 1e-12)


def test_lockstep_driver_d8(engine_factory, monkeypatch):
    """qmps_evolve_bfgs at D = 8 (T = 4, one step): the optimiser algebra on the device against QMPS_EVOLVE_HOST_ALGEBRA - every number
    to the last bit - and the oracle's objective at the final parameters."""
    D, X0, WW = OP.driver_case('lockstep_d8')
    T, P = X0.shape
    eng = engine_factory(D, T * (2 * P + 1))
    out = {}
    for name in ('device', 'host'):
        if name == 'host':
            monkeypatch.setenv('QMPS_EVOLVE_HOST_ALGEBRA', '1')
        out[name] = eng.evolve_bfgs(OP.ANSATZ, X0, WW, n_steps=1, maxiter=30, tol=1e-12, carry_hessian=True)
        monkeypatch.delenv('QMPS_EVOLVE_HOST_ALGEBRA', raising=False)
    dv, hs = out['device'], out['host']
    assert np.array_equal(dv['nit'], hs['nit']), (dv['nit'], hs['nit'])
    assert np.array_equal(dv['fun'], hs['fun']) and np.array_equal(dv['fun_start'], hs['fun_start'])
    assert np.array_equal(dv['x'], hs['x']) and np.array_equal(dv['params_hist'], hs['params_hist'])
    assert np.array_equal(dv['hess_inv'], hs['hess_inv'])
    assert dv['gradient_batches'] == hs['gradient_batches'] and dv['ladder_batches'] == hs['ladder_batches'] and dv['nfev'] == hs['nfev']
    worst = recorded_objectives_are_the_oracles(D, X0, dv, WW)
    print(f'lock-step driver D = 8: {int(dv["nit"][0])} iterations, max |f - oracle| = {worst:.2e}')
    assert worst < F_TOL and np.all(dv['fun'] <= dv['fun_start'] + 1e-12)
