"""GPU: every batched kernel past its grid cap and its batch-size switch (tests/batch_edge_cases.py: the thresholds, the pools and
the tiling).  The rest of the suite stays on one side of each of them: a kernel that reused wave-private LDS, a global slab, a
pending counter or a status word wrongly on its second trip round a stride loop would pass it.

Every test repeats a pool of distinct inputs cyclically to a batch just past the threshold and asserts
  1. every copy is the oracle's value of its original, within the tolerance the suite already applies to that kernel (imported);
  2. all copies of one pool member are byte-identical - energies, environments, rho, eta, fixed points, G, f, g, counts, statuses.
     An evaluation is computed by one wave or one workgroup with the same instruction sequence wherever it sits, so a second-pass
     error of 1e-12, which 1 would let through, shows here.  Device-side sums depend on the order of their terms: they are compared
     with the host sum.

  row  threshold                                                 test
  1    D = 16 energy kernels, 4 096 workgroups x 4 waves         test_d16_energy_past_the_grid_cap
  2    D = 16 finishing pass (64) / environment Krylov (32)      test_d16_pending_passes_beyond_their_grids
  3    D = 8 direct solve, two-kernel path above 4 096           test_d8_direct_two_kernel_path
  4    D = 16 correlator sums, 252 slabs                         test_d16_correlator_sums_beyond_the_slabs
  5    D = 16 overlap, one wave per candidate, 4 096 x 4         test_d16_one_wave_overlap_past_the_grid_cap
  6    D = 4 overlap by squaring, 8 192 x 4                      test_d4_squaring_overlap_past_the_grid_cap
  7    Krylov fall-back, eight candidates per ticket             test_krylov_eight_candidates_per_ticket
  8    D = 16 gradient, default pair launch                      test_d16_gradient_default_pair_launch

Batch sizes, durations and the worst deviation each case saw on an MI355X: profiles/EXPERIMENTS.md.  Every test prints its own
(pytest -s)."""
import numpy as np
import pytest

import batch_edge_cases as BE
import correlator_cases as K
import evolve_replay as ER
import operator_cases as OP
import structure_factor_cases as S
import test_energy_gpu as TE
import test_generic_operator_gpu as TG
import test_structure_factor_gpu as TS
from oracle import qmps_oracle as O

pytestmark = pytest.mark.gpu

F_TOL, G_TOL = 1e-10, 2e-7           # test_evolve_gpu.test_two_sided_gradient_*: f and g against the oracle's central differences
_REF = {}


def cached(key, make):
    """A reference of a pool: computed once, shared by the tests that need it, never changed."""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def identical(what, n=BE.POOL, **results):
    """Check 2: no copy differs from the first copy of its pool member in any byte."""
    for name, a in results.items():
        bad = BE.differing_copies(a, n)
        if bad.size:
            a = np.asarray(a).reshape(len(a), -1)
            worst = np.abs(a[bad].astype(complex) - a[bad % n].astype(complex)).max()
            raise AssertionError(f'{what}: {name} of {bad.size} of {len(a)} copies differs from the first copy of its pool member '
                                 f'(rows {bad[:8].tolist()} ..., by up to {worst:.2e})')


def energy_reference(c_oracle, D):
    return cached(('energy', D), lambda: c_oracle.energy_batch(BE.haar_pool(D), BE.H2, want_r=True, want_rho=True))


def against_the_c_oracle(what, ref, E, st, r, rho):
    """Check 1 of the energy path: every row against the C oracle's value of its pool member."""
    idx = np.arange(len(E)) % BE.POOL
    assert np.all(ref['status'] == 0) and np.all(st == 0), (what, np.flatnonzero(st != 0)[:8])
    dE, dr, drho = np.abs(E - ref['E'][idx]).max(), np.abs(r - ref['r'][idx]).max(), np.abs(rho - ref['rho'][idx]).max()
    print(f'{what}: B = {len(E)}, max |E - oracle| = {dE:.2e} (tolerance {TE.E_TOL:.0e}), |r - oracle| = {dr:.2e}, |rho - oracle| = {drho:.2e} ({TE.R_TOL:.0e})')
    assert dE < TE.E_TOL and dr < TE.R_TOL and drho < TE.R_TOL, (what, dE, dr, drho)


def test_d16_energy_past_the_grid_cap(c_oracle, engine_factory):
    """Row 1: B = 16 384 + 45 Haar tensors, two Hamiltonian terms.  energy_mfma_d16_kernel<true> (the solve; 4 096 workgroups x 4
    waves, every wave strides to a second evaluation, 45 of them to a ragged last pass) and energy_mfma_d16_kernel<false> (rdm() and
    launch_energy_only()).  E, r, rho against the C oracle, iteration counts within one, the device-side sums against the host sum."""
    B = BE.BATCH['energy_d16']
    ref = energy_reference(c_oracle, 16)
    idx = np.arange(B) % BE.POOL
    eng = engine_factory(16)
    eng.set_solver('direct')
    E, it, st = eng.energies(BE.tile(BE.haar_pool(16), B), BE.H2)
    r, rho, cost = eng.environments(B), eng.rdm(B), eng.summed_cost(B)
    against_the_c_oracle('D = 16 energy', ref, E, st, r, rho)
    assert np.abs(it - ref['iters'][idx]).max() <= 1
    identical('D = 16 energy', E=E, iters=it, status=st, r=r, rho=rho)
    assert np.allclose(cost, E.sum(0), rtol=0, atol=1e-9 * max(1, B))
    # the in-kernel cost accumulator, once
    eng.launch(B, accumulate_cost=True)
    eng.cost_launch(B)
    acc = eng.get_cost()
    Ea, ita, sta = eng.results(B)
    assert np.all(sta == 0) and np.abs(Ea - ref['E'][idx]).max() < TE.E_TOL
    identical('D = 16 energy, accumulating launch', E=Ea, iters=ita, status=sta, r=eng.environments(B))
    assert np.allclose(acc, Ea.sum(0), rtol=0, atol=1e-9 * max(1, B))
    # the energy-only kernel on the resident (A, r)
    eng.launch_energy_only(B)
    E3, _, st3 = eng.results(B)
    print(f'D = 16 energy: energy-only launch against the solve {np.abs(E3 - Ea).max():.2e}, accumulated cost against the host sum {np.abs(acc - Ea.sum(0)).max():.2e}')
    assert np.abs(E3 - Ea).max() < 1e-13 and np.all(st3 == 0)
    identical('D = 16 energy-only launch', E=E3, status=st3)


def pending_reference():
    def make():
        out = []
        for a in BE.pending_pool():
            r = O.env_dense_eig(a)[1]               # (one dense eigen-solve per tensor serves both terms)
            out.append([O.energy_closed_form(a, hh, r) for hh in BE.H2])
        return np.array(out)
    return cached('pending', make)


@pytest.mark.parametrize('n_copies', BE.PENDING_COPIES)
def test_d16_pending_passes_beyond_their_grids(n_copies, engine_factory, monkeypatch):
    """Row 2: the eight slow tensors of test_d16_environment_krylov_fallback and 33 Haar tensors, 9 and 13 times over: 72 and 104
    evaluations come back from the Krylov fall-back (32 workgroups draw them) through the finishing pass (64 workgroups look through
    the batch) - behind the two-wave main kernel (B = 369) and the one-wave one (B = 533).  Energies against the dense eigen-solve,
    the accumulated cost against its sum; everything twice on the same context with identical results: the last workgroup of each
    pass cleared its counters.  (Measured: 9.97e-11 on the two tensors of gap 3e-6 - a fixed point accepted at 1e-13 sits 1e-13 / gap off
    the true one - the same tensors the existing test holds to this tolerance.)"""
    B = BE.POOL * n_copies
    pool, ref = BE.pending_pool(), BE.tile(pending_reference(), B)
    A = BE.tile(pool, B)
    eng = engine_factory(16)
    eng.set_solver('direct')
    # which pool members the power iteration alone does not finish: the slow eight, so n_copies x 8 evaluations are handed over
    monkeypatch.setenv('QMPS_NO_KRYLOV', '1')
    _, _, st_plain = eng.energies(pool, BE.H2, max_iter=3000, tol=1e-13)
    monkeypatch.delenv('QMPS_NO_KRYLOV')
    assert np.array_equal(np.flatnonzero(st_plain == 1), np.arange(BE.N_SLOW)) and np.all(st_plain[BE.N_SLOW:] == 0)
    pending = BE.N_SLOW * n_copies
    assert pending > BE.THRESHOLDS['pending_d16'][2] > BE.THRESHOLDS['pending_krylov'][2]
    assert (B <= BE.THRESHOLDS['two_wave_d16'][2]) == (n_copies == BE.PENDING_COPIES[0])
    runs = []
    for _ in range(2):
        E, it, st = eng.energies(A, BE.H2, max_iter=3000, tol=1e-13)
        r = eng.environments(B)
        eng.set_tensors(A)
        eng.set_hamiltonian(BE.H2)
        eng.launch(B, max_iter=3000, accumulate_cost=True)
        eng.cost_launch(B)
        cost = eng.get_cost()
        Ea, ita, sta = eng.results(B)
        runs.append({'E': E, 'iters': it, 'status': st, 'r': r, 'cost': cost, 'E of the accumulating launch': Ea, 'its iters': ita, 'its status': sta,
                     'its r': eng.environments(B)})
    for run in runs:
        assert np.all(run['status'] == 0) and np.all(run['its status'] == 0), (run['status'], run['iters'])
        assert run['iters'].max() <= 1000 and run['its iters'].max() <= 1000, run['iters']
        dE, dEa, dc = np.abs(run['E'] - ref).max(), np.abs(run['E of the accumulating launch'] - ref).max(), np.abs(run['cost'] - ref.sum(axis=0)).max()
        assert dE < TE.E_TOL and dEa < TE.E_TOL, (dE, dEa)
        assert dc < 1e-9 * B / 12, dc
        identical(f'D = 16 pending passes, B = {B}', **{k: v for k, v in run.items() if k != 'cost'})
    for b in range(BE.POOL):                    # the environments are fixed points (the first copies; the others are identical)
        rr = runs[0]['r'][b] / np.trace(runs[0]['r'][b])
        assert np.abs(rr - rr.conj().T).max() < 1e-12 and np.abs(O.apply_transfer(pool[b], rr) - rr).max() < 1e-11
    print(f'D = 16 pending passes: B = {B}, {pending} pending, max |E - dense eigen-solve| = {dE:.2e} (tolerance {TE.E_TOL:.0e}), '
          f'|cost - sum| = {dc:.2e} ({1e-9 * B / 12:.1e}), iterations up to {runs[0]["iters"].max()}')
    for name in runs[0]:
        assert runs[0][name].tobytes() == runs[1][name].tobytes(), f'{name}: the second pass over the same context differs'


def test_d8_direct_two_kernel_path(c_oracle, engine_factory):
    """Row 3: B = 4 096 + 45 Haar tensors with solver='direct': launch_env_direct_d8, then the block kernel started from r_in - every
    evaluation accepted by its first power step.  E, r, rho against the C oracle, and against the same pool at B = 41, the fused
    path (within the tolerances: the two paths are different kernels)."""
    B = BE.BATCH['direct_d8']
    assert B > BE.THRESHOLDS['direct_d8'][2] >= BE.POOL
    ref = energy_reference(c_oracle, 8)
    eng = engine_factory(8)
    out = {}
    for n in (B, BE.POOL):
        eng.set_tensors(BE.tile(BE.haar_pool(8), n))
        eng.set_hamiltonian(BE.H2)
        eng.launch(n, solver='direct', store_env=True)
        E, it, st = eng.results(n)
        out[n] = (E, it, st, eng.environments(n), eng.rdm(n), eng.summed_cost(n))
        against_the_c_oracle(f'D = 8 direct, {"two kernels" if n == B else "fused"}', ref, E, st, out[n][3], out[n][4])
        assert np.all(it == 1), np.flatnonzero(it != 1)[:8]
        assert np.allclose(out[n][5], E.sum(0), rtol=0, atol=1e-9 * max(1, n))
    E, it, st, r, rho, _ = out[B]
    identical('D = 8 direct, two kernels', E=E, iters=it, status=st, r=r, rho=rho)
    idx = np.arange(B) % BE.POOL
    E1, _, _, r1, rho1, _ = out[BE.POOL]
    dE, dr, drho = np.abs(E - E1[idx]).max(), np.abs(r - r1[idx]).max(), np.abs(rho - rho1[idx]).max()
    print(f'D = 8 direct: two-kernel path against the fused path: |E| {dE:.2e}, |r| {dr:.2e}, |rho| {drho:.2e}')
    assert dE < TE.E_TOL and dr < TE.R_TOL and drho < TE.R_TOL


def test_d16_correlator_sums_beyond_the_slabs(engine_factory):
    """Row 4: the five D = 16 states test_structure_factor_gpu references in long double (the same 5 x 3 reference items, no more),
    tiled to B = 90 and 85 with set_tensors + set_env_guess: 270 and 255 items for the 252 workgroups of corrsum_global_kernel, each
    of which rebuilds its tiles and its global slab for its second item (B = 85: exactly three of them do)."""
    eng, s = TS._haar(engine_factory, 16)
    ref = TS._haar_reference(16)
    rows, n_z = BE.CORRSUM_ROWS, BE.CORRSUM_N_Z
    assert rows == TS.D16_ROWS and n_z == len(TS.D16_Z)
    ops = K.generic_ops()
    for B in BE.CORRSUM_BATCHES:
        assert B * n_z > BE.THRESHOLDS['corrsum_d16'][2]
        A, r = BE.tile(s['A'][:rows], B), BE.tile(s['r'][:rows], B)
        eng.set_tensors(A)
        eng.set_env_guess(r)
        assert eng.tensors(B).tobytes() == A.tobytes() and eng.environments(B).tobytes() == r.tobytes()
        G, one, site = eng.correlator_sums(ops, S.Z[:n_z], B=B, want_one_site=True, want_site=True)
        assert G.shape == (B, n_z, 4, 4) and one.shape == (B, 4) and site.shape == (B, 4, 4)
        ratio, e1 = TS._check(G, one, site, ref, np.arange(B) % rows, 4, n_z, 16, 'beyond the slabs')
        print(f'correlator_sums D = 16: B = {B}, {B * n_z} items, worst err / bound {ratio:.3f} (<= 1), worst |one, site - long double| {e1:.2e} ({K.bound(16, 1):.1e})')
        identical(f'correlator sums, B = {B}', n=rows, G=G, one=one, site=site)


def overlap_reference(D, dt):
    def make():
        A, cands, WW = BE.overlap_pool(D, dt)
        first = TG.plain_reference(D, dt)           # the candidates of the plain case: shared with tests/test_generic_operator_gpu.py
        return list(first) + [O.overlap_eta(A, c, WW) for c in cands[len(first):]]
    return cached(('overlap', D, dt), make)


def tiled(refs, B):
    return [refs[b % len(refs)] for b in range(B)]


@pytest.mark.parametrize('dt', OP.DTS)
def test_d16_one_wave_overlap_past_the_grid_cap(dt, engine_factory, monkeypatch):
    """Row 5: QMPS_D16_ONE_WAVE, B = 16 384 + 45: overlap_mfma_d16_kernel with 4 096 workgroups x 4 waves, every wave strides to a
    second candidate.  The candidates of the plain case padded to 41, shared reference, eta and the fixed point's ray."""
    B = BE.BATCH['one_wave_d16']
    A, cands, WW = BE.overlap_pool(16, dt)
    refs = overlap_reference(16, dt)
    eng = engine_factory(16)
    monkeypatch.setenv('QMPS_D16_ONE_WAVE', '1')
    eta, rounds, st, r = eng.overlaps(A, BE.tile(cands, B), WW, want_r=True)
    monkeypatch.delenv('QMPS_D16_ONE_WAVE')
    TG.check(f'one-wave kernel D = 16 dt = {dt}, B = {B}', eta, st, r, tiled(refs, B))
    identical(f'one-wave kernel D = 16 dt = {dt}', eta=eta, rounds=rounds, status=st, r=r)


@pytest.mark.parametrize('dt', OP.DTS)
def test_d4_squaring_overlap_past_the_grid_cap(dt, engine_factory):
    """Row 6: B = 32 768 + 45: overlap_square_d4_kernel with 8 192 workgroups x 4 candidates, then its stride - with a shared
    reference, and with one reference per candidate (overlap_set with B references: overlap_ref_index is part of the second pass)."""
    B = BE.BATCH['square_d4']
    A, cands, WW = BE.overlap_pool(4, dt)
    big = BE.tile(cands, B)
    eng = engine_factory(4)
    eng.overlap_set_group(0)
    eta, rounds, st, r = eng.overlaps(A, big, WW, want_r=True)
    TG.check(f'squaring kernel D = 4 dt = {dt}, B = {B}, shared reference', eta, st, r, tiled(overlap_reference(4, dt), B))
    assert rounds.max() <= 30, rounds.max()
    identical(f'squaring kernel D = 4 dt = {dt}, shared reference', eta=eta, rounds=rounds, status=st, r=r)
    R = BE.overlap_pool_references(4, dt)
    refs = cached(('overlap references', dt), lambda: [O.overlap_eta(a, c, WW) for a, c in zip(R, cands)])
    eng.overlap_set(BE.tile(R, B), WW)
    eng.set_tensors(big)
    eng.overlap_launch(B, want_r=True)
    eta, rounds, st, r = eng.overlap_results(B, want_r=True)
    TG.check(f'squaring kernel D = 4 dt = {dt}, B = {B}, one reference per candidate', eta, st, r, tiled(refs, B))
    assert rounds.max() <= 30, rounds.max()
    identical(f'squaring kernel D = 4 dt = {dt}, one reference per candidate', eta=eta, rounds=rounds, status=st, r=r)


@pytest.mark.parametrize('D', [8, 16])
def test_krylov_eight_candidates_per_ticket(D, engine_factory):
    """Row 7: B = 4 096 + 45, max_rounds = 3 000, tol = 1e-12: above 4 096 candidates a workgroup of the fall-back draws eight per
    ticket and reuses its LDS basis for each.  Haar-far candidates (D = 8: 12 of the 41, D = 16: 4) among plain ones.  Against the
    launch of the bare pool - one candidate per ticket, where test_krylov_fallback shows the far ones to be taken by the fall-back -
    every copy has the map applications and the status of its original: the same route."""
    B = BE.BATCH['krylov_chunk']
    A, cands, WW = BE.krylov_pool(D)
    refs = cached(('krylov', D), lambda: [O.overlap_eta(A, c, WW) for c in cands])
    eng = engine_factory(D)
    eng.overlap_set_group(0)
    eta0, rounds0, st0, r0 = eng.overlaps(A, cands, WW, max_rounds=3000, tol=1e-12, want_r=True)
    TG.check(f'Krylov fall-back D = {D}, the pool', eta0, st0, r0, refs)
    eta, rounds, st, r = eng.overlaps(A, BE.tile(cands, B), WW, max_rounds=3000, tol=1e-12, want_r=True)
    TG.check(f'Krylov fall-back D = {D}, B = {B}', eta, st, r, tiled(refs, B))
    print(f'Krylov fall-back D = {D}: map applications of the pool {rounds0.tolist()}')
    idx = np.arange(B) % BE.POOL
    assert np.array_equal(rounds, rounds0[idx]), np.flatnonzero(rounds != rounds0[idx])[:8]
    assert np.array_equal(st, st0[idx])
    identical(f'Krylov fall-back D = {D}', eta=eta, rounds=rounds, status=st, r=r)


def gradient_reference():
    """(f, {k: g_k}) by the oracle's dense eigen-solves for pool members 0, 20, 40 at the cold and the warm iterates, k = 0 and P - 1."""
    def make():
        ref, X, noise, WW = BE.gradient_pool()
        h, P, out = 1e-6, BE.GRADIENT_P, {}
        for t in BE.GRADIENT_MEMBERS:
            A = ER.tensor(0, 16, ref[t])
            for which, x in (('cold', X[t]), ('warm', X[t] + 1e-3 * noise[t])):
                g = {}
                for k in (0, P - 1):
                    e = np.zeros(P)
                    e[k] = h
                    g[k] = (ER.objective(0, 16, A, x + e, WW) - ER.objective(0, 16, A, x - e, WW)) / (2 * h)
                out[t, which] = (ER.objective(0, 16, A, x, WW), g)
        return out
    return cached('gradient', make)


@pytest.mark.parametrize('T', BE.GRADIENT_T)
def test_d16_gradient_default_pair_launch(T, engine_factory):
    """Row 8: qmps_overlap_gradient at D = 16 on its default path, P = 8, h = 1e-6, 41 parameter rows tiled to T iterates; a cold
    call, then a warm one at X + 1e-3 noise.  The kernels (qmps_capi_overlap.hip, enqueue_gradient_kernels):
      T = 1 030: overlap_mfma_d16x4_pair_kernel<true> (cold; <false> warm) with 1 030 + 1 030 workgroups for the right and the left
        solves, one iterate each, and 4 096 surplus workgroups that build the 16 480 neighbour tensors one wave each - the last 96
        by the stride; the Krylov fall-back only if a status asks for it; then overlap_g_d16_kernel and its probes.
      T = 2 053: the same launch with 2 048 + 2 048 solving workgroups that draw their iterates from two queues in HBM, and the
        neighbour build strides three times (32 848 tensors).
    f and g against the oracle's central differences for pool members 0, 20, 40; f, g and status byte-identical across copies."""
    ref, X, noise, WW = BE.gradient_pool()
    P, h = BE.GRADIENT_P, 1e-6
    assert T * 2 * P > BE.THRESHOLDS['gradient_neighbours'][2] and (T > BE.THRESHOLDS['gradient_pair'][2]) == (T == BE.GRADIENT_T[1])
    eng = engine_factory(16)
    eng.overlap_set_refs_params(0, BE.tile(ref, T), WW)
    eng.overlap_set_group(0)
    eng.overlap_stats(reset=True)
    f, g, st = eng.overlap_gradient(0, BE.tile(X, T), h=h, tol=1e-13)
    assert eng.overlap_stats(reset=True)['evaluations'] == 2 * T
    f2, g2, st2 = eng.overlap_gradient(0, BE.tile(X + 1e-3 * noise, T), h=h, tol=1e-13, warm=True)
    assert eng.overlap_stats(reset=True)['evaluations'] == 2 * T
    assert np.all(st == 0) and np.all(st2 == 0), (np.flatnonzero(st != 0)[:8], np.flatnonzero(st2 != 0)[:8])
    oracle = gradient_reference()
    worst_f, worst_g = 0.0, 0.0
    for which, fv, gv in (('cold', f, g), ('warm', f2, g2)):
        for t in BE.GRADIENT_MEMBERS:
            f_ref, g_ref = oracle[t, which]
            rows = BE.copies(t, T)
            worst_f = max(worst_f, np.abs(fv[rows] - f_ref).max())
            worst_g = max([worst_g] + [np.abs(gv[rows, k] - g_ref[k]).max() for k in g_ref])
    print(f'gradient D = 16, default path: T = {T}, max |f - oracle| = {worst_f:.2e} (tolerance {F_TOL:.0e}), max |g - central difference| = {worst_g:.2e} ({G_TOL:.0e})')
    assert worst_f < F_TOL and worst_g < G_TOL
    identical(f'gradient D = 16, T = {T}, cold', f=f, g=g, status=st)
    identical(f'gradient D = 16, T = {T}, warm', f=f2, g=g2, status=st2)
