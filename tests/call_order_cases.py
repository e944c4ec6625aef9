"""Every entry-point family of include/qmps_hip.h as a function of one context, for the call-order tests (test infrastructure;
tests/test_call_order_cpu.py checks the tables without a GPU, tests/test_call_order_gpu.py runs the families after each other).

A context carries host-side facts about what its buffers hold, and several buffers are shared between families (d_r: environments or
overlap fixed points; d_iters / d_status: energy or overlap launches; d_E: energies or the objective of qmps_evolve_rotosolve;
d_scratch; the work counters of d_queue).  The header states a contract for every family; the tables here restate it:

  FAMILIES   name -> Family: `run(eng, D, I) -> dict of arrays` with fixed inputs I = inputs(D); it returns everything the calls return.
             A family is self-contained (it uploads what it reads), so it means the same on a fresh context and after any other family.
  READERS    name -> function(eng, n): a read-back of the first n resident evaluations.
  LEAVES     what a family leaves resident -> reader -> outcome: 'same' (what was resident before the family), 'of X' (what the family
             left) or 'refuse' (QMPS_ERR_STATE), each with the header sentence it rests on.  EXPECT spells it out per (family, reader).

Shapes: B = 37 evaluations per window (ragged last wave, quad and tile), three windows, two Hamiltonian terms (one not Hermitian),
R = 5 restarts, T = 3 trajectories, P = 4 ShallowCNOT angles, contexts of capacity 256."""
import ctypes
import functools
import inspect
import re

import numpy as np

import batch_edge_cases as BE
import correlator_cases as K
import operator_cases as OP
import overlap_cases as OC
from oracle import qmps_oracle as O
from qmps_amd import _lib as L
from qmps_amd.engine import EnergyEngine, _f64, _i32

DS = (2, 4, 8, 16)
B = 37
WINDOWS = 3
N = B * WINDOWS
R = 5
T = 3
P = 4
G = 3                      # candidates per trajectory of the grouped overlap families
CAPACITY = 256
KIND = L.ANSATZ_SHALLOW_CNOT
KIND_UNFUSED = L.ANSATZ_SHALLOW_CNOT_NONUNIFORM
HANDOFF = {2: 64, 4: 128}          # tests/test_energy_gpu.py: the hand-off of the 'squaring' variant
CAP_SHORT = 3                      # a budget no solve converges in
CAP_KRYLOV = 100                   # D = 8, 16: above the 64 steps below which nothing is handed over; evaluations wait for the fall-back when it ends
N_MAX = 3
Z = np.array([1.0, 0.5 + 0.25j, np.exp(0.3j)], dtype=np.complex128)

# ---------------------------------------------------------------------------------------------------------------------------------
# inputs


def _nq(D):
    return int(np.log2(D)) + 1


def build_inputs(D):
    """Every array the families read at bond dimension D, from fixed seeds (tests/test_call_order_cpu.py builds them twice)."""
    rng = np.random.default_rng(9100 + D)
    I = {}
    I['A'] = np.ascontiguousarray(O.unitary_to_tensor(O.haar_unitaries(rng, 2 * D, N)))
    I['U'] = np.ascontiguousarray(O.haar_unitaries(rng, 2 * D, B))
    G4 = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))           # not Hermitian
    I['h'] = np.stack([O.hamiltonian_matrix({'ZZ': -1, 'X': 1}), G4 / np.linalg.norm(G4, 2)])
    I['h1'] = np.ascontiguousarray(OP.generic_h(9300 + D)[None])
    I['params'] = rng.standard_normal((B, P))
    I['params_unfused'] = rng.standard_normal((B, 4 * _nq(D)))          # two layers of 2 (log2 D + 1) angles
    I['su'] = 0.3 * rng.standard_normal((B, (2 * D) ** 2 - 1))
    I['roto'] = rng.standard_normal((R, P))
    X = rng.standard_normal((B, D, D)) + 1j * rng.standard_normal((B, D, D))
    I['guess'] = np.ascontiguousarray(np.eye(D) + 0.1 * (X + X.conj().transpose(0, 2, 1)) / np.sqrt(D))      # Hermitian, positive trace
    I['q'] = rng.standard_normal((B, D, D)) + 1j * rng.standard_normal((B, D, D))
    I['ops'] = np.ascontiguousarray(K.generic_ops()[:3])
    # the overlap objective: candidates near one reference (tests/batch_edge_cases.py), and trajectories as ansatz parameters
    A_ref, cands, WW = BE.overlap_pool(D, OP.DTS[0])
    I['ref'], I['cands'], I['WW'] = np.ascontiguousarray(A_ref), np.ascontiguousarray(cands[:B]), np.ascontiguousarray(WW)
    I['cands_U'] = np.ascontiguousarray(np.stack([O.tensor_to_unitary(a) for a in cands[:B]]))
    I['moved'] = np.ascontiguousarray(BE.near_candidates(A_ref, np.random.default_rng(9200 + D), B))
    I['traj'] = rng.standard_normal((T, P))
    I['traj_cands'] = (I['traj'][:, None, :] + 0.05 * rng.standard_normal((T, G, P))).reshape(T * G, P)
    I['traj_moved'] = I['traj_cands'] + 0.01 * rng.standard_normal((T * G, P))
    I['iterates'] = I['traj'] + 0.03 * rng.standard_normal((T, P))
    I['iterates2'] = I['iterates'] + 1e-3 * rng.standard_normal((T, P))
    I['cand_params'] = I['traj'][0] + 0.05 * rng.standard_normal((B, P))
    I['abcd'] = rng.standard_normal((16, 4))
    I['su4'] = 0.5 * rng.standard_normal((5, 15))
    # brick-wall calls and the D = 2 only calls (any context serves the former)
    bw = O.haar_unitaries(rng, 4, 4 * 7).reshape(4, 7, 4, 4)
    I['bw'] = np.ascontiguousarray(bw)
    I['bw_O'] = np.ascontiguousarray(OP.generic_h(9400 + D))
    I['bw_M'] = rng.standard_normal((2, 2, 2)) + 1j * rng.standard_normal((2, 2, 2))
    I['bw_W'] = np.ascontiguousarray(O.haar_unitaries(rng, 16, 1)[0])
    if D == 2:
        I['cell_U'] = np.ascontiguousarray(O.haar_unitaries(rng, 4, 2 * B).reshape(2, B, 4, 4))
        I['cell_p'] = 0.5 * rng.standard_normal((B, 30))
        I['optenv_p'] = rng.standard_normal((B, 30))
    if D >= 8:
        # capped variants: slow environments (the tensors of tests/batch_edge_cases.pending_pool(), D = 8: the same generator) and
        # Haar-far overlap candidates - evaluations that are waiting for the Krylov fall-back when a budget of CAP_KRYLOV ends
        if D == 16:
            slow = BE.pending_pool()[:B]
        else:
            srng = np.random.default_rng(80)
            slow = np.stack([OC.slow_environment_tensor(srng, D, t) for t in BE.SLOW_T] + list(I['A'][:B - BE.N_SLOW]))
        I['slow'] = np.ascontiguousarray(slow)
        A_far, far, WW_far = BE.krylov_pool(D)
        I['far_ref'], I['far'], I['far_WW'] = np.ascontiguousarray(A_far), np.ascontiguousarray(far[:B]), np.ascontiguousarray(WW_far)
    for a in I.values():
        a.setflags(write=False)
    return I


@functools.lru_cache(maxsize=None)
def inputs(D):
    return build_inputs(D)


# ---------------------------------------------------------------------------------------------------------------------------------
# families

FAMILIES = {}


class Family:
    def __init__(self, name, run, Ds, leaves, n, sets, states):
        self.name, self.run, self.Ds, self.n, self.sets, self.states = name, run, tuple(Ds), n, frozenset(sets), states
        self._leaves = leaves

    def leaves(self, D):
        return self._leaves(D) if callable(self._leaves) else self._leaves

    def legal(self, D):
        return D in self.Ds


def family(name, Ds=DS, leaves='nothing', n=B, sets=(), states=None):
    """Register run(eng, D, I).  leaves: a key of LEAVES (or D -> key); n: evaluations resident afterwards; sets: the persistent
    settings the family's own calls replace (SETTINGS); states: I -> (kind, array) of the states it leaves resident, for the oracle."""
    def wrap(run):
        assert name not in FAMILIES
        FAMILIES[name] = Family(name, run, Ds, leaves, n, sets, states)
        return run
    return wrap


def canon(eng):
    """The settings every family but the solver families starts from: what qmps_create sets at D = 2, 4, 8 (D = 16 runs the squaring
    solver under this name).  The harness calls it in front of every family, alone or after another one."""
    eng.set_solver('direct', handoff=0)


def _select(eng, solver):
    if solver == 'plain':
        eng.set_solver('plain', handoff=HANDOFF.get(eng.D, 0))
    elif solver == 'direct':
        eng.set_solver('direct', handoff=0)
    else:
        eng.set_solver('squaring', handoff=HANDOFF.get(eng.D, 0) if solver == 'squaring' else 0)


def _solved(eng, E, it, st, n=B):
    return {'E': E, 'iters': it, 'status': st, 'r': eng.environments(n)}


def _tensor_states(key):
    return lambda I: ('tensor', I[key][:B])


for _solver in ('plain', 'squaring', 'squaring0', 'direct'):
    def _run(eng, D, I, _solver=_solver):
        _select(eng, _solver)
        return _solved(eng, *eng.energies(I['A'][:B], I['h']))
    family(f'energies_{_solver}', leaves='solve', sets=('solver', 'handoff', 'hamiltonian'), states=_tensor_states('A'))(_run)

    def _run(eng, D, I, _solver=_solver):
        _select(eng, _solver)
        return _solved(eng, *eng.energies(I['A'][:B], I['h'], max_iter=CAP_SHORT))
    family(f'energies_{_solver}_cap{CAP_SHORT}', leaves='solve', sets=('solver', 'handoff', 'hamiltonian'), states=_tensor_states('A'))(_run)


@family('energies_unitary_guess', leaves='solve', sets=('hamiltonian',), states=lambda I: ('unitary', I['U']))
def _(eng, D, I):
    return _solved(eng, *eng.energies(I['U'], I['h'], kind='unitary', r0=I['guess']))


@family('env_batch', leaves='solve', states=_tensor_states('A'))
def _(eng, D, I):
    eng.set_hamiltonian(I['h'])
    r, it, st = eng.env_batch(I['A'][:B])
    E = eng.results(B)[0]
    return {'E': E, 'iters': it, 'status': st, 'r': r}


def _launch_family(store, acc, warm, kry):
    def run(eng, D, I):
        eng.set_tensors(I['A'][:B])
        eng.set_hamiltonian(I['h'])
        if warm:                                   # something to start from: a cold launch that stores its environments
            eng.launch(B, store_env=True)
        eng.launch(B, store_env=store, accumulate_cost=acc, warm_start=warm, krylov_fallback=kry)
        out = {}
        if acc:
            eng.cost_launch(B)
            out['cost'] = eng.get_cost()
        eng.sync()
        out['E'], out['iters'], out['status'] = eng.results(B)
        if store or warm:                          # (a warm launch that stores nothing leaves the environments of the cold one, of the same states)
            out['r'] = eng.environments(B)
        return out
    return run


for _store in (True, False):
    for _acc in (False, True):
        for _warm in (False, True):
            for _kry in (False, True):
                family(f'launch_store{int(_store)}_acc{int(_acc)}_warm{int(_warm)}_krylov{int(_kry)}', Ds=DS if _store else (4,),
                       leaves=('solve' if _store or _warm else 'noenv') + ('_cost' if _acc else ''), states=_tensor_states('A'))(_launch_family(_store, _acc, _warm, _kry))


@family(f'launch_krylov_cap{CAP_KRYLOV}', Ds=(8, 16), leaves='solve_cost', states=_tensor_states('slow'))
def _(eng, D, I):
    eng.set_tensors(I['slow'])
    eng.set_hamiltonian(I['h'])
    # (the iterative solver: the direct solve of D = 8 is accepted at its first step and no budget ends it)
    eng.launch(B, max_iter=CAP_KRYLOV, solver='squaring', accumulate_cost=True, krylov_fallback=True)
    eng.cost_launch(B)
    cost = eng.get_cost()
    E, it, st = eng.results(B)
    return {'E': E, 'iters': it, 'status': st, 'r': eng.environments(B), 'cost': cost}


@family(f'energies_slow_cap{CAP_KRYLOV}', Ds=(8, 16), leaves='solve', sets=('hamiltonian',), states=_tensor_states('slow'))
def _(eng, D, I):
    _select(eng, 'squaring0')
    return _solved(eng, *eng.energies(I['slow'], I['h'], max_iter=CAP_KRYLOV))


def _noenv_at_d4(D):
    return 'noenv' if D == 4 else 'solve'          # "at D = 4 with the direct solver no environments are stored"


@family('energies_from_params', leaves=_noenv_at_d4, sets=('hamiltonian',), states=lambda I: ('params', I['params']))
def _(eng, D, I):
    E, it, st = eng.energies_from_params(KIND, I['params'], I['h'])
    return {'E': E, 'iters': it, 'status': st}


@family('energies_from_params_unfused', leaves=_noenv_at_d4, sets=('hamiltonian',), states=lambda I: ('params_unfused', I['params_unfused']))
def _(eng, D, I):
    E, it, st = eng.energies_from_params(KIND_UNFUSED, I['params_unfused'], I['h'])
    return {'E': E, 'iters': it, 'status': st}


@family('launch_from_params', leaves='solve', states=lambda I: ('params', I['params']))
def _(eng, D, I):
    """resident ansatz parameters: at D = 4 the direct kernel builds the tensors itself, and they are materialised when asked for"""
    eng.set_ansatz_params(KIND, I['params'])
    eng.set_hamiltonian(I['h'])
    eng.launch(B, krylov_fallback=True)
    return dict(_solved(eng, *eng.results(B)), tensors=eng.tensors(B))


@family('launch_from_su', leaves='solve', states=lambda I: ('su', I['su']))
def _(eng, D, I):
    su = np.ascontiguousarray(I['su'])
    L.check(eng._lib.qmps_set_states_su(eng._ctx, B, _f64(su)))
    eng.set_hamiltonian(I['h'])
    eng.launch(B, krylov_fallback=True)
    return dict(_solved(eng, *eng.results(B)), tensors=eng.tensors(B))


@family('energies_from_su', leaves='solve', sets=('hamiltonian',), states=lambda I: ('su', I['su']))
def _(eng, D, I):
    return _solved(eng, *eng.energies_from_su(I['su'], I['h']))


@family('launch_energy_only', leaves='solve', states=_tensor_states('A'))
def _(eng, D, I):
    """energies of given environments: nothing is solved, so the pass reports 0 iterations and status 0 for them"""
    eng.set_tensors(I['A'][:B])
    eng.set_hamiltonian(I['h'])
    eng.set_env_guess(I['guess'])
    eng.launch_energy_only(B)
    E, it, st = eng.results(B)
    return {'E_only': eng.results(B, counts=False)[0], 'E_given': E, 'iters': it, 'status': st, 'r': eng.environments(B)}


@family('rdm', leaves='solve', states=_tensor_states('A'))
def _(eng, D, I):
    eng.set_tensors(I['A'][:B])
    eng.set_hamiltonian(I['h'])
    eng.launch(B, krylov_fallback=True)
    rho = eng.rdm(B)
    out = _solved(eng, *eng.results(B))          # (the energies are those of the pass that wrote rho)
    out['rho'] = rho
    return out


@family('summed_cost', leaves='solve', states=_tensor_states('A'))
def _(eng, D, I):
    eng.set_tensors(I['A'][:B])
    eng.set_hamiltonian(I['h'])
    eng.launch(B, krylov_fallback=True)
    out = _solved(eng, *eng.results(B))
    out['summed'] = eng.summed_cost(B)
    return out


@family('rotosolve', leaves='solve', n=R)
def _(eng, D, I):
    eng.set_hamiltonian(I['h'])
    hist, p = eng.rotosolve(KIND, I['roto'], n_sweeps=2)
    out = _solved(eng, *eng.results(R), n=R)
    out.update(hist=hist, p=p)
    return out


@family('double_rotosolve', leaves='solve', n=R, sets=('roto_rule',))
def _(eng, D, I):
    eng.set_hamiltonian(I['h'])
    hist, p = eng.double_rotosolve(KIND, I['roto'], n_sweeps=2)
    out = _solved(eng, *eng.results(R), n=R)
    out.update(hist=hist, p=p)
    return out


@family('cell2_energies', Ds=(2,), leaves='cell2', sets=('hamiltonian',))
def _(eng, D, I):
    E, it, st = eng.cell2_energies(I['cell_U'][0], I['cell_U'][1], I['h'])
    return {'E': E, 'iters': it, 'status': st}


@family('cell2_energies_su', Ds=(2,), leaves='cell2', sets=('hamiltonian',))
def _(eng, D, I):
    E, it, st = eng.cell2_energies_su(I['cell_p'], I['h'])
    return {'E': E, 'iters': it, 'status': st}


@family('opt_env_objective', Ds=(2,))
def _(eng, D, I):
    f, parts = eng.opt_env_objective(I['optenv_p'], I['h1'][0], want_parts=True)
    return {'f_env': f, 'parts': parts}


def _overlap_out(got, want_r):
    out = {'eta': got[0], 'rounds': got[1], 'ostatus': got[2]}
    if want_r:
        out['x'] = got[3]
    return out


for _want_r in (False, True):
    _leaves = 'overlap_r' if _want_r else 'overlap'
    _tag = '_r' if _want_r else ''

    def _run(eng, D, I, _want_r=_want_r):
        eng.overlap_stats(reset=True)
        out = _overlap_out(eng.overlaps(I['ref'], I['cands'], I['WW'], want_r=_want_r), _want_r)
        out['f'] = eng.overlap_objective(B)
        out['stats'] = np.array(sorted(eng.overlap_stats().items()), dtype=object)[:, 1].astype(np.int64)
        return out
    family('overlaps_tensor' + _tag, leaves=_leaves, sets=('overlap',), states=_tensor_states('cands'))(_run)

    def _run(eng, D, I, _want_r=_want_r):
        out = _overlap_out(eng.overlaps(I['ref'], I['cands_U'], I['WW'], kind='unitary', want_r=_want_r), _want_r)
        out['f'] = eng.overlap_objective(B)
        return out
    family('overlaps_unitary' + _tag, leaves=_leaves, sets=('overlap',), states=lambda I: ('unitary', I['cands_U']))(_run)

    def _run(eng, D, I, _want_r=_want_r):
        out = _overlap_out(eng.overlaps(OP.tensor(D, I['traj'][0]), I['cand_params'], I['WW'], kind='params', ansatz=KIND, want_r=_want_r), _want_r)
        out['f'] = eng.overlap_objective(B)
        return out
    family('overlaps_params' + _tag, leaves=_leaves, sets=('overlap',), states=lambda I: ('params', I['cand_params']))(_run)


@family(f'overlaps_tensor_r_cap{CAP_SHORT}', leaves='overlap_r', sets=('overlap',), states=_tensor_states('cands'))
def _(eng, D, I):
    out = _overlap_out(eng.overlaps(I['ref'], I['cands'], I['WW'], max_rounds=CAP_SHORT, want_r=True), True)
    out['f'] = eng.overlap_objective(B)
    return out


@family(f'overlaps_far_cap{CAP_KRYLOV}', Ds=(8, 16), leaves='overlap', sets=('overlap',), states=_tensor_states('far'))
def _(eng, D, I):
    eng.overlap_stats(reset=True)
    out = _overlap_out(eng.overlaps(I['far_ref'], I['far'], I['far_WW'], max_rounds=CAP_KRYLOV, tol=1e-12), False)
    out['f'] = eng.overlap_objective(B)
    out['stats'] = np.array(sorted(eng.overlap_stats().items()), dtype=object)[:, 1].astype(np.int64)
    return out


@family('overlap_launch_warm', leaves='overlap_r', sets=('overlap',), states=_tensor_states('moved'))
def _(eng, D, I):
    """the candidates move a little; every slot starts from the fixed point the launch before left there"""
    first = eng.overlaps(I['ref'], I['cands'], I['WW'], want_r=True)
    eng.set_tensors(I['moved'])
    eng.overlap_launch(B, want_r=True, warm=True)
    out = _overlap_out(eng.overlap_results(B, want_r=True), True)
    out.update(f=eng.overlap_objective(B), eta_first=first[0])
    return out


@family('overlap_eval_group', leaves='overlap', n=T * G, sets=('overlap',), states=lambda I: ('params', I['traj_cands']))
def _(eng, D, I):
    eng.overlap_set_refs_params(KIND, I['traj'], I['WW'])
    eng.overlap_set_group(G)
    f, st = eng.overlap_eval_params(KIND, I['traj_cands'])
    eta, rounds, ost = eng.overlap_results(T * G)
    return {'f': f, 'ostatus': st, 'eta': eta, 'rounds': rounds}


@family('overlap_eval_mask', leaves='overlap', n=T * G, sets=('overlap',), states=lambda I: ('params', I['traj_moved']))
def _(eng, D, I):
    """a one-shot mask: trajectory 1 is skipped and keeps what the evaluation before left; the mask is spent afterwards"""
    eng.overlap_set_refs_params(KIND, I['traj'], I['WW'])
    eng.overlap_set_group(G)
    f0, _ = eng.overlap_eval_params(KIND, I['traj_cands'])
    eng.overlap_set_active([1, 0, 1])
    f1, st1 = eng.overlap_eval_params(KIND, I['traj_moved'])
    f2, st2 = eng.overlap_eval_params(KIND, I['traj_moved'])
    return {'f_first': f0, 'f_masked': f1, 'f': f2, 'ostatus': st2}


@family('overlap_gradient', Ds=(4, 8, 16), leaves='gradient', n=T, sets=('overlap',), states=lambda I: ('params', I['iterates2']))
def _(eng, D, I):
    eng.overlap_set_refs_params(KIND, I['traj'], I['WW'])
    f, g, st = eng.overlap_gradient(KIND, I['iterates'])
    f2, g2, st2 = eng.overlap_gradient(KIND, I['iterates2'], warm=True)
    return {'f_cold': f, 'g_cold': g, 'st_cold': st, 'f_warm': f2, 'g_warm': g2, 'st_warm': st2}


@family('overlap_amplitudes', leaves='upload', sets=('overlap',), states=_tensor_states('cands'))
def _(eng, D, I):
    eng.set_tensors(I['cands'])
    eng.overlap_set(I['ref'], I['WW'])
    return {'amp': eng.overlap_amplitudes(I['q'])}


EVOLVE = dict(n_steps=1, maxiter=3)


def _bfgs_leaves(D):
    return 'evolve_bfgs' if D >= 4 else 'evolve_device'      # (D = 2 eigen-solves its neighbours: no gradient batch, no fixed points of one)


@family('evolve_rotosolve', leaves='evolve_rotosolve', n=T, sets=('overlap', 'roto_rule'))
def _(eng, D, I):
    p, ph, fh = eng.evolve_rotosolve(KIND, I['traj'], I['WW'], n_steps=1, n_sweeps=1)
    return {'p': p, 'params_hist': ph, 'f_hist': fh}


_EVOLVE_KEYS = ('x', 'params_hist', 'fun', 'fun_start', 'nit', 'hess_inv')


@family('evolve_bfgs', leaves=_bfgs_leaves, n=T, sets=('overlap',))
def _(eng, D, I):
    got = eng.evolve_bfgs(KIND, I['traj'], I['WW'], counters=False, **EVOLVE)
    return {k: got[k] for k in _EVOLVE_KEYS}


@family('evolve_bfgs_device', Ds=(2, 4, 16), leaves='evolve_device', n=T, sets=('overlap',))
def _(eng, D, I):
    got = eng.evolve_bfgs_device(KIND, I['traj'], I['WW'], **EVOLVE)
    return dict({k: got[k] for k in _EVOLVE_KEYS}, nfev=np.array([got['nfev'], got['failed_evaluations']]))


def _evolve_direct(eng, I, device, through_opts):
    """the spellings of the two drivers that EnergyEngine does not use: qmps_evolve_bfgs by position, qmps_evolve_bfgs_device_opts"""
    al = np.array([1.0, 0.5, 0.25, 0.125, 1 / 16, 1 / 64, 1 / 256, 1 / 4096])
    x = np.array(I['traj'], dtype=np.float64, order='C', copy=True)
    WW = np.ascontiguousarray(I['WW'], dtype=np.complex128)
    ph, fh, hinv = np.empty((1, T, P)), np.empty((1, 2, T)), np.zeros((T, P, P))
    nit = np.zeros((1, T) if device else (1,), dtype=np.int32)
    max_rounds = 60 if eng.D in (2, 4) else 100000
    if through_opts:
        opts = L.EvolveOpts()
        L.check(eng._lib.qmps_evolve_opts_init(ctypes.byref(opts)))
        opts.n_steps, opts.maxiter, opts.n_alphas, opts.flags, opts.max_rounds = 1, EVOLVE['maxiter'], len(al), 0, max_rounds
        opts.gtol, opts.h, opts.c1, opts.tol, opts.alphas = 1e-5, 1e-6, 1e-4, 1e-12, _f64(al)
        res = L.EvolveOut(size=ctypes.sizeof(L.EvolveOut), hinv=_f64(hinv), params_hist=_f64(ph), f_hist=_f64(fh), nit=_i32(nit), counters=None)
        L.check(eng._lib.qmps_evolve_bfgs_device_opts(eng._ctx, T, KIND, P, _f64(x), _f64(WW.view(np.float64)), ctypes.byref(opts), ctypes.byref(res)))
    else:
        L.check(eng._lib.qmps_evolve_bfgs(eng._ctx, T, KIND, P, _f64(x), _f64(WW.view(np.float64)), 1, EVOLVE['maxiter'], 1e-5, 1e-6, 1e-4, len(al), _f64(al), 0,
                                          max_rounds, 1e-12, _f64(hinv), _f64(ph), _f64(fh), _i32(nit), None))
    return {'x': x, 'params_hist': ph, 'fun': fh[:, 1].copy(), 'fun_start': fh[:, 0].copy(), 'nit': nit, 'hess_inv': hinv}


@family('evolve_bfgs_positional', leaves=_bfgs_leaves, n=T, sets=('overlap',))
def _(eng, D, I):
    return _evolve_direct(eng, I, device=False, through_opts=False)


@family('evolve_bfgs_device_opts', Ds=(2, 4, 16), leaves='evolve_device', n=T, sets=('overlap',))
def _(eng, D, I):
    return _evolve_direct(eng, I, device=True, through_opts=True)


def _solve_for_observables(eng, I):
    eng.set_tensors(I['A'][:B])
    eng.set_hamiltonian(I['h'])
    eng.launch(B, krylov_fallback=True)


@family('correlators', leaves='solve', states=_tensor_states('A'))
def _(eng, D, I):
    _solve_for_observables(eng, I)
    C, one = eng.correlators(I['ops'], N_MAX, B, want_one_site=True)
    return dict(_solved(eng, *eng.results(B)), C=C, one=one)


@family('entanglement', leaves='solve', states=_tensor_states('A'))
def _(eng, D, I):
    _solve_for_observables(eng, I)
    p, S, V = eng.entanglement(B, want_vectors=True)
    return dict(_solved(eng, *eng.results(B)), p=p, S=S, V=V)


@family('correlator_sums', leaves='solve', states=_tensor_states('A'))
def _(eng, D, I):
    _solve_for_observables(eng, I)
    Gs, one, site = eng.correlator_sums(I['ops'], Z, B, want_one_site=True, want_site=True)
    return dict(_solved(eng, *eng.results(B)), G=Gs, one=one, site=site)


@family('ansatz_probe')
def _(eng, D, I):
    return {'A_plain': eng.ansatz_probe(KIND, I['params']),
            'A_shifted': eng.ansatz_probe(KIND, I['roto'], nsh=3, index=1),
            'A_shifted6': eng.ansatz_probe(KIND, I['roto'], nsh=6, index=P - 1),
            'A_fd': eng.ansatz_probe(KIND, I['traj'], fd_h=1e-3, active=[1, 0, 1], fill=7 - 2j)}


@family('roto_rule_probe')
def _(eng, D, I):
    return {'theta': eng.roto_rule_probe(I['abcd'], L.ROTO_REFERENCE), 'theta_global': eng.roto_rule_probe(I['abcd'], L.ROTO_GLOBAL_ARGMIN)}


@family('su_unitaries')
def _(eng, D, I):
    return {'U4': eng.su_unitaries(I['su4'], 4), 'U': eng.su_unitaries(I['su'][:5], 2 * D)}


def _c(a):
    a = np.ascontiguousarray(a, dtype=np.complex128)
    return a, _f64(a.view(np.float64))


@family('bw_expval')
def _(eng, D, I):
    U1, U2, Oc = _c(I['bw'][0]), _c(I['bw'][1]), _c(I['bw_O'])          # (array, pointer): the arrays stay referenced during the call
    out = np.empty(7, dtype=np.complex128)
    L.check(eng._lib.qmps_bw_expval(eng._ctx, 7, 2, U1[1], U2[1], Oc[1], 1, _f64(out.view(np.float64))))
    return {'expval': out}


@family('bw_env')
def _(eng, D, I):
    U = [_c(I['bw'][k]) for k in range(4)]
    out = {}
    for side in (0, 1):
        mat, eta, vec, st = np.empty((7, 4, 4), dtype=np.complex128), np.empty(7, dtype=np.complex128), np.empty((7, 2, 2), dtype=np.complex128), np.empty(7, dtype=np.int32)
        L.check(eng._lib.qmps_bw_env(eng._ctx, 7, side, U[0][1], U[1][1], U[2][1], U[3][1], 40, 1e-13, _f64(mat.view(np.float64)), _f64(eta.view(np.float64)),
                                     _f64(vec.view(np.float64)), _i32(st)))
        out.update({f'mat{side}': mat, f'eta{side}': eta, f'vec{side}': vec, f'st{side}': st})
    return out


@family('bw_manifold')
def _(eng, D, I):
    U = [_c(I['bw'][k]) for k in range(4)]
    Mr, Ml, W = _c(I['bw_M'][0]), _c(I['bw_M'][1]), _c(I['bw_W'])
    out = np.empty(7, dtype=np.complex128)
    L.check(eng._lib.qmps_bw_manifold(eng._ctx, 7, U[0][1], U[1][1], U[2][1], U[3][1], Mr[1], Ml[1], 1, W[1], 1, _f64(out.view(np.float64))))
    return {'manifold': out}


@family('upload_tensors', leaves='upload', states=_tensor_states('cands'))
def _(eng, D, I):
    eng.set_tensors(I['cands'])
    return {'tensors': eng.tensors(B)}


CAPPED = tuple(name for name in FAMILIES if '_cap' in name)


def legal(D):
    """the families of bond dimension D, in a fixed order"""
    return [name for name, f in FAMILIES.items() if f.legal(D)]


# Y whose result the header allows to depend on what ran before (compared with the oracle alone); frozen by tests/test_call_order_cpu.py.
# (The one case the header names - a QMPS_BFGS_WARM continuation of qmps_evolve_bfgs_device at D = 2 agrees "to the rounding of a
# solve, not bit for bit" - is a continuation of ONE call by another; no family here continues a run, so nothing is exempt.)
EXEMPT_FROM_BYTES = frozenset()

# ---------------------------------------------------------------------------------------------------------------------------------
# readers


def _refusal(call):
    """the arrays a read-back returns, or the error code it refuses with"""
    try:
        got = call()
    except L.QmpsError as e:
        return ('refused', e.code)
    return tuple(got) if isinstance(got, tuple) else (got,)


def _energy_only(eng, n):
    eng.launch_energy_only(n)
    return eng.results(n, counts=False)[0]


def _launch_warm(eng, n):
    """(eta of the warm launch, statuses, eta of a cold launch over the same candidates, statuses)"""
    eng.overlap_launch(n, tol=1e-13, want_r=True, warm=True)
    eta, _, st = eng.overlap_results(n)
    eng.overlap_launch(n, tol=1e-13, want_r=True)
    eta_c, _, st_c = eng.overlap_results(n)
    return eta, st, eta_c, st_c


def _gradient_warm(eng, n):
    I = inputs(eng.D)
    return eng.overlap_gradient(KIND, I['iterates2'], warm=True)


# in the order the harness reads them: those that leave everything as it is first
ENERGY_READERS = {
    'results': lambda eng, n: eng.results(n),
    'results_status': lambda eng, n: eng.results_status(n),
    'environments': lambda eng, n: eng.environments(n),
    'tensors': lambda eng, n: eng.tensors(n),
    'get_cost': lambda eng, n: eng.get_cost()[:2],
    'correlators': lambda eng, n: eng.correlators(inputs(eng.D)['ops'], N_MAX, n, want_one_site=True),
    'entanglement': lambda eng, n: eng.entanglement(n, want_vectors=True),
    'correlator_sums': lambda eng, n: eng.correlator_sums(inputs(eng.D)['ops'], Z, n, want_one_site=True, want_site=True),
    'launch_energy_only': _energy_only,
    'rdm': lambda eng, n: eng.rdm(n),
}
OVERLAP_READERS = {
    'overlap_results_r': lambda eng, n: eng.overlap_results(n, want_r=True),
    'overlap_objective': lambda eng, n: eng.overlap_objective(n),
    'overlap_launch_warm': _launch_warm,
    'overlap_gradient_warm': _gradient_warm,
}
READERS = dict(ENERGY_READERS, **OVERLAP_READERS)
# the outputs of a family that a reader must return byte for byte when its outcome is 'of X'
OF_X = {'results': ('E|E_given', 'iters', 'status'), 'results_status': ('status|ostatus',), 'environments': ('r',), 'get_cost': ('cost',),
        'overlap_results_r': ('eta', 'rounds', 'ostatus', 'x'), 'overlap_objective': ('f',)}


def reader_legal(reader, D):
    return D >= 4 or reader != 'overlap_gradient_warm'          # "qmps_overlap_gradient: D = 4, 8, 16"


def read(eng, reader, n):
    eng.n_terms = eng.n_terms or 1
    try:
        eng.set_window(0)
    except L.QmpsError as e:
        return ('refused', e.code)
    return _refusal(lambda: READERS[reader](eng, n))


def prepare_energy(eng, D):
    """The resident state the energy readers are read against: three windows of solved states, their environments stored, and a summed cost."""
    I = inputs(D)
    canon(eng)
    eng.set_tensors(I['A'])
    eng.set_hamiltonian(I['h'])
    for w in range(WINDOWS):
        eng.set_window(w * B)
        eng.launch(B, krylov_fallback=True)
    eng.set_window(0)
    eng.launch(B, accumulate_cost=True, krylov_fallback=True)
    eng.cost_launch(B)
    eng.sync()


def prepare_overlap(eng, D):
    """The resident state the overlap readers are read against: candidates, one shared reference, a launch that kept its fixed points."""
    I = inputs(D)
    canon(eng)
    eng.set_hamiltonian(I['h'])
    eng.set_tensors(I['moved'])
    eng.overlap_set(I['ref'], I['WW'])
    eng.overlap_launch(B, tol=1e-13, want_r=True)
    eng.sync()


# ---------------------------------------------------------------------------------------------------------------------------------
# what a family leaves -> what each reader then does, and the header sentence it rests on

_S = {
    'probe': 'qmps_ansatz_probe: "The build goes to scratch memory: the context\'s resident states, parameters and environments are NOT touched"; the brick-wall, '
             'SU and rule probes take "any context" and address no resident array',
    'upload': 'RESIDENT RESULTS: "An upload (qmps_set_states*, also inside the one-shot calls) replaces the resident states and outdates all of them"',
    'launch': 'qmps_energy_launch: "One pass over the resident batch: power-iteration right environment + two-site energy"; qmps_get_energies / qmps_get_env '
              'read the window of the last launch that covered it',
    'observable': '"Resident states, environments, energies, iteration counts and statuses stay exactly as they are."',
    'derived': 'qmps_get_rdm / qmps_energy_only_launch / qmps_correlators / qmps_entanglement / qmps_correlator_sums: "from the resident states and the resident '
               'environments (no solve)"',
    'no_env_out': 'QMPS_FLAG_NO_ENV_OUT: "qmps_get_env / qmps_get_rdm / qmps_energy_only_launch then fail with QMPS_ERR_STATE until a launch without the flag has run"',
    'states': 'qmps_get_states: "read back the resident state tensors"',
    'cost': 'qmps_get_cost: "copies the (all-reduced) cost[n_terms] to the host" - the cost of the last qmps_cost_launch, which no other call writes',
    'cell2': 'the two-site unit cell is "a one-shot call: results at the start of the buffers"; RESIDENT RESULTS: it leaves no single-site states and no environments',
    'overlap_over_energy': 'RESIDENT RESULTS: "An overlap launch takes over the iteration counts and statuses of its window and outdates every environment"',
    'overlap_results': 'qmps_overlap_get: the results of the launch over the resident candidates; "want_r: also keep the fixed points (read back by qmps_overlap_get with r_out != NULL)"',
    'overlap_no_r': 'qmps_overlap_get: r_out needs a launch with QMPS_OVERLAP_WANT_R over the resident candidates (RESIDENT RESULTS)',
    'energy_over_overlap': 'RESIDENT RESULTS: "An energy launch ... outdates the overlap results and fixed points of its window"; QMPS_OVERLAP_WARM "Needs ... what the '
                           'previous launch with QMPS_OVERLAP_WANT_R left there"',
    'warm_keeps': 'QMPS_OVERLAP_WARM: "every candidate starts from the RESIDENT fixed point of its slot - what the previous launch with QMPS_OVERLAP_WANT_R left there" '
                  '(a launch that keeps no fixed points, and an upload of moved candidates, leave them)',
    'status_any': 'qmps_get_status: "per-evaluation status of the last launch over the window (energy or overlap)"',
    'gradient': 'qmps_overlap_gradient: "QMPS_OVERLAP_WARM: both power iterations start from the fixed points the previous call left resident (same T)"; RESIDENT RESULTS: '
                'the gradient and evolve calls outdate environments, counts, statuses and overlap results',
    'evolve_states': 'RESIDENT RESULTS: "qmps_evolve_rotosolve leaves its T final vectors resident as states; qmps_evolve_bfgs and qmps_evolve_bfgs_device leave no '
                     'resident states" - qmps_evolve_bfgs "the fixed points of its last gradient batch, where QMPS_BFGS_WARM and a QMPS_OVERLAP_WARM gradient of the same T '
                     'look for them (D = 4, 8, 16)"',
    'evolve': 'RESIDENT RESULTS: "the gradient and evolve calls outdate environments, energies\' counts and statuses and overlap results"; qmps_evolve_rotosolve also '
              'the energies (d_E is its objective buffer)',
}


def _row(**kw):
    return kw


_ENV_READERS = ('environments', 'correlators', 'entanglement', 'correlator_sums', 'launch_energy_only', 'rdm')


def _leaves(results, status, env, tensors, cost, o_results, o_objective, o_warm, o_grad):
    row = {'results': results, 'results_status': status, 'tensors': tensors, 'get_cost': cost, 'overlap_results_r': o_results,
           'overlap_objective': o_objective, 'overlap_launch_warm': o_warm, 'overlap_gradient_warm': o_grad}
    for r in _ENV_READERS:
        row[r] = env if r == 'environments' or env[0] == 'refuse' else (env[0], _S['derived'])
    return row


_same = ('same', _S['probe'])
LEAVES = {
    'nothing': {r: _same for r in READERS},
    'upload': _leaves(('refuse', _S['upload']), ('refuse', _S['upload']), ('refuse', _S['upload']), ('of X', _S['states']), ('same', _S['cost']),
                      ('refuse', _S['upload']), ('refuse', _S['upload']), ('of X', _S['warm_keeps']), ('same', _S['gradient'])),
    'solve': _leaves(('of X', _S['launch']), ('of X', _S['launch']), ('of X', _S['launch']), ('of X', _S['states']), ('same', _S['cost']),
                     ('refuse', _S['upload']), ('refuse', _S['upload']), ('refuse', _S['energy_over_overlap']), ('refuse', _S['energy_over_overlap'])),
    'noenv': _leaves(('of X', _S['launch']), ('of X', _S['launch']), ('refuse', _S['no_env_out']), ('of X', _S['states']), ('same', _S['cost']),
                     ('refuse', _S['upload']), ('refuse', _S['upload']), ('refuse', _S['energy_over_overlap']), ('refuse', _S['energy_over_overlap'])),
    'cell2': _leaves(('of X', _S['cell2']), ('of X', _S['cell2']), ('refuse', _S['cell2']), ('refuse', _S['cell2']), ('same', _S['cost']),
                     ('refuse', _S['cell2']), ('refuse', _S['cell2']), ('refuse', _S['cell2']), ('same', _S['gradient'])),
    'overlap': _leaves(('refuse', _S['upload']), ('of X', _S['status_any']), ('refuse', _S['overlap_over_energy']), ('of X', _S['states']), ('same', _S['cost']),
                       ('refuse', _S['overlap_no_r']), ('of X', _S['overlap_results']), ('of X', _S['warm_keeps']), ('same', _S['gradient'])),
    'overlap_r': _leaves(('refuse', _S['upload']), ('of X', _S['status_any']), ('refuse', _S['overlap_over_energy']), ('of X', _S['states']), ('same', _S['cost']),
                         ('of X', _S['overlap_results']), ('of X', _S['overlap_results']), ('of X', _S['warm_keeps']), ('refuse', _S['energy_over_overlap'])),
    'gradient': _leaves(('refuse', _S['gradient']), ('refuse', _S['gradient']), ('refuse', _S['gradient']), ('of X', _S['states']), ('same', _S['cost']),
                        ('refuse', _S['gradient']), ('refuse', _S['gradient']), ('refuse', _S['gradient']), ('of X', _S['gradient'])),
    'evolve_rotosolve': _leaves(('refuse', _S['evolve']), ('refuse', _S['evolve']), ('refuse', _S['evolve']), ('of X', _S['evolve_states']), ('same', _S['cost']),
                                ('refuse', _S['evolve']), ('refuse', _S['evolve']), ('refuse', _S['evolve']), ('refuse', _S['evolve'])),
    'evolve_bfgs': _leaves(('refuse', _S['evolve']), ('refuse', _S['evolve']), ('refuse', _S['evolve']), ('refuse', _S['evolve_states']), ('same', _S['cost']),
                           ('refuse', _S['evolve']), ('refuse', _S['evolve']), ('refuse', _S['evolve_states']), ('of X', _S['evolve_states'])),
    'evolve_device': _leaves(('refuse', _S['evolve']), ('refuse', _S['evolve']), ('refuse', _S['evolve']), ('refuse', _S['evolve_states']), ('same', _S['cost']),
                             ('refuse', _S['evolve']), ('refuse', _S['evolve']), ('refuse', _S['evolve_states']), ('refuse', _S['evolve_states'])),
}
for _k in ('solve', 'noenv'):
    LEAVES[_k + '_cost'] = dict(LEAVES[_k], get_cost=('of X', _S['cost']))


def expect(name, D):
    """reader -> (outcome, header sentence) after family `name` at bond dimension D"""
    return LEAVES[FAMILIES[name].leaves(D)]


EXPECT = {(name, D, reader): outcome for name, f in FAMILIES.items() for D in f.Ds for reader, outcome in expect(name, D).items()}

# ---------------------------------------------------------------------------------------------------------------------------------
# persistent settings: what qmps_set_* makes last until it is set again.  `apply` puts odd values in place, `probe` reads them back
# (a getter where the header has one, the behaviour they control where it has none).  A family leaves alone whatever it does not name
# in `sets`.

SETTINGS = ('solver', 'handoff', 'hamiltonian', 'roto_rule', 'evolve_groups', 'overlap')
# the entry points the header documents as replacing a setting: its setter, and the one-shot calls that take it as an argument
REPLACED_BY = {
    'solver': {'qmps_set_default_solver'},
    'handoff': {'qmps_set_handoff'},
    'hamiltonian': {'qmps_set_hamiltonian', 'qmps_energy_batch', 'qmps_energy_batch_ansatz', 'qmps_energy_batch_su', 'qmps_cell2_energy_batch', 'qmps_cell2_energy_batch_su'},
    'roto_rule': {'qmps_set_roto_rule'},
    'evolve_groups': {'qmps_set_evolve_groups'},
    'overlap': {'qmps_overlap_set', 'qmps_overlap_set_refs_ansatz', 'qmps_overlap_set_group', 'qmps_overlap_batch', 'qmps_evolve_bfgs', 'qmps_evolve_bfgs_opts',
                'qmps_evolve_bfgs_device', 'qmps_evolve_bfgs_device_opts', 'qmps_evolve_rotosolve'},
}


def replaced_settings(name):
    """the settings a family's own calls replace: those it names, and those whose replacing entry points it calls"""
    calls = _calls_of(FAMILIES[name].run, set())
    return FAMILIES[name].sets | {s for s, fns in REPLACED_BY.items() if fns & calls}


def apply_settings(eng, D):
    I = inputs(D)
    eng.set_solver('plain', handoff=5)
    eng.set_hamiltonian(I['h1'])
    eng.set_roto_rule(L.ROTO_GLOBAL_ARGMIN)
    eng.set_evolve_groups(1)
    eng.set_exchange_period(3)
    eng.overlap_set_refs_params(KIND, I['traj'], I['WW'])
    eng.overlap_set_group(G)


def probe_settings(eng, D):
    """setting -> arrays that tell it apart from its default and from what any family sets"""
    I = inputs(D)
    rule, skip, period = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    L.check(eng._lib.qmps_get_roto_rule(eng._ctx, ctypes.byref(rule)))
    out = {'handoff': np.array([eng.handoff]), 'roto_rule': np.array([rule.value]), 'evolve_groups': np.array([eng.evolve_groups(4096)]),
           'schedule': np.array(eng.squaring_schedule)}
    # the references, the operator and the group: an evaluation against them (its own upload; nothing else is read)
    out['overlap'] = _refusal(lambda: eng.overlap_eval_params(KIND, I['traj_cands']))
    # the Hamiltonian: a launch over an upload of the probe's own, with the solver named in the call
    eng.set_tensors(I['A'][:B])

    def energies():
        eng.launch(B, solver='squaring', krylov_fallback=True)
        return eng.results(B)[0]
    out['hamiltonian'] = _refusal(energies)
    # the solver of the one-shot calls: rotosolve reads it (and the roto rule is not its business)
    out['solver'] = _refusal(lambda: eng.rotosolve(KIND, I['roto'], n_sweeps=1, max_iter=50)[0]) + _refusal(lambda: eng.results(R)[1])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the header against the tables

# entry points that keep no state in a context's buffers: version and error calls, device info, timers, peak probes, the communicator
# calls and the option-struct helpers
NOT_STATEFUL = frozenset({
    'qmps_abi_version', 'qmps_abi_minor', 'qmps_last_error', 'qmps_selftest_exception', 'qmps_device_count', 'qmps_device_info',
    'qmps_timer_begin', 'qmps_timer_end', 'qmps_kernel_time', 'qmps_set_kernel_timing_period',
    'qmps_probe_fp64_peak', 'qmps_probe_fp64_mfma_peak', 'qmps_probe_hbm_peak',
    'qmps_comm_unique_id', 'qmps_comm_init', 'qmps_comm_destroy', 'qmps_comm_count', 'qmps_allreduce_sum', 'qmps_allreduce_min', 'qmps_allreduce_cost',
    'qmps_exchange_stats',
    'qmps_evolve_opts_init',
})


def declared_entry_points(header_text):
    return sorted(set(re.findall(r'^(?:int|const char\*)\s+(qmps_\w+)\s*\(', header_text, flags=re.M)))


def _calls_of(fn, seen):
    """the qmps_* symbols a function calls: by name in its source, and through the EnergyEngine methods it names"""
    if fn in seen:
        return set()
    seen.add(fn)
    src = inspect.getsource(fn)
    found = set(re.findall(r'\b(qmps_\w+)\s*\(', src))
    for method in set(re.findall(r'\beng\.(\w+)', src)) | set(re.findall(r'\bself\.(\w+)\(', src)):
        attr = inspect.getattr_static(EnergyEngine, method, None)
        if isinstance(attr, property):
            attr = attr.fget
        if inspect.isfunction(attr):
            found |= _calls_of(attr, seen)
    for helper in set(re.findall(r'(?<!def )\b(_[a-z]\w+)\(', src)):
        obj = globals().get(helper)
        if inspect.isfunction(obj):
            found |= _calls_of(obj, seen)
    return found


def called_entry_points():
    """every qmps_* symbol some family, reader, preparation or settings probe calls (and the context's lifetime: the tests create and close their contexts)"""
    fns = [f.run for f in FAMILIES.values()] + list(READERS.values()) + [prepare_energy, prepare_overlap, apply_settings, probe_settings, canon, read,
                                                                         EnergyEngine.__init__, EnergyEngine.close]
    seen, found = set(), set()
    for fn in fns:
        found |= _calls_of(fn, seen)
    return found
