"""GPU: the launch plumbing of the fused D = 4 kernel - pacing of a SIMD's two waves by static priority (LaneArgs::prio_first /
prio_until, QMPS_WAVE_SLOTS) and the tile load both D = 4 quad kernels share (load_tile16: whole slabs straight, the partial last
slab under its bound).  Neither touches an operation on data, so a launch with pacing on returns the bits of the launch with pacing
off, and both stay inside the bounds tests/test_operand_staging_gpu.py holds the kernels to against the emulation and the oracle.

QMPS_WAVE_SLOTS=4 stands for the device's resident wave slots, so that a handful of workgroups crosses the policy: the batches
B = 1, 15, 16, 17, 33, 49, 81 are 1, 1, 1, 2, 3, 4 and 6 workgroups - a partial and a full last tile; grids inside one generation,
which raise nobody; and 6 workgroups, of which the last two (the last half generation) start raised.  Kernels: the tensor kernel cold
with and without its environments stored, warm on stale environments, and the ShallowCNOT kernel.  The energy-only pass, whose only
change is the shared load, against the oracle's density matrix of the resident (A, r) at the same batches, in both instantiations."""
import numpy as np
import pytest

from oracle import qmps_oracle as O
from qmps_amd import _lib
from tests import direct_emu as EMU
from tests import site_factor_cases as SF
from tests.test_operand_staging_gpu import H_ALL, HAMILTONIANS, against_oracle_and_emulation

pytestmark = pytest.mark.gpu

BATCHES = [1, 15, 16, 17, 33, 49, 81]
SLOTS = 4
CAP = 128
# the energy-only pass against numpy's contraction of the oracle's density matrix: sums of at most 256 products of entries of modulus
# <= 1 (isometries, trace-one environments, |h| <= 3) in both - a few hundred roundings of 1.1e-16
ENERGY_ONLY_TOL = 1e-12


def raised_workgroups(B):
    grid = (B + 15) // 16
    return 0 if grid <= SLOTS else SLOTS // 2


def test_the_batches_cross_the_policy():
    assert [(B + 15) // 16 for B in BATCHES] == [1, 1, 1, 2, 3, 4, 6]
    assert [raised_workgroups(B) for B in BATCHES] == [0, 0, 0, 0, 0, 0, 2]
    assert [B % 16 != 0 for B in BATCHES] == [True, True, False, True, True, True, True] and 16 in BATCHES


def both_ways(monkeypatch, run):
    """run() with pacing off and with four wave slots: the same bits"""
    monkeypatch.setenv('QMPS_WAVE_SLOTS', '0')
    off = run()
    monkeypatch.setenv('QMPS_WAVE_SLOTS', str(SLOTS))
    on = run()
    for k in off:
        assert np.array_equal(off[k], on[k]), k
    return on


@pytest.mark.parametrize('B', BATCHES)
def test_tensor_kernel_cold(B, engine_factory, monkeypatch):
    A = O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(9900 + B), 8, B))
    eng = engine_factory(4, CAP)
    eng.set_solver('direct')

    def run():
        E, it, st = eng.energies(A, H_ALL)
        return {'E': E, 'iters': it, 'status': st, 'r': eng.environments()}

    def run_no_env():
        eng.set_tensors(A)
        eng.set_hamiltonian(H_ALL)
        eng.launch(B, solver='direct', store_env=False)
        E, it, st = eng.results(B)
        return {'E': E, 'iters': it, 'status': st}

    out = both_ways(monkeypatch, run)
    assert np.all(out['iters'] == 1) and np.all(out['status'] == 0)
    against_oracle_and_emulation(f'paced, cold B={B}', A, H_ALL, out['E'], out['r'], SF.energies_d4(A, H_ALL))
    lean = both_ways(monkeypatch, run_no_env)
    for k in lean:                # the launch that stores no environments computes what the storing one does
        assert np.array_equal(lean[k], out[k]), k


@pytest.mark.parametrize('B', BATCHES)
def test_tensor_kernel_warm_on_stale_environments(B, engine_factory, monkeypatch):
    rng = np.random.default_rng(10000 + B)
    A0 = O.unitary_to_tensor(O.haar_unitaries(rng, 8, B))
    A = O.unitary_to_tensor(O.haar_unitaries(rng, 8, B))
    eng = engine_factory(4, CAP)
    eng.set_solver('direct')
    eng.energies(A0, H_ALL)
    r0 = eng.environments()

    def run():
        eng.set_hamiltonian(H_ALL)
        eng.set_tensors(A)
        eng.set_env_guess(r0)
        eng.launch(B, solver='direct', store_env=True, warm_start=True)
        E, it, st = eng.results(B)
        return {'E': E, 'iters': it, 'status': st, 'r': eng.environments(B)}

    out = both_ways(monkeypatch, run)
    assert np.all(out['iters'] == 2) and np.all(out['status'] == 0)
    against_oracle_and_emulation(f'paced, warm on stale environments B={B}', A, H_ALL, out['E'], out['r'], EMU.energies_d4(A, H_ALL))


@pytest.mark.parametrize('B', BATCHES)
def test_shallow_cnot_kernel(B, engine_factory, monkeypatch):
    """pacing on == pacing off in the kernel that builds its tensors; and, as in tests/test_operand_staging_gpu.py, that kernel against the
    tensor kernel on host-built tensors of the same angles (the bound there: the device's tensors are the host's to 1e-13, the solve
    amplifies that by at most 1 / gap)"""
    h = HAMILTONIANS['tfim'][None]
    prm = np.random.default_rng(10100 + B).standard_normal((B, 4))
    A = np.stack([O.unitary_to_tensor(O.shallow_cnot_unitary(4, x)[None])[0] for x in prm])
    T = np.einsum('bsij,bskl->bikjl', A, A.conj()).reshape(B, 16, 16)
    w = np.sort(np.abs(np.linalg.eigvals(T)), axis=1)[:, ::-1]
    gap = (w[:, 0] - w[:, 1]).min()
    eng = engine_factory(4, CAP)
    eng.set_solver('direct')

    def run():
        eng.set_hamiltonian(h)
        eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, prm)
        eng.launch(B, solver='direct', store_env=True)
        E, it, st = eng.results(B)
        return {'E': E, 'iters': it, 'status': st, 'r': eng.environments(B)}

    out = both_ways(monkeypatch, run)
    eng.set_tensors(A)
    eng.launch(B, solver='direct', store_env=True)
    Et, itt, stt = eng.results(B)
    rt = eng.environments(B)
    print(f'paced ShallowCNOT B={B}: E {np.abs(out["E"] - Et).max():.2e}, r {np.abs(out["r"] - rt).max():.2e}, smallest gap {gap:.2e}')
    assert np.array_equal(out['iters'], itt) and np.array_equal(out['status'], stt)
    tol = max(1e-11, 1e-13 / gap)
    assert np.abs(out['E'] - Et).max() < tol and np.abs(out['r'] - rt).max() < tol


@pytest.mark.parametrize('terms', [1, 3])
@pytest.mark.parametrize('B', BATCHES)
def test_energy_only_pass_through_the_shared_load(B, terms, engine_factory):
    """launch_energy_only over resident (A, r): one term runs the lean instantiation, three the one that forms rho"""
    h = np.stack([HAMILTONIANS[k] for k in ('tfim', 'xxz', 'w10_only')])[:terms]
    A = O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(10200 + B), 8, B))
    eng = engine_factory(4, CAP)
    eng.set_solver('direct')
    E, it, st = eng.energies(A, h)
    r = eng.environments()
    assert np.all(st == 0)
    eng.launch_energy_only(B)
    E_only = eng.results(B)[0]
    rho = np.stack([O.two_site_rdm(A[b], r[b]) for b in range(B)])
    ref = np.real(np.einsum('tij,bji->bt', h, rho))
    print(f'energy-only B={B} terms={terms}: {np.abs(E_only - ref).max():.2e} from the oracle, {np.abs(E_only - E).max():.2e} from the solve')
    assert np.abs(E_only - ref).max() < ENERGY_ONLY_TOL
