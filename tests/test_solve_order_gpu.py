"""GPU: the D = 4 energy kernels solve their 16 x 16 system by LU elimination with the pivots taken round the quad and back substitution
by columns (DirectD4::solve_gathered / normalise_gathered, qmps_direct_core.h; CPU: test_solve_order_cpu.py).  The cold-start kernel at the
batch sizes where a wave is a lone quad, partly filled, full, and one past a wave boundary; the near-singular family of
tests/conditioning_cases.py; the warm-start instantiation's solve (stale environments); a fused-ansatz instantiation against the tensor
kernel on the same tensors.

Measured on one MI355X: Haar batches E 3.6e-13 (the C oracle's own power iteration) / r 7.8e-16 from the oracles, E 8.3e-16 / r 6.7e-16
from the emulation; the family r 5.9e-15, rho 6.4e-15, E 7.1e-15 from the mpmath reference, r 1.8e-15 from oracle.env_direct, 1 522 rows
status 0 and 342 status 2; warm launch E 5.6e-16 / r 6.1e-16 from the emulation; ansatz kernel E 3.3e-15 / r 2.1e-15 from the tensor kernel
(smallest gap 2.3e-2)."""
import numpy as np
import pytest

from oracle import qmps_oracle as O
from qmps_amd import _lib
from tests import conditioning_cases as CC
from tests import direct_emu as EMU
from tests import rho_need_cases as RN
from tests import site_factor_cases as SF

pytestmark = pytest.mark.gpu

ORACLE_TOL = 1e-10       # E and r against the oracle
EMU_TOL = 1e-13          # E and r against the CPU emulation of the same source
SHAPES = [1, 15, 16, 17, 33]
H2 = np.stack([np.asarray(RN.TFIM).reshape(4, 4), np.asarray(RN.XXZ).reshape(4, 4)])


def against_oracle_and_emulation(label, A, E, r, emu, c_oracle):
    ref = c_oracle.energy_batch(A, H2)
    r_or = np.stack([O.env_direct(a)[0] for a in A])
    figs = {'E_oracle': np.abs(E - np.asarray(ref['E']).reshape(E.shape)).max(), 'r_oracle': np.abs(r - r_or).max(),
            'E_emu': np.abs(E - emu['E']).max(), 'r_emu': np.abs(r - emu['r']).max()}
    print(f'{label}: ' + ' '.join(f'{k}={v:.2e}' for k, v in figs.items()))
    assert np.all(ref['status'] == 0) and np.all(emu['status'] == 0) and np.all(emu['iters'] == 1)
    assert figs['E_oracle'] < ORACLE_TOL and figs['r_oracle'] < ORACLE_TOL
    assert figs['E_emu'] < EMU_TOL and figs['r_emu'] < EMU_TOL


@pytest.mark.parametrize('B', SHAPES)
def test_cold_start_on_haar_batches(B, c_oracle, engine_factory):
    eng = engine_factory(4, 64)
    eng.set_solver('direct')
    A = O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(7400 + B), 8, B))
    E, it, st = eng.energies(A, H2)
    r = eng.environments()
    assert np.all(it == 1) and np.all(st == 0)
    against_oracle_and_emulation(f'cold start B={B}', A, E, r, SF.energies_d4(A, H2), c_oracle)


def test_near_singular_family(engine_factory):
    """Every D = 4 row of tests/conditioning_cases.py in its own order (1 864 rows: 116 waves and a half): every row of status 0 or 2
    against the mpmath reference, r against oracle.env_direct where accepted in one step, the gauged rows accepted in one step."""
    fam = CC.family(4)
    h = CC.hamiltonian_terms()
    eng = engine_factory(4, 8192)
    eng.set_solver('direct', handoff=0)
    E, it, st = eng.energies(fam['A'], h)
    out = {'E': E, 'iters': it, 'status': st, 'r': eng.environments(), 'rho': eng.rdm()}
    CC.compare(4, out, h, 'fused direct kernel, family order', one_step=True, rho_self=True)
    assert not np.any(st == 1) and np.all(it[fam['gauged']] == 1)
    un = ~fam['gauged']
    assert (it[un] > 1).mean() > 0.5


def test_warm_launch_on_stale_environments(c_oracle, engine_factory):
    """The resident environments belong to other tensors: every evaluation is rejected by the warm step and goes through the warm
    instantiation's own solve (iterations 2)."""
    B = 33
    rng = np.random.default_rng(7500)
    A0 = O.unitary_to_tensor(O.haar_unitaries(rng, 8, B))
    A = O.unitary_to_tensor(O.haar_unitaries(rng, 8, B))
    eng = engine_factory(4, 64)
    eng.set_solver('direct')
    E0, it0, st0 = eng.energies(A0, H2)
    r0 = eng.environments()
    assert np.all(it0 == 1) and np.all(st0 == 0)
    eng.set_hamiltonian(H2)
    eng.set_tensors(A)
    eng.set_env_guess(r0)
    eng.launch(B, solver='direct', store_env=True, warm_start=True)
    E, it, st = eng.results(B)
    r = eng.environments(B)
    assert np.all(it == 2) and np.all(st == 0)
    against_oracle_and_emulation('warm launch, stale environments', A, E, r, EMU.energies_d4(A, H2), c_oracle)


def test_fused_ansatz_against_the_tensor_kernel(engine_factory):
    """ShallowCNOT depth-2 angles, 17 rows (a wave and a lone quad): the kernel that builds its tensors in LDS against the tensor kernel
    on host-built tensors of the same angles.  The device's tensors are the host's to 1e-13 (tests/test_api_gpu.py); the fixed-point solve
    amplifies that by at most 1 / gap (tests/test_site_factors_gpu.py: the same bound)."""
    B = 17
    prm = np.random.default_rng(7600).standard_normal((B, 4))
    A = np.stack([O.unitary_to_tensor(O.shallow_cnot_unitary(4, x)[None])[0] for x in prm])
    T = np.einsum('bsij,bskl->bikjl', A, A.conj()).reshape(B, 16, 16)
    w = np.sort(np.abs(np.linalg.eigvals(T)), axis=1)[:, ::-1]
    gap = (w[:, 0] - w[:, 1]).min()
    eng = engine_factory(4, 64)
    eng.set_solver('direct')
    eng.set_hamiltonian(H2)
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, prm)
    eng.launch(B, solver='direct', store_env=True)
    E, it, st = eng.results(B)
    r = eng.environments(B)
    eng.set_tensors(A)
    eng.launch(B, solver='direct', store_env=True)
    Et, itt, stt = eng.results(B)
    rt = eng.environments(B)
    print(f'ansatz kernel against the tensor kernel: E {np.abs(E - Et).max():.2e}, r {np.abs(r - rt).max():.2e}, smallest gap {gap:.2e}')
    assert np.all(st == 0) and np.all(it == 1) and np.array_equal(it, itt) and np.array_equal(st, stt)
    assert np.abs(E - Et).max() < max(1e-11, 1e-13 / gap) and np.abs(r - rt).max() < max(1e-11, 1e-13 / gap)
