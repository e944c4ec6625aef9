"""GPU: the D = 4 direct-solve kernels with their LDS operands staged a block ahead of the arithmetic (QMPS_STAGE_FENCE and the operand sets
of qmps_direct_core.h; CPU: test_operand_staging_cpu.py).  The staging keeps operand sets in registers across blocks - the rows of A_1 from
W_11 to W_01, the columns of A_1 from N_10 to N_11, column q of A_0 from N_00 to N_10 - and which set is live depends on the mask of the
Hamiltonian, so every mask route is run at the batch sizes where a wave is a lone quad, partly filled, full, one past a wave and past two:
TFIM (W_01), XXZ (W_10, not W_01), a Hamiltonian of one off-diagonal pair that reads W_10 and not W_01, and a complex non-Hermitian h that
reads every part and both.  Tensor kernel cold, tensor kernel warm on stale environments (its build is the staged one), the ShallowCNOT
kernel, and a near-singular slice through the power fall-back, whose hand-over (update_sites) meets the staged acceptance step's W.
Tolerances: those of tests/test_solve_order_gpu.py."""
import numpy as np
import pytest

from oracle import qmps_oracle as O
from qmps_amd import _lib
from tests import conditioning_cases as CC
from tests import direct_emu as EMU
from tests import rho_need_cases as RN
from tests import site_factor_cases as SF
from tests.test_solve_order_gpu import EMU_TOL, ORACLE_TOL, SHAPES

pytestmark = pytest.mark.gpu


def _w10_only():
    h = np.diag([0.3, -0.2, 0.5, -0.6]).astype(complex)
    h[1, 2] = h[2, 1] = 0.37            # rho[1][2]: tau = (0, 1), sigma = (1, 0) - N_10 and W_10
    return h


def _non_hermitian():
    rng = np.random.default_rng(9500)
    return rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))


HAMILTONIANS = {'tfim': np.asarray(RN.TFIM).reshape(4, 4), 'xxz': np.asarray(RN.XXZ).reshape(4, 4), 'w10_only': _w10_only(),
                'non_hermitian': _non_hermitian()}
H_ALL = np.stack([HAMILTONIANS[k] for k in ('tfim', 'xxz', 'w10_only', 'non_hermitian')])


def test_the_masks_take_the_routes_they_are_here_for():
    f = {k: SF.factors(RN.mask(h)) for k, h in HAMILTONIANS.items()}
    n_all = SF.N00 | SF.N10 | SF.N11
    assert f['tfim'] == n_all | SF.W01 and f['xxz'] == n_all | SF.W10
    assert f['w10_only'] & SF.W10 and not f['w10_only'] & SF.W01
    assert f['non_hermitian'] == n_all | SF.W01 | SF.W10 and RN.mask(HAMILTONIANS['non_hermitian']) & SF.FULL_UPPER == SF.FULL_UPPER


def against_oracle_and_emulation(label, A, h, E, r, emu):
    """E and r against the emulation of the same source, and against oracle.env_direct with E = Re sum h rho contracted in numpy (h need
    not be Hermitian)"""
    h = np.asarray(h).reshape(-1, 4, 4)
    r_or = np.stack([O.env_direct(a)[0] for a in A])
    E_or = np.real(np.einsum('nst,bts->bn', h, SF.rho_numpy(A, r_or)))
    figs = {'E_oracle': np.abs(E - E_or).max(), 'r_oracle': np.abs(r - r_or).max(), 'E_emu': np.abs(E - emu['E']).max(),
            'r_emu': np.abs(r - emu['r']).max()}
    print(f'{label}: ' + ' '.join(f'{k}={v:.2e}' for k, v in figs.items()))
    assert np.all(emu['status'] == 0) and np.all(emu['iters'] == 1)
    assert figs['E_oracle'] < ORACLE_TOL and figs['r_oracle'] < ORACLE_TOL
    assert figs['E_emu'] < EMU_TOL and figs['r_emu'] < EMU_TOL


@pytest.mark.parametrize('name', sorted(HAMILTONIANS))
@pytest.mark.parametrize('B', SHAPES)
def test_tensor_kernel_cold(B, name, engine_factory):
    h = HAMILTONIANS[name][None]
    eng = engine_factory(4, 64)
    eng.set_solver('direct')
    A = O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(9600 + B), 8, B))
    E, it, st = eng.energies(A, h)
    r = eng.environments()
    assert np.all(it == 1) and np.all(st == 0)
    against_oracle_and_emulation(f'cold {name} B={B}', A, h, E, r, SF.energies_d4(A, h))


@pytest.mark.parametrize('B', SHAPES)
def test_tensor_kernel_warm_on_stale_environments(B, engine_factory):
    """The resident environments belong to other tensors: the warm step rejects every evaluation and the warm instantiation's own build and
    solve follow (iterations 2); all four Hamiltonians as terms of one launch."""
    rng = np.random.default_rng(9700 + B)
    A0 = O.unitary_to_tensor(O.haar_unitaries(rng, 8, B))
    A = O.unitary_to_tensor(O.haar_unitaries(rng, 8, B))
    eng = engine_factory(4, 64)
    eng.set_solver('direct')
    E0, it0, st0 = eng.energies(A0, H_ALL)
    r0 = eng.environments()
    assert np.all(it0 == 1) and np.all(st0 == 0)
    eng.set_hamiltonian(H_ALL)
    eng.set_tensors(A)
    eng.set_env_guess(r0)
    eng.launch(B, solver='direct', store_env=True, warm_start=True)
    E, it, st = eng.results(B)
    r = eng.environments(B)
    assert np.all(it == 2) and np.all(st == 0)
    against_oracle_and_emulation(f'warm, stale environments B={B}', A, H_ALL, E, r, EMU.energies_d4(A, H_ALL))


@pytest.mark.parametrize('name', sorted(HAMILTONIANS))
@pytest.mark.parametrize('B', SHAPES)
def test_shallow_cnot_kernel_against_the_tensor_kernel(B, name, engine_factory):
    """The kernel that builds its tensors in LDS against the tensor kernel on host-built tensors of the same angles; the bound of
    tests/test_solve_order_gpu.py (the device's tensors are the host's to 1e-13, the solve amplifies that by at most 1 / gap)."""
    h = HAMILTONIANS[name][None]
    prm = np.random.default_rng(9800 + B).standard_normal((B, 4))
    A = np.stack([O.unitary_to_tensor(O.shallow_cnot_unitary(4, x)[None])[0] for x in prm])
    T = np.einsum('bsij,bskl->bikjl', A, A.conj()).reshape(B, 16, 16)
    w = np.sort(np.abs(np.linalg.eigvals(T)), axis=1)[:, ::-1]
    gap = (w[:, 0] - w[:, 1]).min()
    eng = engine_factory(4, 64)
    eng.set_solver('direct')
    eng.set_hamiltonian(h)
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, prm)
    eng.launch(B, solver='direct', store_env=True)
    E, it, st = eng.results(B)
    r = eng.environments(B)
    eng.set_tensors(A)
    eng.launch(B, solver='direct', store_env=True)
    Et, itt, stt = eng.results(B)
    rt = eng.environments(B)
    print(f'ShallowCNOT {name} B={B}: E {np.abs(E - Et).max():.2e}, r {np.abs(r - rt).max():.2e}, smallest gap {gap:.2e}')
    assert np.array_equal(it, itt) and np.array_equal(st, stt)
    tol = max(1e-11, 1e-13 / gap)
    assert np.abs(E - Et).max() < tol and np.abs(r - rt).max() < tol


def test_near_singular_slice_through_the_fall_back(engine_factory):
    """The ungauged rows of tests/conditioning_cases.py (the elimination meets a pivot below 1e-10: power fall-back, then update_sites takes
    the W of the final r) between gauged rows that are accepted in one step and keep the W of their own step - in one launch, so that waves
    hold both; its three terms (the last not Hermitian) against the mpmath reference with the bounds of CC.compare."""
    fam = CC.family(4)
    ungauged = np.flatnonzero(~fam['gauged'] & (fam['t'] > 0))
    gauged = np.flatnonzero(fam['gauged'])[::40]
    rows = np.sort(np.concatenate([ungauged, gauged]))
    h = CC.hamiltonian_terms()
    eng = engine_factory(4, 8192)
    eng.set_solver('direct', handoff=0)
    E, it, st = eng.energies(fam['A'][rows], h)
    out = {'E': E, 'iters': it, 'status': st, 'r': eng.environments(), 'rho': eng.rdm()}
    CC.compare(4, out, h, 'staged kernel, near-singular slice', rows=rows, one_step=True, rho_self=True)
    fell = np.isin(rows, ungauged)
    assert not np.any(st == 1) and np.all(it[~fell] == 1) and (it[fell] > 1).mean() > 0.5
