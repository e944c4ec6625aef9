"""GPU: the D = 4 energy kernels compute only the parts of the two-site density matrix that the resident Hamiltonian reads (the mask
qmps_set_hamiltonian derives from h; qmps_direct_core.h).  Energies of every Hamiltonian of tests/rho_need_cases.py against the full
density matrices of the same engine and against the oracle; the mask follows the Hamiltonian from launch to launch and never reaches a
launch that returns rho; the ansatz, warm-start and resident-environment kernels against launches whose Hamiltonian sets every bit.
B = 37: two full tiles of 16 evaluations and a partial one; B = 1."""
import numpy as np
import pytest

from oracle import qmps_oracle as O
from qmps_amd import EnergyEngine, _lib
from tests import rho_need_cases as RN

pytestmark = pytest.mark.gpu

E_TOL = 1e-10          # tests/test_energy_gpu.py: energies against the oracle
# A launch whose Hamiltonian has 1e-300 (1 + i) added to every entry computes every part of rho and moves no energy by more than 1e-298:
# what is left between it and the masked launch is +-0.0 added to the same sums
TWIN_TOL = 1e-14
SHAPES = [37, 1]


def tensors(B):
    return O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(4100 + B), 8, B))


def rho_tol(h):
    """E against Re sum h[s][t] rho[t][s] in numpy: the same <= 28 products summed in another order (2 x 28 eps sum |h| |rho|, |rho| <= 1),
    from a rho the energy-only kernel forms after normalising the stored r once more (a few eps): 1e-13 per unit of sum |h|."""
    return 1e-13 * max(1.0, float(np.abs(h).sum()))


@pytest.mark.parametrize('B', SHAPES)
def test_energies_of_every_hamiltonian(B, c_oracle, engine_factory):
    eng = engine_factory(4, 64)
    A = tensors(B)
    for name, h in dict(RN.table(), three_terms=RN.THREE_TERMS).items():
        h = np.asarray(h).reshape(-1, 4, 4)
        E, it, st = eng.energies(A, h)
        rho = eng.rdm()                       # the rho route: every part computed
        Ef, itf, stf = eng.energies(A, RN.full_mask_twin(h))
        assert np.array_equal(it, itf) and np.array_equal(st, stf), name
        assert np.all(st == 0) and np.all(it == 1), name
        if np.isnan(h).any():
            assert np.isnan(E).all() and np.isnan(Ef).all(), name
            continue
        from_rho = np.real(np.einsum('nst,bts->bn', h, rho))
        print(f'{name} B={B}: |E - E(rho)| {np.abs(E - from_rho).max():.2e} (tol {rho_tol(h):.1e}), |E - E(full mask)| {np.abs(E - Ef).max():.2e}')
        assert np.abs(E - from_rho).max() < rho_tol(h), name
        assert np.abs(E - Ef).max() <= TWIN_TOL, name
        ref = c_oracle.energy_batch(A, h)
        assert np.all(ref['status'] == 0) and np.abs(E - np.asarray(ref['E']).reshape(E.shape)).max() < E_TOL, name


def fresh(A, h):
    with EnergyEngine(4, 64) as eng:
        return eng.energies(A, h)


def test_the_mask_follows_the_hamiltonian():
    A = tensors(37)
    want = {k: fresh(A, h) for k, h in (('tfim', RN.TFIM), ('complex', RN.COMPLEX_HERMITIAN), ('three', RN.THREE_TERMS))}
    with EnergyEngine(4, 64) as eng:
        for k, h in (('tfim', RN.TFIM), ('complex', RN.COMPLEX_HERMITIAN), ('tfim', RN.TFIM), ('three', RN.THREE_TERMS), ('tfim', RN.TFIM)):
            got = eng.energies(A, h)
            for a, b in zip(got, want[k]):
                assert np.array_equal(a, b), k
        # rho right after a masked launch: the mask stays out of it
        rho = eng.rdm()
        assert np.abs(rho - rho.conj().transpose(0, 2, 1)).max() < 1e-13
        assert np.abs(np.trace(rho, axis1=1, axis2=2) - 1).max() < 1e-13
        assert np.abs(rho.imag).max() > 1e-3 and np.abs(rho[:, 0, 3]).max() > 1e-3      # the parts TFIM does not read are there
        # and the launch after it is masked again
        for a, b in zip(eng.energies(A, RN.TFIM), want['tfim']):
            assert np.array_equal(a, b)


@pytest.mark.parametrize('B', SHAPES)
def test_ansatz_warm_start_and_resident_environment_kernels(B, engine_factory):
    """The kernels beside the benchmark's: tensors built from ansatz parameters, the warm start, and the energy pass over resident
    environments with its positive-definiteness test (the plain power iteration's second kernel).  h: the real part of the complex
    Hermitian case - masked - against its twin that sets every bit."""
    eng = engine_factory(4, 64)
    h = RN.COMPLEX_HERMITIAN.real.astype(complex)
    assert RN.mask(h) == RN.mask(RN.TFIM) and RN.mask(RN.full_mask_twin(h)) == 0x08CE8CEF      # every part of the upper triangle
    A = tensors(B)
    prm = np.random.default_rng(4200 + B).standard_normal((B, 4))

    def runs(hh):
        out = {}
        eng.set_hamiltonian(hh)
        eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, prm)
        eng.launch(B)
        out['ansatz'] = eng.results(B)
        eng.set_tensors(A)
        eng.set_env_guess(None)
        eng.launch(B)
        eng.launch(B, warm_start=True)
        out['warm'] = eng.results(B)
        eng.launch(B, solver='plain', max_iter=4000)
        out['resident'] = eng.results(B)
        return out

    masked, full = runs(h), runs(RN.full_mask_twin(h))
    for k in masked:
        (E, it, st), (Ef, itf, stf) = masked[k], full[k]
        print(f'{k} B={B}: |E - E(full mask)| {np.abs(E - Ef).max():.2e}, status 0: {(st == 0).mean():.2f}')
        assert np.array_equal(it, itf) and np.array_equal(st, stf), k
        assert (st == 0).mean() > 0.9 or B == 1, k
        assert np.abs(E - Ef).max() <= TWIN_TOL, k
    assert np.all(masked['warm'][1] == 1) and np.all(masked['resident'][1] > 1)


@pytest.mark.parametrize('double', [False, True])
def test_the_cached_rotosolve_sweep_follows_the_hamiltonian(double):
    """The rotosolve drivers capture one sweep into a graph and keep it between calls of the same shape; the captured energy launches
    carry the mask in their arguments.  TFIM, then XXZ (it reads Re rho[1][2], which TFIM does not), then the complex Hermitian case,
    then TFIM again on ONE engine with the same shapes: every run bit for bit what a fresh engine gives.  12 restarts x 3 (6) shifts:
    more than one tile of 16 evaluations."""
    prm = np.random.default_rng(4300).standard_normal((12, 4))

    def run(eng, h):
        eng.set_hamiltonian(h)
        return (eng.double_rotosolve if double else eng.rotosolve)(_lib.ANSATZ_SHALLOW_CNOT, prm, 2)

    hams = {'tfim': RN.TFIM, 'xxz': RN.XXZ, 'complex': RN.COMPLEX_HERMITIAN}
    want = {}
    for k, h in hams.items():
        with EnergyEngine(4, 128) as eng:
            want[k] = run(eng, h)
    assert not np.array_equal(want['tfim'][0], want['xxz'][0])
    with EnergyEngine(4, 128) as eng:
        for k in ('tfim', 'xxz', 'complex', 'tfim'):
            hist, p = run(eng, hams[k])
            assert np.array_equal(hist, want[k][0]) and np.array_equal(p, want[k][1]), k
