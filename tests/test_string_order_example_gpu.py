"""GPU: examples/string_order.py end to end - the disorder parameter, the string correlators and the Jordan-Wigner fermion function it
returns against the float64 reference of the tensors it made resident, and the fermion function against explicit Jordan-Wigner
operators on the oracle's state vectors (which settles the sign of the site-0 factor)."""
import importlib.util
import os

import numpy as np
import pytest

import correlator_cases as K
import string_correlator_cases as SC
from oracle import qmps_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAX = 8


@pytest.fixture(scope='module')
def example():
    spec = importlib.util.spec_from_file_location('example_string_order', os.path.join(ROOT, 'examples', 'string_order.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def run(example):
    return example.main(['--couplings', '0.5', '0.8', '1.25', '2.0', '--restarts', '4', '--D', '2', '--n-max', str(N_MAX)])


def test_example_against_the_reference_of_its_tensors(example, run):
    out = run
    assert out['C'].shape == (4, 2, 2, N_MAX) and out['one'].shape == (4, 2) and out['str'].shape == (4, N_MAX)
    assert out['fermion'].shape == (4, N_MAX) and out['zz'].shape == (4, N_MAX) and out['status'].shape == (4,)
    assert np.all(out['status'] == 0)
    A = np.stack([O.unitary_to_tensor(O.shallow_cnot_unitary(2, p)) for p in out['params']])
    r = np.stack([O.env_dense_eig(a)[1] for a in A])
    Cr, oner, strr = SC.reference(A, r, out['ops'], K.X, N_MAX, dtype=np.complex128)
    Cz, _ = K.reference(A, r, K.Z, N_MAX, dtype=np.complex128)
    assert np.abs(out['C'] - Cr).max() < 1e-10 and np.abs(out['one'] - oner).max() < 1e-10 and np.abs(out['str'] - strr).max() < 1e-10
    assert np.abs(out['fermion'] - Cr[:, 0, 1, :]).max() < 1e-10 and np.abs(out['zz'] - Cz[:, 0, 0, :].real).max() < 1e-10
    exact = example.exact_disorder(out['couplings'])
    assert np.array_equal(exact[:2], [0.0, 0.0]) and abs(exact[3] - 0.75 ** 0.25) < 1e-15 and np.array_equal(out['disorder_exact'], exact)
    # printed, not asserted: how close the D = 2 ansatz gets to the exact disorder parameter
    for k, lam in enumerate(out['couplings']):
        print(f'lambda {lam}: <X_1 .. X_{N_MAX}> = {out["str"][k, -1].real:+.6f}, exact at n -> inf {exact[k]:.6f}')


def test_fermion_function_against_explicit_jordan_wigner_operators(run):
    """c_j = (prod_(l<j) X_l) (Z_j - iY_j) / 2 as matrices on the n + 1 physical sites of oracle.state_vector, n <= 4: <c^+_0 c_n>."""
    out = run
    down = (K.Z - 1j * K.Y) / 2
    for k, p in enumerate(out['params']):
        U = O.shallow_cnot_unitary(2, p)
        V = O.get_env_exact(U)
        for n in range(1, 5):
            psi = O.state_vector(U, V, n + 1)
            c0 = K.site_operator(2, n + 1, {0: down})
            cn = K.site_operator(2, n + 1, {**{l: K.X for l in range(n)}, n: down})
            want = psi.conj() @ (c0.conj().T @ (cn @ psi))
            assert abs(out['fermion'][k, n - 1] - want) < 1e-10, (k, n, out['fermion'][k, n - 1], want)
