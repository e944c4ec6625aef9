"""GPU: the D = 4 gradient paths at iterates whose mixed transfer map has TIED dominant eigenvalues (QMPS_STATUS_TIED: non-injective states of
the ShallowCNOT ansatz on the grid of multiples of pi / 4 carry 1, 1, -1, -1).  Such a map has no fixed points, so the second-order expansion
eta' = <y, T'(r)> / <y, r> of qmps_overlap_gradient has nothing to stand on and the two-sided quotient <y, T(r)> / <y, r> is not the objective either.
Checked here: qmps_overlap_gradient keeps the solve's own objective (the common modulus, Gelfand) and returns a NaN gradient for such rows without
disturbing the generic rows of the same batch; the numpy lock-step loop and the host C driver eigen-solve the 2 P neighbours of a tied iterate
instead; both host drivers follow the special grid as the device-resident driver does (test_evolve_gpu.py).
Reference: tests/evolve_replay.objective_gelfand (-sqrt(spectral radius) by Gelfand's formula, good to ~1e-13 where numpy's eigvals is not)."""
import numpy as np
import pytest
from scipy.linalg import expm

import evolve_replay as ER
from oracle import qmps_oracle as O
from qmps_amd import _lib as L
from qmps_amd import new_time_evolve as NT

pytestmark = pytest.mark.gpu

H_TFIM = O.hamiltonian_matrix({'ZZ': -1.0, 'X': 1.0})
KIND, P, H = L.ANSATZ_SHALLOW_CNOT, 4, 1e-6
# the starts of test_evolve_gpu.py::test_d4_device_driver_leaves_a_tied_start_as_scipy_does and the points of
# test_overlap_gpu.py::test_tied_dominant_eigenvalues_at_d4_return_the_common_modulus (units of pi / 4)
GRID = np.array([[2, -4, 0, 4], [2, 4, 0, -2], [-2, -4, 0, 2], [-4, 0, 2, 2], [4, 2, -4, 2]])
TIED = {0.0: GRID[[2]], 0.05: GRID, 0.3: GRID}


def WW_of(dt):
    return expm(-1j * dt * H_TFIM)


def mixed_batch(dt, seed):
    """References and iterates: the tied points of dt (iterate = reference) interleaved with generic iterates near their own references."""
    rng = np.random.default_rng(seed)
    tied = TIED[dt] * (np.pi / 4)
    gref = rng.standard_normal((5, P))
    gx = gref + 0.03 * rng.standard_normal((5, P))
    ref = np.concatenate([tied, gref])
    X = np.concatenate([tied, gx])
    is_tied = np.arange(len(ref)) < len(tied)
    order = rng.permutation(len(ref))
    return ref[order], X[order], is_tied[order]


def cd(fun, x):
    """Central differences with the drivers' step h."""
    out = np.empty(P)
    for k in range(P):
        e = np.zeros(P)
        e[k] = H
        out[k] = (fun(x + e) - fun(x - e)) / (2 * H)
    return out


def references(dt, ref, X, is_tied, WW):
    """(f, g) of every row: Gelfand's formula at the tied rows, the dense eigen-solve at the generic ones."""
    f, g = np.empty(len(X)), np.empty((len(X), P))
    for t in range(len(X)):
        A = ER.tensor(KIND, 4, ref[t])
        obj = (lambda x: ER.objective_gelfand(KIND, 4, A, x, WW)) if is_tied[t] else (lambda x: ER.objective(KIND, 4, A, x, WW))
        f[t], g[t] = obj(X[t]), cd(obj, X[t])
    return f, g


@pytest.mark.parametrize('dt', [0.0, 0.05, 0.3])
def test_overlap_gradient_at_tied_iterates_keeps_the_objective_and_withholds_the_gradient(dt, engine_factory):
    """qmps_overlap_gradient on ONE batch of tied and generic iterates, with and without QMPS_OVERLAP_TWO_SIDED_F: a tied row reports
    QMPS_STATUS_TIED, its objective is the common modulus (not the two-sided quotient of the mixtures the solve ends with) and its gradient
    is NaN - there are no fixed points to expand round; the generic rows are what test_evolve_gpu.py's two-sided gradient test asks of them.
    A budget too short to call a tie (20 squarings) reports QMPS_STATUS_NOT_CONVERGED."""
    WW = WW_of(dt)
    ref, X, is_tied = mixed_batch(dt, 90 + int(100 * dt))
    f_ref, g_ref = references(dt, ref, X, is_tied, WW)
    eng = engine_factory(4, 4096)
    eng.overlap_set_refs_params(KIND, ref, WW)
    for two_sided_f in (False, True):
        f, g, st = eng.overlap_gradient(KIND, X, h=H, tol=1e-13, two_sided_f=two_sided_f)
        assert np.all(st[is_tied] == L.STATUS_TIED) and np.all(st[~is_tied] == 0), (two_sided_f, st)
        err_t = np.abs(f - f_ref)[is_tied].max()
        assert err_t < 1e-12, (two_sided_f, err_t, f[is_tied], f_ref[is_tied])
        assert np.isnan(g[is_tied]).all(), (two_sided_f, g[is_tied])
        assert np.abs(f - f_ref)[~is_tied].max() < 1e-10, two_sided_f
        assert np.abs(g - g_ref)[~is_tied].max() < 2e-7, (two_sided_f, np.abs(g - g_ref)[~is_tied].max())
    _, _, st = eng.overlap_gradient(KIND, X, h=H, max_rounds=20, tol=1e-13)
    assert np.all(st[is_tied] == L.STATUS_NOT_CONVERGED) and np.all(st[~is_tied] == 0), st


@pytest.mark.parametrize('dt', [0.0, 0.05, 0.3])
def test_numpy_loop_value_and_grad_eigen_solves_the_neighbours_of_tied_iterates(dt):
    """The numpy lock-step loop (LockstepEvolver(native=False)): at a tied iterate its gradient comes from the 2 P neighbours eigen-solved one by
    one - the central difference of the objective itself, compared with the central difference of Gelfand's formula (the objective has a kink at a
    tie: a slope from an expansion would not do).  1e-6 = the 1e-12 accuracy of the objective over h."""
    WW = WW_of(dt)
    ref, X, is_tied = mixed_batch(dt, 190 + int(100 * dt))
    f_ref, g_ref = references(dt, ref, X, is_tied, WW)
    fg = NT._GroupedObjective(4, KIND, len(X), 2 * P + 1, 60, 1e-13)
    try:
        fg.tight_gradient = False                 # (LockstepEvolver's default: the objective from the two-sided quotient)
        fg.set_reference(ref, WW)
        f, g = fg.value_and_grad(X, H)
    finally:
        fg.close()
    assert np.isfinite(f).all() and np.isfinite(g).all(), (f, g)
    assert np.abs(f - f_ref)[is_tied].max() < 1e-12, (f[is_tied], f_ref[is_tied])
    assert np.abs(g - g_ref)[is_tied].max() < 1e-6, (np.abs(g - g_ref)[is_tied].max(), g[is_tied], g_ref[is_tied])
    assert np.abs(f - f_ref)[~is_tied].max() < 1e-10
    assert np.abs(g - g_ref)[~is_tied].max() < 2e-7


@pytest.mark.parametrize('driver', ['host', 'numpy'])
def test_d4_host_drivers_on_the_special_grid_against_gelfand(driver, engine_factory):
    """The D = 4 companion of test_evolve_gpu.py::test_device_drivers_on_the_special_grid_against_gelfand for the host C driver (qmps_evolve_bfgs)
    and the numpy lock-step loop: the same 120 grid starts per case, dt in {0, 0.05, 0.3}, maxiter 4, two time steps.  Every recorded point - the
    start and the end of each step - is finite and within 1e-9 of Gelfand's formula."""
    rng = np.random.default_rng(606 + 4)            # (the device test's seed and draws: the same starts)
    cases = ((L.ANSATZ_SHALLOW_CNOT, 4), (L.ANSATZ_SHALLOW_CNOT, 8))
    for dt in (0.0, 0.05, 0.3):
        WW = WW_of(dt)
        for kind, Pk in cases:
            X0 = np.concatenate([rng.integers(-4, 5, (60, Pk)) * (np.pi / 4), rng.integers(-2, 3, (60, Pk)) * (np.pi / 2)])
            T, n_steps = len(X0), 2
            if driver == 'host':
                eng = engine_factory(4, max(4096, T * (2 * Pk + 1 + 8)))
                res = eng.evolve_bfgs(kind, X0, WW, n_steps=n_steps, maxiter=4, tol=1e-13)
                fs, fe, ph = res['fun_start'], res['fun'], res['params_hist']
            else:
                ev = NT.LockstepEvolver(4, T, Pk, None, None, 1e-13, maxiter=4, native=False, speculative=True)
                fs, fe, ph = np.empty((n_steps, T)), np.empty((n_steps, T)), np.empty((n_steps, T, Pk))
                try:
                    X = X0
                    for step in range(n_steps):
                        r = ev.step(X, WW)
                        fs[step], fe[step], ph[step] = r['history'][0], r['fun'], r['x']
                        X = r['x']
                finally:
                    ev.close()
            prev = X0
            worst = 0.0
            for step in range(n_steps):
                assert np.isfinite(fe[step]).all() and np.isfinite(fs[step]).all(), (driver, dt, kind, Pk, step)
                for t in range(T):
                    A = ER.tensor(kind, 4, prev[t])
                    worst = max(worst, abs(ER.objective_gelfand(kind, 4, A, prev[t], WW) - fs[step, t]),
                                abs(ER.objective_gelfand(kind, 4, A, ph[step, t], WW) - fe[step, t]))
                prev = ph[step]
            assert worst < 1e-9, (driver, dt, kind, Pk, worst)
