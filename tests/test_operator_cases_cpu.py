"""CPU: what the generic-operator GPU tests can see (tests/operator_cases.py).  With the oracle alone: on every input that
tests/test_generic_operator_gpu.py and the generic-term rotosolve tests use, each wrong operator - transposed, conjugated,
adjoint, sites exchanged - moves the compared quantity by at least 1e-6, 10^4 times the GPU tolerance of 1e-10, so a kernel
that applies one of them cannot pass.  Three exact symmetries are asserted as what they are, not as separations:
  * D = 2, `swap`: eta, the objective and the two-site energy are unchanged to rounding.  D = 2 cases say nothing about site
    order; D >= 4 carries that check.
  * candidate = reference (the start point of a time step), `dagger`: T_{W^+}(x) = T_W(x^+)^+, the spectrum is the complex
    conjugate and -sqrt|eta| is unchanged, and `transpose` = adjoint of `conj` moves it exactly as `conj` does.  The drivers are
    therefore also measured at a point displaced by 0.05 per angle - what a time step moves them by - where every variant
    separates; at the start point and at its central-difference neighbour the other variants do.
The smallest separations are printed (pytest -s) and recorded in profiles/EXPERIMENTS.md."""
import numpy as np
import pytest

import operator_cases as OP
from oracle import qmps_oracle as O

BAR = 1e-6
SYMMETRIC = 1e-13
VARIANTS = ('transpose', 'conj', 'dagger', 'swap')


def eta_of(A, B, WW, D):
    """dominant eigenvalue: the dense eigen-solve; at D = 16 the reference's own route, ARPACK in operator form (40 ms instead of
    400 - cross-checked against the dense solve in tests/test_oracle.py; both are good to 1e-12, the bar here is 1e-6)"""
    if D == 16:
        return O.overlap_eta_arpack(A, B, WW)[0]
    C = np.tensordot(WW, O.merge(A, A), [1, 0])
    w = np.linalg.eigvals(O.transfer_matrix(C, O.merge(B, B)))
    return w[np.argmax(np.abs(w))]


def separations(pairs, WW, D, value=lambda eta: eta):
    """min over the (A, B) pairs of |value(eta(variant)) - value(eta(WW))|, per variant"""
    base = [value(eta_of(A, B, WW, D)) for A, B in pairs]
    out = {}
    for name, V in OP.wrong_variants(WW).items():
        out[name] = min(abs(value(eta_of(A, B, V, D)) - b) for (A, B), b in zip(pairs, base))
    return out


def objective(eta):
    return -np.sqrt(abs(eta))


def report(what, D, sep):
    print(f'{what:34s} D = {D:2d}: ' + '  '.join(f'{k} {sep[k]:.2e}' for k in VARIANTS))


def check(what, D, sep, symmetric=()):
    report(what, D, sep)
    for name in VARIANTS:
        if name in symmetric:
            assert sep[name] < SYMMETRIC, (what, D, name, sep[name])
        else:
            assert sep[name] >= BAR, (what, D, name, sep[name])


@pytest.mark.parametrize('seed', sorted(set(s + k for s in OP.WW_SEED.values() for k in range(5))))
def test_operators_are_unitary_and_far_from_their_variants(seed):
    for dt in OP.DTS:
        WW = OP.generic_ww(seed, dt)
        assert np.abs(WW @ WW.conj().T - np.eye(4)).max() < 1e-14
        for name, V in OP.wrong_variants(WW).items():
            assert np.abs(V - WW).max() > 1e-2, (seed, dt, name)
    h = OP.generic_h(seed)
    assert np.abs(h - h.conj().T).max() == 0.0 and abs(np.linalg.norm(h, 2) - 1.0) < 1e-14


@pytest.mark.parametrize('D', [2, 4, 8, 16])
def test_plain_solve_cases_separate_every_variant(D):
    """eta of the plain solves (both dt), of the one-reference-per-candidate case, and the spectral gap of every candidate."""
    for dt in OP.DTS:
        A, cands, WW = OP.plain_case(D, dt)
        for c in cands:
            assert OP.spectral_ratio(A, c, WW) <= 0.95
        check(f'plain solves, dt = {dt}', D, separations([(A, c) for c in cands], WW, D), symmetric=('swap',) if D == 2 else ())
    ref, cand, WW = OP.refs_case(D)
    pairs = [(OP.tensor(D, p), OP.tensor(D, q)) for p, q in zip(ref, cand)]
    for a, b in pairs:
        assert OP.spectral_ratio(a, b, WW) <= 0.95
    check('one reference per candidate', D, separations(pairs, WW, D), symmetric=('swap',) if D == 2 else ())


@pytest.mark.parametrize('D', [8, 16])
def test_far_cases_separate_every_variant(D):
    """The Krylov fall-back's candidates (D = 16: every third, a dense 256 x 256 eigen-solve each - ARPACK is no reference for a
    crowded spectrum); at least one of them has a spectrum the power method needs > 1 000 steps for."""
    A, cands, WW = OP.far_case(D)
    cands = cands[::3] if D == 16 else cands
    check('Haar-far candidates', D, separations([(A, c) for c in cands], WW, 0))
    ratios = np.array([OP.spectrum(A, c, WW)[2] for c in cands])
    print(f'{"":34s}         |eta_2 / eta_1| {ratios.min():.4f} .. {ratios.max():.4f}')
    assert ratios.max() > 0.98 and ratios.max() < 1 - 1e-6


@pytest.mark.parametrize('D', [4, 8, 16])
def test_gradient_cases_separate_every_variant(D):
    ref, X, WW, _ = OP.gradient_case(D)
    pairs = [(OP.tensor(D, p), OP.tensor(D, q)) for p, q in zip(ref, X)]
    for a, b in pairs:
        assert OP.spectral_ratio(a, b, WW) <= 0.95
    check('gradient iterates, objective', D, separations(pairs, WW, D, objective))


@pytest.mark.parametrize('name', sorted(OP.DRIVER_CASES))
def test_driver_cases_separate_every_variant(name):
    """The objective at the start point, at one central-difference neighbour (h = 1e-6) and at a point a time step away."""
    D, X0, WW = OP.driver_case(name)
    h = np.zeros(X0.shape[1])
    h[1] = 1e-6
    moved = X0 + 0.05 * np.random.default_rng(99).choice([-1.0, 1.0], X0.shape)
    A = [OP.tensor(D, x) for x in X0]
    for a in A:
        assert OP.spectral_ratio(a, a, WW) <= 0.95
    swap = ('swap',) if D == 2 else ()
    for what, cand in (('start point', X0), ('central-difference neighbour', X0 + h)):
        sep = separations([(a, OP.tensor(D, x)) for a, x in zip(A, cand)], WW, D, objective)
        report(f'{name}, {what}', D, sep)
        assert sep['transpose'] >= BAR and sep['conj'] >= BAR and (D == 2 or sep['swap'] >= BAR)
        if D == 2:
            assert sep['swap'] < SYMMETRIC
        if what == 'start point':
            assert sep['dagger'] < SYMMETRIC           # the spectrum of T_{W^+} is the complex conjugate of T_W's when B = A
    check(f'{name}, a time step away', D, separations([(a, OP.tensor(D, x)) for a, x in zip(A, moved)], WW, D, objective), symmetric=swap)


@pytest.mark.parametrize('D,R', [(2, 16), (8, 176)])
def test_rotosolve_hamiltonian_is_not_symmetric_for_the_energy(D, R, c_oracle):
    """Re tr(h rho) of the whole-run rotosolve tests' start vectors under h -> h^T and h -> S h S, for the generic term (C oracle)."""
    g = OP.generic_h(OP.ROTO_H_SEED[D])
    for kind, P in OP.ROTO_RUNS[D]:
        A = np.stack([O.unitary_to_tensor(OP.ROTO_BUILDERS[kind](D, p)) for p in OP.roto_start(D, kind, P, R)])
        out = c_oracle.energy_batch(A, np.stack([g, g.T, OP.SWAP @ g @ OP.SWAP]), tol=1e-14, max_iter=200000)
        e = out['E'][out['status'] == 0]
        assert len(e) >= R - 2
        sep = {'transpose': np.abs(e[:, 1] - e[:, 0]).min(), 'swap': np.abs(e[:, 2] - e[:, 0]).min()}
        print(f'rotosolve start vectors, kind {kind} P {P:2d}   D = {D:2d}: transpose {sep["transpose"]:.2e}  swap {sep["swap"]:.2e}')
        assert sep['transpose'] >= BAR
        assert sep['swap'] < SYMMETRIC if D == 2 else sep['swap'] >= BAR
