"""E, r and rho as the transfer gap closes: every solver, D = 2 .. 16 (GPU, through EnergyEngine).

tests/test_conditioning_gpu.py covers near-singular environments at transfer gaps above 0.08.  Here the rows are the families of
tests/gap_cases.py - second eigenvalue of the transfer map at 1 - gap times +1 (`slow`), -1 (`flip`) or the triple -1, +i, -i
(`cycle4`), gap from ~1e-2 down to ~1e-9, Haar rows mixed in, one fixed shuffle - and every comparison is against the mpmath reference:

    direct solves     every row status 0 in one step, E, r and rho within the direct bound C 2^-52 kappa
    iterative solves  the status follows from the reference spectrum (n* = ln tol / ln|lambda_2| power steps against max_iter; a gap of
                      3e-6 or more where a Krylov hand-over is armed), every status-0 row within (tol + C 2^-52) max(kappa, 1 / gap)

A premature "converged" on a flip or cycle4 row - perfectly conditioned fixed point, slowest possible iteration - is a wrong energy
with status 0: it leaves the iterative bound by orders of magnitude.  Every test prints its worst figures as fractions of its bound;
the figures measured on one MI355X are in the docstrings and in profiles/EXPERIMENTS.md."""
import numpy as np
import pytest

from oracle import qmps_oracle as O
from tests import conditioning_cases as CC
from tests import gap_cases as G

pytestmark = pytest.mark.gpu

TOL = 1e-13
KEYS = ('E', 'r', 'rho', 'iters', 'status')
CAPACITY = {2: 4096, 4: 8192, 8: 4096, 16: 4096}        # the engines tests/test_conditioning_gpu.py already holds
SWITCHES = ('QMPS_POWER_LANE', 'QMPS_D16_BLOCK', 'QMPS_NO_KRYLOV')


def solve(eng, A, h, solver, monkeypatch, max_iter=10000, krylov=None, switch=None, store_env=True):
    """One batch through the engine: the one-shot call with `solver` selected (krylov None), or the stepping entry point with the
    Krylov hand-over on request (D = 8).  switch: one of SWITCHES, set for the call only.  The engine is left on its default solver."""
    default = 'squaring' if eng.D == 16 else 'direct'
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    try:
        if switch is not None:
            monkeypatch.setenv(switch, '1')
        if krylov is None and store_env:
            eng.set_solver(solver, handoff=0)
            E, it, st = eng.energies(A, h, max_iter=max_iter, tol=TOL)
        else:
            eng.set_tensors(A)
            eng.set_hamiltonian(h)
            eng.launch(len(A), max_iter=max_iter, tol=TOL, solver=solver, store_env=store_env, krylov_fallback=bool(krylov))
            E, it, st = eng.results(len(A))
        out = {'E': E.copy(), 'iters': it.copy(), 'status': st.copy()}
        if store_env:
            out.update(r=eng.environments().copy(), rho=eng.rdm().copy(), cost=eng.summed_cost().copy())
    finally:
        if switch is not None:
            monkeypatch.delenv(switch, raising=False)
        eng.set_solver(default, handoff=0)
    return out


def differing(a, b, keys=KEYS):
    return [k for k in keys if not np.array_equal(a[k], b[k])]


def check_iterative(D, out, label, max_iter, krylov=False, compared='three quarters', at_cap=False):
    """The assertions every iterative leg shares: no status but 0 and 1 (lam_min > 1e-3 on every row); the status rule; every status-0 row
    within the iterative bound on E, r and rho; at_cap: status-1 rows report max_iter iterations.  The condition on the test itself,
    `compared`: 'three quarters' of the rows end with status 0; 'rule': every row the rule demands, some in every family the budget reaches
    at all; 'every family': the same and the budget reaches every family.  Prints the figures first.  Returns the mask of compared rows."""
    fam, ref = G.family(D), G.references(D)
    st, it = out['status'], out['iters']
    must = G.must_converge(D, TOL, max_iter, krylov=krylov)
    done = st == 0
    bound = G.iterative_bound(D, TOL)
    fig = G.worst_fraction(D, out, bound, use=done)
    G.show(f'gap D={D} {label}: as a fraction of the iterative bound', fig)
    names = G.families(D) + ('haar',)
    print(f'gap D={D} {label}: status 0 / 1 / other {int(done.sum())} / {int((st == 1).sum())} / {int((st > 1).sum())} of {len(st)}; '
          f'rows that must converge {int(must.sum())} (' + ', '.join(f'{n} {int((must & (fam["family"] == n)).sum())}' for n in names) + '); '
          f'compared per family ' + ', '.join(f'{n} {int((done & (fam["family"] == n)).sum())}' for n in names) +
          f'; iterations max {it.max()}, of status-0 rows {it[done].max() if done.any() else 0}')
    well = done & np.isin(fam['family'], ('flip', 'cycle4'))
    if well.any():
        dr, drho, dE = G.errors(D, out)
        b = np.flatnonzero(well)[np.argmax(dr[well])]
        print(f'gap D={D} {label}: flip / cycle4 rows of status 0, error in units of tol: r {dr[well].max() / TOL:.2f} rho {drho[well].max() / TOL:.2f} '
              f'E {(dE[well] / G.h_norms()).max() / TOL:.2f} (worst r: row {b}, {fam["family"][b]}, gap {ref["gap"][b]:.1e}, kappa {ref["kappa"][b]:.1f}, {it[b]} iterations)')
    wrong = np.flatnonzero(must & ~done)
    assert np.all((st == 0) | (st == 1)), (label, 'a status other than 0 / 1', np.flatnonzero(st > 1)[:8], ref['lam_min'][st > 1][:8])
    assert len(wrong) == 0, (label, 'status 1 where the rule demands 0', wrong[:8], fam['family'][wrong][:8], ref['gap'][wrong][:8], it[wrong][:8])
    assert max(max(v) for v in fig.values()) < 1.0, (label, fig)
    if at_cap:
        assert np.all(it[st == 1] == max_iter), (label, it[st == 1][:8])
    if compared == 'three quarters':
        assert done.sum() >= 0.75 * len(st), (label, int(done.sum()), len(st))
    else:
        for n in names:
            m = fam['family'] == n
            assert (must & m).sum() > 0 or (compared == 'rule' and n != 'haar'), (label, n, 'the budget reaches no row of this family')
            assert (done & m).sum() >= (must & m).sum(), (label, n)
    assert np.abs(out['cost'] - out['E'].sum(0)).max() < 1e-12 * len(st), label
    return done


# ---------------------------------------------------------------------------------------------------------------- direct solves
_DIRECT = {}


@pytest.fixture
def direct(engine_factory, monkeypatch):
    def get(D):
        if D not in _DIRECT:
            _DIRECT[D] = solve(engine_factory(D, CAPACITY[D]), G.family(D)['A'], CC.hamiltonian_terms(), 'direct', monkeypatch)
        return _DIRECT[D]
    return get


@pytest.mark.parametrize('D', [2, 4, 8])
def test_direct_solvers(D, direct, engine_factory, monkeypatch):
    """QMPS_ENV_DIRECT on every family (D = 2: the 4 x 4 solve in the lane; D = 4: the fused kernel; D = 8: the wave-per-evaluation
    solve behind the block kernel): every row status 0 with iterations 1 - the acceptance test is the solve's own residual -, E, r and
    rho within the direct bound, rho within 1e-13 of two_site_rdm of the kernel's own r, summed_cost = E.sum(0); at D = 4 the launch
    that stores no environments returns the same bits.
    Measured on one MI355X, r / rho / E as fractions of the direct bound (rho against its own r in brackets):
      D = 2  slow 0.088 / 0.069 / 0.028, flip 0.688 / 0.125 / 0.083, Haar 0.594 / 0.097 / 0.109 (3.4e-16)
      D = 4  slow 0.078 / 0.063 / 0.047, flip 0.125 / 0.219 / 0.146, cycle4 0.195 / 0.281 / 0.146, Haar 0.062 / 0.188 / 0.060 (1.3e-15)
      D = 8  slow 0.029 / 0.027 / 0.020, flip 0.086 / 0.023 / 0.030, cycle4 0.072 / 0.031 / 0.021, Haar 0.029 / 0.020 / 0.012 (4.4e-16)
    every row status 0 in one step; the launch without the environment store: the same bits."""
    fam = G.family(D)
    out = direct(D)
    fig = G.worst_fraction(D, out, G.direct_bound(D))
    G.show(f'gap D={D} direct: as a fraction of the direct bound', fig)
    rho_self = max(float(np.abs(rho - O.two_site_rdm(a, r)).max()) for a, r, rho in zip(fam['A'], out['r'], out['rho']))
    print(f'gap D={D} direct: statuses {sorted(set(out["status"]))}, iterations {sorted(set(out["iters"]))}, rho against two_site_rdm of its own r {rho_self:.2e}')
    assert np.all(out['status'] == 0) and np.all(out['iters'] == 1)
    assert max(max(v) for v in fig.values()) < 1.0, fig
    assert rho_self < 1e-13
    assert np.abs(out['cost'] - out['E'].sum(0)).max() < 1e-12 * len(fam['A'])
    if D == 4:
        lean = solve(engine_factory(4, CAPACITY[4]), fam['A'], CC.hamiltonian_terms(), 'direct', monkeypatch, store_env=False)
        assert differing(out, lean, ('E', 'iters', 'status')) == []


@pytest.mark.parametrize('D', [2, 4, 8])
def test_direct_results_do_not_depend_on_wave_mates(D, direct, engine_factory, monkeypatch):
    """The same rows under a second permutation, and 16 rows - the smallest gaps of every family and Haar rows - as batches of one:
    E, r, rho, iterations and status bit for bit what the shuffled batch gave - no result may depend on the evaluations that share its quad,
    wave or workgroup.  Measured on one MI355X: identical throughout at D = 2, 4 and 8."""
    fam, ref = G.family(D), G.references(D)
    out, h = direct(D), CC.hamiltonian_terms()
    eng = engine_factory(D, CAPACITY[D])
    p2 = np.random.default_rng(7400 + D).permutation(len(fam['A']))
    second = solve(eng, np.ascontiguousarray(fam['A'][p2]), h, 'direct', monkeypatch)
    assert differing({k: out[k][p2] for k in KEYS}, second) == []
    names = G.families(D) + ('haar',)
    chosen = []
    for n in names:
        idx = np.flatnonzero(fam['family'] == n)
        chosen += list(idx[np.argsort(ref['gap'][idx])][:16 // len(names)])
    chosen += [b for b in range(len(fam['A'])) if b not in chosen][:16 - len(chosen)]
    assert len(set(chosen)) == 16
    for b in chosen:
        alone = solve(eng, fam['A'][b:b + 1], h, 'direct', monkeypatch)
        assert differing({k: out[k][b:b + 1] for k in KEYS}, alone) == [], b


# ---------------------------------------------------------------------------------------------------------------- iterative solves
@pytest.mark.parametrize('D', [2, 4])
def test_squaring(D, engine_factory, monkeypatch):
    """QMPS_ENV_POWER_SQUARING from the start (hand-off 0) with max_iter = 2^30: the status rule (a gap above ~1.1e-7 must converge), every
    status-0 row within the iterative bound, at least three quarters of the rows compared; for the flip and cycle4 rows the error in units
    of tol - what the compare-two-powers test lets through.
    Measured on one MI355X, r / rho / E as fractions of the iterative bound, status 0 : 1:
      D = 2  slow 0.336 / 0.195 / 0.203, flip and Haar <= 0.001; 93 : 20 (90 rows must converge); flip rows 361 / 286 / 65 tol at worst
             (gap 2.0e-7, kappa 1.3, 2^29 steps)
      D = 4  slow 0.002 / 0.001 / 0.001, flip and cycle4 < 0.0005, Haar 0.002; 125 : 36 (113 must); flip and cycle4 rows 541 / 395 / 361 tol
             at worst (cycle4, gap 9.1e-8, kappa 2.4, 4.0e8 steps)
    so on a perfectly conditioned fixed point behind a gap of ~1e-7 the squaring solvers return 4 - 5e-11 with status 0: the rounding of
    ~29 squarings, not the stopping test (on the CPU restatement the iterate of the round before the accepted one is as close)."""
    out = solve(engine_factory(D, CAPACITY[D]), G.family(D)['A'], CC.hamiltonian_terms(), 'squaring', monkeypatch, max_iter=2 ** 30)
    check_iterative(D, out, 'squaring', 2 ** 30)


_PLAIN = {}


def plain(engine_factory, monkeypatch, D, route):
    if (D, route) not in _PLAIN:
        switch = 'QMPS_POWER_LANE' if (D, route) == (4, 'lane') else None
        _PLAIN[D, route] = solve(engine_factory(D, CAPACITY[D]), G.family(D)['A'], CC.hamiltonian_terms(), 'plain', monkeypatch, max_iter=20000,
                                 switch=switch)
    return _PLAIN[D, route]


@pytest.mark.parametrize('D,route', [(4, 'quad'), (4, 'lane'), (2, 'lane')])
def test_plain_power(D, route, engine_factory, monkeypatch):
    """QMPS_ENV_POWER with max_iter = 20 000 (D = 4: env_power_d4_kernel, and the lane kernel under QMPS_POWER_LANE; D = 2: the lane kernel):
    the status rule - n* <= 5 000, a gap above ~6e-3, must converge -, status-0 rows within the iterative bound, status-1 rows with
    iterations = max_iter, rows that must converge compared in every family.
    Measured on one MI355X, r / rho / E as fractions of the iterative bound, status 0 : 1 (rows that must converge):
      D = 4 quad  slow 0.461 / 0.503 / 0.399, flip 0.009 / 0.007 / 0.003, cycle4 0.004 / 0.004 / 0.002, Haar 0.250 / 0.139 / 0.162; 47 : 114 (34)
      D = 4 lane  the same (the same environments; the energies come from another kernel: Haar E 0.161); 47 : 114
      D = 2       slow 0.653 / 0.456 / 0.363, flip 0.025 / 0.014 / 0.005, Haar 0.573 / 0.210 / 0.204; 38 : 75 (30)
    flip and cycle4 rows of status 0: 0.37 tol at worst - the plain test lets nothing through."""
    check_iterative(D, plain(engine_factory, monkeypatch, D, route), f'plain ({route})', 20000, compared='every family', at_cap=True)


def test_plain_power_d4_routes_agree(engine_factory, monkeypatch):
    """The two D = 4 routes of QMPS_ENV_POWER - env_power_d4_kernel and the lane kernel of QMPS_POWER_LANE - give identical iteration counts
    and statuses on every row (include/qmps_hip.h, QMPS_POWER_LANE: "same iterates, same iteration counts and statuses"), and the same
    environments bit for bit.  Where the residual falls by a factor 1 - gap per step, the step at which it crosses tol is decided by its
    last bits, so equal counts need the same arithmetic in both kernels: they take it from qmps_power_d4_core.h.
    Measured on one MI355X: statuses, iteration counts and environments identical on all 161 rows (19 711 steps on the slowest converged
    row).  Before the two kernels shared their arithmetic - the lane kernel iterated A r A^+ on the packed Hermitian matrix - the counts
    differed on 13 rows, all converged on both routes, by up to 16 steps (|difference| x gap <= 2.5e-2), the environments by 2.0e-13."""
    ref = G.references(4)
    a, b = plain(engine_factory, monkeypatch, 4, 'quad'), plain(engine_factory, monkeypatch, 4, 'lane')
    d = a['iters'].astype(np.int64) - b['iters']
    rows = np.flatnonzero(d)
    print(f'gap D=4 plain, quad against lane: statuses differ on {int((a["status"] != b["status"]).sum())} rows, iteration counts on {len(rows)} of {len(d)}'
          + (f': largest |difference| {np.abs(d).max()} steps, largest |difference| x gap {np.abs(d * ref["gap"]).max():.1e}, largest gap among them '
             f'{ref["gap"][rows].max():.1e}; both converged on {int(((a["status"] == 0) & (b["status"] == 0))[rows].sum())} of them; '
             f'max |dr| between the routes {np.abs(a["r"] - b["r"]).max():.1e}' if len(rows) else ''))
    assert np.array_equal(a['status'], b['status'])
    assert np.array_equal(a['iters'], b['iters']), (rows[:8], d[rows][:8])
    assert np.array_equal(a['r'], b['r'])


@pytest.mark.parametrize('krylov,max_iter', [(True, 3000), (False, 3000), (False, 20000)])
def test_d8_power_kernel(krylov, max_iter, engine_factory, monkeypatch):
    """D = 8 'squaring' - the power iteration of the block kernel - with max_iter = 3 000, with and without the Krylov hand-over
    (QMPS_FLAG_KRYLOV_FALLBACK): with it a gap of 3e-6 or more must end with status 0 - on the flip and cycle4 rows the hand-over has to
    pick the eigenvalue +1 among two or four of nearly equal modulus - and three quarters of the rows are compared; without it the power
    rule alone applies and status-1 rows report max_iter iterations.  Every status-0 row within the iterative bound on E, r and rho.
    Without the hand-over 3 000 steps reach no row of the three families (their largest gap, 1.1e-2, needs n* = 2 800 > 750 steps: the
    rule demands only the Haar rows); a third leg with max_iter = 20 000 reaches every family.
    Measured on one MI355X, r / rho / E as fractions of the iterative bound, status 0 : 1:
      armed, 3 000      slow 0.014 / 0.015 / 0.010, flip and cycle4 < 0.0005 (0.09 tol), Haar 0.164 / 0.119 / 0.082; 81 : 0
      off, 3 000        slow 0.192 / 0.080 / 0.081 (one row), Haar as above; 10 : 71
      off, 20 000       slow 0.192 / 0.164 / 0.159, flip 0.001, cycle4 0.001 / 0.002 / 0.001 (0.27 tol); 18 : 63 (13 must converge)"""
    out = solve(engine_factory(8, CAPACITY[8]), G.family(8)['A'], CC.hamiltonian_terms(), 'squaring', monkeypatch, max_iter=max_iter, krylov=krylov)
    check_iterative(8, out, f'power kernel, max_iter {max_iter}, Krylov hand-over ' + ('armed' if krylov else 'off'), max_iter, krylov=krylov,
                    compared='three quarters' if krylov else ('rule' if max_iter == 3000 else 'every family'), at_cap=not krylov)


@pytest.mark.parametrize('switch,max_iter', [(None, 3000), ('QMPS_D16_BLOCK', 3000), ('QMPS_NO_KRYLOV', 3000), ('QMPS_NO_KRYLOV', 60000)])
def test_d16(switch, max_iter, engine_factory, monkeypatch):
    """D = 16 with max_iter = 3 000: the matrix-core power iteration with its Krylov hand-over (the default), the block kernel
    (QMPS_D16_BLOCK: the same hand-over - it ran the power iteration alone until these rows showed status 1 at max_iter where the default
    returns 0) and the power iteration alone (QMPS_NO_KRYLOV).  Same rule as D = 8.  Without the hand-over 3 000 steps reach no row of the
    three families (largest gap 3.2e-3: n* = 9 400); the leg with max_iter = 60 000 reaches every family.
    Measured on one MI355X, r / rho / E as fractions of the iterative bound, status 0 : 1:
      default, 3 000            every family <= 0.001, Haar 0.052 / 0.038 / 0.034; 15 : 0, at most 2 990 iterations
      QMPS_D16_BLOCK, 3 000     the same; 15 : 0 (3 : 12 before the hand-over was armed there)
      QMPS_NO_KRYLOV, 3 000     Haar rows only; 3 : 12
      QMPS_NO_KRYLOV, 60 000    slow 0.118 / 0.104 / 0.061, flip and cycle4 < 0.0005 (0.15 tol); 6 : 9 (6 must converge)"""
    krylov = switch != 'QMPS_NO_KRYLOV'
    out = solve(engine_factory(16, CAPACITY[16]), G.family(16)['A'], CC.hamiltonian_terms(), 'squaring', monkeypatch, max_iter=max_iter, switch=switch)
    check_iterative(16, out, f'{switch or "default"}, max_iter {max_iter}', max_iter, krylov=krylov,
                    compared='three quarters' if krylov else ('rule' if max_iter == 3000 else 'every family'), at_cap=not krylov)
