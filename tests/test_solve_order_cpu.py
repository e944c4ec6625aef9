"""CPU: the 16 x 16 solve of the D = 4 energy kernels (DirectD4::solve_gathered / normalise_gathered of qmps_amd/csrc/qmps_direct_core.h:
LU elimination below the pivot only, the pivots taken round the quad - step k on lane k % 4, register k / 4 - and back substitution by
columns) through the lock-step emulation tests/csrc/solve_order_emu.cpp, on 512 Haar rows and every D = 4 row of
tests/conditioning_cases.py.  The reference is a test-only copy of the Gauss-Jordan elimination in the natural pivot order (lane 0's four
rows first), which the kernels ran before.  The D = 4 energy kernels are compiled from this very source; their GPU tests are in
test_solve_order_gpu.py.

Measured: environments of the accepted rows against oracle.env_direct 7.2e-16 (natural order 2.8e-15) and against the mpmath reference
5.8e-16 (natural 2.7e-15); Haar rows: largest |1 / pivot| 19.6 (natural 11.1), largest distance of one power step 6.2e-16 (6.0e-16);
family: the 1 728 gauged rows accepted by both orders (largest |1 / pivot| 1.2e3, natural 5.1e3), the 136 rows of the ungauged slice
refused by both.
With the mask of the pivot's own register removed (the elimination then also changes rows of U, which the back substitution reads)
every test of this file but the bit comparison of the two routes fails: no row is accepted."""
import numpy as np

from oracle import qmps_oracle as O
from tests import conditioning_cases as CC
from tests import solve_order_cases as SO


def same_bits(a, b):
    """identical bit patterns; a NaN equals a NaN (its sign and payload are the compiler's choice of operand order)"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def test_both_routes_give_the_same_bits():
    """solve -> normalise -> gather (the older emulations) and solve_gathered -> normalise_gathered (the kernels): x and us identical on
    every row, and every lane of the quad holds the same sixteen coordinates."""
    for res in SO.results():
        a, b = res['solve'], res['gathered']
        assert same_bits(a['x'], b['x']) and same_bits(a['us'], b['us'])
        assert same_bits(a['pivmax'], b['pivmax']) and same_bits(a['d2'], b['d2'])
        assert same_bits(b['us'], np.repeat(b['us'][:, :, :1], 4, axis=2))
        # the lane's own coordinates are those of the gathered copy: x[q][r] = us[4 q + r]
        assert same_bits(b['x'], b['us'][:, :, 0].reshape(-1, 4, 4))


def test_accepted_rows_against_the_references():
    """Rows that both pivot orders accept: r against oracle.env_direct (pivoted LU) within R_DIRECT_TOL = 1e-12 and against the mpmath
    solve within R_TOL = 1e-10."""
    haar, fam = SO.results()
    dref = CC.direct_references(4)
    rows = [(haar, SO.haar_rows(), [O.env_direct(a) for a in SO.haar_rows()], None),
            (fam, CC.family(4)['A'], dref, CC.references(4)['r'])]
    for res, A, direct, exact in rows:
        both = np.flatnonzero(res['gathered']['accepted'] & res['natural']['accepted'])
        assert len(both) > 500
        if exact is None:
            exact = {b: CC.reference_mp(A[b])[0] for b in both}
        for name in ('gathered', 'natural'):
            r = res[name]['r']
            one = [b for b in both if direct[b][1:] == (1, 0)]
            assert len(one) > 500
            err_d = max(np.abs(r[b] - direct[b][0]).max() for b in one)
            err_m = max(np.abs(r[b] - exact[b]).max() for b in both)
            print(f'{name} order, {len(both)} rows accepted by both: |r - env_direct| {err_d:.2e}, |r - mpmath| {err_m:.2e}')
            if name == 'gathered':
                assert err_d < CC.R_DIRECT_TOL and err_m < CC.R_TOL


def test_haar_rows_are_accepted():
    haar, fam = SO.results()
    t = CC.family(4)['t']
    for res, sel in ((haar, slice(None)), (fam, t == 0)):
        for name in ('gathered', 'natural'):
            out = res[name]
            print(f'{name} order, Haar rows: largest |1 / pivot| {out["pivmax"][sel].max():.3g}, largest step {np.sqrt(out["d2"][sel].max()):.2e}')
        out = res['gathered']
        assert np.all(out['d2'][sel] < SO.TOL ** 2) and np.all(out['pivmax'][sel] < SO.MAX_INVERSE_PIVOT)
        assert out['accepted'][sel].all()


def test_near_singular_rows_accepted_behind_the_gauge_and_refused_without_it():
    """The gauged sweep t = 1 .. 1e-9 is accepted in one step (tests/test_conditioning_gpu.py asks that of the kernel); of the ungauged slice
    more than half is refused (a pivot below 1e-10 without pivoting): the condition tests/test_direct_core_cpu.py states."""
    _, fam = SO.results()
    F = CC.family(4)
    for name in ('gathered', 'natural'):
        acc = fam[name]['accepted']
        g = F['gauged']
        with np.errstate(invalid='ignore'):
            print(f'{name} order: gauged rows accepted {acc[g].sum()} of {g.sum()} (largest |1 / pivot| {fam[name]["pivmax"][g].max():.3g}); '
                  f'ungauged rows refused {(~acc[~g]).sum()} of {(~g).sum()}')
    acc = fam['gathered']['accepted']
    assert acc[F['gauged']].all()
    assert (~acc[~F['gauged']]).mean() > 0.5
