"""tests/gap_cases.py checked without a GPU: the families are what they claim to be, the mpmath reference converged on every row, and the
double-precision references and the CPU emulation of the D = 4 kernel's arithmetic stay within a third of the direct bound - the
margin the kernels are then granted on the GPU (tests/test_gap_gpu.py)."""
import numpy as np
import pytest

from oracle import qmps_oracle as O
from tests import conditioning_cases as CC
from tests import direct_emu as EMU
from tests import gap_cases as G

BATCH = {2: 113, 4: 161, 8: 81, 16: 15}
PLACE = {'slow': (1,), 'flip': (-1,), 'cycle4': (-1, 1j, -1j)}


@pytest.mark.parametrize('D', G.DS)
def test_families_are_what_they_claim(D):
    """Batch sizes (no multiple of 16), isometry to 1e-13, lambda_2 where the family puts it (the direction of every near-unit eigenvalue
    within 0.05 of +1 / -1 / the triple -1, +i, -i - 0.35 at t = 0.3 -; the triple's 1 - |lambda| within a factor 4 of each other), the gap falling in median
    from strength to strength down to below 1e-8, Haar rows with a gap above 0.05, lam_min > 1e-3 on every row."""
    fam, ref = G.family(D), G.references(D)
    A = fam['A']
    B = len(A)
    assert B == BATCH[D] and B % 16 != 0 and B % 64 != 0
    assert B == len(G.families(D)) * len(G.STRENGTHS[D]) * G.ROWS[D] + G.N_HAAR[D]
    assert np.abs(np.einsum('bsij,bsik->bjk', A.conj(), A) - np.eye(D)).max() < 1e-13
    for name in G.families(D):
        m = fam['family'] == name
        n = len(PLACE[name])
        lam = ref['lam3'][m][:, :n]
        for row, t in zip(lam / np.abs(lam), fam['t'][m]):
            off = 0.05 if t <= 0.1 else 0.35             # (the strongest kick moves a D = 2 eigenvalue 0.31 off the axis)
            assert max(min(abs(z - p) for z in row) for p in PLACE[name]) < off, (name, row)      # every place is taken ...
            assert max(min(abs(z - p) for p in PLACE[name]) for z in row) < off, (name, row)      # ... and nothing sits elsewhere
        g = 1.0 - np.abs(lam)
        assert np.all(g.max(1) <= 4.0 * g.min(1)), name
        med = [np.median(ref['gap'][m & (fam['t'] == t)]) for t in G.STRENGTHS[D]]
        print(f'gap D={D} {name}: median gap per strength ' + ' '.join(f'{x:.1e}' for x in med) + f'; kappa {ref["kappa"][m].min():.1e} .. {ref["kappa"][m].max():.1e}')
        assert np.all(np.diff(med) < 0) and med[0] > 1e-3 and med[-1] < 1e-8, (name, med)
        if name != 'slow':
            # the fixed point stays well conditioned whatever the gap (D = 2: 223 on a row whose THIRD eigenvalue is +0.9955, at any strength)
            assert ref['kappa'][m].max() < 1e3 and np.median(ref['kappa'][m]) < 10 and (ref['kappa'] * ref['gap'])[m & (ref['gap'] < 1e-6)].max() < 1e-3
        else:
            assert ref['kappa'][m].max() > 1e8
    assert ref['gap'][fam['family'] == 'haar'].min() > 0.05
    print(f'gap D={D}: smallest lam_min {ref["lam_min"].min():.2e}')
    assert ref['lam_min'].min() > G.LAM_MIN_FLOOR


@pytest.mark.parametrize('D', G.DS)
def test_reference_and_double_precision_solves(D):
    """The mpmath refinement converged on every row (references() raises otherwise; its rounded r is a fixed point, Hermitian, of
    unit trace, to the rounding of one application of T), and oracle.env_direct - accepted in one step with status 0 - stays within a
    third of the direct bound on E, r and rho."""
    fam, ref = G.family(D), G.references(D)
    for a, r in zip(fam['A'], ref['r']):
        assert np.abs(O.apply_transfer(a, r) - r).max() < 8 * D * G.EPS
        assert np.abs(r - r.conj().T).max() == 0.0 and abs(np.trace(r) - 1) < 4 * D * G.EPS
    out = G.cpu_direct(D)
    assert np.all(out['iters'] == 1) and np.all(out['status'] == 0)
    G.show(f'gap D={D} env_direct in units of 2^-52 kappa', G.worst_fraction(D, out, G.EPS * ref['kappa']))
    fig = G.worst_fraction(D, out, G.direct_bound(D))
    G.show(f'gap D={D} env_direct as a fraction of the direct bound', fig)
    assert max(max(v) for v in fig.values()) < 1 / 3


def test_d4_emulation_within_a_third_of_the_direct_bound():
    """direct_emu.energies_d4, the arithmetic of energy_direct_d4_kernel on the CPU: every row accepted in one step with status 0; E (both
    the rho route and the density-matrix-free one), r and rho within a third of the direct bound."""
    ref = G.references(4)
    out = EMU.energies_d4(G.family(4)['A'], CC.hamiltonian_terms())
    assert np.all(out['iters'] == 1) and np.all(out['status'] == 0)
    G.show('gap D=4 emulation in units of 2^-52 kappa', G.worst_fraction(4, out, G.EPS * ref['kappa']))
    for label, E in (('rho route', out['E']), ('lean route', out['E_lean'])):
        fig = G.worst_fraction(4, dict(out, E=E), G.direct_bound(4))
        G.show(f'gap D=4 emulation ({label}) as a fraction of the direct bound', fig)
        assert max(max(v) for v in fig.values()) < 1 / 3


def test_dense_eig_is_no_reference_here():
    """oracle.env_dense_eig - the reference of tests/test_direct_gpu.py and tests/test_energy_gpu.py - leaves the direct bound on some
    slow row: LAPACK's eigenvector of a nearly degenerate eigenvalue loses more than a backward-stable solve of the pinned system does."""
    worst = {}
    for D in G.DS:
        fig = G.worst_fraction(D, G.cpu_dense_eig(D), G.direct_bound(D))
        G.show(f'gap D={D} env_dense_eig as a fraction of the direct bound', fig)
        worst[D] = max(fig['slow'])
    assert max(worst.values()) > 1.0, worst


def test_status_rule():
    """The rule for iterative solves on a synthetic spectrum: must / may bands of n* = ln(tol) / ln|lambda_2| and the Krylov clause."""
    ref = G.references(4)
    n = G.power_steps_needed(4, 1e-13)
    assert np.allclose(n, np.log(1e-13) / np.log1p(-ref['gap']), rtol=1e-6)
    must, may = G.must_converge(4, 1e-13, 20000), G.may_fail(4, 1e-13, 20000)
    assert not np.any(must & may) and must.any() and may.any() and np.any(~must & ~may)
    assert np.all(ref['gap'][must] > 30 * 4 / 20000 * 0.9) and np.all(ref['gap'][may] < 30 / 4 / 20000 * 1.1)
    mk = G.must_converge(4, 1e-13, 3000, krylov=True)
    assert np.all(mk[ref['gap'] >= G.KRYLOV_GAP]) and np.all(mk >= G.must_converge(4, 1e-13, 3000))
    assert not np.any(G.may_fail(4, 1e-13, 3000, krylov=True) & mk)
