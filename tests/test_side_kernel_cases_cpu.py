"""The conditions that tests/test_side_kernels_gpu.py relies on, proved on the references alone (no GPU): the gauge identity of the
two-site cells, their transfer gap, which of them leave the 4 x 4 direct solve, the status shares on the reference side; the tie-break of
the brick-wall reference against LAPACK's complex eigen-solver, the conjugate-pair counts, the absence of both status-1 classes from the
Haar-orthogonal, Haar-unitary and state-like rows; the SU(N) references."""
import numpy as np

import side_kernel_cases as SK
from oracle import brickwall_oracle as BW
from oracle import qmps_oracle as O
from qmps_amd import ground_state as G
from tests import conditioning_cases as CC


def test_gauged_unitaries_are_the_gauged_tensors():
    """U' = (G x 1_2) U blockdiag(G^H, 1_D) is A_s -> G A_s G^H under unitary_to_tensor: the unitaries of this module against
    conditioning_cases.near_product_tensors from the same generator state, D = 2 and 4, gauged and not; U' stays unitary."""
    for D in (2, 4):
        for gauge in (True, False):
            for t in (1.0, 1e-3, 1e-9):
                U = SK.near_product_unitaries(np.random.default_rng(31 + D), D, t, 5, gauge)
                A = CC.near_product_tensors(np.random.default_rng(31 + D), D, t, 5, gauge)
                assert np.abs(O.unitary_to_tensor(U) - A).max() < 1e-15
                assert np.abs(U.conj().transpose(0, 2, 1) @ U - np.eye(2 * D)).max() < 1e-14


def test_cell_family_gap_pivots_and_status_shares():
    """169 cells, not a multiple of 64.  The gap of T_A1 T_A2 is at least 0.17 everywhere (measured: 0.314, a Haar cell).
    |T[0][0] - 1| < 1e-10 on the 24 ungauged cells with t <= 1e-6 (median 1.9e-12 at t = 1e-6, at most 3.6e-12) and on no other row (ungauged
    t = 1e-4: at least 1.0e-8; gauged and Haar rows: at least 1.1e-2).  Reference side of the status shares: of the 80 rows with
    0 < t <= 1e-5, 19 have min(lam_min(r12), lam_min(r21)) at or above the band 1e-13 and must be status 0; 61 lie inside it (15 of them
    negative), where the kernel's own rounding decides."""
    fam, ref = SK.cell_family(), SK.cell_references()
    t, gauged = fam['t'], fam['gauged']
    assert len(t) == 169 and len(t) % 64 != 0
    assert ref['gap'].min() >= SK.CELL_GAP, ref['gap'].min()
    power = ~gauged & (t <= SK.CELL_POWER_T)
    assert power.sum() == 3 * SK.CELL_PER_T
    print(f'first pivot: ungauged t <= 1e-6 max {ref["pivot"][power].max():.2e} (median at 1e-6 {np.median(ref["pivot"][~gauged & (t == 1e-6)]):.2e}), '
          f'all other rows min {ref["pivot"][~power].min():.2e}; gap min {ref["gap"].min():.3f}')
    assert ref['pivot'][power].max() < SK.CELL_PIVOT and ref['pivot'][~power].min() > SK.CELL_PIVOT
    small = (t > 0) & (t <= SK.CELL_SMALL_T)
    lam = ref['lam_min'][small]
    above, inside = int((lam >= CC.BAND[2]).sum()), int((lam < CC.BAND[2]).sum())
    print(f'rows with t <= 1e-5: {small.sum()}, lam_min >= band {above}, inside {inside}, negative {(lam < 0).sum()}')
    assert small.sum() == 80
    # both shares of a fifth are possible: enough rows that MUST be status 0, enough rows inside the band that MAY be status 2
    assert above >= 0.2 * small.sum() and inside >= 0.2 * small.sum()
    # outside the small strengths every row is far above the band: status 0 is the only right answer there
    assert ref['lam_min'][~small].min() > 1e-12


def test_cell_reference_is_a_fixed_point_and_numpy_eig_is_not_a_reference():
    """r12 and r21 of the mpmath solve are fixed points of their maps to 1e-14 (the residual is formed in double: two sandwiches, ~20
    roundings; measured 3.9e-15) and have unit trace.  oracle.env_dense_eig (numpy's eig) on the same cells returns a smallest eigenvalue
    of the wrong sign, or off by more than a factor of two, on 46 of the 80 rows with t <= 1e-5: it must not be the reference."""
    fam, ref = SK.cell_family(), SK.cell_references()
    A1s, A2s = O.unitary_to_tensor(fam['U1']), O.unitary_to_tensor(fam['U2'])
    worst, off = 0.0, 0
    for k, (a1, a2) in enumerate(zip(A1s, A2s)):
        r12, r21 = ref['r12'][k], ref['r21'][k]
        f12 = O.apply_transfer(a1, O.apply_transfer(a2, r12))
        f21 = O.apply_transfer(a2, O.apply_transfer(a1, r21))
        worst = max(worst, np.abs(f12 - r12).max(), np.abs(f21 - r21).max(), abs(np.trace(r12) - 1), abs(np.trace(r21) - 1))
        if 0 < fam['t'][k] <= SK.CELL_SMALL_T:
            _, r = O.env_dense_eig(O.merge(a1, a2))
            lam = np.linalg.eigvalsh(r)[0]
            off += int(np.sign(lam) != np.sign(ref['lam12'][k]) or not 0.5 < lam / ref['lam12'][k] < 2.0)
    print(f'fixed-point residual of the reference environments {worst:.2e}; numpy eig lam_min off in sign or by a factor of two on {off} of 80 rows')
    assert worst < 1e-14
    assert off >= 10


def test_cell_energies_agree_with_the_circuit_oracle_where_it_applies():
    """On the Haar cells (r far from singular) the closed form with the mpmath environments equals the oracle's two 4-qubit circuits."""
    fam, ref = SK.cell_family(), SK.cell_references()
    h = CC.hamiltonian_terms()
    haar = np.flatnonzero(fam['t'] == 0)[:6]
    err = max(abs(O.two_site_cell_energy(fam['U1'][k], fam['U2'][k], h[q]) - ref['E'][k, q]) for k in haar for q in range(3))
    assert err < 1e-12, err


def test_leading_eigenpair_breaks_ties_towards_the_positive_imaginary_part():
    """Real environment matrices (Haar-orthogonal gates): at least 30 per side lead with a conjugate pair of |Im| >= 1e-3 (measured: 36 of
    150 on either side, smallest |Im| 1.28e-2).  leading_eigenpair names the member with the positive imaginary part on every one of
    them; oracle.brickwall_oracle.dominant (LAPACK's complex eig + argmax) names the negative one on a good part of them."""
    rows = SK.bw_rows()
    a = rows['kind'] == 'a'
    for name in ('U1', 'U2', 'U1p', 'U2p'):
        assert not np.any(rows[name][a].imag)
    for side in (0, 1):
        M, cls = SK.bw_matrices(side)[a], SK.bw_classes(side)
        assert not np.any(M.imag)
        pim = cls['pair_im'][a]
        pairs = np.flatnonzero(pim >= SK.PAIR_IM)
        lead = [SK.leading_eigenpair(M[k]) for k in pairs]
        wrong = sum(BW.dominant(M[k])[0].imag < 0 for k in pairs)
        print(f'side {side}: {len(pairs)} of {a.sum()} real matrices lead with a conjugate pair, smallest |Im| {pim[pim > 0].min():.3e}; '
              f'brickwall_oracle.dominant picks the negative imaginary part on {wrong}')
        assert len(pairs) >= 30 and np.all(pim[pim > 0] >= SK.PAIR_IM)
        assert all(len(w) == 1 and w[0].imag > 0 for w in lead)
        assert wrong >= 5
    # the rule itself on matrices with known spectra
    R = np.array([[0.3, -0.4, 0, 0], [0.4, 0.3, 0, 0], [0, 0, 0.1, 0], [0, 0, 0, -0.5]])
    assert np.allclose(SK.leading_eigenpair(R), [0.3 + 0.4j])
    assert np.allclose(SK.leading_eigenpair(np.diag([0.5, 0.5, 0.2, 0.5 - 2e-9])), [0.5, 0.5])
    assert np.allclose(SK.leading_eigenpair(np.diag([0.5 + 0.1j, 0.5 + 1e-8 - 0.1j, 0, 0])), [0.5 + 0.1j])      # 2e-7 of tilt beat 1e-8 of real part
    assert SK.status1_class(np.diag([0.5, 0.5, 0.2, 0.1])) is None                                                   # equal: degenerate, not close
    assert SK.status1_class(np.diag([0.5, 0.5 - 1e-9, 0.2, 0.1])) == 'close'
    assert SK.status1_class(np.diag([0.5, 0.5 - 1e-7, 0.2, 0.1])) is None
    assert SK.status1_class(np.diag([1.0, 1.0, 1.0], k=1)) == 'nilpotent'


def test_no_status_1_class_outside_the_special_gates():
    """Rows (a) to (c) hold no nilpotent matrix and no pair of different leading eigenvalues closer than 1e-8 under the tilted order: every
    one of them must come back status 0.  The state-like rows lead with eta = 1.  The grid of special gates holds 196 nilpotent matrices of
    612 on either side and none of the other class; the 12 rows of the existing regression are among its rows."""
    rows = SK.bw_rows()
    kind = rows['kind']
    assert [int((kind == c).sum()) for c in 'abcd'] == [150, 150, 150, 612]
    for side in (0, 1):
        M, cls = SK.bw_matrices(side), SK.bw_classes(side)['cls']
        counts = {c: (int((cls[kind == c] == 'nilpotent').sum()), int((cls[kind == c] == 'close').sum())) for c in 'abcd'}
        print(f'side {side}: (nilpotent, close) per row class {counts}')
        assert counts['a'] == counts['b'] == counts['c'] == (0, 0)
        assert counts['d'][0] > 0
        assert max(abs(SK.leading_eigenpair(m)[0] - 1) for m in M[kind == 'c']) < 1e-13
    Z, X, I = np.diag([1.0, -1.0]), np.array([[0, 1.0], [1.0, 0]]), np.eye(2)
    assert np.array_equal(rows['U1p'][-12:], np.stack([np.kron(Z, X)] * 12)) and np.array_equal(rows['U2p'][-12:], np.stack([np.kron(X, I)] * 12))
    g = SK.special_gates()
    assert len(g) == 11 and np.abs(g.conj().transpose(0, 2, 1) @ g - np.eye(4)).max() < 1e-15
    assert np.allclose(g[10] @ g[10], g[1])                                                    # sqrt(SWAP)^2 = SWAP


def test_brickwall_pool_values_differ_between_shared_and_per_item_operators():
    """The four manifold references differ from each other on every item but the first (a kernel that ignored a shared flag would miss
    them by ~1), and agree on item 0, whose operators are the shared ones."""
    p = SK.bw_pool()
    keys = [(0, 0), (0, 1), (1, 0), (1, 1)]
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert np.abs(p[('ov',) + a] - p[('ov',) + b])[1:].min() > 1e-6
            assert p[('ov',) + a][0] == p[('ov',) + b][0]


def test_su_rows_and_references():
    """32 rows per N: every aligned group of four holds the scales 1, 6, 300, 1e5.  mpmath's expm of the host mirror's generator and the
    host mirror (scipy's expm) agree to 1e-13 on the standard-normal and 6 x rows at N = 4, 8; the tiled tensor batches are 4 k + 1, 2, 3."""
    for N in SK.SU_N:
        sp = SK.su_params(N)
        assert sp['P'].shape == (32, N * N - 1)
        assert np.array_equal(sp['scale'].reshape(8, 4), np.tile(SK.SU_SCALES, (8, 1)))
        size = np.abs(sp['P']).max(axis=1)
        assert np.all(size[sp['scale'] == 1e5] > 1e5) and np.all(size[sp['scale'] == 1.0] < 6.0)
    for N in SK.SU_MP_N:
        rows, U = SK.su_references(N)
        assert len(rows) == 16
        err = max(np.abs(U[k] - G.SU(SK.su_params(N)['P'][r], N)).max() for k, r in enumerate(rows))
        print(f'SU({N}): scipy expm against mpmath expm {err:.2e}')
        assert err < 1e-13
        assert np.abs(U.conj().transpose(0, 2, 1) @ U - np.eye(N)).max() < 1e-14
    assert [B % 4 for B in SK.SU_TENSOR_BATCHES] == [1, 2, 3] and SK.SU_TENSOR_POOL % 4 == 1
    mixed = SK.cell_su_mixed()
    assert sorted(mixed['big'] // 4) == [0, 1, 2, 3] and sorted(mixed['big'] % 4) == [0, 1, 2, 3]
