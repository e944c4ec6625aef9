"""CPU: the site-factor route of the two-site density matrix (DirectD4::power_step_sites / update_sites / density_sites of
qmps_amd/csrc/qmps_direct_core.h) through the lock-step emulation, tests/csrc/site_factor_emu.cpp:

    rho[(t1 t2)][(s1 s2)] = tr(N_{s1 t1} W_{t2 s2}),   N_{s1 t1} = A_s1^+ A_t1,   W_{t2 s2} = A_t2 r A_s2^+

holds for any tensor and any r - Haar isometries, the near-singular environments of tests/conditioning_cases.py, complex Gaussian tensors
with indefinite and singular r - against the route it replaces in the cold-start kernel (tests/csrc/rho_reference.h) and against numpy;
under every mask a computed part is the full mask's bit for bit and a part left out is exactly 0.0.  The cold-start D = 4 energy kernels
are compiled from this very source; their GPU tests are in test_site_factors_gpu.py."""
import numpy as np

from tests import direct_emu as EMU
from tests import rho_need_cases as RN
from tests import site_factor_cases as SF


def test_factor_set_of_a_mask():
    assert SF.factors(RN.mask(RN.TFIM)) == SF.N00 | SF.N10 | SF.N11 | SF.W01
    assert SF.factors(RN.mask(RN.XXZ)) == SF.N00 | SF.N10 | SF.N11 | SF.W10
    assert SF.factors(RN.mask(RN.COMPLEX_HERMITIAN)) == SF.N00 | SF.N10 | SF.N11 | SF.W01
    assert SF.factors(0xFFFFFFFF) == SF.factors(SF.FULL_UPPER) == 31 and SF.factors(0) == 0
    # bits that stand for no part of the upper triangle ask for nothing
    assert SF.factors(0xFFFFFFFF & ~SF.FULL_UPPER) == 0
    # tau = 2 t1 + t2 <= sigma = 2 s1 + s2 reads N_{s1 t1} and, where t2 != s2, W_{t2 s2}
    for m, t, s, im in SF.single_part_masks():
        t1, t2, s1, s2 = t >> 1, t & 1, s >> 1, s & 1
        want = {(0, 0): SF.N00, (1, 0): SF.N10, (1, 1): SF.N11}[(s1, t1)] | {(0, 0): 0, (1, 1): 0, (0, 1): SF.W01, (1, 0): SF.W10}[(t2, s2)]
        assert SF.factors(m) == want, (t, s, im)


def test_rho_and_energies_against_the_older_route_and_numpy():
    A, r, kind = SF.inputs()
    h = RN.THREE_TERMS
    got = SF.density_energy(A, r, h, 0xFFFFFFFF)
    ref = RN.density_energy(A, r, h, reference=True)
    want = np.triu(np.ones((4, 4)))[None] * SF.rho_numpy(A, r)
    tol = SF.rho_tol(A, r)
    rho = SF.rho_of(got)
    err_np = np.abs(rho - want).max(axis=(1, 2))
    err_ref = np.abs(rho - SF.rho_of(ref)).max(axis=(1, 2))
    ref_np = np.abs(SF.rho_of(ref) - want).max(axis=(1, 2))
    E_np = np.real(np.einsum('nst,bts->bn', h, SF.rho_numpy(A, r)))
    errE = np.abs(got['E'] - E_np).max(axis=1)
    errE_ref = np.abs(got['E'] - ref['E']).max(axis=1)
    tolE = SF.energy_tol(A, r, h)
    for k in ('haar', 'conditioning', 'general'):
        m = kind == k
        print(f'{k}: rows {m.sum()}, not positive definite {(got["pd"][m] == 0).sum()}; max |rho - numpy| {err_np[m].max():.2e} '
              f'(x tol {(err_np[m] / tol[m]).max():.3f}), |rho - older route| {err_ref[m].max():.2e} (x tol {(err_ref[m] / tol[m]).max():.3f}), '
              f'|older route - numpy| {ref_np[m].max():.2e}; |E - numpy| {errE[m].max():.2e} (x tol {(errE[m] / tolE[m]).max():.3f}), '
              f'|E - older route| {errE_ref[m].max():.2e} (x tol {(errE_ref[m] / tolE[m]).max():.3f})')
    # the positive-definiteness test is the older route's, operation for operation
    assert np.array_equal(got['pd'], ref['pd'])
    assert (got['pd'][kind == 'general'] == 0).sum() >= 64 and (got['pd'][kind == 'conditioning'] == 0).sum() > 100
    assert np.all(err_np <= tol) and np.all(errE <= tolE)
    # The older route divides by the pivots of r: where it is itself within the bound of numpy (every row but environments that are singular
    # to rounding and pass the pivot test), the two routes agree to the bound
    sound = ref_np <= tol
    assert sound[kind != 'general'].all() and sound.sum() >= len(A) - 32
    assert np.all(err_ref[sound] <= tol[sound]) and np.all(errE_ref[sound] <= tolE[sound])


def test_the_power_step_is_the_kernels_older_one_to_rounding():
    """y = (W_00 + W_11) / tr against the environment it started from where that is a fixed point (Haar and conditioning rows: the
    emulation's accepted environments), and d2 below the solver's tolerance there."""
    A, r, kind = SF.inputs()
    fix = kind != 'general'
    out = SF.density_energy(A[fix], r[fix], RN.TFIM, RN.mask(RN.TFIM))
    q, l = np.meshgrid(np.arange(4), np.arange(4), indexing='ij')
    coords = np.where(q <= l, r[fix][:, q, l].real, r[fix][:, l, q].imag)      # lane q, coordinate l: Re r[q][l] (q <= l) | Im r[l][q]
    print(f'power step on {fix.sum()} fixed points: max |y - r| {np.abs(out["y"] - coords).max():.2e}, max d2 {out["d2"].max():.2e}')
    assert np.abs(out['y'] - coords).max() < 1e-13
    assert (out['d2'] < 1e-26).mean() > 0.95


def test_masks_leave_parts_out_exactly_and_change_no_bit_of_the_rest():
    A, r, kind = SF.inputs()
    h = RN.THREE_TERMS
    full = SF.density_energy(A, r, h, 0xFFFFFFFF)
    for name, need in SF.masks().items():
        got = SF.density_energy(A, r, h, need)
        assert np.array_equal(got['pd'], full['pd']), name
        assert np.array_equal(got['y'], full['y']) and np.array_equal(got['d2'], full['d2']), name
        for m, t, s, im in SF.single_part_masks():
            key = 'pim' if im else 'pre'
            if need & m:
                assert np.array_equal(got[key][:, t, s], full[key][:, t, s]), (name, key, t, s)
            else:
                assert np.all(got[key][:, t, s] == 0.0) and not np.signbit(got[key][:, t, s]).any(), (name, key, t, s)
    # the energies of a Hamiltonian under its own mask: the full mask's bit for bit (what is left out adds +-0.0 to the same sums)
    for name, hh in dict(RN.table(), three_terms=RN.THREE_TERMS).items():
        if np.isnan(hh).any():
            continue
        a = SF.density_energy(A, r, hh, RN.mask(hh))['E']
        b = SF.density_energy(A, r, hh, 0xFFFFFFFF)['E']
        assert np.array_equal(a, b), name


def test_the_fall_backs_hand_over_keeps_and_replaces_bit_for_bit():
    """update_sites for every lane gives the W of power_step_sites (mode 1), for no lane it leaves W alone (mode 2) - under every mask."""
    A, r, kind = SF.inputs()
    h = RN.THREE_TERMS
    for name, need in SF.masks().items():
        base = SF.density_energy(A, r, h, need)
        for mode in (1, 2):
            got = SF.density_energy(A, r, h, need, via_update=mode)
            for key in ('E', 'pre', 'pim', 'pd'):
                assert np.array_equal(got[key], base[key]), (name, mode, key)


def test_the_whole_cold_start_kernel_against_its_older_emulation():
    """Every row of the conditioning family and 64 Haar rows through the sequence of core calls of the cold-start kernel: iterations and
    statuses identical to tests/csrc/direct_emu.cpp (the acceptance step sums its two halves apart: another rounding of the distance
    only), the environments identical on accepted rows, rho and E within the bounds - the rows that take the power fall-back included."""
    from tests import conditioning_cases as CC
    from oracle import qmps_oracle as O
    A = np.concatenate([O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(77), 8, 64)), CC.family(4)['A']])
    h = RN.THREE_TERMS
    old = EMU.energies_d4(A, h)
    new = SF.energies_d4(A, h, need=0xFFFFFFFF)         # (rho is compared: every part)
    assert np.array_equal(new['iters'], old['iters']) and np.array_equal(new['status'], old['status'])
    fell = old['iters'] > 1
    assert fell.sum() > 50 and (old['status'] == 2).sum() > 100
    assert np.array_equal(new['r'], old['r'])
    use = old['status'] != 1
    tol, tolE = SF.rho_tol(A, old['r']), SF.energy_tol(A, old['r'], h)
    err = np.abs(new['rho'] - old['rho']).max(axis=(1, 2))
    errE = np.abs(new['E'] - old['E']).max(axis=1)
    print(f'rows {len(A)}, fell back {fell.sum()}, status 0 / 1 / 2: {[(old["status"] == k).sum() for k in range(3)]}; max |rho - older| '
          f'{err[use].max():.2e} (x tol {(err[use] / tol[use]).max():.3f}; fall-back rows {err[use & fell].max():.2e}), '
          f'|E - older| {errE[use].max():.2e} (x tol {(errE[use] / tolE[use]).max():.3f})')
    assert np.all(err[use] <= tol[use]) and np.all(errE[use] <= tolE[use])
    # under the Hamiltonian's own mask: the same energies bit for bit
    for hh in (RN.TFIM, RN.XXZ, RN.COMPLEX_HERMITIAN, h):
        a, b = SF.energies_d4(A, hh), SF.energies_d4(A, hh, need=0xFFFFFFFF)
        for key in ('E', 'iters', 'status', 'r'):
            assert np.array_equal(a[key], b[key]), key
