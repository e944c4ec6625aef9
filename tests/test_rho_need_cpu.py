"""CPU: the "needed entries" mask of the two-site density matrix (qmps::rho_need_mask and the masked DirectD4::density / energy of
qmps_amd/csrc/qmps_direct_core.h) through the lock-step emulation: which bits a Hamiltonian sets, and that the masked routes give the
energies of the routes without a mask bit for bit while they leave every entry nobody reads at exactly 0.0.
"Without a mask" is the REFERENCE, tests/csrc/rho_reference.h: density / rho_row / energy word for word as they stood before the mask.
The functions of those names in qmps_direct_core.h now forward to the masked ones with every bit set; they are held to the reference too.
The D = 4 energy kernels are compiled from this very source; their GPU tests are in test_rho_need_gpu.py."""
import functools

import numpy as np

from oracle import qmps_oracle as O
from tests import direct_emu as EMU
from tests import rho_need_cases as RN


def bits(m):
    return {k for k in range(32) if (m >> k) & 1}


def test_mask_table():
    assert bits(RN.mask(RN.TFIM)) == RN.TFIM_BITS
    xxz = bits(RN.mask(RN.XXZ))
    assert xxz and all(k < 16 for k in xxz)
    ch = bits(RN.mask(RN.COMPLEX_HERMITIAN))
    assert RN.TFIM_BITS <= ch and {k for k in ch if k >= 16} == {16 + 2, 16 + 4 * 1 + 3}      # Y x 1 couples 0 <-> 2 and 1 <-> 3
    assert RN.mask(RN.ZERO) == 0
    cases = RN.single_entry_cases()
    assert len(cases) == 32
    for h, expect in cases:
        assert RN.mask(h) == expect, (h.nonzero(), bits(RN.mask(h)), bits(expect))
    assert RN.mask(RN.table()['minus_zero']) == 0
    for s in range(4):
        for t in range(4):
            assert RN.mask(RN.single_entry(s, t, False, np.nan)) == 1 << RN.bit(s, t, False)
            assert RN.mask(RN.single_entry(s, t, True, np.nan)) == (0 if s == t else 1 << RN.bit(s, t, True))
    # not Hermitian: one triangle is enough to need the entry
    assert RN.mask(RN.single_entry(3, 0, False)) == RN.mask(RN.single_entry(0, 3, False)) == 1 << 3
    # several terms: the union
    assert RN.mask(RN.THREE_TERMS) == RN.mask(RN.TFIM) | RN.mask(RN.COMPLEX_HERMITIAN) | RN.mask(RN.XXZ)
    assert RN.mask(np.stack([RN.single_entry(0, 1, True), RN.ZERO, RN.single_entry(2, 2, False)])) == (1 << 17) | (1 << 10)


@functools.lru_cache(maxsize=None)
def inputs():
    """64 Haar tensors, then every row of tests/conditioning_cases.py at D = 4 that the solve finishes (status 0 or 2), with the
    environments of the emulation of the whole kernel -> (A, r, status)."""
    from tests import conditioning_cases as CC
    A = np.concatenate([O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(77), 8, 64)), CC.family(4)['A']])
    out = EMU.energies_d4(A, RN.TFIM)
    keep = (out['status'] == 0) | (out['status'] == 2)
    assert keep[:64].all() and (out['status'][64:] == 2).sum() > 100 and (out['status'][64:] == 0).sum() > 1000
    return A[keep], out['r'][keep], out['status'][keep]


def test_masked_routes_against_the_routes_without_a_mask():
    A, r, status = inputs()
    hams = dict(RN.table(), three_terms=RN.THREE_TERMS)
    nonfinite_full = nonfinite_masked = 0
    for name, h in hams.items():
        need = RN.mask(h)
        full = RN.density_energy(A, r, h, reference=True)
        got = RN.density_energy(A, r, h, need)
        # the routes that take no mask (they forward to the masked ones with every bit set): the reference in every output
        fwd = RN.density_energy(A, r, h)
        for key in ('E', 'pre', 'pim', 'pd'):
            assert np.array_equal(fwd[key], full[key], equal_nan=True), (name, key)
        # status: 2 where the environment is not positive definite - the flag decides it, and the route it selects
        assert np.array_equal(got['pd'], full['pd']), name
        assert np.array_equal(np.where(full['pd'] == 1, 0, 2), status), name
        bad = ~(np.isfinite(full['pre']).all(axis=(1, 2, 3)) & np.isfinite(full['pim']).all(axis=(1, 2, 3)))
        bad_masked = ~(np.isfinite(got['pre']).all(axis=(1, 2, 3)) & np.isfinite(got['pim']).all(axis=(1, 2, 3)))
        nonfinite_full += int(bad.sum())
        nonfinite_masked += int(bad_masked.sum())
        assert not np.any(bad_masked & ~bad), name
        if bad.any():
            assert not np.isfinite(full['E'][bad]).any() and not np.isfinite(got['E'][bad]).any(), name
        ok = ~bad
        # (a NaN in h makes every energy NaN on both routes: equal as NaNs)
        assert np.array_equal(got['E'][ok], full['E'][ok], equal_nan=bool(np.isnan(h).any())), name
        for t in range(4):
            for s in range(t, 4):
                for im, key in ((False, 'pre'), (True, 'pim')):
                    if im and s == t:
                        continue
                    if (need >> RN.bit(s, t, im)) & 1:
                        assert np.array_equal(got[key][ok, t, s], full[key][ok, t, s]), (name, key, t, s)
                    else:
                        assert np.all(got[key][:, t, s] == 0.0) and not np.signbit(got[key][:, t, s]).any(), (name, key, t, s)
    print(f'rows {len(A)} x {len(hams)} Hamiltonians; rows with a non-finite rho: {nonfinite_full} without a mask, {nonfinite_masked} with it')
    assert nonfinite_masked <= nonfinite_full


def test_the_reference_is_the_kernel_emulation():
    """The helper's calls against DirectD4::density / energy as tests/csrc/direct_emu.cpp calls them: same energies, bit for bit."""
    A, r, status = inputs()
    h = RN.THREE_TERMS
    whole = EMU.energies_d4(A, h)
    assert np.array_equal(whole['status'], status)
    assert np.array_equal(RN.density_energy(A, r, h)['E'], whole['E'])
    assert np.array_equal(RN.density_energy(A, r, h, reference=True)['E'], whole['E'])
    assert np.array_equal(RN.density_energy(A, r, h, RN.mask(h))['E'], whole['E'])
