"""GPU: the device ansatz builders on their own (qmps_ansatz_probe) against the long-double reference of tests/ansatz_cases.py.

Every optimiser path starts by turning parameters into state tensors: plain batches (launch_ansatz), rotosolve batches with the
parameter index in device memory (launch_ansatz_shifted) and central-difference batches with an optional mask (launch_ansatz_fd), at
D = 16 through two different kernels behind one dispatch.  Here the tensors themselves are compared, elementwise max-abs, at every
kind, depth, angle family and batch edge; bounds: ansatz_cases.bound (1e-13 up to three layers, linear in the layers beyond; the
float64 builds of tests/test_ansatz_cases_cpu.py stay within a third of it).  Unitarity sum_s A_s^dagger A_s = 1 is held to the same
bound and needs no reference.  Each test prints the largest deviation it saw (profiles/EXPERIMENTS.md records them)."""
import numpy as np
import pytest

import ansatz_cases as AC
from oracle import qmps_oracle as O

pytestmark = pytest.mark.gpu


def _dev(A, ref):
    return float(np.abs(A - ref).max())


def _plain_params():
    return [(D, kind) for D in (2, 4, 8, 16) for kind in AC.KINDS[D]]


@pytest.mark.parametrize('D,kind', _plain_params())
def test_plain_builds_every_depth_and_angle_family(D, kind, engine_factory):
    """1, 3 and 32 layers (D = 16: both sides of the wave / lane dispatch at 64 | 66 and 63 | 66 parameters); standard-normal
    angles, grid angles {0, +-pi/4, +-pi/2, pi, 2 pi}, non-generic exponents of the fractional powers, one angle per row of
    +-1e-300, +-1e-9, +-1e3, +-1e6, all-zero rows."""
    eng = engine_factory(D)
    worst = {}
    for k, n_params, family in AC.plain_cases(D):
        if k != kind:
            continue
        prm, ref = AC.family_params(D, kind, n_params, family), AC.family_reference(D, kind, n_params, family)
        A = eng.ansatz_probe(kind, prm)
        b = AC.bound(kind, D, n_params, family)
        d, u = _dev(A, ref), AC.unitarity_defect(A)
        worst[(n_params, family)] = (d, u, b)
        if b > AC.bound(kind, D, n_params):
            # the wide bound of this family is the float64 product pi t (ansatz_cases.bound); the oracle forms the same product, so
            # against IT the ordinary bound holds: what is left is the device's range reduction and the rounding of the gates
            d2 = _dev(A, AC.oracle_tensors(D, kind, prm))
            worst[(n_params, family + ' vs oracle')] = (d2, u, AC.bound(kind, D, n_params))
            print(f'plain D={D} kind={kind} P={n_params} {family}: max|A - oracle| {d2:.2e}, bound {AC.bound(kind, D, n_params):.1e}')
        print(f'plain D={D} kind={kind} P={n_params} {family}: max|A - ref| {d:.2e}, unitarity {u:.2e}, bound {b:.1e}')
    for (n_params, family), (d, u, b) in worst.items():
        assert d <= b and u <= b, (D, kind, n_params, family, d, u, b)
    # the all-zero rows of the gate lists without Hadamards are exact
    if kind in (1, 4, 5, 6):
        n_params = AC.depth_params(kind, D)[0]
        A = eng.ansatz_probe(kind, AC.family_params(D, kind, n_params, 'zero'))
        assert np.array_equal(A, AC.family_reference(D, kind, n_params, 'zero'))


@pytest.mark.parametrize('D', [2, 4, 8, 16])
def test_plain_builds_second_reference_and_batch_edges(D, engine_factory):
    """B = 1, 3, 37, B D = 64 exactly, 65 .. 127 (one block of the lane kernel, and a second, ragged one), at D = 16 five tensors
    = 40 waves in 10 blocks of the wave kernel: every size against the reference, and a tensor does not depend on how many others
    share its launch (bit for bit).  The 37-row batch also against the float64 oracle, the suite's second reference."""
    eng = engine_factory(D)
    for kind in AC.KINDS[D]:
        n_params = AC.roto_n_params(kind, D)
        prm, ref = AC.family_params(D, kind, n_params, 'normal'), AC.family_reference(D, kind, n_params, 'normal')
        b = AC.bound(kind, D, n_params)
        full = eng.ansatz_probe(kind, prm)
        assert _dev(full, AC.oracle_tensors(D, kind, prm)) <= b
        for B in AC.batch_sizes(D):
            A = eng.ansatz_probe(kind, prm[:B], fill=complex(np.nan, np.nan))
            assert A.shape == (B, 2, D, D) and _dev(A, ref[:B]) <= b and AC.unitarity_defect(A) <= b, (D, kind, B)
            assert np.array_equal(A, full[:B]), (D, kind, B)


@pytest.mark.parametrize('D', [2, 4, 8, 16])
@pytest.mark.parametrize('nsh', [3, 6])
def test_rotosolve_batches(D, nsh, engine_factory):
    """Evaluation nsh r + k = row r with shift k of the drivers' table on parameter `index` (first, middle, last; read from device
    memory), 1 and 5 rows, every kind."""
    eng = engine_factory(D)
    worst = 0.0
    for kind in AC.KINDS[D]:
        for rows in (1, 5):
            P = AC.roto_params(D, kind, 5)[:rows]
            b = AC.bound(kind, D, P.shape[1])
            for index in AC.roto_indices(P.shape[1]):
                ref = AC.reference_tensors(D, kind, AC.shifted_params(P, index, AC.SHIFTS[nsh]))
                A = eng.ansatz_probe(kind, P, nsh=nsh, index=index)
                d = _dev(A, ref)
                worst = max(worst, d)
                assert A.shape[0] == nsh * rows and d <= b and AC.unitarity_defect(A) <= b, (D, kind, rows, index, d)
                # the shift-0 evaluation is the plain build of the row
                assert np.array_equal(A[::nsh], eng.ansatz_probe(kind, P)), (D, kind, rows, index)
    print(f'rotosolve batches D={D} nsh={nsh}: max|A - ref| {worst:.2e}')


@pytest.mark.parametrize('nsh', [3, 6])
def test_rotosolve_batches_across_the_d16_kernel_boundary(nsh, engine_factory):
    """D = 16, ShallowCNOT: shifted batches of up to 512 evaluations run the wave kernel, larger ones the lane kernel.  170 | 171 rows
    of three shifts (510 | 513 evaluations), 85 | 86 rows of six (510 | 516): each kernel against the reference, and the largest
    difference between the two on the rows they share (they round differently: twice the bound at most)."""
    eng = engine_factory(16)
    lo, hi = AC.D16_BOUNDARY_ROWS[nsh]
    P = AC.roto_params(16, 0, hi)
    b = AC.bound(0, 16, P.shape[1])
    for index in AC.roto_indices(P.shape[1])[1:2]:          # (the middle parameter: the general test walks first, middle and last)
        ref = AC.reference_tensors(16, 0, AC.shifted_params(P, index, AC.SHIFTS[nsh]))
        wave = eng.ansatz_probe(0, P[:lo], nsh=nsh, index=index)
        lane = eng.ansatz_probe(0, P, nsh=nsh, index=index)
        assert wave.shape[0] == nsh * lo <= 512 < nsh * hi == lane.shape[0]
        dw, dl, dd = _dev(wave, ref[:nsh * lo]), _dev(lane, ref), _dev(wave, lane[:nsh * lo])
        print(f'D=16 boundary nsh={nsh} index={index}: wave vs ref {dw:.2e}, lane vs ref {dl:.2e}, wave vs lane {dd:.2e}')
        assert dw <= b and dl <= b and dd <= 2 * b, (nsh, index, dw, dl, dd)
        assert AC.unitarity_defect(wave) <= b and AC.unitarity_defect(lane) <= b


@pytest.mark.parametrize('D', [2, 4, 8, 16])
def test_central_difference_batches(D, engine_factory):
    """Evaluation 2 P r + k = row r with +h on parameter k (k < P) or -h on parameter k - P; h = 1e-6 and 1e-3, P = 4, 6 (15 for
    ShallowFull), 1 and 3 rows.  At h = 1e-6 the two neighbours differ by less than a sign or column error would need to show at a
    loose tolerance, so the difference quotient is held to the reference's own as well."""
    eng = engine_factory(D)
    worst = 0.0
    for kind in AC.KINDS[D]:
        for n_params in AC.fd_param_counts(kind, D):
            b = AC.bound(kind, D, n_params)
            for rows in (1, 3):
                P = AC.fd_params(D, kind, n_params)[:rows]
                for h in AC.FD_STEPS:
                    ref = AC.reference_tensors(D, kind, AC.central_difference_params(P, h))
                    A = eng.ansatz_probe(kind, P, fd_h=h)
                    d = _dev(A, ref)
                    worst = max(worst, d)
                    assert A.shape[0] == 2 * n_params * rows and d <= b and AC.unitarity_defect(A) <= b, (D, kind, n_params, rows, h, d)
                    if h == 1e-6:
                        q = lambda T: (T.reshape(rows, 2, n_params, 2, D, D)[:, 0] - T.reshape(rows, 2, n_params, 2, D, D)[:, 1]) / (2 * h)
                        assert np.abs(q(A) - q(ref)).max() <= b / (2 * h), (D, kind, n_params, rows)
                        assert np.abs(q(ref)).max() > 0.1              # (every parameter moves the tensor: a wrong column would show)
    print(f'central-difference batches D={D}: max|A - ref| {worst:.2e}')


@pytest.mark.parametrize('D', [4, 16])
def test_central_difference_mask_leaves_skipped_rows_untouched(D, engine_factory):
    """active = [1, 0, 1]: rows 0 and 2 are built, bit-identical to the unmasked build; every element of row 1's 2 P tensors still
    holds the fill value.  D = 4: the lane kernel; D = 16 (ShallowCNOT): the wave kernel."""
    eng = engine_factory(D)
    P = AC.fd_params(D, 0, 4)
    fill = complex(-7.25, 3.5)
    open_ = eng.ansatz_probe(0, P, fd_h=1e-3)
    A = eng.ansatz_probe(0, P, fd_h=1e-3, active=[1, 0, 1], fill=fill)
    assert np.array_equal(A[:8], open_[:8]) and np.array_equal(A[16:], open_[16:])
    assert np.all(A[8:16] == fill)
    assert _dev(open_, AC.reference_tensors(D, 0, AC.central_difference_params(P, 1e-3))) <= AC.bound(0, D, 4)
    all_on = eng.ansatz_probe(0, P, fd_h=1e-3, active=[1, 1, 1], fill=fill)
    assert np.array_equal(all_on, open_)
    none = eng.ansatz_probe(0, P, fd_h=1e-3, active=[0, 0, 0], fill=fill)
    assert np.all(none == fill)


@pytest.mark.parametrize('D', [2, 4, 8, 16])
def test_set_ansatz_params_builds_the_same_bits_as_the_probe(D, engine_factory):
    """qmps_set_states_ansatz + qmps_get_states == the probe's plain build, bit for bit, for every kind; and the probe builds into
    scratch: resident states survive it."""
    eng = engine_factory(D)
    for kind in AC.KINDS[D]:
        prm = AC.family_params(D, kind, AC.roto_n_params(kind, D), 'normal')
        eng.set_ansatz_params(kind, prm)
        A = eng.tensors()
        assert np.array_equal(A, eng.ansatz_probe(kind, prm)), (D, kind)
        eng.ansatz_probe(kind, prm[::-1][:5], nsh=3, index=1, fill=complex(9, 9))
        assert np.array_equal(eng.tensors(), A), (D, kind)
    T = O.unitary_to_tensor(O.haar_unitaries(np.random.default_rng(5), 2 * D, 7))
    eng.set_tensors(T)
    eng.ansatz_probe(0, AC.family_params(D, 0, 6, 'normal'))
    assert np.array_equal(eng.tensors(), T)


def test_tensors_after_a_fused_launch_equal_the_reference(engine_factory):
    """D = 4: qmps_set_states_ansatz builds nothing, the direct kernel consumes the parameters (tensor built in LDS); the tensors
    materialised afterwards are the reference's (tests/test_direct_gpu.py checks a sample of them against the float64 oracle)."""
    from qmps_amd import _lib as L
    eng = engine_factory(4, 2048)
    eng.set_hamiltonian(O.hamiltonian_matrix({'ZZ': -1, 'X': 1}))
    for kind in (L.ANSATZ_SHALLOW_CNOT, L.ANSATZ_SHALLOW_QAOA, L.ANSATZ_SHALLOW_CNOT3):
        n_params = AC.roto_n_params(kind, 4)
        prm, ref = AC.family_params(4, kind, n_params, 'normal'), AC.family_reference(4, kind, n_params, 'normal')
        eng.set_ansatz_params(kind, prm)
        eng.launch(len(prm), solver='direct')
        E, it, st = eng.results(len(prm))
        A = eng.tensors(len(prm))
        assert _dev(A, ref) <= AC.bound(kind, 4, n_params) and (st == 0).mean() > 0.9, kind
        for r in np.flatnonzero(st == 0)[::9]:
            assert abs(E[r, 0] - O.energy_closed_form(ref[r], O.hamiltonian_matrix({'ZZ': -1, 'X': 1}))) < 1e-10


def test_probe_argument_errors(engine_factory):
    from qmps_amd import _lib as L
    rng = np.random.default_rng(3)
    e2, e4 = engine_factory(2, 64), engine_factory(4)
    bad = [
        lambda: e4._lib.qmps_ansatz_probe(e4._ctx, 7, 0, 4, None, 3, 0, 0.0, None, None, None),                # null buffers
        lambda: _raw(e4, 7, 0, 4, nsh=3),                                 # 7 is no multiple of 3 shifts
        lambda: _raw(e4, 10, 0, 4, nsh=6),
        lambda: _raw(e4, 12, 0, 4, fd_h=1e-6),                            # ... nor 12 of 2 P = 8 neighbours
        lambda: _raw(e4, 8, 0, 4, nsh=4),                                 # shift tables: 3 or 6
        lambda: _raw(e4, 8, 0, 4, nsh=3, fd_h=1e-6),
        lambda: _raw(e4, 6, 0, 4, nsh=3, index=4),                        # index outside [0, P)
        lambda: _raw(e4, 6, 0, 4, nsh=3, index=-1),
        lambda: _raw(e4, 3, 0, 5),                                        # odd number of angles
        lambda: _raw(e4, 3, 3, 4),                                        # triples
        lambda: _raw(e4, 3, 2, 15),                                       # ShallowFull and StateGate: D = 2 only
        lambda: _raw(e4, 3, 6, 6),
        lambda: _raw(e4, 3, 7, 6),
        lambda: _raw(e4, 3, 4, 4),                                        # _nonuniform: 2 (log2 D + 1) = 6 angles per layer
        lambda: _raw(e4, 0, 0, 4),
        lambda: _raw(e2, 66, 0, 4, nsh=3),                                # above max_batch = 64
        lambda: _raw(e4, 3, 0, 4, active=b'\x01\x01\x01'),                # a mask without central differences
    ]
    for call in bad:
        assert call() == L.QMPS_ERR_ARG, e4._lib.qmps_last_error()
    assert _raw(e2, 63, 0, 4, nsh=3) == 0 and _raw(e2, 64, 0, 4, fd_h=1e-6) == 0 and _raw(e2, 3, 2, 15) == 0 and _raw(e2, 3, 6, 6) == 0
    with pytest.raises(L.QmpsError):
        e4.ansatz_probe(L.ANSATZ_SHALLOW_CNOT, rng.standard_normal((3, 5)))
    with pytest.raises(ValueError):
        e4.ansatz_probe(L.ANSATZ_SHALLOW_CNOT, rng.standard_normal((3, 4)), fd_h=1e-3, active=[1, 0])
    # the probe neither creates nor destroys resident states: a context without any still has none
    from qmps_amd import EnergyEngine
    with EnergyEngine(4, 16) as fresh:
        fresh.ansatz_probe(L.ANSATZ_SHALLOW_CNOT, rng.standard_normal((3, 4)))
        with pytest.raises(L.QmpsError) as err:
            fresh.tensors(3)
        assert err.value.code == L.QMPS_ERR_STATE


def _raw(eng, B, kind, n_params, nsh=0, index=0, fd_h=0.0, active=None):
    """The C entry point with buffers large enough for any reading of the arguments."""
    import ctypes
    dp = ctypes.POINTER(ctypes.c_double)
    prm = np.full((max(B, 1), max(n_params, 1)), 0.25)
    out = np.empty((max(B, 1), 2, eng.D, eng.D), dtype=np.complex128)
    return eng._lib.qmps_ansatz_probe(eng._ctx, B, kind, n_params, prm.ctypes.data_as(dp), nsh, index, fd_h, active, None,
                                      out.view(np.float64).ctypes.data_as(dp))
