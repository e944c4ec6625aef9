"""GPU: qmps_block_entanglement - density matrices, spectra and entropies of blocks of n = 1 .. 4 sites - against the long-double reference
of tests/block_rdm_cases.py (the cases go in verbatim through qmps_set_env_guess, so the reference is evaluated with the very
environments the device holds and no solver tolerance enters), against the entry points that compute the same numbers another way,
and the contract of the call: NULL outputs, the window, refusals."""
import itertools

import numpy as np
import pytest

import block_rdm_cases as K
import correlator_cases as CC
import resident_cases as RS
from qmps_amd import _lib

pytestmark = pytest.mark.gpu


def _resident_cases(engine_factory, D, B):
    """Engine with the case list cycled over B rows: the tensors, and their environments copied verbatim."""
    A, r = K.batch(D, B)
    eng = engine_factory(D)
    eng.set_tensors(A)
    eng.set_env_guess(r)
    return eng


@pytest.mark.parametrize('D', K.DS)
def test_every_shape_holds_the_three_bounds(engine_factory, D):
    """n = 1 .. 4 and every batch size (16 / 4 / 1 / 1 evaluations per workgroup at D = 2 / 4 / 8 / 16: 17, 31, 65 and 130 leave tails of
    1, 15, 1, 2 of 16 and 1, 3, 1, 2 of 4): every finite row meets the rho, p and S bounds; NaN sits exactly on the two bad rows, in every output."""
    kinds = K.kinds(D)
    worst = np.zeros(3)
    for n, B in itertools.product(K.NS, K.BATCHES):
        T = 2 ** n
        eng = _resident_cases(engine_factory, D, B)
        # the reference rests on the environments the device holds: they are the cases', bit for bit
        assert np.array_equal(eng.environments(B), K.batch(D, B)[1], equal_nan=True)
        p, S, rho = eng.block_entanglement(n, B=B, want_rdm=True)
        assert rho.shape == (B, T, T) and rho.dtype == np.complex128 and p.shape == (B, T) and S.shape == (B,)
        idx = K.batch_index(D, B)
        rho_ref, p_ref, S_ref = (x[idx] for x in K.case_reference(D, n))
        nan = kinds[idx] == 'nan'
        for out in (rho.reshape(B, -1).real, rho.reshape(B, -1).imag, p, S[:, None]):
            assert np.array_equal(np.isnan(out).any(axis=1), nan) and np.array_equal(np.isnan(out).all(axis=1), nan), (D, n, B)
        ok = ~nan
        scale = np.abs(rho_ref[ok]).max(axis=(1, 2)).astype(float)
        e_rho = np.abs(rho[ok] - rho_ref[ok]).max(axis=(1, 2)).astype(float) / K.rho_bound(D, n, scale)
        e_p = np.abs(p[ok] - p_ref[ok]).max(axis=1).astype(float) / K.p_bound(D, n, scale)
        e_S = np.abs(S[ok] - S_ref[ok]).astype(float) / K.entropy_bound(D, n, scale)
        print(f'block rdm D={D} n={n} B={B}: fractions of the bounds: rho {e_rho.max():.3f}, p {e_p.max():.3f}, S {e_S.max():.4f}')
        worst = np.maximum(worst, [e_rho.max(), e_p.max(), e_S.max()])
        names = [K.cases(D)[i][0] for i in idx[ok]]
        assert np.all(e_rho <= 1), (D, n, B, [nm for nm, e in zip(names, e_rho) if e > 1], e_rho.max())
        assert np.all(e_p <= 1), (D, n, B, [nm for nm, e in zip(names, e_p) if e > 1], e_p.max())
        assert np.all(e_S <= 1), (D, n, B, [nm for nm, e in zip(names, e_S) if e > 1], e_S.max())
        assert np.all(np.diff(p[ok], axis=1) <= 0)
    print(f'block rdm D={D}: worst fractions of the bounds: rho {worst[0]:.3f}, p {worst[1]:.3f}, S {worst[2]:.4f}')


@pytest.mark.parametrize('D', K.DS)
def test_against_the_other_entry_points(engine_factory, D):
    """After an energy launch on Haar tensors: n = 2 is `rdm()` and Re tr(h rho_2) is the energy; n = 1 gives the one-site expectations
    of `correlators`; a three-site expectation equals the long-double reference on the device's environments.
    Tolerances: an expectation tr(O rho) of two float64 evaluations of rho differs from the exact one by at most sum |O_ts| times the
    rho bound each."""
    B = 12 if D < 16 else 6
    A = CC.haar_tensors(D)[:B]
    eng = engine_factory(D)
    RS.solve(eng, A, D)
    E = eng.results(B)[0]
    r = eng.environments(B)
    rho2 = eng.block_rdm(2, B)
    # the energies the launch wrote are still there, and so is everything else (`rdm` below is an energy-only launch: it writes them)
    assert eng.results(B)[0].tobytes() == E.tobytes() and eng.environments(B).tobytes() == r.tobytes()
    scale2 = np.maximum(1.0, np.abs(rho2).max(axis=(1, 2)))
    e = np.abs(np.einsum('st,bts->b', RS.H_TFIM, rho2).real - E[:, 0])
    print(f'block rdm D={D}: |Re tr(h rho_2) - E| {e.max():.2e}')
    assert np.all(e <= np.abs(RS.H_TFIM).sum() * K.rho_bound(D, 2, scale2))
    d = np.abs(rho2 - eng.rdm(B)).max(axis=(1, 2))
    print(f'block rdm D={D}: |rho_2 - rdm()| {d.max():.2e} (bound {K.rho_bound(D, 2):.2e})')
    assert np.all(d <= K.rho_bound(D, 2, scale2))
    _, one = eng.correlators(CC.PAULIS, 1, B, want_one_site=True)
    got = eng.expectation(CC.PAULIS, B)
    assert got.shape == (B, 4) and got.dtype == np.complex128
    d1 = np.abs(got - one)
    print(f'block rdm D={D}: |tr(sigma rho_1) - one| {d1.max():.2e}')
    assert np.all(d1 <= 2 * 2 * K.rho_bound(D, 1))
    Z, X = CC.PAULIS[3], CC.PAULIS[1]
    rng = np.random.default_rng(7300 + D)
    ops = np.stack([np.kron(Z, np.kron(X, Z)), rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))])
    ref3 = K.reference_rho(A, r, 3)
    want = np.einsum('ats,bst->ba', ops.astype(K.CLD), ref3)
    got3 = eng.expectation(ops, B)
    scale3 = np.maximum(1.0, np.abs(ref3).max(axis=(1, 2)).astype(float))
    d3 = np.abs(got3 - want).astype(float)
    print(f'block rdm D={D}: three-site expectations against the reference {d3.max():.2e}')
    assert np.all(d3 <= np.abs(ops).sum(axis=(1, 2))[None, :] * K.rho_bound(D, 3, scale3)[:, None])
    assert np.abs(got3[:, 0].imag).max() <= 64 * K.rho_bound(D, 3)           # Z X Z is Hermitian
    # the alias of `rdm`
    assert eng.rdm(B, n_sites=3).tobytes() == eng.block_rdm(3, B).tobytes()


def _raw(eng, B, n, rho, p, S):
    f = lambda a: None if a is None else a.ctypes.data_as(RS.DP)
    return eng._lib.qmps_block_entanglement(eng._ctx, B, n, f(rho), f(p), f(S))


@pytest.mark.parametrize('D', K.DS)
def test_null_outputs_and_window_give_the_same_bits(engine_factory, D):
    """Every combination of NULL outputs returns the bits of the full call in the outputs that remain; a window that starts in the
    middle of a workgroup of the whole-batch launch (5: no multiple of 16, 4 or 1 .. of 16 and 4) returns the bits of its rows."""
    B = 130
    eng = _resident_cases(engine_factory, D, B)
    for n in K.NS:
        T = 2 ** n
        full = (np.empty((B, T, T), dtype=np.complex128), np.empty((B, T)), np.empty(B))
        assert _raw(eng, B, n, full[0].view(np.float64), full[1], full[2]) == _lib.QMPS_OK
        for keep in itertools.product((False, True), repeat=3):
            if not any(keep):
                continue
            out = [np.full_like(x, 7.0) if k else None for x, k in zip(full, keep)]
            assert _raw(eng, B, n, None if out[0] is None else out[0].view(np.float64), out[1], out[2]) == _lib.QMPS_OK
            for x, y in zip(full, out):
                assert y is None or x.tobytes() == y.tobytes(), (D, n, keep)
        eng.set_window(5)
        p, S, rho = eng.block_entanglement(n, B=60, want_rdm=True)
        eng.set_window(0)
        assert rho.tobytes() == full[0][5:65].tobytes() and p.tobytes() == full[1][5:65].tobytes() and S.tobytes() == full[2][5:65].tobytes(), (D, n)


def test_refusals(engine_factory):
    """n = 0 and 5, all outputs NULL, a window past the resident states, no resident environment: refused with the code and a message
    that names the reason, and nothing is written (sentinel-filled buffers); B = 0 succeeds and writes nothing."""
    D = 4
    eng = _resident_cases(engine_factory, D, 40)
    lib = eng._lib
    rho, p, S = np.full((64, 16, 16), 7.0 + 7.0j), np.full((64, 16), 7.0), np.full(64, 7.0)

    def untouched():
        return np.all(rho == 7.0 + 7.0j) and np.all(p == 7.0) and np.all(S == 7.0)

    def refused(rc, code, word):
        msg = lib.qmps_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        assert untouched()

    full = (rho.view(np.float64), p, S)
    refused(_raw(eng, 17, 0, *full), _lib.QMPS_ERR_ARG, 'n_sites')
    refused(_raw(eng, 17, 5, *full), _lib.QMPS_ERR_ARG, 'n_sites')
    refused(_raw(eng, 17, 2, None, None, None), _lib.QMPS_ERR_ARG, 'nothing to return')
    # the call's own arguments come first: a bad n_sites is reported even where the window is bad too
    refused(_raw(eng, -1, 5, *full), _lib.QMPS_ERR_ARG, 'n_sites')
    refused(_raw(eng, -1, 2, *full), _lib.QMPS_ERR_ARG, 'window')
    refused(_raw(eng, eng.max_batch + 1, 2, *full), _lib.QMPS_ERR_ARG, 'max_batch')
    refused(_raw(eng, 41, 2, *full), _lib.QMPS_ERR_STATE, 'resident')          # beyond the resident states
    assert _raw(eng, 0, 2, *full) == _lib.QMPS_OK and untouched()               # empty batch: nothing written
    with pytest.raises(_lib.QmpsError) as info:
        eng.block_rdm(5, 17)
    assert info.value.code == _lib.QMPS_ERR_ARG
    with pytest.raises(ValueError):
        eng.expectation(np.eye(3))
    # a launch that keeps its environments out of HBM leaves none resident
    P = np.random.default_rng(7204).standard_normal((21, 4))
    eng.set_hamiltonian(RS.H_TFIM)
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)
    eng.launch(21, solver='direct', store_env=False)
    refused(_raw(eng, 21, 2, *full), _lib.QMPS_ERR_STATE, 'environment')
    # the same batch with its environments stored: the call works, on tensors the library builds from the resident parameters
    eng.set_ansatz_params(_lib.ANSATZ_SHALLOW_CNOT, P)
    eng.launch(21, solver='direct', store_env=True)
    got = eng.block_rdm(2, 21)
    assert np.abs(got - K.reference_rho(eng.tensors(21), eng.environments(21), 2)).max() <= K.rho_bound(D, 2)
    assert untouched()


def test_size_limit_counts_the_device_side_rho(engine_factory):
    """B * 4^n * 16 bytes may not exceed 1 GiB whether or not rho_out is given: at n = 4 that is 2^18 evaluations.  (The size is
    checked before the resident states are looked at: nothing needs to be uploaded.)"""
    eng = engine_factory(2, (1 << 18) + 1)
    S = np.full(4, 7.0)
    rc = _raw(eng, (1 << 18) + 1, 4, None, None, S)
    assert rc == _lib.QMPS_ERR_ARG and '1 GiB' in eng._lib.qmps_last_error().decode() and np.all(S == 7.0)
