"""Near-singular right environments (test infrastructure): state tensors close to a product state, hidden behind a
random gauge, and a reference for their environment r, two-site density matrix rho and smallest eigenvalue of r that does
not lose digits where the double-precision routes do.

The family.  U = exp(-i t H) with H a random Hermitian 2D x 2D matrix (GUE-like: (X + X^H)/2, X complex standard normal),
A = unitary_to_tensor(U), then A_s -> G A_s G^H with G a Haar D x D unitary.  The gauge turn keeps sum_s A_s^H A_s = 1 and
sends r to G r G^H: the nearly null directions of r are no longer aligned with the pivots of an LDL^H / Cholesky
factorisation.  From t = 1 down to 1e-9 the smallest eigenvalue of r falls from ~1e-2 through ~1e-9 (t = 1e-2) and ~1e-15
(t = 1e-4) to far below the rounding error of r; the transfer gap stays above 0.08, so every solver converges and the
direct solves are accepted in one step.  Without the gauge turn the elimination of the D = 4 kernel (no pivoting) meets a
pivot below 1e-10 from t ~ 3e-6 downwards and hands the evaluation to the power method 2^m steps at a time: the only
cheap way to send a near-singular r through that fall-back.

The reference.  r solves the trace-pinned fixed-point system of oracle.env_direct, (E - 1 + e t^T) vec(r) = e.  Here it
is solved in mpmath at 60 digits: LAPACK's pivoted LU of the double-precision matrix is the preconditioner of an iterative
refinement whose residual T(r) - r, tr r - 1 is formed in mpmath from the tensor itself (the doubles of A are exact
inputs); it stops at a residual below 1e-45 and the condition number of the system (<= ~1e3: 1 / gap) leaves 40 digits.
The smallest eigenvalue comes from mpmath's Hermitian eigen-solver on that r; r is then rounded to double and rho is
oracle.two_site_rdm of the rounded r (a few ulps: ||B_tau|| <= 1).  The doubles of A are an isometry to ~4e-15 only, so
the solution of the pinned system differs from the exactly positive dominant eigen-matrix by about that: below t ~ 1e-4
(D >= 4) lam_min is +-1e-15, either sign - far inside every status band used by the tests.

Measured agreement of the double-precision references with the mpmath one over the rows of `family` (max |dr|):
    D = 2   env_direct 7.2e-16, env_dense_eig 3.7e-12 (growing from 1.3e-14 at t = 1e-4 as t falls: LAPACK's
            eigenvector of a nearly defective matrix; 608 rows)
    D = 4   env_direct 6.7e-16, env_dense_eig 6.9e-15 (1 864 rows)
    D = 8   env_direct 9.4e-16, env_dense_eig 3.5e-15 (8 rows per t: 152)
    D = 16  env_direct 9.0e-16, env_dense_eig 2.1e-15 (2 rows per t: 14)
so at D = 2 it is the dense eigen-solve that loses digits, and oracle.env_direct (pivoted LU) is a sound double-precision
reference where mpmath is too slow (the other rows of D = 8 and D = 16); tests/test_direct_core_cpu.py asserts this."""
import functools

import mpmath as mp
import numpy as np
import scipy.linalg

from oracle import qmps_oracle as O

T_SWEEP = 10.0 ** np.linspace(0, -9, 19)
MP_DIGITS = 60
# rows per strength, gauged sweep / ungauged slice; strengths of the sweep used (D = 16: every third)
LAYOUT = {2: (32, 0, 1), 4: (64, 17, 1), 8: (32, 0, 1), 16: (8, 0, 3)}
T_UNGAUGED = T_SWEEP[11:]        # 3.2e-6 .. 1e-9: the elimination without pivoting is not accepted from here on
N_HAAR = {2: 0, 4: 512, 8: 0, 16: 0}
MP_ROWS_PER_T = {2: None, 4: None, 8: 8, 16: 2}      # None: every row


def near_product_tensors(rng, D, t, n, gauge=True):
    """n state tensors (n, 2, D, D) of strength t: exp(-i t H) of a GUE-like H, optionally behind a Haar gauge."""
    N = 2 * D
    X = rng.standard_normal((n, N, N)) + 1j * rng.standard_normal((n, N, N))
    w, V = np.linalg.eigh((X + X.conj().transpose(0, 2, 1)) / 2)
    U = np.einsum('bij,bj,bkj->bik', V, np.exp(-1j * t * w), V.conj())
    A = O.unitary_to_tensor(U)
    if gauge:
        G = O.haar_unitaries(rng, D, n)
        A = np.einsum('bij,bsjk,blk->bsil', G, A, G.conj())
    return np.ascontiguousarray(A)


def _mp_apply(A, r, D):
    """T(r) = sum_s A_s r A_s^H on lists of mpc."""
    out = [[mp.mpc(0) for _ in range(D)] for _ in range(D)]
    for s in range(len(A)):
        As = A[s]
        Ac = [[As[i][j].conjugate() for j in range(D)] for i in range(D)]
        X = [[mp.fdot(As[i], [r[k][l] for k in range(D)]) for l in range(D)] for i in range(D)]       # A_s r
        for i in range(D):
            for l in range(D):
                out[i][l] += mp.fdot(X[i], Ac[l])                                                         # (A_s r) A_s^H
    return out


def reference_mp(A):
    """(r, lam_min) of ONE tensor (2, D, D) from the mpmath solve; r complex128 (rounded), lam_min float."""
    D = A.shape[1]
    N = D * D
    with mp.workdps(MP_DIGITS):
        M = O.transfer_matrix(A) - np.eye(N)
        M[N - 1, :] += np.eye(D).reshape(N)
        lu = scipy.linalg.lu_factor(M)
        Amp = [[[mp.mpc(A[s, i, j]) for j in range(D)] for i in range(D)] for s in range(A.shape[0])]
        r = [[mp.mpc(0) for _ in range(D)] for _ in range(D)]
        for _ in range(12):
            Tr = _mp_apply(Amp, r, D)
            res = [[r[i][j] - Tr[i][j] for j in range(D)] for i in range(D)]                # rhs - (E - 1) vec r
            res[D - 1][D - 1] += 1 - mp.fsum(r[i][i] for i in range(D))                     # the pinned row: e - t^T vec r
            size = max(abs(x) for row in res for x in row)
            if size < mp.mpf(10) ** -45:
                break
            scale = mp.mpf(2) ** int(mp.floor(mp.log(size, 2)))
            dx = scipy.linalg.lu_solve(lu, np.array([[complex(x / scale) for x in row] for row in res]).reshape(N)).reshape(D, D)
            for i in range(D):
                for j in range(D):
                    r[i][j] += mp.mpc(dx[i, j]) * scale
        else:
            raise RuntimeError('the refinement of the mpmath reference did not converge: the system is singular to double precision')
        tr = mp.fsum(r[i][i].real for i in range(D))
        R = mp.matrix(D, D)
        for i in range(D):
            for j in range(D):
                R[i, j] = (r[i][j] + r[j][i].conjugate()) / (2 * tr)
        lam = mp.eigh(R, eigvals_only=True)
        lam_min = float(min(lam[k] for k in range(D)))
        out = np.array([[complex(R[i, j]) for j in range(D)] for i in range(D)])
    return out, lam_min


def two_site_rdm_mp(A, r):
    """oracle.two_site_rdm evaluated in mpmath (inputs: the doubles of A and r), rounded to double: the check of the reference rho."""
    D = A.shape[1]
    with mp.workdps(MP_DIGITS):
        Am = [mp.matrix(A[s].tolist()) for s in range(2)]
        Bm = [Am[s1] * Am[s2] for s1 in range(2) for s2 in range(2)]
        rm = mp.matrix(r.tolist())
        tr = mp.fsum(rm[i, i].real for i in range(D))
        Br = [b * rm for b in Bm]
        rho = [[mp.fsum(Br[t][i, k] * Bm[s][i, k].conjugate() for i in range(D) for k in range(D)) / tr for s in range(4)] for t in range(4)]
        return np.array([[complex(x) for x in row] for row in rho])


def reference(A, exact=True):
    """(r, rho, lam_min) of one tensor.  exact: the mpmath solve; otherwise oracle.env_direct (pivoted LU in double, the
    stand-in where mpmath is too slow) with the smallest eigenvalue from LAPACK's eigvalsh."""
    if exact:
        r, lam_min = reference_mp(A)
    else:
        r, it, st = O.env_direct(A)
        assert (it, st) == (1, 0)
        lam_min = float(np.linalg.eigvalsh(r)[0])
    return r, O.two_site_rdm(A, r), lam_min


@functools.lru_cache(maxsize=None)
def family(D):
    """The rows of bond dimension D every conditioning test uses, in a fixed order: the gauged sweep (strength by strength),
    the ungauged slice, Haar rows.  dict(A, t (0 for Haar rows), gauged, exact (rows with the mpmath reference))."""
    n, n_un, every = LAYOUT[D]
    rng = np.random.default_rng(9100 + D)
    A, t, gauged, exact = [], [], [], []
    rows_mp = MP_ROWS_PER_T[D]
    for tt in T_SWEEP[::every]:
        A.append(near_product_tensors(rng, D, tt, n))
        t += [tt] * n
        gauged += [True] * n
        exact += [rows_mp is None or k < rows_mp for k in range(n)]
    if n_un:
        for tt in T_UNGAUGED:
            A.append(near_product_tensors(rng, D, tt, n_un, gauge=False))
            t += [tt] * n_un
            gauged += [False] * n_un
            exact += [True] * n_un
    if N_HAAR[D]:
        A.append(O.unitary_to_tensor(O.haar_unitaries(rng, 2 * D, N_HAAR[D])))
        t += [0.0] * N_HAAR[D]
        gauged += [True] * N_HAAR[D]
        exact += [True] * N_HAAR[D]
    out = {'A': np.concatenate(A), 't': np.array(t), 'gauged': np.array(gauged), 'exact': np.array(exact)}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def references(D):
    """dict(r, rho, lam_min) for the rows of family(D)."""
    fam = family(D)
    refs = [reference(a, bool(e)) for a, e in zip(fam['A'], fam['exact'])]
    out = {'r': np.stack([x[0] for x in refs]), 'rho': np.stack([x[1] for x in refs]), 'lam_min': np.array([x[2] for x in refs])}
    for v in out.values():
        v.setflags(write=False)
    return out


def hamiltonian_terms():
    """Three two-site terms, the last one not Hermitian."""
    rng = np.random.default_rng(9099)
    return np.stack([O.hamiltonian_matrix({'ZZ': -1, 'X': 1}), O.hamiltonian_matrix({'XX': 1, 'YY': 1, 'ZZ': 0.5}),
                     rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))])


def reference_energies(D, h):
    """E[b, term] = Re sum h[s, t] rho_ref[t, s]."""
    return np.real(np.einsum('nst,bts->bn', h, references(D)['rho']))


E_TOL = 1e-10            # BASELINE.json north star: energies, environments and density matrices against the reference
R_TOL = 1e-10
RHO_SELF_TOL = 1e-13     # D = 4: rho against two_site_rdm of the kernel's own r (tests/test_direct_gpu.py)
R_DIRECT_TOL = 1e-12     # r against oracle.env_direct where the solve is accepted in one step
BAND = {2: 1e-13, 4: 1e-13, 8: 1e-12, 16: 1e-12}      # lam_min at or above: status 0; a status 2 row lies below


@functools.lru_cache(maxsize=None)
def direct_references(D):
    """oracle.env_direct (r, iterations, status) for the rows of family(D)."""
    return [O.env_direct(a) for a in family(D)['A']]


def compare(D, out, h, label, rows=None, one_step=False, rho_self=False):
    """Compares what a kernel returned for rows `rows` of family(D) (default: all, in order) with the reference on EVERY row of
    status 0 or 2 - no mask on status 0 - prints the worst figures, then asserts them.  out: dict(E (n, terms), r, rho,
    status[, E_lean]).  one_step: rows with iters == 1 also against oracle.env_direct; rho_self: rho against two_site_rdm
    of the kernel's own r.  Returns the figures."""
    fam, ref = family(D), references(D)
    rows = np.arange(len(fam['A'])) if rows is None else np.asarray(rows)
    st = np.asarray(out['status'])
    use = np.flatnonzero((st == 0) | (st == 2))
    g = rows[use]
    Eref = reference_energies(D, h)[g]
    r, rho, E = out['r'][use], out['rho'][use], out['E'][use]
    fig = {'rows': len(rows), 'status0': int((st == 0).sum()), 'status1': int((st == 1).sum()), 'status2': int((st == 2).sum())}
    fig['r'] = float(np.abs(r - ref['r'][g]).max())
    fig['rho'] = float(np.abs(rho - ref['rho'][g]).max())
    fig['E'] = float(np.abs(E - Eref).max())
    if 'E_lean' in out:
        fig['E_lean'] = float(np.abs(out['E_lean'][use] - Eref).max())
    fig['rho_hermitian'] = float(np.abs(rho - rho.conj().transpose(0, 2, 1)).max())
    fig['rho_trace'] = float(np.abs(np.trace(rho, axis1=1, axis2=2) - 1).max())
    fig['rho_min_eig'] = float(np.linalg.eigvalsh((rho + rho.conj().transpose(0, 2, 1)) / 2)[:, 0].min())
    if rho_self:
        fig['rho_self'] = max(float(np.abs(rho[k] - O.two_site_rdm(fam['A'][b], r[k])).max()) for k, b in enumerate(g))
    if one_step:
        dref = direct_references(D)
        one = [k for k, b in enumerate(g) if out['iters'][use[k]] == 1 and dref[b][1] == 1]
        if one:
            fig['r_direct'] = max(float(np.abs(r[k] - dref[g[k]][0]).max()) for k in one)
    lam = ref['lam_min'][rows]
    wrong0 = np.flatnonzero((lam >= BAND[D]) & (st != 0))
    wrong2 = np.flatnonzero((st == 2) & ~(lam < BAND[D]))
    fig['in_band'] = int((lam < BAND[D]).sum())
    print(f'conditioning D={D} {label}: ' + ' '.join(f'{k}={v:.2e}' if isinstance(v, float) else f'{k}={v}' for k, v in fig.items()))
    assert len(wrong0) == 0, (label, 'lam_min >= band but status != 0', rows[wrong0][:8], lam[wrong0][:8], st[wrong0][:8])
    assert len(wrong2) == 0, (label, 'status 2 outside the band', rows[wrong2][:8], lam[wrong2][:8])
    assert fig['r'] < R_TOL and fig['rho'] < R_TOL and fig['E'] < E_TOL, (label, fig)
    assert fig.get('E_lean', 0.0) < E_TOL, (label, fig)
    # (Hermitian: the D = 2, 4 kernels fill the lower triangle from the upper one - exactly 0; D = 8, 16 compute both, entries of modulus <= 1
    # may differ by a few ulps of 2.2e-16)
    assert fig['rho_hermitian'] < 1e-15 and fig['rho_trace'] < 1e-13 and fig['rho_min_eig'] > -1e-13, (label, fig)
    assert fig.get('rho_self', 0.0) < RHO_SELF_TOL and fig.get('r_direct', 0.0) < R_DIRECT_TOL, (label, fig)
    return fig
