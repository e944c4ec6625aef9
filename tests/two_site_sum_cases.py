"""Correlator sums of two-site operators (qmps_correlator_sums_two_site): the long-double reference, the operator sets and inputs of
the tests that use it, and the rounding bounds (test infrastructure; tests/test_two_site_sum_cases_cpu.py checks all of it without a
GPU).

Conventions are those of tests/structure_factor_cases.py; an operator is O[2 t1 + t2, 2 s1 + s2] = o[t1, t2, s1, s2] with site 1 the
left one (the index of h in qmps_set_hamiltonian).  For one evaluation, with tau = tr r and AA_(s1 s2) = A_s1 A_s2:

    E2_O(x)        = sum o[t1 t2 s1 s2] AA_(s1 s2) x AA_(t1 t2)^+       L_a = sum o_a[t1 t2 s1 s2] AA_(t1 t2)^+ AA_(s1 s2)
    one[a]         = tr(E2_(O_a)(r)) / tau
    b_c            = E2_(O_c)(r) - one[c] r
    G[j, a, c]     = z_j^2 tr(L_a (1 - z_j Tt)^(-1)(b_c)) / tau           ( = sum_(n >= 2) z_j^n (<O_a(0,1) O_c(n,n+1)> - one[a] one[c]) )
    near[a, c, 0]  = tr(E2_(O_a O_c)(r)) / tau                            (the 4 x 4 product)
    near[a, c, 1]  = <(O_a (x) 1)(1 (x) O_c)> on three sites              (O_c one site to the right)
    near[a, c, 2]  = <(1 (x) O_a)(O_c (x) 1)> on three sites              (O_c one site to the left)
    S[q, a, c]     = sum_d w_d (near[a, c, d] - one[a] one[c]) + G_ac(z) + G_ca(conj z),   w = (1, z, conj z),  z = e^(-i k_q)

The reference contracts the three-site expectations through the full 8 x 8 operator and the 8 x 8 three-site density matrix - the
definition as written, which the kernels are forbidden to do - so it shares no staging with them.

Bounds (the rule of structure_factor_cases.bound and correlator_cases.bound: three times the worst error of float64 numpy against the
long-double reference over every case of this module, rounded up to one digit; tests/test_two_site_sum_cases_cpu.py prints the
measurements and holds float64 numpy to a third):
    |G - reference|          <= C_G 2^-52 ||(1 - z Tt)^(-1)||_2      C_G = 5        (worst measured ratio 1.49, times three 4.5)
    |one, near - reference|  <= C_NEAR 2^-52                          C_NEAR = 40    (worst measured 10.4 units of 2^-52, times three 31.3)
Measured worst err / (2^-52 kappa) of G, Haar / family / product rows (all 130 Haar rows at D <= 8, 5 at D = 16, with
r = env_direct(A); every family row; th = 0, 0.7, pi/2), over all eight operators and all six points:
    D = 2: 1.21 / 1.49 / 0,  D = 4: 0.27 / 1.30 / 0,  D = 8: 0.16 / 0.98 / 0,  D = 16: 0.08 / 0.61 / 0
(the worst is the D = 2 family row 8 at z = -1, resolvent norm up to 7.2e3; on a product state b_c vanishes and G is exactly 0),
and of one and near in units of 2^-52:
    D = 2: 3.4 / 3.3 / 1.5,  D = 4: 1.5 / 2.5 / 1.5,  D = 8: 2.7 / 5.1 / 1.5,  D = 16: 4.9 / 10.4 / 1.5
(the three-site traces sum D^2 products of three tensors each; the D = 16 family row carries the 10.4)."""
import functools

import numpy as np

import correlator_cases as K
import structure_factor_cases as S

LD, CLD, EPS = S.LD, S.CLD, S.EPS
DS = S.DS
Z = S.Z
N_Z, BATCHES = S.N_Z, S.BATCHES
N_OPS = (1, 2, 3, 4)                  # D <= 8: n_ops is a compile-time value of the D = 2 and D = 4 kernels
D16_BATCHES, D16_N_Z, D16_N_OPS = S.D16_BATCHES, S.D16_N_Z, S.D16_N_OPS
THETAS = (0.0, 0.7, np.pi / 2)
C_G = 5.0
C_NEAR = 40.0

I2, X, Y, ZP = K.I2, K.X, K.Y, K.Z
ZZ = np.kron(ZP, ZP)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _unit(op):
    return op / np.linalg.norm(op, 2)


@functools.lru_cache(maxsize=None)
def hermitian_ops():
    """The bond terms of the transverse-field Ising chain at g = 1 and of the XXZ chain at Delta = 1/2, unit spectral norm."""
    tfim = -ZZ + 0.5 * (np.kron(X, I2) + np.kron(I2, X))
    xxz = np.kron(X, X) + np.kron(Y, Y) + 0.5 * ZZ
    return _frozen(np.stack([_unit(tfim), _unit(xxz)]))


@functools.lru_cache(maxsize=None)
def generic_ops():
    """Four complex 4 x 4 operators of unit spectral norm, neither Hermitian nor normal: seeded complex Gaussians."""
    rng = np.random.default_rng(5002)
    G = rng.standard_normal((4, 4, 4)) + 1j * rng.standard_normal((4, 4, 4))
    return _frozen(G / np.linalg.norm(G, 2, axis=(1, 2))[:, None, None])


def embedded_ops(O):
    """O (x) 1 and 1 (x) O of a one-site operator."""
    return np.stack([np.kron(O, I2), np.kron(I2, O)])


@functools.lru_cache(maxsize=None)
def all_ops():
    """Every operator of the module: the Hermitian terms, the generic ones, and the first generic one-site operator on either site."""
    return _frozen(np.concatenate([hermitian_ops(), generic_ops(), embedded_ops(K.generic_ops()[0])]))


def product_rows(D):
    """A[:, 0, 0] = (cos th/2, sin th/2), everything else zero, r = e_00, th in THETAS: the product state of cos th/2 |0> + sin th/2 |1>
    at any bond dimension.  -> A (3, 2, D, D), r (3, D, D), cos th."""
    A = np.zeros((len(THETAS), 2, D, D), dtype=np.complex128)
    r = np.zeros((len(THETAS), D, D), dtype=np.complex128)
    for n, th in enumerate(THETAS):
        A[n, 0, 0, 0], A[n, 1, 0, 0] = np.cos(th / 2), np.sin(th / 2)
        r[n, 0, 0] = 1.0
    return A, r, np.cos(np.array(THETAS))


def zz_variance(c):
    """Variance per site of H = sum ZZ on the product state with <Z> = c: (1 - c^4) + 2 (c^2 - c^4)."""
    return 1 + 2 * c ** 2 - 3 * c ** 4


def _o4(ops, dtype):
    return np.asarray(ops, dtype=dtype).reshape(-1, 2, 2, 2, 2)


def reference(A, r, ops, z, dtype=CLD, solve=None):
    """The definitions of the module docstring, evaluated as written in `dtype` (np.clongdouble with structure_factor_cases.solve_gepp:
    the reference; np.complex128 with np.linalg.solve: what float64 numpy gives for them).  A (B, 2, D, D), r (B, D, D), ops (m, 4, 4),
    z (n_z,) -> G (B, n_z, m, m), one (B, m), near (B, m, m, 3)."""
    if solve is None:
        solve = S.solve_gepp if dtype == CLD else np.linalg.solve
    A = np.asarray(A, dtype=dtype)
    r = np.asarray(r, dtype=dtype)
    ops = np.asarray(ops, dtype=dtype).reshape(-1, 4, 4)
    o = _o4(ops, dtype)
    z = np.asarray(z, dtype=dtype).reshape(-1)
    B, D, m, nz = A.shape[0], A.shape[-1], ops.shape[0], z.shape[0]
    N = D * D
    G = np.empty((B, nz, m, m), dtype=dtype)
    one = np.empty((B, m), dtype=dtype)
    near = np.empty((B, m, m, 3), dtype=dtype)
    eye2 = np.eye(2, dtype=dtype)
    prod = np.einsum('aij,cjk->acik', ops, ops)                                              # O_a O_c on one bond
    right = np.einsum('aij,cjk->acik', np.stack([np.kron(x, eye2) for x in ops]), np.stack([np.kron(eye2, x) for x in ops]))
    left = np.einsum('aij,cjk->acik', np.stack([np.kron(eye2, x) for x in ops]), np.stack([np.kron(x, eye2) for x in ops]))
    eye = np.eye(N, dtype=dtype)
    for b in range(B):
        Ab, rb = A[b], r[b]
        tau = np.trace(rb)
        AA = np.einsum('sik,ukj->suij', Ab, Ab)                                              # A_s1 A_s2
        AAA = np.einsum('suik,vkj->suvij', AA, Ab).reshape(8, D, D)
        X2 = np.einsum('suik,kl,tvjl->tvsuij', AA, rb, AA.conj())                            # AA_(s1 s2) r AA_(t1 t2)^+ at [t1 t2 s1 s2]
        rho2 = np.einsum('tvsuii->tvsu', X2).reshape(4, 4)
        rho3 = np.einsum('Sik,kl,Til->TS', AAA, rb, AAA.conj())
        one[b] = np.einsum('ats,ts->a', ops, rho2) / tau
        near[b, :, :, 0] = np.einsum('acts,ts->ac', prod, rho2) / tau
        near[b, :, :, 1] = np.einsum('acTS,TS->ac', right, rho3) / tau
        near[b, :, :, 2] = np.einsum('acTS,TS->ac', left, rho3) / tau
        rhs = np.einsum('ctvsu,tvsuij->cij', o, X2) - one[b][:, None, None] * rb           # b_c
        L = np.einsum('atvsu,tvki,sukj->aij', o, AA.conj(), AA)
        Tt = S.deflated(Ab, rb, dtype)
        M = eye[None] - z[:, None, None] * Tt[None]
        Rm = np.broadcast_to(rhs.reshape(m, N).T[None], (nz, N, m))
        Xs = solve(M, np.ascontiguousarray(Rm))
        G[b] = (z * z)[:, None, None] * np.einsum('aji,zijc->zac', L, Xs.reshape(nz, D, D, m)) / tau
    return G, one, near


def bound(A, r, z):
    """Largest |G - reference| (elementwise, operators of unit spectral norm) granted to a float64 evaluation: (B, n_z)."""
    return C_G * EPS * S.kappa(A, r, z)


def bound_near():
    """Largest |one - reference| and |near - reference| granted to a float64 evaluation (operators of unit spectral norm; no solve is
    involved, so nothing scales it)."""
    return C_NEAR * EPS


def bound_S(A, r, k):
    """What the composed S[b, q] may be off by: the two sums it adds, and three near terms each with its product one[a] one[c]
    (|one| <= 1: three values of bound_near() per term).  (B, n_k)."""
    bnd = bound(A, r, S.k_to_z(k))
    return bnd[:, 0::2] + bnd[:, 1::2] + 9 * bound_near()


def structure_factor(G, one, near, z):
    """Host composition: G (B, 2 n_k, m, m) at z = structure_factor_cases.k_to_z(k) -> S (B, n_k, m, m)."""
    z = np.asarray(z).reshape(-1)
    w = np.stack([np.ones_like(z[0::2]), z[0::2], z[1::2]], axis=-1)
    conn = near - (one[:, :, None] * one[:, None, :])[..., None]
    return np.einsum('qd,bacd->bqac', w, conn) + G[:, 0::2] + np.swapaxes(G[:, 1::2], -1, -2)


def series(A, r, ops, z, n_last):
    """sum_(n = 2 .. n_last) z^n (<O_a(0,1) O_c(n,n+1)> - one[a] one[c]) in long double, one transfer-map application per term:
    (n_z, m, m).  A (2, D, D), r (D, D)."""
    A = np.asarray(A, dtype=CLD)
    r = np.asarray(r, dtype=CLD)
    o = _o4(ops, CLD)
    z = np.asarray(z, dtype=CLD).reshape(-1)
    tau = np.trace(r)
    AA = np.einsum('sik,ukj->suij', A, A)
    x = np.einsum('ctvsu,suik,kl,tvjl->cij', o, AA, r, AA.conj())
    L = np.einsum('atvsu,tvki,sukj->aij', o, AA.conj(), AA)
    one = np.einsum('cii->c', x) / tau
    out = np.zeros((len(z), len(o), len(o)), dtype=CLD)
    for n in range(2, n_last + 1):
        conn = np.einsum('aji,cij->ac', L, x) / tau - one[:, None] * one[None, :]
        out += (z ** LD(n))[:, None, None] * conn[None]
        x = np.einsum('sik,ckl,sjl->cij', A, x, A.conj())
    return out


def haar_rows(D):
    return K.HAAR_B if D <= 8 else max(D16_BATCHES)


def points(D):
    return Z if D <= 8 else Z[:max(D16_N_Z)]


@functools.lru_cache(maxsize=None)
def haar_reference(D):
    """(G, one, near, bound) of the generic operators on the Haar rows with the oracle's direct-solve environments, at the points the
    GPU comparison uses; computed once per process."""
    A, r = K.haar_tensors(D)[:haar_rows(D)], S.haar_environments(D, haar_rows(D))
    return reference(A, r, generic_ops(), points(D)) + (bound(A, r, points(D)),)


@functools.lru_cache(maxsize=None)
def family_reference(D):
    A, r, _ = S.family(D)
    return reference(A, r, generic_ops(), points(D)) + (bound(A, r, points(D)),)
