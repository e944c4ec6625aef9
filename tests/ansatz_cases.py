"""Inputs and the reference of the tests of the device ansatz builders (test infrastructure).

`reference_tensors` builds the state tensor of every ansatz kind from explicit 2^n x 2^n gate matrices multiplied in
`numpy.clongdouble`: the angles are the float64 values the device receives, cosines and sines are taken in long double of those
values (the factors pi/2 and pi of the fractional powers X**t, ZZ**t, XX**t, YY**t are long double as well), and only the finished
tensor is rounded to complex128.  It shares no structure with the kernels (no register file, no lane butterflies, no
powers-by-popcount) and none with the float64 oracle beyond the gate formulas of oracle/qmps_oracle.py, which stays the second
reference.  tests/test_ansatz_cases_cpu.py measures, on exactly the case lists built here, how far a float64 build (the oracle,
the classes of qmps_amd/represent.py) is from this reference: the rounding floor that gates the bounds of
tests/test_ansatz_gpu.py.

Shifted parameters are formed on the host as the kernels form them, by ONE float64 addition `p[i] + shift`, and then built."""
import functools

import numpy as np

from oracle import qmps_oracle as O
from qmps_amd import represent as R

LD, CLD = np.longdouble, np.clongdouble
PI_LD = LD('3.14159265358979323846264338327950288')

KINDS = {2: (0, 1, 2, 3, 4, 5, 6), 4: (0, 1, 3, 4, 5), 8: (0, 1, 3, 4, 5), 16: (0, 1, 3, 4, 5)}
DEPTHS = (1, 3, 32)
ROWS = 37
# shift tables of the rotosolve drivers (roto_shift_value, qmps_circuit.h; qmps/rotosolve.py:175, qmps/tools.py:434-438)
SHIFTS = {3: (0.0, np.pi / 2, -np.pi / 2), 6: (0.0, np.pi, np.pi / 2, -np.pi / 2, np.pi / 4, -np.pi / 4)}
GRID = (0.0, np.pi / 4, -np.pi / 4, np.pi / 2, -np.pi / 2, np.pi, 2 * np.pi)
POWER_GRID = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0)          # non-generic exponents of the fractional powers (kinds 1, 6)
EXTREME = (1e-300, -1e-300, 1e-9, -1e-9, 1e3, -1e3, 1e6, -1e6)
FAMILIES = ('normal', 'grid', 'power_grid', 'tiny', 'large', 'zero')


def n_qubits(D):
    return int(np.log2(D)) + 1


def per_layer(kind, D):
    return {0: 2, 1: 2, 2: 15, 3: 3, 4: 2 * n_qubits(D), 5: 6, 6: 6}[kind]


def layers(kind, D, n_params):
    return max(1, n_params // per_layer(kind, D))


def fractional(kind, D, n_params):
    """Mask over the parameters: True where the angle is the exponent t of a Pauli power (it enters as pi t / 2 or pi t)."""
    m = np.zeros(n_params, dtype=bool)
    if kind == 1:
        m[:] = True
    if kind == 6:
        m[4:6] = True
    return m


# ---------------------------------------------------------------------------------------------
# the long-double reference
# ---------------------------------------------------------------------------------------------
def _cs(angle):
    angle = np.asarray(angle, dtype=LD)
    return np.cos(angle), np.sin(angle)


def _gate(rows):
    """(R,) arrays or scalars, row-major 2 x 2 or 4 x 4 -> (R, k, k) clongdouble."""
    k = len(rows)
    R_ = max(np.size(e) for row in rows for e in row)
    g = np.zeros((R_, k, k), dtype=CLD)
    for a in range(k):
        for b in range(k):
            g[:, a, b] = rows[a][b]
    return g


def _rz(t):
    c, s = _cs(np.asarray(t, dtype=LD) / 2)
    return _gate([[c - 1j * s, 0], [0, c + 1j * s]])


def _rx(t):
    c, s = _cs(np.asarray(t, dtype=LD) / 2)
    return _gate([[c, -1j * s], [-1j * s, c]])


def _ry(t):
    c, s = _cs(np.asarray(t, dtype=LD) / 2)
    return _gate([[c, -s], [s, c]])


def _xpow(t):
    """cirq.X**t = e^{i pi t / 2} (cos(pi t / 2) - i sin(pi t / 2) X)."""
    c, s = _cs(PI_LD * np.asarray(t, dtype=LD) / 2)
    ph = c + 1j * s
    return _gate([[ph * c, -1j * ph * s], [-1j * ph * s, ph * c]])


def _zzpow(t):
    c, s = _cs(PI_LD * np.asarray(t, dtype=LD))
    e = c + 1j * s
    one = np.ones_like(e)
    g = np.zeros((len(e), 4, 4), dtype=CLD)
    for k, v in enumerate((one, e, e, one)):
        g[:, k, k] = v
    return g


def _pppow(P, t):
    """cirq.XX**t / YY**t: 1 on the +1 eigenspace of P x P, e^{i pi t} on the -1 eigenspace."""
    c, s = _cs(PI_LD * np.asarray(t, dtype=LD))
    e = (c + 1j * s)[:, None, None]
    PP = np.kron(P, P).astype(CLD)[None]
    return (1 + e) / 2 * np.eye(4, dtype=CLD)[None] + (1 - e) / 2 * PP


def _kron(a, b):
    Ra = max(a.shape[0], b.shape[0])
    out = np.einsum('rij,rkl->rikjl', np.broadcast_to(a, (Ra,) + a.shape[1:]), np.broadcast_to(b, (Ra,) + b.shape[1:]))
    return out.reshape(Ra, a.shape[1] * b.shape[1], a.shape[2] * b.shape[2])


def _eye(k):
    return np.eye(k, dtype=CLD)[None]


def _on(n, g, q):
    """A gate on qubits q, q + 1, ... (adjacent, big-endian: qubit 0 is the most significant bit) of an n-qubit register."""
    k = int(np.log2(g.shape[1]))
    return _kron(_kron(_eye(2 ** q), g), _eye(2 ** (n - q - k)))


def _each(n, gates):
    """One single-qubit gate per qubit: their Kronecker product."""
    out = gates[0]
    for g in gates[1:]:
        out = _kron(out, g)
    return out


def _bit(n, q):
    return 1 << (n - 1 - q)


def _permutation(n, image):
    m = np.zeros((2 ** n, 2 ** n), dtype=CLD)
    for x in range(2 ** n):
        m[image(x), x] = 1
    return m[None]


def _cnot(n, c, t):
    return _permutation(n, lambda x: x ^ _bit(n, t) if x & _bit(n, c) else x)


def _swap(n, a, b):
    def image(x):
        ba, bb = bool(x & _bit(n, a)), bool(x & _bit(n, b))
        return x if ba == bb else x ^ _bit(n, a) ^ _bit(n, b)
    return _permutation(n, image)


def _ladder(n):
    """CNOT(q[n-2], q[n-1]) first ... CNOT(q0, q1) last."""
    m = _eye(2 ** n)
    for i in reversed(range(n - 1)):
        m = _cnot(n, i, i + 1) @ m
    return m


_HAD = (np.array([[1, 1], [1, -1]], dtype=CLD) / np.sqrt(LD(2)))[None]
_X = np.array([[0, 1], [1, 0]], dtype=CLD)
_Y = np.array([[0, -1j], [1j, 0]], dtype=CLD)


def reference_columns(D, kind, params):
    """params (R, P) float64 -> the first D columns of the ansatz unitary, (R, 2 D, D) clongdouble."""
    p = np.ascontiguousarray(np.atleast_2d(params), dtype=np.float64)
    n = n_qubits(D)
    N = 2 ** n
    S = np.broadcast_to(np.eye(N, dtype=CLD)[:, :D], (p.shape[0], N, D)).copy()
    per = per_layer(kind, D)

    def apply(m):
        nonlocal S
        S = np.matmul(m, S)

    if kind in (0, 3):
        lad, had = _ladder(n), _on(n, _HAD, 0)
        for l in range(0, p.shape[1] - per + 1, per):
            apply(_each(n, [_rz(p[:, l])] * n))
            apply(_each(n, [_rx(p[:, l + 1])] * n))
            if kind == 3:
                apply(_each(n, [_rz(p[:, l + 2])] * n))
            apply(had)
            apply(lad)
    elif kind == 1:
        for l in range(0, p.shape[1] - 1, 2):
            apply(_each(n, [_xpow(p[:, l])] * n))
            for i in range(n - 1):
                apply(_on(n, _zzpow(p[:, l + 1]), i))
    elif kind == 4:
        lad = _ladder(n)
        for l in range(0, p.shape[1] - per + 1, per):
            apply(_each(n, [_rz(p[:, l + i]) for i in range(n)]))
            apply(_each(n, [_rx(p[:, l + n + i]) for i in range(n)]))
            apply(lad)
    elif kind == 5:
        lad = _ladder(n)
        swaps = _eye(N)
        for i in range(n):
            swaps = _swap(n, i, i + 1 if i != n - 1 else 0) @ swaps
        for l in range(0, p.shape[1] - 5, 6):
            a, b, c, d, e, f = (p[:, l + k] for k in range(6))
            apply(_on(n, _kron(_rz(a), _rz(d)), 0))
            apply(_on(n, _kron(_rx(b), _rx(e)), 0))
            apply(_on(n, _kron(_rz(c), _rz(f)), 0))
            apply(lad)
            apply(swaps)
    elif kind == 6:
        assert D == 2
        apply(_kron(_rx(p[:, 0]), _rx(p[:, 1])))
        apply(_kron(_rz(p[:, 2]), _rz(p[:, 3])))
        apply(_pppow(_X, p[:, 4]))
        apply(_pppow(_Y, p[:, 5]))
    elif kind == 2:
        assert D == 2 and p.shape[1] == 15
        v = [p[:, k] for k in range(15)]
        i2 = _eye(2)
        q0 = lambda g: _kron(g, i2)
        q1 = lambda g: _kron(i2, g)
        for m in (q0(_rz(v[0])), q0(_rx(v[1])), q0(_rz(v[2])), q1(_rz(v[3])), q1(_rx(v[4])), q1(_rz(v[5])), _cnot(2, 0, 1), q0(_ry(v[6])),
                  _cnot(2, 1, 0), q0(_ry(v[7])), q1(_rz(v[8])), _cnot(2, 0, 1), q0(_rz(v[9])), q0(_rx(v[10])), q0(_rz(v[11])),
                  q1(_rz(v[12])), q1(_rx(v[13])), q1(_rz(v[14]))):
            apply(m)
    else:
        raise ValueError(kind)
    return S


def reference_tensors(D, kind, params):
    """A[r][s][i][j] = U_r[2 i + s][j], rounded to complex128 once, at the end."""
    S = reference_columns(D, kind, params)
    return np.ascontiguousarray(np.swapaxes(S.reshape(S.shape[0], D, 2, D), 1, 2).astype(np.complex128))


def oracle_unitary(D, kind, p):
    return {0: lambda: O.shallow_cnot_unitary(D, p), 1: lambda: O.shallow_qaoa_unitary(D, p), 2: lambda: O.shallow_full_unitary(p),
            3: lambda: O.shallow_cnot3_unitary(D, p), 4: lambda: O.shallow_cnot_nonuniform_unitary(D, p),
            5: lambda: O.exact_after4_unitary(D, p), 6: lambda: O.state_gate_unitary(p)}[kind]()


def oracle_tensors(D, kind, params):
    return np.stack([O.unitary_to_tensor(oracle_unitary(D, kind, p)) for p in np.atleast_2d(params)])


def represent_tensors(D, kind, params):
    from qmps_amd import tools as T
    cls = {0: R.ShallowCNOTStateTensor, 1: R.ShallowQAOAStateTensor, 2: R.ShallowFullStateTensor, 3: R.ShallowCNOTStateTensor3,
           4: R.ShallowCNOTStateTensor_nonuniform, 5: R.ExactAfter4}.get(kind)
    make = (lambda p: R.StateGate(p)) if kind == 6 else (lambda p: cls(D, p))
    return np.stack([T.unitary_to_tensor(R.unitary(make(p))) for p in np.atleast_2d(params)])


def unitarity_defect(A):
    """max | sum_s A_s^dagger A_s - 1 | over a batch of tensors (B, 2, D, D)."""
    G = np.einsum('bsij,bsik->bjk', A.conj(), A)
    return float(np.abs(G - np.eye(A.shape[-1])).max())


# ---------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------
# A float64 build of the fractional powers forms pi t (or pi t / 2) in float64: the product is rounded (2^-53 relative) and so is pi
# (1.2e-16 absolute), so the angle under the cosine is off by up to ~1.5e-16 |pi t| whatever the trigonometric routine does, and the
# gate by as much.  At |t| = 1e6 that is 5e-10 per gate - not a rounding error of the build but of its INPUT, and the long-double
# reference does not share it.  For the `large` family of kinds 1 and 6 the bound is therefore three times the distance the float64
# ORACLE keeps from the reference on the same case lists (measured by tests/test_ansatz_cases_cpu.py, which asserts that the oracle
# stays within a third of this figure; largest measured floor: see FRACTIONAL_LARGE_FLOOR).  Every other family keeps the project's
# figure, 1e-13 up to three layers, growing linearly with the number of layers.
FRACTIONAL_LARGE_FLOOR = 9.0e-10      # measured: 8.9e-10 (kind 1, D = 16, one layer: an exponent of 1e6 enters five X**t or four ZZ**t gates)


def bound(kind, D, n_params, family='normal'):
    base = 1e-13 * max(1.0, layers(kind, D, n_params) / 3.0)
    if family == 'large' and kind in (1, 6):
        return max(base, 3.0 * FRACTIONAL_LARGE_FLOOR)
    return base


# ---------------------------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([20260101] + [int(k) for k in key])


def depth_params(kind, D):
    """The numbers of parameters of the plain-build cases: 1, 3 and 32 layers, and the dispatch boundaries of D = 16."""
    if kind == 2:
        return (15,)
    if kind == 6:
        return (6,)
    per = per_layer(kind, D)
    out = [per * L for L in DEPTHS]
    if D == 16 and kind == 0:
        out += [66]              # 64 = 32 layers is the last value of the wave kernel, 66 the first of the lane kernel
    if D == 16 and kind == 3:
        out += [63, 66]
    return tuple(out)


def normal_rows(kind, D, n_params):
    return ROWS if n_params == roto_n_params(kind, D) else 6


@functools.lru_cache(maxsize=None)
def family_params(D, kind, n_params, family):
    """The batch of one angle family, (rows, n_params) float64 (read-only), or None where the family does not apply."""
    rng = _rng(D, kind, n_params, FAMILIES.index(family))
    full = layers(kind, D, n_params) <= 3           # the batch-size edges are taken at three layers; deeper circuits get short batches
    if family == 'normal':
        P = rng.standard_normal((normal_rows(kind, D, n_params), n_params))
    elif family == 'grid':
        P = rng.choice(np.array(GRID), size=(16 if full else 6, n_params))
    elif family == 'power_grid':
        if not fractional(kind, D, n_params).any():
            return None
        P = rng.choice(np.array(GRID), size=(16, n_params))
        f = fractional(kind, D, n_params)
        P[:, f] = rng.choice(np.array(POWER_GRID), size=(16, int(f.sum())))
    elif family in ('tiny', 'large'):
        vals = EXTREME[:4] if family == 'tiny' else EXTREME[4:]
        P = rng.standard_normal(((2 if full else 1) * len(vals), n_params))
        for r in range(P.shape[0]):                       # every value on a random parameter (and, in the full batches, once on the last)
            col = rng.integers(n_params) if r < len(vals) else n_params - 1
            P[r, col] = vals[r % len(vals)]
    elif family == 'zero':
        P = np.zeros((2, n_params))
    else:
        raise ValueError(family)
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def family_reference(D, kind, n_params, family):
    A = reference_tensors(D, kind, family_params(D, kind, n_params, family))
    A.setflags(write=False)
    return A


def plain_cases(D):
    """(kind, n_params, family) of every plain-build case at bond dimension D."""
    out = []
    for kind in KINDS[D]:
        for n_params in depth_params(kind, D):
            for family in FAMILIES:
                if family_params(D, kind, n_params, family) is not None:
                    out.append((kind, n_params, family))
    return out


def batch_sizes(D):
    """Prefixes of the 37-row `normal` batch of the three-layer cases (kinds 2 and 6: of their one depth): 1, 3, 37; B D = 64 exactly and 65 .. 127 (one and two 64-thread blocks of the lane
    kernel); at D = 16 five tensors = 40 waves = 10 blocks of 4."""
    edge = {2: (32, 37), 4: (16, 19), 8: (8, 11), 16: (4, 5)}[D]
    return tuple(sorted({1, 3, ROWS} | set(edge)))


def shifted_params(P, index, shifts):
    """Evaluation len(shifts) r + k = row r with shifts[k] added (one float64 addition) to parameter `index`."""
    P = np.asarray(P, dtype=np.float64)
    out = np.repeat(P, len(shifts), axis=0)
    out[:, index] = out[:, index] + np.tile(np.asarray(shifts, dtype=np.float64), P.shape[0])
    return out


def central_difference_params(P, h):
    """Evaluation 2 P r + k = row r with +h on parameter k (k < P) or -h on parameter k - P."""
    P = np.asarray(P, dtype=np.float64)
    rows, n = P.shape
    out = np.repeat(P, 2 * n, axis=0).reshape(rows, 2 * n, n)
    for k in range(n):
        out[:, k, k] = out[:, k, k] + h
        out[:, n + k, k] = out[:, n + k, k] - h
    return out.reshape(rows * 2 * n, n)


def roto_n_params(kind, D):
    """Three layers (the fixed gates of kinds 2 and 6: their own number)."""
    return {2: 15, 6: 6}.get(kind, 3 * per_layer(kind, D))


@functools.lru_cache(maxsize=None)
def roto_params(D, kind, rows):
    P = _rng(D, kind, 77).standard_normal((rows, roto_n_params(kind, D)))
    P.setflags(write=False)
    return P


def roto_indices(n_params):
    return (0, n_params // 2, n_params - 1)


# the shifted-batch boundary of D = 16 (the wave kernel up to 512 evaluations, the lane kernel above): rows on either side
D16_BOUNDARY_ROWS = {3: (170, 171), 6: (85, 86)}


def fd_param_counts(kind, D):
    if kind == 2:
        return (15,)
    per = per_layer(kind, D)
    return tuple(P for P in (4, 6) if P % per == 0)


@functools.lru_cache(maxsize=None)
def fd_params(D, kind, n_params):
    P = _rng(D, kind, n_params, 99).standard_normal((3, n_params))
    P.setflags(write=False)
    return P


FD_STEPS = (1e-6, 1e-3)
