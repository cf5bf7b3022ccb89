"""Host-side input generators for the hot path: closed-form operator /
vector cores the reference builds once on the host, plus the portable seeded generator the
benchmark uses for "rank-r random TTvector" inputs.

    zeros_tt / zeros_tto            src/tt_operators.jl:548-573, :601-616
    toeplitz_to_qtto, Δ, shift, ∇   src/tt_operators.jl:4-19, :24, :276-285
    id_tto                          src/tt_operators.jl:519-532
    qtt_sin / qtt_cos / qtt_exp     src/qtt_tools.jl:116-175
    qtt_polynom                     src/qtt_tools.jl:88-110
    rand_tt                         src/tt_tools.jl:100-139 (randn replaced by a portable stream)
    qtt_to_vector                   src/qtt_tools.jl:57-71 (densifier used by small tests; real or complex trains)
    fourier_qtto, reverse_qtt_bits  src/tt_transformations.jl (the QFT as a complex TToperator of rank K + 1)
    function_to_qtt_uniform         src/qtt_tools.jl:73-82
    qtto_prolongation, qtto_constant_prolongation, qtto_linear_prolongation   src/tt_operators.jl:418-504 (grid transfer; the last two
                                    are RECTANGULAR: d + 1 sites, the extra one with a singleton input index)
    qtt_basis_vector, function_to_tensor, function_to_qtt, qtt_to_function    src/qtt_tools.jl:190-199, :15-55

These are rank-<=5 closed forms evaluated once per problem: host code, not GPU work.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np

from .tt import TToperator, TTvector, r_and_d_to_rks


def zeros_tt(dims: Sequence[int], rks: Sequence[int], ot=None) -> TTvector:
    assert len(dims) + 1 == len(rks), "Dimensions and ranks are not compatible"
    d = len(dims)
    vec = [np.zeros((int(dims[i]), int(rks[i]), int(rks[i + 1])), order="F") for i in range(d)]
    return TTvector(d, vec, tuple(dims), list(rks), [0] * d if ot is None else list(ot))


def zeros_tto(dims: Sequence[int], rks: Sequence[int]) -> TToperator:
    assert len(dims) + 1 == len(rks), "Dimensions and ranks are not compatible"
    d = len(dims)
    vec = [np.zeros((int(dims[i]), int(dims[i]), int(rks[i]), int(rks[i + 1])), order="F") for i in range(d)]
    return TToperator(d, vec, tuple(dims), list(rks), [0] * d)


def _qtt_ranks(d: int, r: int) -> List[int]:
    """zeros_tt(2, d, r): r_and_d_to_rks(r*ones(d+1), (2,...,2)) — src/tt_operators.jl:560-569."""
    return r_and_d_to_rks([r] * (d + 1), (2,) * d)


def toeplitz_to_qtto(alpha: float, beta: float, gamma: float, d: int) -> TToperator:
    """QTT cores of the Toeplitz matrix alpha*I + beta*(super-diagonal) + gamma*(sub-diagonal)."""
    rks = r_and_d_to_rks([3] * (d + 1), (4,) * d, rmax=3)          # zeros_tto(2, d, 3): dims.^2, rmax = r
    out = zeros_tto((2,) * d, rks)
    Id = np.eye(2)
    J = np.array([[0.0, 1.0], [0.0, 0.0]])
    first = np.stack([Id, J.T, J], axis=-1)                          # [i, j, :] = (I, J', J)
    out.tto_vec[0][:, :, 0, :] = first
    mid = np.zeros((2, 2, 3, 3))
    mid[:, :, 0, 0], mid[:, :, 0, 1], mid[:, :, 0, 2] = Id, J.T, J
    mid[:, :, 1, 1] = J
    mid[:, :, 2, 2] = J.T
    for k in range(1, d - 1):
        out.tto_vec[k][...] = mid
    last = np.stack([alpha * Id + beta * J + gamma * J.T, gamma * J, beta * J.T], axis=-1)
    out.tto_vec[d - 1][:, :, :, 0] = last
    return out


def Delta(d: int) -> TToperator:
    """Δ(d): Dirichlet–Dirichlet Laplacian tridiag(-1, 2, -1)."""
    return toeplitz_to_qtto(2, -1, -1, d)


def _bc_laplacian(d: int, corner: np.ndarray) -> TToperator:
    """Δ_DN / Δ_ND (src/tt_operators.jl:290-327): the Toeplitz cores of Δ with a fourth channel that carries `corner` through every
    site and is subtracted at the last one, i.e. tridiag(-1, 2, -1) minus 1 at the diagonal entry whose bits all select `corner`."""
    assert d >= 4, "Dimension must be at least 4"
    out = zeros_tto((2,) * d, [1] + [4] * (d - 1) + [1])
    Id = np.eye(2)
    J = np.array([[0.0, 1.0], [0.0, 0.0]])
    out.tto_vec[0][:, :, 0, :] = np.stack([Id, J.T, J, corner], axis=-1)
    mid = np.zeros((2, 2, 4, 4))
    mid[:, :, 0, 0], mid[:, :, 0, 1], mid[:, :, 0, 2] = Id, J.T, J
    mid[:, :, 1, 1] = J
    mid[:, :, 2, 2] = J.T
    mid[:, :, 3, 3] = corner
    for k in range(1, d - 1):
        out.tto_vec[k][...] = mid
    out.tto_vec[d - 1][:, :, :, 0] = np.stack([2 * Id - J - J.T, -J, -J.T, -corner], axis=-1)
    return out


def Delta_DN(d: int) -> TToperator:
    """Δ_DN(d): Dirichlet–Neumann Laplacian, tridiag(-1, 2, -1) with the LAST diagonal entry 1 — src/tt_operators.jl:290-306."""
    return _bc_laplacian(d, np.array([[0.0, 0.0], [0.0, 1.0]]))


def Delta_ND(d: int) -> TToperator:
    """Δ_ND(d): Neumann–Dirichlet Laplacian, tridiag(-1, 2, -1) with the FIRST diagonal entry 1 — src/tt_operators.jl:311-327."""
    return _bc_laplacian(d, np.array([[1.0, 0.0], [0.0, 0.0]]))


def Delta_NN(d: int) -> TToperator:
    """Δ_NN(d) — src/tt_operators.jl:332-349, cores as the reference writes them: ranks [4, 5, ..., 5, 4], i.e. end ranks that are not
    1 (the first and the last core only fill row 1 / column 1 of their rank-4 ends)."""
    assert d >= 4, "Dimension must be at least 4"
    out = zeros_tto((2,) * d, [4] + [5] * (d - 1) + [4])
    Id = np.eye(2)
    J = np.array([[0.0, 1.0], [0.0, 0.0]])
    I1 = np.array([[1.0, 0.0], [0.0, 0.0]])
    I2 = np.array([[0.0, 0.0], [0.0, 1.0]])
    out.tto_vec[0][:, :, 0, :] = np.stack([Id, J.T, J, I2, I1], axis=-1)
    mid = np.zeros((2, 2, 5, 5))
    mid[:, :, 0, 0], mid[:, :, 0, 1], mid[:, :, 0, 2] = Id, J.T, J
    mid[:, :, 1, 1] = J
    mid[:, :, 2, 2] = J.T
    mid[:, :, 3, 3] = I2
    mid[:, :, 4, 4] = -I1
    for k in range(1, d - 1):
        out.tto_vec[k][...] = mid
    out.tto_vec[d - 1][:, :, :, 0] = np.stack([2 * Id - J - J.T, -J, -J.T, -I2, -I1], axis=-1)
    return out


def shift(d: int) -> TToperator:
    return toeplitz_to_qtto(0, 1, 0, d)


def Nabla(d: int) -> TToperator:
    """∇(d): the backward-difference matrix tridiag(-1, 1, 0) — src/tt_operators.jl:276-278."""
    return toeplitz_to_qtto(1, 0, -1, d)


def id_tto(d: int, n_dim: int = 2) -> TToperator:
    vec = [np.asfortranarray(np.eye(2).reshape(2, 2, 1, 1)) for _ in range(d)]
    return TToperator(d, vec, (n_dim,) * d, [1] * (d + 1), [0] * d)


# ---------------------------------------------------------------------------------------------
# Grid transfer — src/tt_operators.jl:418-504.  The constant and the linear prolongation take a train of d binary sites to d + 1: their
# cores have shape (n_out, n_in, R_l, R_r) and the last one is (2, 1, r, 1), a site that consumes no input site (tt.apply's
# rectangular form, src/tt_operations.jl:116-148).
# ---------------------------------------------------------------------------------------------
def qtto_prolongation(d: int) -> TToperator:
    """qtto_prolongation(d) — src/tt_operators.jl:418-436: the multigrid prolongation as a SQUARE operator of ranks 2."""
    assert d >= 2, "Dimension must be at least 2"
    out = zeros_tto((2,) * d, [1] + [2] * (d - 1) + [1])
    Id = np.eye(2)
    J = np.array([[0.0, 1.0], [0.0, 0.0]])
    out.tto_vec[0][:, :, 0, :] = 0.5 * np.stack([Id, J.T], axis=-1)
    mid = np.zeros((2, 2, 2, 2))
    mid[:, :, 0, 0], mid[:, :, 0, 1], mid[:, :, 1, 1] = Id, J.T, J
    for k in range(1, d - 1):
        out.tto_vec[k][...] = mid
    out.tto_vec[d - 1][:, :, 0, 0] = [[1.0, 1.0], [2.0, 0.0]]
    return out


def qtto_constant_prolongation(d: int) -> TToperator:
    """qtto_constant_prolongation(d) — src/tt_operators.jl:441-458: every coarse value copied to its two fine points.  d + 1 sites: the
    cores of id_tto(d), then ones(2, 1, 1, 1)."""
    assert d >= 1, "Dimension must be at least 1"
    vec = id_tto(d).tto_vec + [np.ones((2, 1, 1, 1), order="F")]
    return TToperator(d + 1, vec, (2,) * (d + 1), [1] * (d + 2), [0] * (d + 1))


def _average_branch(d: int) -> TToperator:
    """0.5 * (id_tto(d) + shift(d)) restated on the host (the sum of src/tt_operations.jl:71-95: first core [I S], middle cores block
    diagonal, last core [I; S]; the scalar of :271-281 on the first core), so that building an operator needs no device.  d == 1 is the
    reference's special case (src/tt_operators.jl:467-470)."""
    if d == 1:
        return TToperator(1, [np.asfortranarray((0.5 * np.array([[1.0, 1.0], [0.0, 1.0]])).reshape(2, 2, 1, 1))], (2,), [1, 1], [0])
    I, S = id_tto(d), shift(d)
    out = zeros_tto((2,) * d, [1] + [a + b for a, b in zip(I.tto_rks[1:-1], S.tto_rks[1:-1])] + [1])
    for k in range(d):
        li, ri = I.tto_rks[k], I.tto_rks[k + 1]
        if k == 0:
            out.tto_vec[k][:, :, :, :ri], out.tto_vec[k][:, :, :, ri:] = I.tto_vec[k], S.tto_vec[k]
        elif k == d - 1:
            out.tto_vec[k][:, :, :li, :], out.tto_vec[k][:, :, li:, :] = I.tto_vec[k], S.tto_vec[k]
        else:
            out.tto_vec[k][:, :, :li, :ri], out.tto_vec[k][:, :, li:, ri:] = I.tto_vec[k], S.tto_vec[k]
    out.tto_vec[0] = np.asfortranarray(0.5 * out.tto_vec[0])
    return out


def qtto_linear_prolongation(d: int) -> TToperator:
    """qtto_linear_prolongation(d) — src/tt_operators.jl:463-504: fine point 2a takes coarse value a, fine point 2a + 1 the mean of a and
    a + 1 (the last one: half of the last value).  d + 1 sites, interior ranks 5: the block-diagonal join of id_tto(d) and
    0.5 (id_tto(d) + shift(d)); the last core (2, 1, r, 1) selects the identity branch for output bit 0, the average for bit 1."""
    assert d >= 1, "Dimension must be at least 1"
    I, Av = id_tto(d), _average_branch(d)
    rks = [1] + [a + b for a, b in zip(I.tto_rks[1:], Av.tto_rks[1:])] + [1]
    vec = []
    for k in range(d):
        li, ri = I.tto_rks[k], I.tto_rks[k + 1]
        core = np.zeros((2, 2, rks[k], rks[k + 1]), order="F")
        if k == 0:
            core[:, :, :, :ri], core[:, :, :, ri:] = I.tto_vec[0], Av.tto_vec[0]
        else:
            core[:, :, :li, :ri], core[:, :, li:, ri:] = I.tto_vec[k], Av.tto_vec[k]
        vec.append(core)
    last = np.zeros((2, 1, rks[d], 1), order="F")
    last[0, 0, :I.tto_rks[d], 0] = 1.0
    last[1, 0, I.tto_rks[d]:, 0] = 1.0
    vec.append(last)
    return TToperator(d + 1, vec, (2,) * (d + 1), rks, [0] * (d + 1))


def qtt_basis_vector(d: int, pos: int, val: float = 1.0) -> TTvector:
    """qtt_basis_vector(d, pos, val = 1.0) — src/qtt_tools.jl:190-199: val times the pos-th (1-based) unit vector of 2^d entries, rank 1,
    site 1 the most significant bit, val on the first core."""
    out = zeros_tt((2,) * d, [1] * (d + 1))
    for k in range(d):
        out.ttv_vec[k][((pos - 1) >> (d - 1 - k)) & 1, 0, 0] = val if k == 0 else 1.0
    return out


def function_to_tensor(f, d: int, a: float = 0.0, b: float = 1.0) -> np.ndarray:
    """function_to_tensor(f, d; a, b) — src/qtt_tools.jl:15-31: out[t_1, ..., t_d] = f(sum_i 2^(d - i) t_i / (2^d - 1)), t_i in {0, 1},
    site 1 the most significant bit.  As in the reference, the interval is accepted and NOT used (index_to_point takes L = b - a and
    never reads it): the points are k / (2^d - 1) in [0, 1] whatever a and b are."""
    out = np.zeros((2,) * d, order="F")
    scale = 2 ** d - 1
    for t in np.ndindex(*(2,) * d):
        x = 2.0 ** (d - 1) * t[0] / scale
        for i in range(2, d + 1):
            x = x + 2.0 ** (d - i) * t[i - 1] / scale
        out[t] = f(x)
    return out


def function_to_qtt(f, d: int, a: float = 0.0, b: float = 1.0) -> TTvector:
    """function_to_qtt(f, d; a = 0.0, b = 1.0) — src/qtt_tools.jl:45-48: ttv_decomp (on the device, tol 1e-12) of the samples of f at
    k / (2^d - 1), k = 0 .. 2^d - 1, site 1 the most significant bit.  a and b do not move the points (see function_to_tensor): the
    reference's behaviour, restated."""
    from .qtt import ttv_decomp
    return ttv_decomp(function_to_tensor(f, d, a, b))


def _trig_train(d, a, b, lam, first_of):
    out = zeros_tt((2,) * d, _qtt_ranks(d, 2))
    h = (b - a) / (2 ** d - 1)
    w = lam * math.pi
    for row, t in ((0, a), (1, a + h * 2 ** (d - 1))):
        out.ttv_vec[0][row, 0, :] = first_of(w * t)
    for k in range(2, d):
        th = w * (h * 2 ** (d - k))
        c, s = math.cos(th), math.sin(th)
        out.ttv_vec[k - 1][0] = np.eye(2)
        out.ttv_vec[k - 1][1] = [[c, -s], [s, c]]
    out.ttv_vec[d - 1][0, 0, 0] = 1.0
    out.ttv_vec[d - 1][1, :, 0] = [math.cos(w * h), math.sin(w * h)]
    return out


def qtt_sin(d: int, a: float = 0.0, b: float = 1.0, lam: float = 1.0) -> TTvector:
    return _trig_train(d, a, b, lam, lambda t: [math.sin(t), math.cos(t)])


def qtt_cos(d: int, a: float = 0.0, b: float = 1.0, lam: float = 1.0) -> TTvector:
    return _trig_train(d, a, b, lam, lambda t: [math.cos(t), -math.sin(t)])


def qtt_exp(d: int, a: float = 0.0, b: float = 1.0, alpha: float = 1.0, beta: float = 0.0) -> TTvector:
    out = zeros_tt((2,) * d, _qtt_ranks(d, 1))
    h = (b - a) / (2 ** d - 1)
    out.ttv_vec[0][:, 0, 0] = [math.exp(alpha * a + beta), math.exp(alpha * (a + h * 2 ** (d - 1)) + beta)]
    for k in range(2, d):
        out.ttv_vec[k - 1][:, 0, 0] = [1.0, math.exp(alpha * (h * 2 ** (d - k)))]
    out.ttv_vec[d - 1][:, 0, 0] = [1.0, math.exp(alpha * h)]
    return out


def qtt_polynom(coef: Sequence[float], d: int, a: float = 0.0, b: float = 1.0) -> TTvector:
    """QTT of the polynomial sum_k coef[k] x^k on the 2^d uniform points of [a, b], all bonds of rank p = len(coef)
    (zeros_tt(2, d, p; r_and_d = false)) — src/qtt_tools.jl:88-110.  d >= 2."""
    assert d >= 2, "qtt_polynom needs d >= 2"
    coef = [float(c) for c in coef]
    p = len(coef)
    h = (b - a) / (2 ** d - 1)
    out = zeros_tt((2,) * d, [1] + [p] * (d - 1) + [1])

    def phi(x, s):                        # the s-th Taylor coefficient of the polynomial at x
        return sum(coef[k] * x ** (k - s) * math.comb(k, s) for k in range(s, p))

    for row, t in ((0, a), (1, a + h * 2 ** (d - 1))):                 # coarsest bit first
        out.ttv_vec[0][row, 0, :] = [phi(t, s) for s in range(p)]
    for k in range(2, d):
        tk = h * 2 ** (d - k)
        core = out.ttv_vec[k - 1]
        core[0] = np.eye(p)
        for i in range(p):
            for j in range(i + 1):
                core[1, i, j] = math.comb(i, j) * tk ** (i - j)
    out.ttv_vec[d - 1][0, 0, 0] = 1.0
    out.ttv_vec[d - 1][1, :, 0] = [h ** s for s in range(p)]
    return out


def qtt_to_vector(qtt: TTvector) -> np.ndarray:
    """Dense 2^d vector (site 1 = most significant bit).  Test/debug helper only (exponential cost)."""
    P = qtt.ttv_vec[0][:, 0, :]
    for k in range(1, qtt.N):
        G = qtt.ttv_vec[k]
        P = np.stack([P @ G[0], P @ G[1]], axis=1).reshape(2 * P.shape[0], G.shape[2])
    return P[:, 0].copy() if P.shape[1] == 1 else P.reshape(-1)


def qtt_to_function(qtt: TTvector) -> np.ndarray:
    """qtt_to_function(qtt) — src/qtt_tools.jl:53-55: qtt_to_vector."""
    return qtt_to_vector(qtt)


# ---------------------------------------------------------------------------------------------
# portable seeded N(0,1) stream: splitmix64 -> 53-bit uniforms -> Box–Muller.
# Same bits from any language that implements these 64-bit integer steps and IEEE double math
# with correctly rounded log/sqrt and the same cos/sin; the benchmark only needs determinism.
# ---------------------------------------------------------------------------------------------
def _splitmix64(n: int, seed: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        idx = np.arange(1, n + 1, dtype=np.uint64)
        z = np.uint64(seed) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def portable_randn(n: int, seed: int) -> np.ndarray:
    m = (n + 1) // 2
    bits = _splitmix64(2 * m, seed)
    u = ((bits >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)   # (0,1)
    r = np.sqrt(-2.0 * np.log(u[0::2]))
    th = 2.0 * math.pi * u[1::2]
    out = np.empty(2 * m)
    out[0::2] = r * np.cos(th)
    out[1::2] = r * np.sin(th)
    return out[:n]


def rand_tt(dims: Sequence[int], rks, seed: int = 0) -> TTvector:
    """rand_tt(dims, rks) / rand_tt(dims, rmax) — src/tt_tools.jl:100-139, entries i.i.d. N(0,1)
    in column-major core order from the portable stream (core k uses seed*1000003 + k)."""
    d = len(dims)
    if isinstance(rks, (int, np.integer)):
        rmax = int(rks)
        rks = r_and_d_to_rks([rmax] * (d + 1), dims, rmax=rmax)
    y = zeros_tt(dims, rks)
    for k in range(d):
        shape = (int(dims[k]), int(rks[k]), int(rks[k + 1]))
        y.ttv_vec[k] = portable_randn(shape[0] * shape[1] * shape[2], seed * 1000003 + k).reshape(shape, order="F")
    return y


# ---------------------------------------------------------------------------------------------------------------------
# Spin-chain Hamiltonians (src/tt_operators.jl:56-64, :162-260): rank-5 open-boundary TT operators on d spin-1/2 sites, Float64 only.
# ---------------------------------------------------------------------------------------------------------------------
_PAULI_X = np.array([[0.0, 1.0], [1.0, 0.0]])
_PAULI_Z = np.array([[1.0, 0.0], [0.0, -1.0]])
_Y_REAL = np.array([[0.0, -1.0], [1.0, 0.0]])        # sigma_y = i * _Y_REAL
_PAULI_Y = np.array([[0.0, -1.0j], [1.0j, 0.0]])


def _pauli_dtype(dtype):
    """np.float64 (the default: real operators, a lone sigma_y refused) or np.complex128 (every axis, complex cores)."""
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float64), np.dtype(np.complex128)):
        raise TypeError(f"dtype must be float64 or complex128, got {dt}")
    return dt == np.dtype(np.complex128)


def _pauli_axis(mu) -> str:
    a = str(mu).lstrip(":").lower()
    if a not in ("x", "y", "z"):
        from ._lib import TTNError
        raise TTNError(f"unknown Pauli axis {mu!r}: use 'x', 'y' or 'z'")
    return a


def _pauli_pair_factors(mu, nu):
    """Real factors (P1, P2) with P1 (x) P2 = sigma_mu (x) sigma_nu (src/tt_operators.jl:56-64): sigma_y (x) sigma_y = (-Y) (x) Y, Y real."""
    a, b = _pauli_axis(mu), _pauli_axis(nu)
    if a == "y" and b == "y":
        return -_Y_REAL, _Y_REAL.copy()
    if a == "y" or b == "y":
        from ._lib import TTNError
        raise TTNError("a single sigma_y factor is complex: only real (Float64) operators are offered")
    m = {"x": _PAULI_X, "z": _PAULI_Z}
    return m[a].copy(), m[b].copy()


def heisenberg_xyz_tto(d: int, jx: float = 1.0, jy: float = 1.0, jz: float = 1.0, lam: float = 0.0, field="x") -> TToperator:
    """H = jx sum_k X_k X_{k+1} + jy sum_k Y_k Y_{k+1} + jz sum_k Z_k Z_{k+1} + lam sum_k P_k (P = the field's Pauli matrix), as the
    reference's direct rank-5 TT operator (src/tt_operators.jl:162-217).  A field along y with lam != 0 is complex: TTNError."""
    assert d >= 2, "Heisenberg XYZ chain needs at least 2 spin sites"
    f = _pauli_axis(field)
    if f == "y":
        if lam != 0.0:
            from ._lib import TTNError
            raise TTNError("field = :y with lam != 0 gives a complex operator: only real (Float64) operators are offered")
        Pf = np.zeros((2, 2))
    else:
        Pf = _PAULI_X if f == "x" else _PAULI_Z
    Px1, Px2 = _pauli_pair_factors("x", "x")
    Py1, Py2 = _pauli_pair_factors("y", "y")
    Pz1, Pz2 = _pauli_pair_factors("z", "z")
    Id = np.eye(2)
    rks = [1] + [5] * (d - 1) + [1]
    out = zeros_tto((2,) * d, rks)
    c = out.tto_vec[0]
    c[:, :, 0, 0], c[:, :, 0, 1], c[:, :, 0, 2], c[:, :, 0, 3], c[:, :, 0, 4] = lam * Pf, jx * Px1, jy * Py1, jz * Pz1, Id
    for k in range(1, d - 1):
        c = out.tto_vec[k]
        c[:, :, 0, 0], c[:, :, 1, 0], c[:, :, 2, 0], c[:, :, 3, 0], c[:, :, 4, 0] = Id, Px2, Py2, Pz2, lam * Pf
        c[:, :, 4, 1], c[:, :, 4, 2], c[:, :, 4, 3], c[:, :, 4, 4] = jx * Px1, jy * Py1, jz * Pz1, Id
    c = out.tto_vec[d - 1]
    c[:, :, 0, 0], c[:, :, 1, 0], c[:, :, 2, 0], c[:, :, 3, 0], c[:, :, 4, 0] = Id, Px2, Py2, Pz2, lam * Pf
    return out


def ising_tto(d: int, J: float = 1.0, h: float = 0.0, interaction="z", field="x") -> TToperator:
    """J sum_k S_k S_{k+1} (S = the interaction axis) + h sum_k P_k (src/tt_operators.jl:219-237)."""
    a = _pauli_axis(interaction)
    return heisenberg_xyz_tto(d, jx=J if a == "x" else 0.0, jy=J if a == "y" else 0.0, jz=J if a == "z" else 0.0, lam=h, field=field)


def xxz_tto(d: int, J: float = 1.0, Delta: float = 1.0, h: float = 0.0, field="z") -> TToperator:
    """J (H_xx + H_yy) + J Delta H_zz + h H_field (src/tt_operators.jl:239-248)."""
    return heisenberg_xyz_tto(d, jx=J, jy=J, jz=J * Delta, lam=h, field=field)


def xxx_tto(d: int, J: float = 1.0, h: float = 0.0, field="z") -> TToperator:
    """J (H_xx + H_yy + H_zz) + h H_field (src/tt_operators.jl:250-259)."""
    return heisenberg_xyz_tto(d, jx=J, jy=J, jz=J, lam=h, field=field)


def xy_tto(d: int, jx: float = 1.0, jy: float = 1.0, h: float = 0.0, field="z") -> TToperator:
    """jx H_xx + jy H_yy + h H_field (src/tt_operators.jl:262-271)."""
    return heisenberg_xyz_tto(d, jx=jx, jy=jy, jz=0.0, lam=h, field=field)


# Pauli sums (src/tt_operators.jl:45-151): the one- and two-site building blocks of the Hamiltonians above as operators of their own —
# what a measurement such as the magnetisation sum_k Z_k contracts against a state (device.expect).
def pauli_matrix(mu, dtype=np.float64) -> np.ndarray:
    """The Pauli matrix of axis x or z (src/tt_operators.jl:45-54).  sigma_y alone is complex: TTNError, as in _pauli_pair_factors —
    unless ``dtype=np.complex128``, which gives any of the three as a complex matrix."""
    a = _pauli_axis(mu)
    if _pauli_dtype(dtype):
        return {"x": _PAULI_X.astype(np.complex128), "y": _PAULI_Y.copy(), "z": _PAULI_Z.astype(np.complex128)}[a]
    if a == "y":
        from ._lib import TTNError
        raise TTNError("a single sigma_y factor is complex: only real (Float64) operators are offered")
    return (_PAULI_X if a == "x" else _PAULI_Z).copy()


def _complex_cores(out: TToperator) -> TToperator:
    out.tto_vec = [np.asfortranarray(c, dtype=np.complex128) for c in out.tto_vec]
    return out


def pauli_sum_tto(mu, d: int, dtype=np.float64) -> TToperator:
    """H_mu = sum_k I (x) ... (x) P_mu (x) ... (x) I on d spin-1/2 sites, open boundaries, ranks [1, 2, ..., 2, 1]
    (src/tt_operators.jl:75-107): bond state 1 = "P not placed yet", bond state 0 = "placed"; d == 1 is the single core P.
    ``dtype=np.complex128``: complex cores, any axis (sigma_y included)."""
    assert d >= 1, "number of spin sites must be at least 1"
    cplx = _pauli_dtype(dtype)
    P, Id = pauli_matrix(mu, dtype), np.eye(2)
    if d == 1:
        out = zeros_tto((2,), [1, 1])
        if cplx:
            _complex_cores(out)
        out.tto_vec[0][:, :, 0, 0] = P
        return out
    out = zeros_tto((2,) * d, [1] + [2] * (d - 1) + [1])
    if cplx:
        _complex_cores(out)
    c = out.tto_vec[0]
    c[:, :, 0, 0], c[:, :, 0, 1] = P, Id
    for k in range(1, d - 1):
        c = out.tto_vec[k]
        c[:, :, 0, 0], c[:, :, 1, 0], c[:, :, 1, 1] = Id, P, Id
    c = out.tto_vec[d - 1]
    c[:, :, 0, 0], c[:, :, 1, 0] = Id, P
    return out


def pauli_pair_sum_tto(mu, nu, d: int, dtype=np.float64) -> TToperator:
    """H_{mu,nu} = sum_k I (x) ... (x) P_mu (x) P_nu (x) ... (x) I (sites k, k + 1), open boundaries, ranks [1, 3, ..., 3, 1]
    (src/tt_operators.jl:118-148): bond state 2 = "nothing placed", 1 = "P_mu placed, P_nu is due", 0 = "both placed".  Mixed pairs
    with one sigma_y are complex: TTNError; (y, y) is real.  ``dtype=np.complex128``: complex cores, all nine pairs."""
    assert d >= 2, "nearest-neighbor Pauli pair sum needs at least 2 spin sites"
    cplx = _pauli_dtype(dtype)
    if cplx and not (_pauli_axis(mu) == "y" and _pauli_axis(nu) == "y"):      # (y, y) keeps its real factors, as in the reference
        P1, P2 = pauli_matrix(mu, dtype), pauli_matrix(nu, dtype)
    else:
        P1, P2 = _pauli_pair_factors(mu, nu)
    Id = np.eye(2)
    out = zeros_tto((2,) * d, [1] + [3] * (d - 1) + [1])
    if cplx:
        _complex_cores(out)
    c = out.tto_vec[0]
    c[:, :, 0, 1], c[:, :, 0, 2] = P1, Id
    for k in range(1, d - 1):
        c = out.tto_vec[k]
        c[:, :, 0, 0], c[:, :, 1, 0], c[:, :, 2, 1], c[:, :, 2, 2] = Id, P2, P1, Id
    c = out.tto_vec[d - 1]
    c[:, :, 0, 0], c[:, :, 1, 0] = Id, P2
    return out


def H_mu(mu, d: int, dtype=np.float64) -> TToperator:
    """Alias of pauli_sum_tto (src/tt_operators.jl:150)."""
    return pauli_sum_tto(mu, d, dtype)


def H_munu(mu, nu, d: int, dtype=np.float64) -> TToperator:
    """Alias of pauli_pair_sum_tto (src/tt_operators.jl:151)."""
    return pauli_pair_sum_tto(mu, nu, d, dtype)


# ---------------------------------------------------------------------------------------------
# QTT Fourier transform — src/tt_transformations.jl (arXiv:2404.03182): Chebyshev-Lobatto interpolation of the phase in every core.
# ---------------------------------------------------------------------------------------------
def _sincospi(x: float):
    """(sin(pi x), cos(pi x)) with the argument reduced exactly first, so that integers and half-integers give exact zeros and ones
    as Julia's sinpi / cospi / cispi do."""
    r = math.remainder(x, 2.0)                      # exact, in [-1, 1]
    if abs(r) <= 0.5:
        return math.sin(math.pi * r), math.cos(math.pi * r)
    t = math.copysign(1.0, r) - r                   # exact (Sterbenz): sin(pi r) = sin(pi t), cos(pi r) = -cos(pi t)
    return math.sin(math.pi * t), -math.cos(math.pi * t)


def _cheb_lobatto_grid(K: int):
    """cheb_lobatto_grid(K) (:6-11): nodes c_j = (1 - cos(pi j / K)) / 2 in [0, 1] and barycentric weights."""
    c = np.array([0.5 * (1.0 - _sincospi(j / K)[1]) for j in range(K + 1)])
    w = np.array([(0.5 if j in (0, K) else 1.0) * (-1.0) ** j for j in range(K + 1)])
    return c, w


def _lagrange_eval(c: np.ndarray, w: np.ndarray, alpha: int, x: float) -> float:
    """lagrange_eval (:13-24): the barycentric form; 1 within 1e-14 of the node itself."""
    xa = float(c[alpha])
    if abs(x - xa) <= 1.0e-14:
        return 1.0
    with np.errstate(divide="ignore"):
        num = w[alpha] / np.float64(x - xa)
        denom = np.float64(0.0)
        for j in range(len(c)):
            denom = denom + w[j] / np.float64(x - c[j])
    return float(num / denom)


def fourier_qtto(d: int, sign: float = -1.0, K: int = 25, normalize: bool = True) -> TToperator:
    """fourier_qtto(d; sign = -1.0, K = 25, normalize = true) — src/tt_transformations.jl:38-77: the discrete Fourier transform of 2^d
    points as a ComplexF64 TToperator of ranks [1, K + 1, ..., K + 1, 1]; the output comes in bit-reversed order (reverse_qtt_bits).
    Core entries A[s, t, a, b] = L_a((s + c_b) / 2) cispi(sign (s + c_b) t); the first core sums over a, the last keeps b = 1;
    ``normalize`` scales the first core by 1 / sqrt(2^d).  Host code (NumPy), evaluated once per problem.  d = 1 reproduces the
    reference literally: its single core is the LAST core (2, 2, K + 1, 1) while tto_rks says [1, 1]."""
    assert d >= 1
    c, w = _cheb_lobatto_grid(K)
    r = K + 1
    A = np.zeros((2, 2, r, r), dtype=np.complex128, order="F")
    for al in range(r):
        for be in range(r):
            for sg in range(2):
                L = _lagrange_eval(c, w, al, 0.5 * (sg + c[be]))
                for ta in range(2):
                    sn, cs = _sincospi(sign * (sg + c[be]) * ta)
                    A[sg, ta, al, be] = complex(L * cs, L * sn)          # real * cispi(...)
    AL = np.zeros((2, 2, 1, r), dtype=np.complex128, order="F")
    for be in range(r):
        for sg in range(2):
            for ta in range(2):
                acc = complex(0.0, 0.0)
                for al in range(r):
                    acc = acc + complex(A[sg, ta, al, be])
                AL[sg, ta, 0, be] = acc
    AR = np.array(A[:, :, :, :1], order="F")
    cores = [AL] + [A.copy(order="F") for _ in range(max(d - 2, 0))] + [AR]
    if d == 1:
        cores = [AR]
    if normalize:
        cores[0] = np.asfortranarray(cores[0] * (1.0 / math.sqrt(2.0 ** d)))
    return TToperator(d, cores, (2,) * d, [1] + [r] * (d - 1) + [1], [0] * d)


def reverse_qtt_bits(x: TTvector) -> TTvector:
    """reverse_qtt_bits(x) — src/tt_transformations.jl:79-86: the sites in reverse order, each core with its two bond indices exchanged."""
    vec = [np.asfortranarray(np.transpose(cr, (0, 2, 1))) for cr in reversed(x.ttv_vec)]
    rks = [1] + list(reversed(x.ttv_rks[1:-1])) + [1]
    return TTvector(x.N, vec, tuple(reversed(x.ttv_dims)), rks, list(reversed(x.ttv_ot)))


def _ttv_decomp_host(tensor: np.ndarray, tol: float = 1.0e-12) -> TTvector:
    """ttv_decomp(tensor; index = 1, tol) (src/tt_tools.jl:186-252) with LAPACK on the host, for complex tensors: the right-to-left
    hierarchical SVD, singular values below tol (absolute) dropped, gauge flags [0, 1, ..., 1]."""
    dims = tuple(int(v) for v in tensor.shape)
    d = len(dims)
    rks = [1] * (d + 1)
    vec: list = [None] * d
    cur = np.asarray(tensor)
    for i in range(d, 1, -1):
        cur = np.reshape(cur, (-1, dims[i - 1] * rks[i]), order="F")
        u, sv, vt = np.linalg.svd(cur, full_matrices=False)
        r = int(np.count_nonzero(sv >= tol))
        rks[i - 1] = r
        vec[i - 1] = np.asfortranarray(np.transpose(np.reshape(vt[:r, :], (r, dims[i - 1], rks[i]), order="F"), (1, 0, 2)))
        cur = u[:, :r] * sv[None, :r]
    vec[0] = np.asfortranarray(np.reshape(cur, (dims[0], 1, rks[1]), order="F"))
    return TTvector(d, vec, dims, rks, [0] + [1] * (d - 1))


def function_to_qtt_uniform(f, d: int) -> TTvector:
    """function_to_qtt_uniform(f, d) — src/qtt_tools.jl:73-82: the samples f(n / 2^d), n = 0 .. 2^d - 1, as a QTT whose site 1 carries
    the LEAST significant bit of n, by ttv_decomp of the 2 x ... x 2 tensor (tol 1e-12).  Real samples are decomposed on the device
    (qtt.ttv_decomp, Float64).  Complex samples are decomposed on the HOST (NumPy's LAPACK SVD): the device decomposition is Float64
    only, and a real-part + i imaginary-part sum would double the ranks."""
    N = 2 ** d
    y = np.array([f(n / N) for n in range(N)])
    A = np.reshape(y, (2,) * d, order="F")          # A[b_1, ..., b_d] with n = sum b_k 2^(k-1): Julia's digits(n, base = 2) as a CartesianIndex
    if np.iscomplexobj(A):
        return _ttv_decomp_host(A.astype(np.complex128))
    from .qtt import ttv_decomp
    return ttv_decomp(A.astype(np.float64))
