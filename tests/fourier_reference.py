"""NumPy restatement of the reference's spectral corner (src/tt_transformations.jl; src/qtt_tools.jl:73-82), on the oracle's
containers (oracle.tt_oracle.TToperator / TTvector).

Written function by function from the Julia source — ``cheb_lobatto_grid``, ``lagrange_eval``, ``qft_core_entry``, ``fourier_qtto``,
``reverse_qtt_bits``, ``function_to_qtt_uniform`` and the ``function_to_qtt_uniform_msb`` of test/test_tt_transformations.jl — in
scalar arithmetic and in the source's order of operations.  ``sinpi`` / ``cospi`` / ``cispi`` reduce their argument exactly before
they call libm, as Julia's do, so integers and half-integers give exact zeros and ones.
"""
import math

import numpy as np

from oracle import tt_oracle as O


def sincospi(x):
    r = math.remainder(x, 2.0)
    if abs(r) <= 0.5:
        return math.sin(math.pi * r), math.cos(math.pi * r)
    t = math.copysign(1.0, r) - r
    return math.sin(math.pi * t), -math.cos(math.pi * t)


def cispi(x):
    s, c = sincospi(x)
    return complex(c, s)


class LagrangePolynomials:
    def __init__(self, grid, w):
        self.grid, self.w = grid, w


def cheb_lobatto_grid(K):
    """:6-11"""
    c = np.array([0.5 * (1.0 - sincospi(j / K)[1]) for j in range(K + 1)])
    w = np.array([0.5 if (j == 0 or j == K) else 1.0 for j in range(K + 1)])
    w = w * np.array([(-1.0) ** j for j in range(K + 1)])
    return LagrangePolynomials(c, w)


def lagrange_eval(P, alpha, x):
    """:13-24 (isapprox(x, xα; atol = 1e-14, rtol = 0) is |x - xα| <= 1e-14)"""
    xa = float(P.grid[alpha])
    if abs(x - xa) <= 1.0e-14:
        return 1.0
    with np.errstate(divide="ignore"):
        num = P.w[alpha] / np.float64(x - xa)
        denom = np.float64(0.0)
        for j in range(len(P.grid)):
            denom = denom + P.w[j] / np.float64(x - P.grid[j])
    return float(num / denom)


def qft_core_entry(P, alpha, beta, sigma, tau, sign=-1.0):
    """:26-33"""
    cb = float(P.grid[beta])
    x = 0.5 * (sigma + cb)
    L = lagrange_eval(P, alpha, x)
    z = cispi(sign * (sigma + cb) * tau)
    return complex(L * z.real, L * z.imag)                      # Float64 * ComplexF64


def fourier_qtto(d, sign=-1.0, K=25, normalize=True):
    """:38-77, d = 1 included as the source has it (cores[1] = AL is overwritten by cores[d] = AR; rks = [1, 1])"""
    assert d >= 1
    P = cheb_lobatto_grid(K)
    r = K + 1
    A = np.zeros((2, 2, r, r), dtype=np.complex128)
    for a in range(K + 1):
        for b in range(K + 1):
            for s in range(2):
                for t in range(2):
                    A[s, t, a, b] = qft_core_entry(P, a, b, s, t, sign=sign)
    AL = np.zeros((2, 2, 1, r), dtype=np.complex128)
    for b in range(r):
        for s in range(2):
            for t in range(2):
                acc = complex(0.0, 0.0)
                for a in range(r):
                    acc += complex(A[s, t, a, b])
                AL[s, t, 0, b] = acc
    AR = np.zeros((2, 2, r, 1), dtype=np.complex128)
    AR[:, :, :, 0] = A[:, :, :, 0]
    cores = [None] * d
    cores[0] = AL
    for k in range(1, d - 1):
        cores[k] = A.copy()
    cores[d - 1] = AR
    if normalize:
        cores[0] = cores[0] * (1.0 / math.sqrt(2.0 ** d))         # inv(sqrt(ComplexF64(2^d))) has a zero imaginary part
    return O.TToperator(d, cores, (2,) * d, [1] + [r] * (d - 1) + [1], [0] * d)


def reverse_qtt_bits(x):
    """:79-86"""
    vec = [np.transpose(c, (0, 2, 1)).copy() for c in reversed(x.ttv_vec)]
    return O.TTvector(x.N, vec, tuple(reversed(x.ttv_dims)), [1] + list(reversed(x.ttv_rks[1:-1])) + [1], list(reversed(x.ttv_ot)))


def ttv_decomp_any(tensor, tol=1.0e-12):
    """ttv_decomp(tensor; index = 1, tol) (src/tt_tools.jl:186-252) for real or complex tensors (the oracle's casts to float):
    right-to-left hierarchical SVD, absolute threshold."""
    dims = tuple(int(v) for v in tensor.shape)
    d = len(dims)
    rks = [1] * (d + 1)
    vec = [None] * d
    cur = np.asarray(tensor)
    for i in range(d, 1, -1):
        cur = np.reshape(cur, (-1, dims[i - 1] * rks[i]), order="F")
        u, sv, vt = np.linalg.svd(cur, full_matrices=False)
        r = int(np.count_nonzero(sv >= tol))
        rks[i - 1] = r
        core = np.zeros((dims[i - 1], r, rks[i]), dtype=cur.dtype)
        for x in range(dims[i - 1]):
            core[x, :, :] = vt[:r, [dims[i - 1] * be + x for be in range(rks[i])]]
        vec[i - 1] = core
        cur = u[:, :r] * sv[None, :r]
    vec[0] = np.reshape(cur, (dims[0], 1, rks[1]), order="F")
    return O.TTvector(d, vec, dims, rks, [0] + [1] * (d - 1))


def samples(f, d):
    N = 2 ** d
    return np.array([f(n / N) for n in range(N)])


def function_to_qtt_uniform(f, d):
    """src/qtt_tools.jl:73-82: A[digits(n, base = 2) .+ 1] = f(n / N) — site 1 is the least significant bit — then ttv_decomp."""
    y = samples(f, d)
    A = np.zeros((2,) * d, dtype=y.dtype)
    for n in range(2 ** d):
        bits = tuple((n >> k) & 1 for k in range(d))
        A[bits] = y[n]
    return ttv_decomp_any(A)


function_to_qtt_uniform_msb = function_to_qtt_uniform          # test/test_tt_transformations.jl:8-17 has the same body under this name


def matricize_vector(x):
    """matricize(x, d) (src/tt_tools.jl:694-705): entry i of the dense vector is the tensor entry whose index is the binary expansion of
    i read from the MOST significant bit on site 1 — a row-major flattening of the 2 x ... x 2 tensor."""
    return np.reshape(_dense(x), -1, order="C")


def _dense(x):
    T = x.ttv_vec[0][:, 0, :]                                    # (n_1, r_1)
    for k in range(1, x.N):
        G = x.ttv_vec[k]                                          # (n, r_l, r_r)
        T = np.einsum("...a,nab->...nb", T, G)
    return T[..., 0]


def spikes_problem(d=10, K=50, r=12, seed=1234):
    """The inputs of the "Spikes" test (test/test_tt_transformations.jl:19-33) and examples/dft.jl: r random complex Fourier
    coefficients (a NumPy generator in place of Random.seed!(1234): the inequalities do not depend on the draw)."""
    rng = np.random.default_rng(seed)
    coeffs = rng.standard_normal(r) + 1j * rng.standard_normal(r)

    def f(x):
        return sum(coeffs[m] * cispi(2 * m * x) for m in range(r))
    return coeffs, f


def spikes_errors(spec, coeffs, d):
    """The two quantities the reference asserts on (:35-39): the error of the first r entries and the weight of the rest."""
    r = len(coeffs)
    scale = math.sqrt(2 ** d)
    e1 = np.linalg.norm(spec[:r] - scale * coeffs) / (scale * np.linalg.norm(coeffs))
    e2 = np.linalg.norm(spec[r:]) / np.linalg.norm(spec)
    return float(e1), float(e2)
