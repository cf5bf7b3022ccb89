"""CPU tests of the spectral constructors (no GPU): ``fourier_qtto``, ``reverse_qtt_bits``, ``function_to_qtt_uniform``.

The restatement of src/tt_transformations.jl in tests/fourier_reference.py is pinned to the reference's own unit tests
(test/test_tt_transformations.jl:43-127), the package's constructors to the restatement bit for bit, and the reference's "Spikes" test
(:6-41) is run through the ORACLE's ``apply`` — the device runs it in tests/test_gpu_complex.py."""
import math

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import fourier_reference as FR
from tests.helpers import to_oracle


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    return ttn_amd


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- the reference's known answers on the restatement (test_tt_transformations.jl:43-127) ----
def test_cheb_lobatto_grid():
    K = 4
    P = FR.cheb_lobatto_grid(K)
    assert len(P.grid) == K + 1 and P.grid.dtype == np.float64
    assert len(P.w) == K + 1 and P.w.dtype == np.float64
    assert abs(P.grid[0]) <= 1e-14 and abs(P.grid[-1] - 1.0) <= 1e-14
    assert abs(abs(P.w[0]) - 0.5) <= 1e-14 and abs(abs(P.w[-1]) - 0.5) <= 1e-14
    for j in range(K + 1):
        assert P.w[j] == pytest.approx((0.5 if j in (0, K) else 1.0) * (-1.0) ** j)


def test_lagrange_eval():
    K = 4
    P = FR.cheb_lobatto_grid(K)
    for a in range(K + 1):
        assert abs(FR.lagrange_eval(P, a, P.grid[a]) - 1.0) <= 1e-12
        for b in range(K + 1):
            if b != a:
                assert abs(FR.lagrange_eval(P, a, P.grid[b])) <= 1e-12
    for x in np.linspace(0.0, 1.0, 10):
        assert abs(sum(FR.lagrange_eval(P, a, float(x)) for a in range(K + 1)) - 1.0) <= 1e-12
    assert all(isinstance(FR.lagrange_eval(P, a, 0.3), float) for a in range(K + 1))


def test_qft_core_entry():
    K = 4
    P = FR.cheb_lobatto_grid(K)
    for a in range(K + 1):
        for b in range(K + 1):
            for s in range(2):
                for t in range(2):
                    val = FR.qft_core_entry(P, a, b, s, t, sign=-1.0)
                    assert isinstance(val, complex)
                    if t == 0:
                        expected = FR.lagrange_eval(P, a, 0.5 * (s + P.grid[b]))
                        assert abs(val.real - expected) <= 1e-12 and abs(val.imag) <= 1e-12
                    assert abs(val) <= 1.0 + 1e-12
    for a in range(K + 1):
        expected = FR.lagrange_eval(P, a, 0.5 * (0 + P.grid[a]))
        assert abs(FR.qft_core_entry(P, a, a, 0, 0, sign=-1.0) - expected) <= 1e-12


# ---- the package's constructors against the restatement ----
@pytest.mark.parametrize("d", [1, 2, 6])
@pytest.mark.parametrize("K", [4, 25])
@pytest.mark.parametrize("sign", [-1.0, 1.0])
@pytest.mark.parametrize("normalize", [True, False])
def test_fourier_qtto_equals_restatement(T, d, K, sign, normalize):
    got = T.fourier_qtto(d, sign=sign, K=K, normalize=normalize)
    ref = FR.fourier_qtto(d, sign=sign, K=K, normalize=normalize)
    assert got.N == d and tuple(got.tto_dims) == (2,) * d
    assert got.tto_rks == [1] + [K + 1] * (d - 1) + [1] == ref.tto_rks
    assert got.tto_ot == [0] * d
    for g, r in zip(got.tto_vec, ref.tto_vec):
        assert g.dtype == np.complex128 and g.shape == r.shape
        assert np.array_equal(_bits(np.ascontiguousarray(g)), _bits(np.ascontiguousarray(r)))


def test_fourier_qtto_is_the_dft(T):
    """F (normalised) applied to e_n is column n of the unitary DFT matrix, output bits reversed: a direct check of the operator."""
    d = 4
    F = to_oracle(T.fourier_qtto(d, K=25))
    M = np.zeros((2 ** d, 2 ** d), dtype=complex)
    for n in range(2 ** d):
        e = np.zeros(2 ** d)
        e[n] = 1.0
        x = FR.ttv_decomp_any(np.reshape(e, (2,) * d, order="F"), tol=1e-14)
        M[:, n] = FR.matricize_vector(O.apply(F, x))
    W = np.exp(-2j * np.pi * np.outer(np.arange(2 ** d), np.arange(2 ** d)) / 2 ** d) / math.sqrt(2 ** d)
    assert np.max(np.abs(M - W)) < 1e-12


def test_reverse_qtt_bits(T):
    rng = np.random.default_rng(5)
    dims, rks = (2, 3, 2, 4), [1, 2, 5, 3, 1]
    vec = [np.asfortranarray(rng.standard_normal((dims[k], rks[k], rks[k + 1])) + 1j * rng.standard_normal((dims[k], rks[k], rks[k + 1])))
           for k in range(4)]
    x = T.TTvector(4, vec, dims, rks, [1, 0, -1, -1])
    y = T.reverse_qtt_bits(x)
    assert y.ttv_dims == tuple(reversed(dims)) and y.ttv_rks == [1, 3, 5, 2, 1] and y.ttv_ot == [-1, -1, 0, 1]
    ref = FR.reverse_qtt_bits(to_oracle(x))
    for g, r in zip(y.ttv_vec, ref.ttv_vec):
        assert g.shape == r.shape and np.array_equal(g, r)
    z = T.reverse_qtt_bits(y)
    assert z.ttv_dims == x.ttv_dims and z.ttv_rks == x.ttv_rks and z.ttv_ot == x.ttv_ot
    for g, r in zip(z.ttv_vec, x.ttv_vec):
        assert np.array_equal(_bits(np.ascontiguousarray(g)), _bits(np.ascontiguousarray(r)))
    # the dense tensor has its axes reversed (to rounding: the contraction runs in the other order)
    dense = FR._dense(to_oracle(x))
    assert np.allclose(FR._dense(to_oracle(y)), np.transpose(dense, (3, 2, 1, 0)), rtol=1e-13, atol=1e-13 * np.max(np.abs(dense)))


def test_function_to_qtt_uniform_complex_on_the_host(T):
    """complex samples are decomposed on the host: least significant bit on site 1, the samples reproduced to the SVD threshold"""
    d = 7
    f = lambda x: np.exp(2j * np.pi * 3 * x) + 0.5 * np.exp(-2j * np.pi * 5 * x) * (1 + x)
    x = T.function_to_qtt_uniform(f, d)
    assert np.iscomplexobj(x.ttv_vec[0]) and x.ttv_ot == [0] + [1] * (d - 1)
    ref = FR.function_to_qtt_uniform(f, d)
    assert x.ttv_rks == ref.ttv_rks
    y = FR.samples(f, d)
    assert np.max(np.abs(np.reshape(FR._dense(to_oracle(x)), -1, order="F") - y)) < 1e-11
    # qtt_to_vector takes complex trains (site 1 = most significant bit): the bit-reversed train gives the samples in order
    assert np.max(np.abs(T.qtt_to_vector(T.reverse_qtt_bits(x)) - y)) < 1e-11


def test_complex_refused_where_float64_only(T):
    """orthogonalize and the Float64-only paths raise on complex input instead of dropping the imaginary part (no device needed:
    the check runs before the library is loaded)"""
    x = T.function_to_qtt_uniform(lambda t: np.exp(2j * np.pi * t), 4)
    with pytest.raises(TypeError, match="complex"):
        T.orthogonalize(x)
    with pytest.raises(TypeError, match="complex"):
        T.ttv_decomp(np.ones((2, 2, 2)) * 1j)
    with pytest.raises(TypeError, match="complex"):
        T.tt._f(x.ttv_vec[0])


# ---- the reference's "Spikes" test through the oracle's apply (test_tt_transformations.jl:6-41) ----
def test_spikes_through_the_oracle(T):
    d, K, r = 10, 50, 12
    coeffs, f = FR.spikes_problem(d, K, r)
    F = to_oracle(T.fourier_qtto(d, K=K, sign=-1.0, normalize=True))
    x = to_oracle(T.function_to_qtt_uniform(f, d))
    spec = FR.matricize_vector(O.apply(F, x))
    e1, e2 = FR.spikes_errors(spec, coeffs, d)
    print("spikes (oracle apply): e1 = %.3e, e2 = %.3e" % (e1, e2))
    assert e1 < 1.0e-8
    assert e2 < 1.0e-10
