"""Grid transfer without a GPU: the three prolongation constructors and the rectangular apply's NumPy restatement
(tests/rect_reference.py) pinned to the reference's own testsets (test/test_tt_operators.jl:404-523), the host helpers those testsets
are written with, the host-side regrouping of rectangular cores, the ctypes table of include/ttn_rect.h, and the refusals that are
decided before the library touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import rect_reference as R
from tests.helpers import to_oracle, to_product

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import __graft_entry__ as g
    g.build()
    import ttn_amd
    return ttn_amd


def _same_operator(got, ref):
    assert got.N == ref.N and tuple(got.tto_dims) == tuple(ref.tto_dims)
    assert list(got.tto_rks) == list(ref.tto_rks) and list(got.tto_ot) == list(ref.tto_ot)
    for a, b in zip(got.tto_vec, ref.tto_vec):
        assert np.asarray(a).shape == np.asarray(b).shape
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ---- constructors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 5])
def test_qtto_prolongation_cores(T, d):
    _same_operator(T.qtto_prolongation(d), R.qtto_prolongation(d))


def test_qtto_prolongation_reference_entries(T):
    """test/test_tt_operators.jl:430-433, through the oracle's qtto_to_matrix."""
    d = 3
    M = O.qtto_to_matrix(to_oracle(T.qtto_prolongation(d)))
    P = R.prolongation_matrix(d)
    for i, j in ((0, 0), (0, 2), (0, 3), (1, 0)):
        assert M[i, j] == P[i, j]
    with pytest.raises(AssertionError, match="Dimension must be at least 2"):
        T.qtto_prolongation(1)


@pytest.mark.parametrize("d", [1, 2, 3, 5])
def test_rectangular_constructor_cores(T, d):
    _same_operator(T.qtto_constant_prolongation(d), R.qtto_constant_prolongation(d))
    _same_operator(T.qtto_linear_prolongation(d), R.qtto_linear_prolongation(d))


@pytest.mark.parametrize("name", ["qtto_constant_prolongation", "qtto_linear_prolongation"])
def test_rectangular_constructor_shape_facts(T, name):
    """:449-452 and :493-496."""
    d = 3
    P = getattr(T, name)(d)
    assert isinstance(P, T.TToperator)
    assert P.N == d + 1
    assert P.tto_dims == (2,) * (d + 1)
    assert P.tto_vec[-1].shape[1] == 1
    assert len(P.tto_vec) == d + 1 and len(P.tto_rks) == d + 2 and P.tto_ot == [0] * (d + 1)
    for k, c in enumerate(P.tto_vec):
        assert c.shape == (2, 1 if k == d else 2, P.tto_rks[k], P.tto_rks[k + 1])
    with pytest.raises(AssertionError, match="Dimension must be at least 1"):
        getattr(T, name)(0)


def test_linear_prolongation_ranks(T):
    assert T.qtto_linear_prolongation(1).tto_rks == [1, 2, 1]
    assert T.qtto_linear_prolongation(2).tto_rks == [1, 5, 2, 1]          # identity (1) + average (1 + 3); the last bond: one per branch
    assert T.qtto_linear_prolongation(6).tto_rks == [1, 5, 5, 5, 5, 5, 2, 1]


@pytest.mark.parametrize("d", [1, 2, 3])
def test_dense_forms_are_the_reference_matrices(T, d):
    """The cores of the two rectangular operators contracted to a (2^(d+1), 2^d) matrix: entry for entry the reference's
    constant_prolongation_matrix / linear_prolongation_matrix (every entry is a sum of products of 0, 1/2 and 1: exact)."""
    assert np.array_equal(R.rect_to_matrix(to_oracle(T.qtto_constant_prolongation(d))), R.constant_prolongation_matrix(d))
    assert np.array_equal(R.rect_to_matrix(to_oracle(T.qtto_linear_prolongation(d))), R.linear_prolongation_matrix(d))


# ---- the restatement of the rectangular apply -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 5])
def test_restated_apply_is_the_dense_product(d):
    rng = np.random.default_rng(d)
    u = O.rand_tt((2,) * d, 3, rng)
    ud = O.qtt_to_vector(u)
    for P, Pd in ((R.qtto_constant_prolongation(d), R.constant_prolongation_matrix(d)), (R.qtto_linear_prolongation(d), R.linear_prolongation_matrix(d))):
        y = R.apply_rect(P, u)
        assert y.N == d + 1 and y.ttv_dims == (2,) * (d + 1) and y.ttv_ot == [0] * (d + 1)
        assert y.ttv_rks == R.out_ranks(P.tto_rks, d + 1, u.ttv_rks)
        ref = Pd @ ud
        assert np.allclose(O.qtt_to_vector(y), ref, rtol=0, atol=1e-14 * np.max(np.abs(ref)))


def test_restated_apply_with_the_singleton_in_the_middle():
    """qtto_linear_prolongation(2) ⊗ id_tto(3) on a 5-site train: ranks [1, 10, 6, 3, 3, 2, 1] from [1, 2, 3, 3, 2, 1], and the dense product."""
    rng = np.random.default_rng(7)
    P, I3 = R.qtto_linear_prolongation(2), O.id_tto(3)
    A = O.TToperator(6, P.tto_vec + I3.tto_vec, (2,) * 6, P.tto_rks[:-1] + I3.tto_rks, [0] * 6)
    rks = [1, 2, 3, 3, 2, 1]
    u = O.TTvector(5, [rng.standard_normal((2, rks[k], rks[k + 1])) for k in range(5)], (2,) * 5, rks, [0] * 5)
    y = R.apply_rect(A, u)
    assert y.ttv_rks == [1, 10, 6, 3, 3, 2, 1]
    ref = np.kron(R.linear_prolongation_matrix(2), np.eye(8)) @ O.qtt_to_vector(u)
    assert np.allclose(O.qtt_to_vector(y), ref, rtol=0, atol=1e-14 * np.max(np.abs(ref)))


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def test_qtt_basis_vector(T):
    for d in (1, 3, 4):
        for pos in range(1, 2 ** d + 1):
            e, ref = T.qtt_basis_vector(d, pos, 2.5), R.qtt_basis_vector(d, pos, 2.5)
            assert e.ttv_rks == [1] * (d + 1) and e.ttv_dims == (2,) * d and e.ttv_ot == [0] * d
            for a, b in zip(e.ttv_vec, ref.ttv_vec):
                assert np.array_equal(a, b)
            dense = np.zeros(2 ** d)
            dense[pos - 1] = 2.5
            assert np.array_equal(T.qtt_to_function(e), dense)
    assert np.array_equal(T.qtt_to_function(T.qtt_basis_vector(2, 3)), [0.0, 0.0, 1.0, 0.0])


def test_function_to_tensor_samples(T):
    """The sampling half of function_to_qtt (its ttv_decomp runs on the device: tests/test_gpu_prolongation.py).  The points are
    k / (2^d - 1) with site 1 the most significant bit, and a and b do not move them."""
    f = lambda x: np.cos(np.pi * x) + x * x
    for d in (1, 3, 5):
        got, ref = T.function_to_tensor(f, d), R.function_to_tensor(f, d)
        assert got.shape == (2,) * d and np.array_equal(got, ref)
        assert np.array_equal(T.function_to_tensor(f, d, a=-3.0, b=7.0), ref)
        grid = np.reshape(got, -1)                                          # C order: site 1 the most significant bit
        assert np.allclose(grid, f(np.arange(2 ** d) / (2 ** d - 1)), rtol=0, atol=1e-15)


# ---- host regrouping of rectangular cores -----------------------------------------------------------------------------------------------
def test_kron_and_concatenate_keep_rectangular_cores(T):
    P, I2, I3 = T.qtto_linear_prolongation(2), T.id_tto(2), T.id_tto(3)
    Py = T.kron(I2, P)
    assert Py.N == 5 and Py.tto_dims == (2,) * 5 and Py.tto_rks == [1, 1, 1, 5, 2, 1]
    assert [c.shape for c in Py.tto_vec] == [(2, 2, 1, 1), (2, 2, 1, 1), (2, 2, 1, 5), (2, 2, 5, 2), (2, 1, 2, 1)]
    Px = T.kron(P, I3)
    assert Px.N == 6 and Px.tto_rks == [1, 5, 2, 1, 1, 1, 1]
    assert [c.shape[1] for c in Px.tto_vec] == [2, 2, 1, 2, 2, 2]
    assert T.tt.rect_singleton_sites(Px) == [3] and T.tt.rect_singleton_sites(Py) == [5]
    Pc = T.concatenate(P, I3)
    for a, b in zip(Pc.tto_vec, Px.tto_vec):
        assert np.array_equal(a, b)
    dense = R.rect_to_matrix(to_oracle(Px))
    assert np.array_equal(dense, np.kron(R.linear_prolongation_matrix(2), np.eye(8)))
    two = T.kron(T.qtto_constant_prolongation(1), T.qtto_constant_prolongation(1))       # two singleton sites: a valid container
    assert T.tt.rect_singleton_sites(two) == [2, 4]


# ---- the C ABI of include/ttn_rect.h ------------------------------------------------------------------------------------------------------
def test_rect_header_and_ctypes_table_agree(T):
    hdr = open(os.path.join(ROOT, "include", "ttn_rect.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert {n for n, _ in protos} == set(T._lib.RECT_SIGNATURES)
    assert not set(T._lib.RECT_SIGNATURES) & set(T._lib.SIGNATURES)
    L = ctypes
    table = {"int64_t": L.c_int64, "int64_t*": L.POINTER(L.c_int64), "double**": L.POINTER(L.POINTER(L.c_double)),
             "ttn_rtto_t": L.c_void_p, "ttn_tt_t": L.c_void_p, "ttn_rtto_t*": L.POINTER(L.c_void_p)}
    lib = T._lib.lib()
    for name, args in protos:
        res, argt = T._lib.RECT_SIGNATURES[name]
        assert res is L.c_int and hasattr(lib, name)
        types = []
        for a in [x.strip() for x in args.split(",")]:
            t = re.sub(r"\s*[A-Za-z_][A-Za-z0-9_]*$", "", re.sub(r"\bconst\b", "", a).strip())
            types.append(re.sub(r"\s+", "", t))
        assert len(types) == len(argt), name
        for ct, at in zip(types, argt):
            want = table[ct]
            assert at is want or (hasattr(at, "_type_") and hasattr(want, "_type_") and at._type_ is want._type_), (name, ct)
    main = open(os.path.join(ROOT, "include", "ttn.h")).read()
    assert '#include "ttn_rect.h"' in main


# ---- refusals decided on the host -----------------------------------------------------------------------------------------------------
def test_apply_raises_the_reference_assertions(T):
    x3 = T.rand_tt((2, 2, 2), [1, 2, 2, 1], seed=1)
    P3 = T.qtto_linear_prolongation(3)
    with pytest.raises(AssertionError, match="Rectangular TToperator must have one additional output site"):
        T.apply(T.qtto_linear_prolongation(4), x3)
    with pytest.raises(AssertionError, match="Rectangular TToperator must have one additional output site"):
        T.qtto_linear_prolongation(1) * x3
    with pytest.raises(AssertionError, match="Rectangular TToperator must have exactly one singleton input site"):
        T.apply(T.Delta(4), x3)                                            # no singleton site
    with pytest.raises(AssertionError, match="Rectangular TToperator must have exactly one singleton input site"):
        T.kron(T.qtto_constant_prolongation(1), T.qtto_constant_prolongation(1))(x3)          # two
    with pytest.raises(AssertionError, match="Incompatible input dimensions"):
        P3 * T.rand_tt((2, 3, 2), [1, 2, 2, 1], seed=2)
    with pytest.raises(AssertionError, match="Input TTvector must have a closed right boundary rank"):
        P3 * T.rand_tt((2, 2, 2), [1, 2, 2, 2], seed=3)
    with pytest.raises(AssertionError, match="Incompatible dimensions"):      # a rectangular core in an operator of v's own length
        T.apply(T.TToperator(3, P3.tto_vec[1:], (2, 2, 2), P3.tto_rks[1:], [0] * 3), x3)


def test_complex_cores_are_refused(T):
    x3 = T.rand_tt((2, 2, 2), [1, 2, 2, 1], seed=1)
    P3 = T.qtto_linear_prolongation(3)
    Pc = T.TToperator(4, [c.astype(np.complex128) for c in P3.tto_vec], P3.tto_dims, P3.tto_rks, P3.tto_ot)
    with pytest.raises(TypeError, match="Float64 only"):
        Pc * x3
    xc = T.TTvector(3, [c.astype(np.complex128) for c in x3.ttv_vec], x3.ttv_dims, x3.ttv_rks, x3.ttv_ot)
    with pytest.raises(TypeError, match="Float64 only"):
        P3 * xc


def test_rank_capacity_helper(T):
    from ttn_amd import device as D
    assert D.rect_rank_capacity([1, 5, 2, 1, 1, 1, 1], 3, [1, 2, 3, 3, 2, 1]) == [1, 10, 6, 3, 3, 2, 1]
    assert D.rect_rank_capacity([1, 5, 2, 1], 3, [1, 64, 1]) == [1, 320, 2, 1]
    assert D.rect_rank_capacity([2, 3, 1], 1, [1, 4]) == R.out_ranks([2, 3, 1], 1, [1, 4]) == [2, 3, 4]
