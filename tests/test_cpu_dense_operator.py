"""CPU tests of the dense bridge for operators (no GPU): the NumPy restatement of tto_decomp (tests/dense_operator_reference.py) pinned to
the reference's own tests (test/test_tt_tools.jl:327-368), the stride tables of opalg.operator_strides against NumPy's index
arithmetic, the host-side refusals, and the C header against the ctypes table."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import dense_operator_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    return ttn_amd


# ---- the restatement against the reference's tests ---------------------------------------------------------------------------------------
def test_restatement_round_trip_of_tto_to_tensor():
    """:329-343: tto_decomp(tto_to_tensor(tto)) has N = 3, dims (2, 2, 2) and the same tensor (rtol 1e-10)"""
    tto = R.round_trip_operator()
    M = O.tto_to_tensor(tto)
    for index in (1, 2, 3):
        tto2 = R.tto_decomp(M, index=index)
        assert tto2.N == 3 and tto2.tto_dims == (2, 2, 2)
        assert tto2.tto_ot == [-1] * (index - 1) + [0] + [1] * (3 - index)
        assert np.allclose(O.tto_to_tensor(tto2), M, rtol=1e-10, atol=0)
    assert R.tto_decomp(M, tol=1e-10 * np.max(np.abs(M))).tto_rks == [1, 2, 2, 1]


@pytest.mark.parametrize("dims, seed", R.REFERENCE_MATVEC_CASES)
def test_restatement_reproduces_dense_non_symmetric_matvec(dims, seed):
    """:345-368: reshape(tto_to_tensor(A_tt), n, n) == A_mat and vec(ttv_to_tensor(A_tt * v_tt)) == A_mat * v (rtol 1e-10); a symmetric
    matrix would hide a wrong interleave, these are not symmetric"""
    A_mat, tensor, v = R.matvec_case(dims, seed)
    n = A_mat.shape[0]
    assert not np.allclose(A_mat, A_mat.T)
    A_tt = R.tto_decomp(tensor)
    assert A_tt.tto_dims == tuple(dims)
    assert np.allclose(np.reshape(O.tto_to_tensor(A_tt), (n, n), order="F"), A_mat, rtol=1e-10, atol=0)
    v_tt = O.ttv_decomp(np.reshape(v, dims, order="F"))
    Av = O.ttv_to_tensor(O.apply(A_tt, v_tt))
    assert np.allclose(np.ravel(Av, order="F"), A_mat @ v, rtol=1e-10, atol=0)


# ---- stride tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(2, 3, 2), (2, 2, 2)])
def test_operator_strides_equal_numpys_addresses(T, dims):
    N = int(np.prod(dims))
    d = len(dims)
    xs, ys = T.operator_strides(dims, "tensor")
    addr = R.address_table(dims, xs, ys)
    for idx in np.ndindex(*(dims + dims)):
        assert addr[idx] == np.ravel_multi_index(idx, dims + dims, order="F")
    xs, ys = T.operator_strides(dims, "matrix")
    addr = R.address_table(dims, xs, ys)
    for idx in np.ndindex(*(dims + dims)):
        row, col = np.ravel_multi_index(idx[:d], dims), np.ravel_multi_index(idx[d:], dims)       # C order: site 1 most significant
        assert addr[idx] == row + N * col
    assert sorted(addr.ravel()) == list(range(N * N))
    # a pair passes through
    assert T.operator_strides(dims, (xs, ys)) == (xs, ys)


def test_operator_strides_refuses_what_is_not_mixed_radix(T):
    for bad in (([1, 2, 6], [12, 24, 73]), ([2, 4, 12], [24, 48, 144]), ([1, 2, 6], [12, 24, 48]), ([1, 2, 6], [1, 2, 6]), ([0, 2, 6], [12, 24, 72])):
        with pytest.raises(ValueError, match="mixed-radix"):
            T.operator_strides((2, 3, 2), bad)
    with pytest.raises(ValueError, match="strides for 3 sites"):
        T.operator_strides((2, 3, 2), ([1, 2], [12, 24, 72]))
    with pytest.raises(ValueError, match="layout must be"):
        T.operator_strides((2, 3, 2), "rows")
    # sites of dimension 1 carry no digit: their strides are free
    assert T.operator_strides((2, 1, 3), ([1, 999, 2], [6, 7, 12])) == ([1, 999, 2], [6, 7, 12])


# ---- refusals that never reach the device ------------------------------------------------------------------------------------------------
def test_host_forms_refuse_before_any_device_work(T):
    with pytest.raises(AssertionError, match="even number of axes"):
        T.tto_decomp(np.zeros((2, 2, 2)))
    with pytest.raises(AssertionError, match="x and y dimensions differ"):
        T.tto_decomp(np.zeros((2, 3, 3, 2)))
    with pytest.raises(AssertionError, match="index must be in 1:d"):
        T.tto_decomp(np.zeros((2, 2, 2, 2)), index=0)
    with pytest.raises(AssertionError, match="index must be in 1:d"):
        T.tto_decomp(np.zeros((2, 2, 2, 2)), index=3)
    with pytest.raises(TypeError, match="Float64 only"):
        T.tto_decomp(np.zeros((2, 2), dtype=complex))
    Z = T.TToperator(2, [np.zeros((2, 2, 1, 1), dtype=complex, order="F")] * 2, (2, 2), [1, 1, 1], [0, 0])
    for f in (T.tto_to_tensor, T.qtto_to_matrix):
        with pytest.raises(TypeError, match="Float64 only"):
            f(Z)
        with pytest.raises(TypeError, match="rectangular"):
            f(T.qtto_linear_prolongation(2))
        with pytest.raises(TypeError):
            f(T.rand_tt((2, 2), [1, 2, 1], seed=1))
    with pytest.raises(AssertionError, match="must be 2"):
        T.qtto_to_matrix(T.TToperator(1, [np.zeros((3, 3, 1, 1), order="F")], (3,), [1, 1], [0]))


# ---- the C ABI of include/ttn_dense.h ----------------------------------------------------------------------------------------------------
def test_dense_header_and_ctypes_table_agree(T):
    hdr = open(os.path.join(ROOT, "include", "ttn_dense.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert {n for n, _ in protos} == set(T._lib.DENSE_SIGNATURES) == {"ttn_tto_to_dense", "ttn_tto_decomp_dev", "ttn_debug_dense_plan",
                                                                           "ttn_debug_gather_plan"}
    assert not set(T._lib.DENSE_SIGNATURES) & (set(T._lib.SIGNATURES) | set(T._lib.RECT_SIGNATURES))
    L = ctypes
    table = {"int64_t": L.c_int64, "int64_t*": L.POINTER(L.c_int64), "double": L.c_double, "double*": L.c_void_p, "ttn_tto_t": L.c_void_p,
             "ttn_tto_t*": L.POINTER(L.c_void_p)}
    lib = T._lib.lib()
    for name, args in protos:
        res, argt = T._lib.DENSE_SIGNATURES[name]
        assert res is L.c_int and hasattr(lib, name)
        types = []
        for a in [x.strip() for x in args.split(",")]:
            t = re.sub(r"\s*[A-Za-z_][A-Za-z0-9_]*$", "", re.sub(r"\bconst\b", "", a).strip())
            types.append(re.sub(r"\s+", "", t))
        assert len(types) == len(argt), name
        for ct, at in zip(types, argt):
            want = table[ct]
            assert at is want or (hasattr(at, "_type_") and hasattr(want, "_type_") and at._type_ is want._type_), (name, ct)
    assert '#include "ttn_dense.h"' in open(os.path.join(ROOT, "include", "ttn.h")).read()
    for name in ("operator_strides", "tto_to_tensor", "qtto_to_matrix", "tto_decomp"):
        assert name in T.__all__
