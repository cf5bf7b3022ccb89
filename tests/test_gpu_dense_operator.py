"""The dense bridge for operators on the GPU: ttn_tto_to_dense, ttn_tto_decomp_dev and the Python layer on top (DeviceTTO.to_dense /
from_dense, tto_to_tensor, qtto_to_matrix, tto_decomp) against the CPU oracle (O.tto_to_tensor, O.qtto_to_matrix, O.rand_tto,
O.ttv_decomp through the restatement of tests/dense_operator_reference.py).

to_dense is checked entry by entry against the componentwise bound of a matrix-product chain, 8 eps N r_max tto_to_tensor(|A|) (the bound
of tests/test_gpu_qttnd.py: no hand-set number).  tto_decomp carries the tolerances of tests/test_gpu_ttv_decomp.py: ranks and gauge flags
exact on inputs with a spectral gap around tol, reconstruction 1e-12 max|dense|."""
import ctypes as C
import math

import numpy as np
import pytest

import ttn_amd as T
from oracle import tt_oracle as O
from tests import dense_operator_reference as R
from tests.helpers import to_oracle, to_product
from ttn_amd import _lib
from ttn_amd import device as D

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LAYOUTS = ("tensor", "matrix")


def _torch():
    from ttn_amd.tdvp import _dev
    return _dev()


def _abs_op(A):
    return O.TToperator(A.N, [np.abs(c) for c in A.tto_vec], A.tto_dims, list(A.tto_rks), list(A.tto_ot))


def _dense_bound(A):
    """entrywise 8 eps N r_max (|A_1| ... |A_N|): the componentwise bound of a matrix-product chain, from the oracle's own chain"""
    return 8 * EPS * A.N * max(A.tto_rks) * O.tto_to_tensor(_abs_op(A))


def _as_tensor(flat, dims, layout):
    """the flat device array of `layout` as the array of shape dims + dims"""
    N = int(np.prod(dims))
    if layout == "tensor":
        return np.reshape(flat, tuple(dims) * 2, order="F")
    return np.reshape(np.reshape(flat, (N, N), order="F"), tuple(dims) * 2)            # row / column in C order: site 1 most significant


def _check_to_dense(A, label):
    ref, bound = O.tto_to_tensor(A), _dense_bound(A)
    N = int(np.prod(A.tto_dims))
    h = D.DeviceTTO(to_product(A))
    out = {}
    for layout in LAYOUTS:
        flat = h.to_dense(layout).cpu().numpy()
        assert flat.shape == (N * N,)
        got = _as_tensor(flat, A.tto_dims, layout)
        if layout == "matrix":
            assert np.all(np.abs(np.reshape(flat, (N, N), order="F") - ref.reshape(N, N)) <= bound.reshape(N, N))
        err = np.abs(got - ref)
        print("to_dense", label, layout, "dims", A.tto_dims, "rks", A.tto_rks, "max err %.3e" % err.max(),
              "max err/bound %.3e" % np.max(err / np.maximum(bound, 1e-300)))
        assert np.all(err <= bound), (label, layout)
        out[layout] = flat
    h.free()
    return out


# ---- to_dense ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims, r, seed", [
    ((5,), 1, 1),                     # one site: the left side is empty
    ((2, 3, 2), 2, 1),                # mixed dims, a rank that is no multiple of 4
    ((3, 2, 2, 3), 3, 5),
    ((2, 1, 3), 2, 4),                # a site without digits
    ((65, 2), 3, 1),                  # n^2 = 4225 > the tile of 4096: the tile splits a site between its two digits
    ((2,) * 7, 5, 7),                 # 16 384 entries: four tiles, padded leading dimension
])
def test_to_dense_entrywise_both_layouts(dims, r, seed):
    _check_to_dense(R.random_operator(dims, r, seed), "random")
    D.status_all()


def test_to_dense_ill_scaled_cores():
    A = R.random_operator((2, 3, 2), 2, 1)
    for k, s in enumerate((1e8, 1e-6, 1e3)):
        A.tto_vec[k] = A.tto_vec[k] * s
    _check_to_dense(A, "ill-scaled")


@pytest.mark.parametrize("dims, r, seed", [((2, 3, 2), 2, 1), ((3, 2, 2, 3), 3, 5), ((2,) * 7, 5, 7)])
def test_to_dense_is_bitwise_the_train_route(dims, r, seed):
    """the tensor layout against what the library already offered: tto_to_ttv on the device, ttn_tt_to_dense in the merged-site layout,
    the permutation on the host.  Same chains, same cut, same K loop per entry: the same bits."""
    A = R.random_operator(dims, r, seed)
    d = len(dims)
    h = D.DeviceTTO(to_product(A))
    new = np.reshape(h.to_dense().cpu().numpy(), tuple(dims) * 2, order="F")
    t = h.to_tt()
    merged = t.to_dense().cpu().numpy()[0]
    t.free(), h.free()
    pairs = np.reshape(merged, [n for k in range(d) for n in (dims[k], dims[k])], order="F")       # axes x_1, y_1, x_2, y_2, ...
    old = np.transpose(pairs, list(range(0, 2 * d, 2)) + list(range(1, 2 * d, 2)))
    assert np.array_equal(new, old)


def test_to_dense_takes_a_pair_of_stride_tables():
    A = R.random_operator((2, 3, 2), 2, 1)
    ref, bound = O.tto_to_tensor(A), _dense_bound(A)
    xs, ys = T.operator_strides(A.tto_dims, "tensor")
    h = D.DeviceTTO(to_product(A))
    flat = h.to_dense((ys, xs)).cpu().numpy()                 # y digits fastest: the transposed operator in the tensor layout
    h.free()
    got = np.transpose(np.reshape(flat, (2, 3, 2) * 2, order="F"), [3, 4, 5, 0, 1, 2])
    assert np.all(np.abs(got - ref) <= bound)


def test_host_forms_of_the_reference():
    # qtto_to_matrix(Delta(4)) is the tridiagonal 2I - E+ - E-: small integers
    M = T.qtto_to_matrix(T.Delta(4))
    want = 2 * np.eye(16) - np.eye(16, k=1) - np.eye(16, k=-1)
    assert M.shape == (16, 16) and np.allclose(M, want, rtol=0, atol=1e-14)
    Md = T.qtto_to_matrix(T.Delta(4), device=True)
    assert tuple(Md.shape) == (16, 16) and np.array_equal(Md.cpu().numpy(), M)
    assert float(Md[1, 0]) == M[1, 0] == -1.0
    # test/test_tt_operations.jl:124-133: tto_to_tensor of a product reshapes to the product of the matrices
    dims, n = (2, 3), 6
    A, B = O.rand_tto(dims, 2, np.random.default_rng(21)), O.rand_tto(dims, 2, np.random.default_rng(22))
    Cm = np.reshape(T.tto_to_tensor(to_product(A) * to_product(B)), (n, n), order="F")
    A_mat, B_mat = np.reshape(O.tto_to_tensor(A), (n, n), order="F"), np.reshape(O.tto_to_tensor(B), (n, n), order="F")
    assert np.allclose(Cm, A_mat @ B_mat, rtol=0, atol=1e-12)
    got = T.tto_to_tensor(to_product(A))
    assert got.shape == dims + dims and np.all(np.abs(got - O.tto_to_tensor(A)) <= _dense_bound(A))
    D.status_all()


# ---- tto_decomp / from_dense ----------------------------------------------------------------------------------------------------------------
def _gauge_flags(d, index):
    return [-1] * (index - 1) + [0] + [1] * (d - index)


@pytest.mark.parametrize("dims, r, seed, rks", R.RANDOM_OPERATORS)
def test_tto_decomp_recovers_exact_ranks(dims, r, seed, rks):
    A = R.random_operator(dims, r, seed)
    assert list(A.tto_rks) == rks
    dense = O.tto_to_tensor(A)
    mx = np.max(np.abs(dense))
    tol = 1e-10 * mx
    d = len(dims)
    for index in sorted({1, d}):
        kept, dropped = R.spectral_gap(dense, index, tol)         # the input's gap around tol, on the CPU oracle
        assert kept >= 1e10 * tol and dropped <= 2e-5 * tol, (kept / tol, dropped / tol)
        ref = R.tto_decomp(dense, index=index, tol=tol)
        got = T.tto_decomp(dense, index=index, tol=tol)
        assert isinstance(got, T.TToperator) and got.N == d and tuple(got.tto_dims) == tuple(dims)
        assert list(got.tto_rks) == list(ref.tto_rks) == rks
        assert list(got.tto_ot) == list(ref.tto_ot) == _gauge_flags(d, index)
        err = np.max(np.abs(O.tto_to_tensor(to_oracle(got)) - dense))
        print("tto_decomp", dims, "index", index, "ranks", got.tto_rks, "err/max %.3e" % (err / mx))
        assert err <= 1e-12 * mx
    D.status_all()


@pytest.mark.parametrize("d, index", [(4, 1), (4, 2), (4, 4), (7, 1), (7, 4), (7, 7)])
def test_tto_decomp_of_the_dense_laplacian(d, index):
    """Delta(d) with the default tol; d = 7 is a multi-tile gather (the oracle alone reconstructs these to 1.2e-14)"""
    dense = O.tto_to_tensor(O.Delta(d))
    got = T.tto_decomp(dense, index=index)
    assert list(got.tto_rks) == [1] + [3] * (d - 1) + [1]
    assert list(got.tto_ot) == _gauge_flags(d, index)
    err = np.max(np.abs(O.tto_to_tensor(to_oracle(got)) - dense))
    print("tto_decomp Delta", d, index, "err %.3e" % err)
    assert err <= 1e-12 * np.max(np.abs(dense))
    D.status_all()


def test_tto_decomp_reference_cases_with_their_matvec():
    """test/test_tt_tools.jl:327-368 (see the CPU pin of the same inputs): full-rank inputs, reconstruction and the non-symmetric
    matvec at rtol 1e-10 — a wrong interleave of (x_k, y_k) fails the matvec"""
    tto = R.round_trip_operator()
    M = O.tto_to_tensor(tto)
    v8 = np.random.default_rng(14).standard_normal(8)
    cases = [((2, 2, 2), M, np.reshape(M, (8, 8), order="F"), v8)]
    for dims, seed in R.REFERENCE_MATVEC_CASES:
        A_mat, tensor, v = R.matvec_case(dims, seed)
        cases.append((dims, tensor, A_mat, v))
    for dims, tensor, A_mat, v in cases:
        n = A_mat.shape[0]
        A_tt = T.tto_decomp(tensor)
        assert A_tt.N == len(dims) and tuple(A_tt.tto_dims) == tuple(dims)
        assert R.isapprox(O.tto_to_tensor(to_oracle(A_tt)), tensor, 1e-10)
        assert R.isapprox(np.reshape(T.tto_to_tensor(A_tt), (n, n), order="F"), A_mat, 1e-10)
        v_tt = T.ttv_decomp(np.reshape(v, dims, order="F"))
        Av = O.ttv_to_tensor(to_oracle(A_tt * v_tt))
        assert R.isapprox(np.ravel(Av, order="F"), A_mat @ v, 1e-10)
    D.status_all()


def test_from_dense_matrix_layout_round_trip():
    torch, stream = _torch()
    M = np.random.default_rng(13).standard_normal((8, 8))
    assert not np.allclose(M, M.T)
    with torch.cuda.stream(stream):
        dt = torch.from_numpy(np.ascontiguousarray(np.ravel(M, order="F"))).to("cuda")
        keep = dt.clone()
    h = D.DeviceTTO.from_dense(dt, (2, 2, 2), layout="matrix")
    assert bool((dt == keep).all())                              # the input is only read
    A = h.download()
    assert list(h.ot) == [0, 1, 1] and A.tto_rks[0] == A.tto_rks[-1] == 1
    assert np.max(np.abs(O.qtto_to_matrix(to_oracle(A)) - M)) <= 1e-12 * np.max(np.abs(M))
    # ... and straight back on the device
    back = h.to_dense("matrix").cpu().numpy()
    assert np.max(np.abs(np.reshape(back, (8, 8), order="F") - M)) <= 1e-12 * np.max(np.abs(M))
    h.free()
    D.status_all()


def _normal_call_succeeds():
    D.status_all()
    y = T.tt_compress_(T.id_tto(6) * T.qtt_sin(6, lam=math.pi), 2)
    assert y.ttv_rks == [1, 2, 2, 2, 2, 2, 1]
    A = R.random_operator((2, 3, 2), 2, 1)
    assert np.all(np.abs(T.tto_to_tensor(to_product(A)) - O.tto_to_tensor(A)) <= _dense_bound(A))
    D.status_all()


def test_rank_cap_overflow_is_reported_and_leaves_the_library_usable():
    dims, r, seed, rks = R.RANDOM_OPERATORS[2]
    dense = O.tto_to_tensor(R.random_operator(dims, r, seed))
    tol = 1e-10 * np.max(np.abs(dense))
    with pytest.raises(T.TTNError, match="ttn error -5: ttn_tto_decomp_dev"):
        T.tto_decomp(dense, tol=tol, rank_cap=2)
    _normal_call_succeeds()
    assert list(T.tto_decomp(dense, tol=tol, rank_cap=3).tto_rks) == rks


# ---- refusals: argument checks that return before any launch -----------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    torch, stream = _torch()
    L = _lib.lib()
    dims = (2, 3, 2)
    A = to_product(R.random_operator(dims, 2, 1))
    h = D.DeviceTTO(A)
    with torch.cuda.stream(stream):
        out = torch.full((144,), -7.0, dtype=torch.float64, device="cuda")
    p = C.c_void_p(out.data_ptr())
    i3 = lambda v: (C.c_int64 * 3)(*v)
    xs, ys = T.operator_strides(dims, "tensor")
    assert L.ttn_tto_to_dense(None, None, None, p) == _lib.TTN_ERR_ARG
    assert L.ttn_tto_to_dense(h.h, None, None, None) == _lib.TTN_ERR_ARG
    for a, b in ((i3(xs), None), (None, i3(ys))):
        assert L.ttn_tto_to_dense(h.h, a, b, p) == _lib.TTN_ERR_ARG
        assert "ttn_tto_to_dense" in _lib.last_error() and "both" in _lib.last_error()
    for bx, by in (([1, 2, 6], [12, 24, 73]), ([2, 4, 12], [24, 48, 144]), ([1, 2, 6], [1, 2, 6]), ([0, 2, 6], [12, 24, 72]), ([1, 2, 6], [12, 24, 48]),
                   ([-1, 2, 6], [12, 24, 72])):
        assert L.ttn_tto_to_dense(h.h, i3(bx), i3(by), p) == _lib.TTN_ERR_ARG, (bx, by)
        assert "ttn_tto_to_dense" in _lib.last_error() and "mixed-radix" in _lib.last_error()
        _normal_call_succeeds()
    with pytest.raises(ValueError, match="mixed-radix"):
        h.to_dense(([1, 2, 6], [12, 24, 73]))
    # a ComplexF64 operator
    Z = T.TToperator(2, [np.ones((2, 2, 1, 1), dtype=complex, order="F")] * 2, (2, 2), [1, 1, 1], [0, 0])
    z = D.DeviceTTO(Z)
    assert L.ttn_tto_to_dense(z.h, None, None, p) == _lib.TTN_ERR_UNSUPPORTED
    assert "ttn_tto_to_dense" in _lib.last_error() and "ComplexF64" in _lib.last_error()
    with pytest.raises(T.TTNError, match="ttn_tto_to_dense"):
        z.to_dense()
    for f in (T.tto_to_tensor, T.qtto_to_matrix):
        with pytest.raises(TypeError, match="Float64 only"):
            f(Z)
    z.free()
    _normal_call_succeeds()
    # 4^14 = 2^28 entries
    big = D.DeviceTTO(T.Delta(14))
    assert L.ttn_tto_to_dense(big.h, None, None, p) == _lib.TTN_ERR_UNSUPPORTED
    assert "ttn_tto_to_dense" in _lib.last_error() and "2^27" in _lib.last_error()
    big.free()
    _normal_call_succeeds()
    D.sync()
    assert bool((out == -7.0).all())
    # ttn_tto_decomp_dev: the same buffer as the input of calls that are refused before they read it
    hh = C.c_void_p()
    dec = lambda d, dm, t, x, y, index, tol, cap, o=C.byref(hh): L.ttn_tto_decomp_dev(d, None if dm is None else (C.c_int64 * len(dm))(*dm), t, x, y, index, tol, cap, o)
    for args, code, word in (((3, dims, None, None, None, 1, 1e-12, 8), _lib.TTN_ERR_ARG, "null"),
                             ((3, None, p, None, None, 1, 1e-12, 8), _lib.TTN_ERR_ARG, "null"),
                             ((3, dims, p, None, None, 1, 1e-12, 8, None), _lib.TTN_ERR_ARG, "null"),
                             ((0, dims, p, None, None, 1, 1e-12, 8), _lib.TTN_ERR_ARG, "sites"),
                             ((3, dims, p, None, None, 0, 1e-12, 8), _lib.TTN_ERR_ARG, "index"),
                             ((3, dims, p, None, None, 4, 1e-12, 8), _lib.TTN_ERR_ARG, "index"),
                             ((3, dims, p, i3(xs), None, 1, 1e-12, 8), _lib.TTN_ERR_ARG, "both"),
                             ((3, dims, p, i3([1, 2, 6]), i3([12, 24, 73]), 1, 1e-12, 8), _lib.TTN_ERR_ARG, "mixed-radix"),
                             ((3, dims, p, None, None, 1, -1.0, 8), _lib.TTN_ERR_ARG, "tol"),
                             ((3, dims, p, None, None, 1, float("nan"), 8), _lib.TTN_ERR_ARG, "tol"),
                             ((3, dims, p, None, None, 1, 1e-12, 0), _lib.TTN_ERR_ARG, "rank_cap"),
                             ((3, (2, 0, 2), p, None, None, 1, 1e-12, 8), _lib.TTN_ERR_ARG, "dims"),
                             ((14, (2,) * 14, p, None, None, 1, 1e-12, 8), _lib.TTN_ERR_UNSUPPORTED, "2^27"),
                             ((1, (4097,), p, None, None, 1, 1e-12, 8), _lib.TTN_ERR_UNSUPPORTED, "4096"),
                             ((2, (100, 100), p, None, None, 1, 1e-12, 10000), _lib.TTN_ERR_UNSUPPORTED, "short side above 4096")):
        assert dec(*args) == code, args
        assert "ttn_tto_decomp_dev" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
        assert not hh.value
    _normal_call_succeeds()
    with torch.cuda.stream(stream):
        short = torch.zeros((10,), dtype=torch.float64, device="cuda")
    with pytest.raises(T.TTNError, match="10 entries for dims"):
        D.DeviceTTO.from_dense(short, dims)
    with pytest.raises(T.TTNError, match="CUDA tensor"):
        D.DeviceTTO.from_dense(torch.zeros((144,), dtype=torch.float64), dims)
    with pytest.raises(TypeError, match="Float64 only"):
        D.DeviceTTO.from_dense(short.to(torch.complex128), dims)
    for bad, exc in ((np.zeros((2, 2, 2)), AssertionError), (np.zeros((2, 3, 3, 2)), AssertionError)):
        with pytest.raises(exc):
            T.tto_decomp(bad)
    with pytest.raises(AssertionError):
        T.tto_decomp(np.zeros((2, 2, 2, 2)), index=0)
    D.sync()
    assert bool((out == -7.0).all())
    # a good call into the same buffer: the matrix layout
    mx, my = T.operator_strides(dims, "matrix")
    assert L.ttn_tto_to_dense(h.h, i3(mx), i3(my), p) == _lib.TTN_OK
    D.sync()
    ref = O.tto_to_tensor(to_oracle(A)).reshape(12, 12)
    assert np.allclose(np.reshape(out.cpu().numpy(), (12, 12), order="F"), ref, rtol=0, atol=1e-12)
    h.free()
    _normal_call_succeeds()
