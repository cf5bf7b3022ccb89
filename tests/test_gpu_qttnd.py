"""The multi-dimensional QTT layer on the GPU: ttn_tt_to_dense, ttn_qtt_grid_points, ttn_ttv_decomp_dev and the Python layer on top
(function_to_qttv, qttv_to_array, reorder, qtt_laplacian, entanglemententropy) against the NumPy restatement of the reference
(tests/qttnd_reference.py, pinned to the reference's own known answers by tests/test_cpu_qttnd.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import ttn_amd as T
from oracle import tt_oracle as O
from tests import qttnd_reference as R
from tests.helpers import to_oracle, to_product
from ttn_amd import _lib
from ttn_amd import device as D

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ORDERINGS = ("serial", "interleaved")


def _torch():
    from ttn_amd.tdvp import _dev
    return _dev()


def _abs_train(x):
    return O.TTvector(x.N, [np.abs(c) for c in x.ttv_vec], x.ttv_dims, list(x.ttv_rks), list(x.ttv_ot))


def _dense_bound(x):
    """entrywise 8 eps N r_max (|G_1| ... |G_N|): the componentwise bound of a matrix-product chain, from the oracle's own chain"""
    return 8 * EPS * x.N * max(x.ttv_rks) * O.ttv_to_tensor(_abs_train(x))


def _check_dense(x, strides=None):
    """DeviceTT.to_dense of the oracle train x against O.ttv_to_tensor, entry by entry"""
    h = D.DeviceTT.from_host(to_product(x))
    got = h.to_dense(strides).cpu().numpy()[0]
    h.free()
    ref, bound = O.ttv_to_tensor(x), _dense_bound(x)
    if strides is None:
        got_t = np.reshape(got, x.ttv_dims, order="F")
    else:
        got_t = np.empty(x.ttv_dims)
        for idx in np.ndindex(*x.ttv_dims):
            got_t[idx] = got[sum(i * s for i, s in zip(idx, strides))]
    err = np.abs(got_t - ref)
    print("to_dense dims", x.ttv_dims, "rks", x.ttv_rks, "max err %.3e" % err.max(), "max err/bound %.3e" % np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound)
    return got_t


# ---- to_dense -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims, rks", [
    ((2, 3, 4, 2, 5), 4),
    ((7,), 1),
    ((3, 5), 3),
    ((5, 2), 2),
    ((2, 2, 2, 2, 2, 2), 1),
    ((4, 3, 2, 2), [1, 1, 1, 1, 1]),
    ((2, 2, 64), 4),                  # the cut falls behind the next-to-last site
    ((64, 2, 2), 4),                  # ... and behind the first one
    ((4096,), 1),                     # one site: the left side is empty (the only way to a cut at the very end)
    ((512, 2, 3), 3),                 # a dominant first site: the cut falls right behind it
    ((1, 1, 6), 1),                   # leading sites of dimension 1: the left side is empty with N > 1
    ((2, 1, 3, 1, 2), 2),
])
def test_to_dense_shapes(dims, rks):
    x = O.rand_tt(dims, rks, np.random.default_rng(len(dims) * 100 + dims[0]))
    _check_dense(x)


@pytest.mark.parametrize("r", [1, 7, 16, 64])
def test_to_dense_binary_d20(r):
    x = O.rand_tt((2,) * 20, r, np.random.default_rng(20 + r))
    _check_dense(x)


def test_to_dense_ill_scaled_train():
    # cores of very different magnitude: the bound scales with the chain of absolute values, no hand-set number
    x = O.rand_tt((2, 3, 4, 2, 5), 4, np.random.default_rng(9))
    for k, s in enumerate((1e8, 1e-6, 1.0, 1e5, 1e-9)):
        x.ttv_vec[k] = x.ttv_vec[k] * s
    _check_dense(x)


def test_to_dense_batch_of_three():
    dims = (2, 3, 4, 2, 5)
    xs = [O.rand_tt(dims, r, np.random.default_rng(30 + r)) for r in (2, 4, 3)]
    h = D.DeviceTT(dims, [1, 2, 4, 4, 4, 1], batch=3)
    for b, x in enumerate(xs):
        h.upload(b, to_product(x))
    got = h.to_dense().cpu().numpy()
    h.free()
    assert got.shape == (3, 240)
    for b, x in enumerate(xs):
        assert np.all(np.abs(np.reshape(got[b], dims, order="F") - O.ttv_to_tensor(x)) <= _dense_bound(x))


def test_to_dense_permuted_strides_on_mixed_dims():
    dims = (2, 3, 4, 2, 5)
    x = O.rand_tt(dims, 4, np.random.default_rng(41))
    # memory order of the sites, fastest first: 3, 5, 1, 4, 2 (1-based)
    order = [2, 4, 0, 3, 1]
    strides, s = [0] * 5, 1
    for k in order:
        strides[k] = s
        s *= dims[k]
    assert strides == [20, 80, 1, 40, 4]
    _check_dense(x, strides)
    # C order (last site fastest) is the transposed tensor
    c_strides = [120, 40, 10, 5, 1]
    got = _check_dense(x, c_strides)
    assert got.shape == dims


def test_to_dense_qtt_strides_both_orderings():
    for n_dims, bits in ((2, 5), (3, 3)):
        for ordering in ORDERINGS:
            x = O.rand_tt((2,) * (n_dims * bits), 5, np.random.default_rng(7))
            got = T.qttv_to_array(T.QTTvector(to_product(x), n_dims, bits, ordering))
            ref = R.qttv_to_array(R.QTTv(x, n_dims, bits, ordering))
            bound = R.qttv_to_array(R.QTTv(_abs_train(x), n_dims, bits, ordering)) * 8 * EPS * x.N * max(x.ttv_rks)
            assert got.shape == (2 ** bits,) * n_dims
            assert np.all(np.abs(got - ref) <= bound)
            dev = T.qttv_to_array(T.QTTvector(to_product(x), n_dims, bits, ordering), device=True)
            assert tuple(dev.shape) == got.shape and np.array_equal(dev.cpu().numpy(), got)
            assert float(dev[(1,) + (0,) * (n_dims - 1)]) == got[(1,) + (0,) * (n_dims - 1)]


def test_ttv_to_tensor_host_form():
    x = O.rand_tt((2, 3, 4, 2, 5), 4, np.random.default_rng(51))
    got = T.ttv_to_tensor(to_product(x))
    assert got.shape == (2, 3, 4, 2, 5)
    assert np.all(np.abs(got - O.ttv_to_tensor(x)) <= _dense_bound(x))


def _normal_call_succeeds():
    D.status_all()
    y = T.tt_compress_(T.id_tto(6) * T.qtt_sin(6, lam=math.pi), 2)
    assert y.ttv_rks == [1, 2, 2, 2, 2, 2, 1]
    x = O.rand_tt((2, 3, 2), 2, np.random.default_rng(1))
    assert np.all(np.abs(T.ttv_to_tensor(to_product(x)) - O.ttv_to_tensor(x)) <= _dense_bound(x))
    D.status_all()


def test_to_dense_refusals_leave_the_output_untouched():
    torch, stream = _torch()
    L = _lib.lib()
    dims = (2, 3, 4)
    x = to_product(O.rand_tt(dims, 2, np.random.default_rng(2)))
    h = D.DeviceTT.from_host(x)
    with torch.cuda.stream(stream):
        out = torch.full((24,), -7.0, dtype=torch.float64, device="cuda")
    p = C.c_void_p(out.data_ptr())
    bad_tables = [[1, 2, 7], [2, 4, 12], [1, 3, 6], [1, 2, 2], [0, 1, 2], [1, 2, 8], [-1, 2, 6], [6, 2, 1]]
    for st in bad_tables:
        assert L.ttn_tt_to_dense(h.h, (C.c_int64 * 3)(*st), p) == _lib.TTN_ERR_ARG, st
        assert "mixed-radix" in _lib.last_error()
        _normal_call_succeeds()
    assert L.ttn_tt_to_dense(h.h, None, None) == _lib.TTN_ERR_ARG
    with pytest.raises(T.TTNError, match="2 strides for 3 sites"):
        h.to_dense([1, 2])
    # a ComplexF64 handle is refused before any launch
    z = D.DeviceTT(dims, [1, 2, 2, 1], dtype=np.complex128)
    assert L.ttn_tt_to_dense(z.h, None, p) == _lib.TTN_ERR_UNSUPPORTED
    assert "ttn_tt_to_dense" in _lib.last_error() and "ComplexF64" in _lib.last_error()
    assert L.ttn_ttv_decomp_dev(z.h, p, 1, 1e-12) == _lib.TTN_ERR_UNSUPPORTED
    assert "ttn_ttv_decomp_dev" in _lib.last_error()
    with pytest.raises(T.TTNError):
        z.to_dense()
    _normal_call_succeeds()
    # more than 2^27 entries
    big = D.DeviceTT((2,) * 28, [1] * 29)
    assert L.ttn_tt_to_dense(big.h, None, p) == _lib.TTN_ERR_UNSUPPORTED
    _normal_call_succeeds()
    # a physical dimension above the tile size
    wide = D.DeviceTT((4097, 2), [1, 1, 1])
    assert L.ttn_tt_to_dense(wide.h, None, p) == _lib.TTN_ERR_UNSUPPORTED
    assert "4096" in _lib.last_error()
    wide.free()
    _normal_call_succeeds()
    D.sync()
    assert bool((out == -7.0).all())
    # the same buffer through a valid table: C order, last site fastest
    assert L.ttn_tt_to_dense(h.h, (C.c_int64 * 3)(12, 4, 1), p) == _lib.TTN_OK
    D.sync()
    assert np.allclose(out.cpu().numpy().reshape(dims), O.ttv_to_tensor(to_oracle(x)), rtol=0, atol=1e-12)
    for t in (h, z, big):
        t.free()


# ---- grid points --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a, b", [(0.0, 1.0), (-2.0, 3.5)])
@pytest.mark.parametrize("ordering", ORDERINGS)
def test_grid_points_bit_identical_to_numpy(a, b, ordering):
    torch, stream = _torch()
    L = _lib.lib()
    for n_dims, bits, first, count in ((2, 5, 0, 1024), (3, 4, 1000, 3000), (1, 7, 3, 100), (2, 10, (1 << 20) - 777, 777)):
        N = n_dims * bits
        h = (b - a) / (2 ** bits - 1)
        with torch.cuda.stream(stream):
            X = torch.empty((n_dims, count), dtype=torch.float64, device="cuda")
        _lib.check(L.ttn_qtt_grid_points(n_dims, bits, 1 if ordering == "interleaved" else 0, a, b, first, count, C.c_void_p(X.data_ptr())))
        D.sync()
        got = X.cpu().numpy()
        e = np.arange(first, first + count, dtype=np.int64)
        g = np.zeros((n_dims, count), dtype=np.int64)
        for site in range(1, N + 1):
            dim, level = R._dim_level(site, n_dims, bits, ordering)
            g[dim - 1] += ((e >> (site - 1)) & 1) * 2 ** (bits - 1 - level)
        ref = a + g * h
        assert np.array_equal(got.view(np.int64), ref.view(np.int64)), (n_dims, bits, first)
    with torch.cuda.stream(stream):
        X = torch.zeros((2, 8), dtype=torch.float64, device="cuda")
    p = C.c_void_p(X.data_ptr())
    for args in ((2, 5, 1, a, b, 1020, 8), (0, 5, 1, a, b, 0, 8), (2, 40, 1, a, b, 0, 8), (2, 5, 1, a, b, -1, 8)):
        assert L.ttn_qtt_grid_points(*args, p) == _lib.TTN_ERR_ARG
    D.sync()
    assert bool((X == 0).all())
    _normal_call_succeeds()


# ---- ttv_decomp_dev -----------------------------------------------------------------------------------------------------------------
def test_ttv_decomp_dev_is_bitwise_ttv_decomp():
    torch, stream = _torch()
    rng = np.random.default_rng(77)
    dims = (2, 3, 4, 2, 5)
    batch = 3
    tensors = np.stack([O.ttv_to_tensor(O.rand_tt(dims, 3, rng)) + 1e-3 * rng.standard_normal(dims) for _ in range(batch)])
    cap = [1, 2, 6, 10, 5, 1]
    for index in (1, 3):
        z1, z2 = D.DeviceTT(dims, cap, batch), D.DeviceTT(dims, cap, batch)
        T.qtt.ttv_decomp_(z1, tensors, index, 1e-12)
        flat = np.ascontiguousarray(np.stack([np.ravel(tensors[b], order="F") for b in range(batch)]))
        with torch.cuda.stream(stream):
            dt = torch.from_numpy(flat).to("cuda")
            keep = dt.clone()
        T.qtt.ttv_decomp_dev_(z2, dt, index, 1e-12)
        D.compress_status(z1), D.compress_status(z2)
        assert bool((dt == keep).all())                     # the input buffer is not modified
        for b in range(batch):
            a, c = z1.download(b), z2.download(b)
            assert a.ttv_rks == c.ttv_rks and a.ttv_ot == c.ttv_ot
            for ca, cc in zip(a.ttv_vec, c.ttv_vec):
                assert np.array_equal(ca, cc)
        z1.free(), z2.free()
    with torch.cuda.stream(stream):
        short = torch.zeros((10,), dtype=torch.float64, device="cuda")
    z = D.DeviceTT(dims, cap, batch)
    with pytest.raises(T.TTNError, match="entries for"):
        T.qtt.ttv_decomp_dev_(z, short)
    with pytest.raises(T.TTNError):
        T.qtt.ttv_decomp_dev_(z, torch.zeros((720,), dtype=torch.float64))          # a host tensor
    z.free()
    _normal_call_succeeds()


# ---- function_to_qttv ---------------------------------------------------------------------------------------------------------------
def _grid(bits, a=0.0, b=1.0):
    n = 2 ** bits
    h = (b - a) / (n - 1)
    return np.array([a + h * i for i in range(n)])


def _cases():
    import torch
    pi = math.pi
    g = _grid
    s = lambda bits: np.sin(pi * g(bits))
    return [
        # (name, n_dims, bits, a, b, scalar f, torch f on (P, n_dims), direct grid evaluation)
        ("sin 1d", 1, 4, 0.0, 1.0, lambda x: math.sin(pi * x[0]), lambda X: torch.sin(pi * X[:, 0]), s(4)),
        ("sin sin", 2, 3, 0.0, 1.0, lambda x: math.sin(pi * x[0]) * math.sin(pi * x[1]), lambda X: torch.sin(pi * X[:, 0]) * torch.sin(pi * X[:, 1]),
         s(3)[:, None] * s(3)[None, :]),
        ("sin sin sin", 3, 3, 0.0, 1.0, lambda x: math.sin(pi * x[0]) * math.sin(pi * x[1]) * math.sin(pi * x[2]),
         lambda X: torch.sin(pi * X[:, 0]) * torch.sin(pi * X[:, 1]) * torch.sin(pi * X[:, 2]), s(3)[:, None, None] * s(3)[None, :, None] * s(3)[None, None, :]),
        ("gaussian", 2, 5, 0.0, 1.0, lambda x: math.exp(-10 * ((x[0] - 0.3) ** 2 + (x[1] - 0.7) ** 2)),
         lambda X: torch.exp(-10 * ((X[:, 0] - 0.3) ** 2 + (X[:, 1] - 0.7) ** 2)), np.exp(-10 * ((g(5)[:, None] - 0.3) ** 2 + (g(5)[None, :] - 0.7) ** 2))),
        ("interval", 2, 4, -1.0, 2.0, lambda x: math.sin(x[0]) * math.cos(x[1]), lambda X: torch.sin(X[:, 0]) * torch.cos(X[:, 1]),
         np.sin(g(4, -1.0, 2.0))[:, None] * np.cos(g(4, -1.0, 2.0))[None, :]),
    ]


@pytest.mark.parametrize("case", range(5))
@pytest.mark.parametrize("ordering", ORDERINGS)
def test_function_to_qttv_reference_cases(case, ordering):
    name, n_dims, bits, a, b, f, ft, direct = _cases()[case]
    ref = R.function_to_qttv(f, n_dims, bits, ordering, a, b)
    ref_err = float(np.max(np.abs(R.qttv_to_array(ref) - direct)))
    tol = max(10 * ref_err, 1e-12)
    fn = lambda X: np.array([f(row) for row in X.cpu().numpy()])           # a NumPy f: it brings the points to the host itself
    for kind, fun in (("torch", ft), ("numpy", fn)):
        q = T.function_to_qttv(fun, n_dims, bits, ordering=ordering, a=a, b=b)
        assert isinstance(q, T.QTTvector) and (q.N, q.n_dims, q.bits_per_dim, q.ordering) == (n_dims * bits, n_dims, bits, ordering)
        assert q.ttv_ot == list(ref.ttv.ttv_ot)
        arr = T.qttv_to_array(q)
        err = float(np.max(np.abs(arr - direct)))
        print(name, ordering, kind, "ranks", q.ttv_rks, "ref ranks", ref.ttv.ttv_rks, "err %.3e ref err %.3e tol %.3e" % (err, ref_err, tol))
        assert arr.shape == (2 ** bits,) * n_dims
        assert err <= tol
        if name == "gaussian":
            assert q.ttv_rks == list(ref.ttv.ttv_rks)            # the Gaussian's spectrum is cut at tol where it has a gap
    D.status_all()


def test_function_to_qttv_orderings_agree():
    import torch
    ft = lambda X: torch.sin(math.pi * X[:, 0]) * torch.cos(math.pi * X[:, 1])
    a_il = T.qttv_to_array(T.function_to_qttv(ft, 2, 3, ordering="interleaved"))
    a_sr = T.qttv_to_array(T.function_to_qttv(ft, 2, 3, ordering="serial"))
    assert np.max(np.abs(a_il - a_sr)) < 1e-12


def test_separable_function_is_rank_one_in_serial_ordering():
    import torch
    bits = 6
    f = lambda x: math.exp(-x[0]) * math.exp(-x[1])
    q = T.function_to_qttv(lambda X: torch.exp(-X[:, 0]) * torch.exp(-X[:, 1]), 2, bits, ordering="serial")
    ref = R.function_to_qttv(f, 2, bits, "serial")
    assert q.ttv_rks == list(ref.ttv.ttv_rks)
    q_c = q.copy()
    T.qttnd.tt_compress_(q_c, 10, truncerr=1e-12)
    assert isinstance(q_c, T.QTTvector) and q_c.ordering == "serial"
    assert q_c.ttv_rks[bits] == 1 and max(q_c.ttv_rks) == 1
    g = _grid(bits)
    assert np.max(np.abs(T.qttv_to_array(q_c) - np.exp(-g)[:, None] * np.exp(-g)[None, :])) < 1e-10


@pytest.mark.parametrize("ordering", ORDERINGS)
def test_function_to_qttv_two_by_ten_bits(ordering):
    # 2^20 grid points: beyond what the reference's tests try; the restatement samples with the vectorised loop
    import torch
    bits = 10
    fv = lambda X: np.exp(-10 * ((X[:, 0] - 0.3) ** 2 + (X[:, 1] - 0.7) ** 2)) + 0.5 * np.sin(3 * X[:, 0]) * X[:, 1]
    ft = lambda X: torch.exp(-10 * ((X[:, 0] - 0.3) ** 2 + (X[:, 1] - 0.7) ** 2)) + 0.5 * torch.sin(3 * X[:, 0]) * X[:, 1]
    g = _grid(bits)
    direct = np.exp(-10 * ((g[:, None] - 0.3) ** 2 + (g[None, :] - 0.7) ** 2)) + 0.5 * np.sin(3 * g)[:, None] * g[None, :]
    ref = R.QTTv(O.ttv_decomp(R.sample_tensor_fast(fv, 2, bits, ordering)), 2, bits, ordering)
    st = R.grid_strides(2, bits, ordering)
    full = np.ravel(O.ttv_to_tensor(ref.ttv), order="F")
    e = np.arange(1 << 20)
    tgt = np.zeros(1 << 20, dtype=np.int64)
    for site in range(20):
        tgt += ((e >> site) & 1) * st[site]
    ref_arr = np.empty(1 << 20)
    ref_arr[tgt] = full
    ref_err = float(np.max(np.abs(np.reshape(ref_arr, (1024, 1024), order="F") - direct)))
    tol = max(10 * ref_err, 1e-12)
    q = T.function_to_qttv(ft, 2, bits, ordering=ordering)
    err = float(np.max(np.abs(T.qttv_to_array(q) - direct)))
    print("2x10 bits", ordering, "ranks", q.ttv_rks, "ref", ref.ttv.ttv_rks, "err %.3e ref err %.3e" % (err, ref_err))
    assert err <= tol
    D.status_all()


def test_function_to_qttv_refusals():
    import torch
    with pytest.raises(T.TTNError, match="non-finite value \\(chunk 0"):
        T.function_to_qttv(lambda X: 1.0 / (X[:, 0] - X[0, 0]), 2, 3)
    _normal_call_succeeds()
    with pytest.raises(T.TTNError, match="returned 5 values for 64 points \\(chunk 0"):
        T.function_to_qttv(lambda X: torch.zeros(5, dtype=torch.float64), 2, 3)
    _normal_call_succeeds()
    with pytest.raises(T.TTNError, match="complex"):
        T.function_to_qttv(lambda X: X[:, 0].to(torch.complex128), 2, 3)
    _normal_call_succeeds()


# ---- reorder (:182-205) ---------------------------------------------------------------------------------------------------------------
def test_reorder_round_trips():
    import torch
    bits = 3
    q_serial = T.function_to_qttv(lambda X: torch.sin(math.pi * X[:, 0]) * torch.cos(math.pi * X[:, 1]), 2, bits, ordering="serial")
    q_il = q_serial.reorder("interleaved")
    assert isinstance(q_il, T.QTTvector) and q_il.ordering == "interleaved"
    q_back = T.qttnd.reorder(q_il, "serial")
    assert q_back.ordering == "serial"
    arr_serial, arr_il, arr_back = T.qttv_to_array(q_serial), T.qttv_to_array(q_il), T.qttv_to_array(q_back)
    assert np.max(np.abs(arr_serial - arr_il)) < 1e-10
    assert np.max(np.abs(arr_serial - arr_back)) < 1e-10
    q_same = q_serial.reorder("serial")
    assert q_same.ordering == "serial"
    assert np.max(np.abs(T.qttv_to_array(q_same) - arr_serial)) < 1e-14
    D.status_all()


# ---- metadata-keeping arithmetic -----------------------------------------------------------------------------------------------------
def test_arithmetic_keeps_the_metadata():
    rng = np.random.default_rng(3)
    ttv, ttv2 = to_product(O.rand_tt((2,) * 6, 2, rng)), to_product(O.rand_tt((2,) * 6, 2, rng))
    tto = to_product(O.rand_tto((2,) * 6, 2, rng))
    q1, q2 = T.QTTvector(ttv, 2, 3, "interleaved"), T.QTTvector(ttv2, 2, 3, "interleaved")
    A = T.QTToperator(tto, 2, 3, "interleaved")
    a1, a2 = T.qttv_to_array(q1), T.qttv_to_array(q2)
    scale = max(np.max(np.abs(a1)), np.max(np.abs(a2)))
    for got, want in ((q1 + q2, a1 + a2), (q1 - q2, a1 - a2), (2.0 * q1, 2 * a1), (q1 * 2.0, 2 * a1), (q1 / 4.0, a1 / 4), (T.qttnd.hadamard(q1, q2), a1 * a2)):
        assert isinstance(got, T.QTTvector) and (got.n_dims, got.bits_per_dim, got.ordering) == (2, 3, "interleaved")
        assert np.max(np.abs(T.qttv_to_array(got) - want)) < 1e-12 * max(scale, scale * scale)
    assert abs(T.qttnd.dot(q1, q2) - np.sum(a1 * a2)) < 1e-12 * scale * scale * 64
    assert abs(T.qttnd.dot(q1, ttv2) - np.sum(a1 * a2)) < 1e-12 * scale * scale * 64
    assert abs(T.qttnd.norm(q1) - np.linalg.norm(a1)) < 1e-12 * scale * 8
    qo = T.qttnd.orthogonalize(q1)
    assert isinstance(qo, T.QTTvector) and qo.ordering == "interleaved"
    assert np.max(np.abs(T.qttv_to_array(qo) - a1)) < 1e-12 * scale
    # mixed forms return bare containers (:599-647)
    for got in (q1 + ttv2, ttv + q2, q1 - ttv2, ttv - q2, tto * q1, A * ttv):
        assert isinstance(got, T.TTvector) and not isinstance(got, T.QTTvector)
    for got in (A + tto, tto + A, A - tto, tto - A):
        assert isinstance(got, T.TToperator) and not isinstance(got, T.QTToperator)
    for got in (A + A, 2.0 * A, A * 2.0):
        assert isinstance(got, T.QTToperator) and got.ordering == "interleaved"
    Aq = A * q1
    assert isinstance(Aq, T.QTTvector) and (Aq.n_dims, Aq.bits_per_dim, Aq.ordering) == (2, 3, "interleaved")
    want = O.ttv_to_tensor(O.apply(to_oracle(tto), to_oracle(ttv)))
    assert np.max(np.abs(O.ttv_to_tensor(to_oracle(Aq.ttvector())) - want)) < 1e-12 * np.max(np.abs(want))
    D.status_all()


# ---- qtt_laplacian ------------------------------------------------------------------------------------------------------------------
def _dense_op(A):
    return O.tto_to_tensor(to_oracle(A.ttoperator()))


# (the boundary-condition constructors need d >= 4, as in the reference: the 3-bit case is Dirichlet-Dirichlet)
@pytest.mark.parametrize("n_dims, bits, bc", [(2, 4, "DD"), (2, 4, "DN"), (2, 4, "ND"), (3, 3, "DD")])
@pytest.mark.parametrize("ordering", ORDERINGS)
def test_qtt_laplacian_equals_the_restatement(n_dims, bits, bc, ordering):
    A = T.qtt_laplacian(n_dims, bits, ordering=ordering, bc=bc)
    ref = R.qtt_laplacian(n_dims, bits, ordering, bc=bc)
    assert isinstance(A, T.QTToperator) and (A.n_dims, A.bits_per_dim, A.ordering, A.N) == (n_dims, bits, ordering, n_dims * bits)
    got, want = _dense_op(A), O.tto_to_tensor(ref.tto)
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print("qtt_laplacian", n_dims, bits, ordering, bc, "ranks", A.tto_rks, "rel err %.3e" % err)
    assert err < 1e-8
    D.status_all()


def test_qtt_laplacian_one_dimension_and_intervals():
    for bc in ("DD", "DN", "ND", "NN"):
        A = T.qtt_laplacian(1, 4, ordering="serial", a=-1.0, b=2.0, bc=bc)
        ref = R.qtt_laplacian(1, 4, "serial", -1.0, 2.0, bc)
        assert list(A.tto_rks) == list(ref.tto.tto_rks)
        for ca, cb in zip(A.tto_vec, ref.tto.tto_vec):
            assert np.max(np.abs(ca - cb)) <= 4 * EPS * np.max(np.abs(cb))
    assert T.qtt_laplacian(1, 4, bc="NN").tto_rks[0] == 4
    D.status_all()


def test_qtt_laplacian_action_agrees_between_orderings():
    import torch
    d = 3
    n = 2 ** d
    h = 1.0 / (n - 1)
    M1d = O.qtto_to_matrix(O.Delta(d)) / h ** 2
    M2d = np.kron(M1d, np.eye(n)) + np.kron(np.eye(n), M1d)
    ft = lambda X: torch.sin(math.pi * X[:, 0]) * torch.sin(math.pi * X[:, 1])
    arrs = {}
    for ordering in ORDERINGS:
        A = T.qtt_laplacian(2, d, ordering=ordering, bc="DD")
        v = T.function_to_qttv(ft, 2, d, ordering=ordering)
        Av = A * v
        assert isinstance(Av, T.QTTvector) and (Av.ordering, Av.n_dims, Av.bits_per_dim) == (ordering, 2, d)
        arr_v = T.qttv_to_array(v)
        ref_Av = np.reshape(M2d @ np.ravel(arr_v, order="F"), (n, n), order="F")
        arrs[ordering] = T.qttv_to_array(Av)
        assert np.max(np.abs(arrs[ordering] - ref_Av)) < 1e-8
    assert np.max(np.abs(arrs["serial"] - arrs["interleaved"])) < 1e-8
    D.status_all()


# ---- entanglement entropy -----------------------------------------------------------------------------------------------------------
def _entropy_tol(spectra):
    """1e-10 singular-value parity (relative to sigma_1, the project's stated bar) propagated through -p log p, per bond"""
    out = []
    for S in spectra:
        nrm2 = float(np.sum(S ** 2))
        p = S ** 2 / nrm2
        ds = 1e-10 * S[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(p > 0, np.abs(np.log(p) + 1.0), 0.0)
        out.append(float(np.sum(w * 2 * S * ds / nrm2)) + 1e-12)
    return np.array(out)


def _check_entropy(x, label):
    ref = R.entanglemententropy(x)
    tol = _entropy_tol(R.schmidt_spectra(x))
    got = T.entanglemententropy(to_product(x))
    print("entropy", label, "max err %.3e" % np.max(np.abs(got - ref)), "min tol %.3e" % tol.min())
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= tol), (got - ref, tol)
    got2 = T.entanglemententropy(to_product(x), base=2)
    assert np.all(np.abs(got2 - ref / math.log(2)) <= tol / math.log(2))


@pytest.mark.parametrize("r", [1, 2, 6])
def test_entropy_random_trains(r):
    _check_entropy(O.rand_tt((2,) * 8, r, np.random.default_rng(80 + r)), f"random d=8 r={r}")
    D.status_all()


def test_entropy_sampled_function_and_bell_pair():
    import torch
    q = T.function_to_qttv(lambda X: torch.exp(-10 * ((X[:, 0] - 0.3) ** 2 + (X[:, 1] - 0.7) ** 2)), 2, 4, ordering="interleaved")
    x = to_oracle(q.ttvector())
    ref, tol = R.entanglemententropy(x), _entropy_tol(R.schmidt_spectra(x))
    got = T.entanglemententropy(q)
    print("entropy 2-D gaussian: max err %.3e" % np.max(np.abs(got - ref)))
    assert np.all(np.abs(got - ref) <= tol)
    bell = np.zeros((2, 2))
    bell[0, 0] = bell[1, 1] = 1 / math.sqrt(2)
    qb = T.QTTvector(T.ttv_decomp(bell), 1, 2, "serial")
    assert abs(T.entanglemententropy(qb)[0] - math.log(2)) < 1e-12
    assert abs(T.entanglemententropy(qb, base=2)[0] - 1.0) < 1e-12
    D.status_all()
