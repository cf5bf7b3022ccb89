"""TT operator algebra on the device (DeviceTTO / DeviceTT methods, csrc/ttn_opalg_kernels.h) against the NumPy restatement of the
reference (tests/opalg_reference.py).

Copies and single products (+, kron, concatenate, diag, the conversions, outer, ⨝, scalar *) must agree in every bit.  A * B sums n
products per entry, so it is held to |Y_gpu − Y_ref| <= 2 n ε (|A_k| ⋆ |B_k|) elementwise (ε = 2⁻⁵³): the bound of an n-term dot product
in any summation order, with or without FMA.  Rounding is checked on well-posed cases only (relative truncerr 1e-6, decades away from
every kept and every dropped singular value), where the ranks must EQUAL the restatement's, and through dense matrices / applied
vectors at 1e-9 of the largest entry rather than through norms of differences of trains."""
import ctypes as C
import math

import numpy as np
import pytest

import ttn_amd as T
from oracle import tt_oracle as O
from tests import opalg_reference as R
from tests.helpers import to_oracle, to_product, worst_of
from ttn_amd import _lib
from ttn_amd import device as D

pytestmark = pytest.mark.gpu

# dims, ranks of A, ranks of B (ragged, up to 12)
CASES = [
    ((2,) * 6, [1, 3, 12, 5, 7, 2, 1], [1, 2, 4, 12, 3, 6, 1]),
    ((2, 3), [1, 5, 1], [1, 12, 1]),
    ((2, 3, 2), [1, 4, 7, 1], [1, 12, 2, 1]),
    ((3, 4, 2, 5), [1, 2, 12, 3, 1], [1, 6, 5, 4, 1]),
    ((2, 2, 2), [1, 33, 33, 1], [1, 3, 2, 1]),        # n = 2, A cores of 4356 doubles: beyond the LDS staging of k_tto_mul
    ((2, 2, 2), [1, 48, 48, 1], [1, 48, 48, 1]),      # n = 2, a 2304 x 2304 middle core: more tiles than the grid has blocks (grid-stride loop)
]
SMALL = CASES[:4]


def up(A):
    return T.DeviceTTO(to_product(A))


def upv(x, batch=1):
    return T.DeviceTT.from_host(to_product(x), batch=batch)


def assert_same_operator(got, ref):
    """Handle metadata and the downloaded operator against a restatement operator: dims, ranks, flags, shapes, every bit."""
    assert tuple(got.dims) == tuple(ref.tto_dims) and got.ranks() == list(ref.tto_rks) and got.N == ref.N
    A = got.download()
    assert A.tto_dims == tuple(ref.tto_dims) and A.tto_rks == list(ref.tto_rks) and A.tto_ot == list(ref.tto_ot)
    for k, (g, r) in enumerate(zip(A.tto_vec, ref.tto_vec)):
        assert g.shape == r.shape, (k, g.shape, r.shape)
        assert np.array_equal(g, r), (k, float(np.abs(g - r).max()))


def assert_same_train(got, ref):
    assert got.ttv_dims == tuple(ref.ttv_dims) and got.ttv_rks == list(ref.ttv_rks) and got.ttv_ot == list(ref.ttv_ot)
    for g, r in zip(got.ttv_vec, ref.ttv_vec):
        assert g.shape == r.shape and np.array_equal(g, r)


def rel_max(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("dims,ra,rb", CASES)
def test_mul(dims, ra, rb):
    rng = np.random.default_rng(11)
    A, B = R.rand_tto(dims, ra, rng), R.rand_tto(dims, rb, rng)
    ref, bound = R.tto_mul(A, B), R.tto_mul_bound(A, B)
    dA, dB = up(A), up(B)
    Y = dA.mul(dB)
    assert Y.dims == tuple(dims) and Y.ranks() == ref.tto_rks and Y.ot == [0] * len(dims)
    got = Y.download()
    worst = 0.0
    for k in range(len(dims)):
        assert got.tto_vec[k].shape == ref.tto_vec[k].shape
        err = np.abs(got.tto_vec[k] - ref.tto_vec[k])
        worst = worst_of(worst, float((err / np.maximum(bound[k], 1e-300)).max()))
        assert (err <= bound[k]).all(), (k, worst)
    print(f"mul {dims} {ra} x {rb}: max error / bound = {worst:.3f}")
    for h in (dA, dB, Y):
        h.free()


@pytest.mark.parametrize("dims,ra,rb", SMALL)
def test_add_sub_scale(dims, ra, rb):
    rng = np.random.default_rng(12)
    A, B = R.rand_tto(dims, ra, rng), R.rand_tto(dims, ra[::-1], rng)
    A.tto_ot = [1] * (len(dims) - 1) + [0]                  # the scaled core is the first with ot == 0: the last one here
    dA, dB = up(A), up(B)
    assert_same_operator(dA.add(dB), R.tto_add(A, B))
    assert_same_operator(dA.sub(dB), R.tto_sub(A, B))
    for a in (-2.5, 1.0 / 3.0, 0.0):
        assert_same_operator(dA.scale(a), R.tto_scale(a, A))
    assert_same_operator(dA, A)                              # operands untouched
    A.tto_ot = [1] * len(dims)                               # none: core 1
    assert_same_operator(up(A).scale(7.0), R.tto_scale(7.0, A))


@pytest.mark.parametrize("dims,ra,rb", SMALL)
def test_inner_and_kron(dims, ra, rb):
    rng = np.random.default_rng(13)
    A = R.rand_tto(dims, ra, rng)
    Bi = R.rand_tto(dims[::-1], [1] + [min(r, 5) for r in rb[1:-1]] + [1], rng)      # ⨝ needs the same d only: other dims
    Bk = R.rand_tto((3, 2), [1, 4, 1], rng)
    A.tto_ot, Bk.tto_ot = [0] * (len(dims) - 1) + [-1], [1, 0]
    dA, dBi, dBk = up(A), up(Bi), up(Bk)
    assert_same_operator(dA.inner(dBi), R.tto_inner(A, Bi))
    assert_same_operator(dA.kron(dBk), R.kron(A, Bk))
    assert_same_operator(dBk.kron(dA), R.kron(Bk, A))
    # concatenate: open trains joined at a common rank != 1
    L, Rt = R.rand_tto(dims, ra[:-1] + [5], rng), R.rand_tto((3, 2), [5, 4, 1], rng)
    assert_same_operator(up(L).kron(up(Rt)), R.concatenate(L, Rt))


def test_inner_d1_is_the_kronecker_product():
    rng = np.random.default_rng(42)
    A1, B1 = O.rand_tto((3,), 1, rng), O.rand_tto((4,), 1, rng)
    Cd = up(A1).inner(up(B1))
    assert Cd.dims == (12,) and Cd.ranks() == [1, 1]
    got = Cd.download().tto_vec[0][:, :, 0, 0]
    assert np.array_equal(got, np.kron(A1.tto_vec[0][:, :, 0, 0], B1.tto_vec[0][:, :, 0, 0]))


@pytest.mark.parametrize("dims,ra,rb", SMALL)
def test_vector_side(dims, ra, rb):
    rng = np.random.default_rng(14)
    x, y = R.rand_ttv(dims, ra, rng), R.rand_ttv(dims, rb, rng)
    x.ttv_ot = [0] * (len(dims) - 1) + [1]
    dx, dy = upv(x, batch=3), upv(y, batch=3)
    x2 = R.rand_ttv(dims, [min(r, 2) for r in ra], rng)
    dx.upload(2, to_product(x2))                              # train 2 differs, ranks included
    assert_same_operator(dx.outer(dy), R.outer_product(x, y))
    assert_same_operator(dx.outer(dy, b=2), R.outer_product(x2, y))
    assert_same_operator(dx.diag_tto(), R.ttv_to_diag_tto(x))
    assert_same_operator(dx.diag_tto(b=2), R.ttv_to_diag_tto(x2))
    z = dx.kron(dy)
    assert z.dims == tuple(dims) * 2 and z.batch == 3
    assert_same_train(z.download(0), to_product(R.kron(x, y)))
    assert_same_train(z.download(1), to_product(R.kron(x, y)))
    assert_same_train(z.download(2), to_product(R.kron(x2, y)))
    assert z.max_ranks() == list(ra[:-1]) + list(rb)


@pytest.mark.parametrize("dims,ra,rb", SMALL)
def test_conversions(dims, ra, rb):
    rng = np.random.default_rng(15)
    A = R.rand_tto(dims, ra, rng)
    A.tto_ot = [1] + [0] * (len(dims) - 1)
    dA = up(A)
    v = dA.to_tt(batch=2, cap_rks=[r + 1 for r in ra])       # a roomier handle: the slots differ from the operator's
    ref = to_product(R.tto_to_ttv(A))
    assert_same_train(v.download(0), ref)
    assert_same_train(v.download(1), ref)
    assert_same_operator(T.DeviceTTO.from_tt(v, b=1), A)
    assert_same_operator(T.DeviceTTO.from_tt(dA.to_tt()), A)
    # the operator as a vector serves the existing vector kernels: <A, A> by ttn_dot
    w = dA.to_tt()
    fro2 = float(D.dot(w, w)[0])
    assert math.isclose(fro2, O.dot(R.tto_to_ttv(A), R.tto_to_ttv(A)), rel_tol=1e-12)


def test_host_forms_and_operators():
    rng = np.random.default_rng(16)
    dims = (2, 3, 2)
    A, B = R.rand_tto(dims, [1, 3, 4, 1], rng), R.rand_tto(dims, [1, 2, 5, 1], rng)
    x, y = R.rand_ttv(dims, [1, 2, 3, 1], rng), R.rand_ttv(dims, [1, 3, 2, 1], rng)
    pA, pB, px, py = (to_product(t) for t in (A, B, x, y))
    same = lambda g, r: all(np.array_equal(p, q) for p, q in zip(g.tto_vec, r.tto_vec)) and g.tto_rks == r.tto_rks and g.tto_ot == r.tto_ot
    assert same(pA + pB, R.tto_add(A, B)) and same(pA - pB, R.tto_sub(A, B))
    assert same(2.5 * pA, R.tto_scale(2.5, A)) and same(pA * 2.5, R.tto_scale(2.5, A)) and same(0 * pA, R.tto_scale(0.0, A))
    assert same(T.tto_inner(pA, pB), R.tto_inner(A, B))
    assert same(T.outer_product(px, py), R.outer_product(x, y)) and same(T.ttv_to_diag_tto(px), R.ttv_to_diag_tto(x))
    P, ref, bound = pA * pB, R.tto_mul(A, B), R.tto_mul_bound(A, B)
    assert isinstance(P, T.TToperator) and P.tto_rks == ref.tto_rks
    assert all((np.abs(g - r) <= b).all() for g, r, b in zip(P.tto_vec, ref.tto_vec, bound))
    # TToperator * TTvector keeps returning the applied vector
    v = pA * px
    assert isinstance(v, T.TTvector) and v.ttv_rks == [a * b for a, b in zip(A.tto_rks, x.ttv_rks)]
    assert np.allclose(R.ttv_vector(to_oracle(v)), R.tto_matrix(A) @ R.ttv_vector(x), atol=1e-11, rtol=0)
    # tto_compress_ rebinds and returns its argument
    D2 = T.Delta(8) * T.Delta(8)
    assert D2.tto_rks == [1] + [9] * 7 + [1]
    out = T.tto_compress_(D2, truncerr=1e-6)
    assert out is D2 and D2.tto_rks == [1, 4, 5, 5, 5, 5, 5, 4, 1]


# ---- refusals: each before any launch, the out-pointer stays null ------------------------------------------------------------------
def _refused(fn, *args):
    h = C.c_void_p()
    rc = fn(*args, C.byref(h))
    assert not h, "a refused call must not return a handle"
    return rc


def test_refusals():
    _lib.ensure_init()
    L = _lib.lib()
    rng = np.random.default_rng(17)
    A, B3, A1 = up(R.rand_tto((2, 3), [1, 2, 1], rng)), up(R.rand_tto((3, 2), [1, 2, 1], rng)), up(R.rand_tto((2,), [1, 1], rng))
    A3 = up(R.rand_tto((2, 3, 2), [1, 2, 2, 1], rng))
    x, xs = upv(R.rand_ttv((2, 3), [1, 2, 1], rng)), upv(R.rand_ttv((3, 2), [1, 2, 1], rng))
    # null handles
    for fn in (L.ttn_tto_mul, L.ttn_tto_inner, L.ttn_tto_add, L.ttn_tto_kron):
        assert _refused(fn, None, A.h) == _lib.TTN_ERR_ARG and _refused(fn, A.h, None) == _lib.TTN_ERR_ARG
        assert fn(A.h, A.h, None) == _lib.TTN_ERR_ARG
    assert _refused(L.ttn_tto_scale, 2.0, None) == _lib.TTN_ERR_ARG
    assert _refused(L.ttn_tt_outer, None, x.h, 0) == _lib.TTN_ERR_ARG and _refused(L.ttn_tt_outer, x.h, None, 0) == _lib.TTN_ERR_ARG
    assert _refused(L.ttn_tt_diag_tto, None, 0) == _lib.TTN_ERR_ARG and _refused(L.ttn_tto_from_tt, None, 0) == _lib.TTN_ERR_ARG
    assert _refused(L.ttn_tto_compress, None, 4, 0.0, 1) == _lib.TTN_ERR_ARG
    assert L.ttn_tt_kron(None, x.h, x.h) == _lib.TTN_ERR_ARG and L.ttn_tto_to_tt(None, x.h) == _lib.TTN_ERR_ARG
    assert L.ttn_tto_to_tt(A.h, None) == _lib.TTN_ERR_ARG
    assert L.ttn_tto_ranks(None, None, None, None, None) == _lib.TTN_ERR_ARG and L.ttn_tto_download(None, None) == _lib.TTN_ERR_ARG
    # train index outside the batch
    assert _refused(L.ttn_tt_outer, x.h, x.h, 1) == _lib.TTN_ERR_ARG and _refused(L.ttn_tt_diag_tto, x.h, -1) == _lib.TTN_ERR_ARG
    # different dims / d
    assert _refused(L.ttn_tto_mul, A.h, B3.h) == _lib.TTN_ERR_DIMS and _refused(L.ttn_tto_add, A.h, B3.h) == _lib.TTN_ERR_DIMS
    assert _refused(L.ttn_tto_mul, A.h, A3.h) == _lib.TTN_ERR_DIMS and _refused(L.ttn_tto_add, A.h, A3.h) == _lib.TTN_ERR_DIMS
    assert _refused(L.ttn_tto_inner, A.h, A3.h) == _lib.TTN_ERR_DIMS
    assert _refused(L.ttn_tt_outer, x.h, xs.h, 0) == _lib.TTN_ERR_DIMS
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        A.mul(B3)
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        A.add(B3)
    with pytest.raises(AssertionError, match="same number of cores"):
        A.inner(A3)
    # + needs d >= 2
    assert _refused(L.ttn_tto_add, A1.h, A1.h) == _lib.TTN_ERR_UNSUPPORTED
    # concatenate: ranks at the joint
    open_l, open_r = up(R.rand_tto((2,), [1, 3], rng)), up(R.rand_tto((2,), [2, 1], rng))
    assert _refused(L.ttn_tto_kron, open_l.h, open_r.h) == _lib.TTN_ERR_DIMS
    with pytest.raises(AssertionError, match="final rank"):
        open_l.kron(open_r)
    # from_tt: dims that are not squares; to_tt: wrong dims / too little room
    assert _refused(L.ttn_tto_from_tt, x.h, 0) == _lib.TTN_ERR_DIMS
    assert L.ttn_tto_to_tt(A.h, x.h) == _lib.TTN_ERR_DIMS
    tight = T.DeviceTT((4, 9), [1, 1, 1])
    assert L.ttn_tto_to_tt(A.h, tight.h) == _lib.TTN_ERR_CAPACITY
    # vector kron: dims of the destination, capacity
    z_bad = T.DeviceTT((2, 3, 2, 3), [1, 2, 1, 2, 1])
    assert L.ttn_tt_kron(x.h, xs.h, z_bad.h) == _lib.TTN_ERR_DIMS
    z_tight = T.DeviceTT((2, 3, 3, 2), [1, 1, 1, 2, 1])
    assert L.ttn_tt_kron(x.h, xs.h, z_tight.h) == _lib.TTN_ERR_CAPACITY
    # compress arguments
    assert _refused(L.ttn_tto_compress, A.h, 4, 0.0, 0) == _lib.TTN_ERR_SWEEPS and _refused(L.ttn_tto_compress, A.h, 0, 0.0, 1) == _lib.TTN_ERR_ARG
    D.status_all()


def _thin(n, r):
    """d = 2, ranks [1, r, 1], every entry one."""
    return T.DeviceTTO(T.TToperator(2, [np.ones((n, n, 1, r), order="F"), np.ones((n, n, r, 1), order="F")], (n, n), [1, r, 1], [0, 0]))


def test_refusals_by_size():
    """Small operands whose product is out of reach: a bond of r^2 >= 2^31 (32-bit fibre indices), and, just below that, 4 x 4 sites whose
    two output cores of 16 r^2 doubles (2 x 271 GB) exceed the memory of the device."""
    _lib.ensure_init()
    L = _lib.lib()
    a = _thin(2, 46341)                                       # 46341^2 = 2^31 + 4633
    assert _refused(L.ttn_tto_mul, a.h, a.h) == _lib.TTN_ERR_UNSUPPORTED
    assert "2^31" in _lib.last_error()
    with pytest.raises(T.TTNError, match="2\\^31"):
        a.mul(a)
    xa = T.DeviceTT.from_host(T.TTvector(2, [np.ones((2, 1, 46341), order="F"), np.ones((2, 46341, 1), order="F")], (2, 2), [1, 46341, 1], [0, 0]))
    assert _refused(L.ttn_tt_outer, xa.h, xa.h, 0) == _lib.TTN_ERR_UNSUPPORTED
    b = _thin(4, 46000)                                       # 46000^2 < 2^31
    assert _refused(L.ttn_tto_mul, b.h, b.h) == _lib.TTN_ERR_CAPACITY
    assert "device memory" in _lib.last_error()
    # the library is as usable as before
    c = _thin(2, 3)
    assert c.mul(c).ranks() == [1, 9, 1]
    D.status_all()


def test_handles_in_a_loop_leave_nothing_behind():
    """A few hundred products, sums and roundings on handles that are created and freed as they go (ttn_tto_compress creates and frees
    a working train inside): the sums never change a bit, the rounded ranks stay what max_bond = 16 and the dimensions allow, no status is left over, and the free memory of the device does not shrink with
    the iterations (each iteration allocates about 1 MB of results: 150 leaked iterations would be far above the 64 MB allowed;
    the smaller of two measured rounds is taken, since other processes may allocate on the same device meanwhile)."""
    import torch
    rng = np.random.default_rng(18)
    dims = (2,) * 6
    A, B = R.rand_tto(dims, [1, 4, 8, 8, 8, 4, 1], rng), R.rand_tto(dims, [1, 4, 8, 8, 8, 4, 1], rng)
    dA, dB = up(A), up(B)
    first = None

    def round_of(n):
        nonlocal first
        for _ in range(n):
            P = dA.mul(dB)
            S = P.add(dA)
            Cc = S.compress(max_bond=16)
            assert Cc.ranks() == [1, 4, 16, 16, 16, 4, 1]
            got = [c.copy() for c in S.download().tto_vec] if first is None or _ == n - 1 else None
            for h in (P, S, Cc):
                h.free()
            if got is not None:
                if first is None:
                    first = got
                assert all(np.array_equal(g, f) for g, f in zip(got, first))
        D.status_all()
        D.sync()
        return torch.cuda.mem_get_info(0)[0]

    f0 = round_of(20)
    f1 = round_of(150)
    f2 = round_of(150)
    growth = min(f0 - f1, f1 - f2)
    print(f"free memory after the rounds: {f0} {f1} {f2}")
    assert growth < 64 * 2 ** 20, (f0, f1, f2)


# ---- rounding, end to end ------------------------------------------------------------------------------------------------------------
class DeviceOps:
    """The algebra of opalg_reference.ornstein2d_coupled on DeviceTTO methods, from uploaded shift, id_tto, Nabla, Delta and qtt_polynom."""
    add = staticmethod(lambda A, B: A.add(B))
    sub = staticmethod(lambda A, B: A.sub(B))
    mul = staticmethod(lambda A, B: A.mul(B))
    kron = staticmethod(lambda A, B: A.kron(B))
    scale = staticmethod(lambda a, A: A.scale(a))
    shift = staticmethod(lambda d: T.DeviceTTO(T.shift(d)))
    id = staticmethod(lambda d: T.DeviceTTO(T.id_tto(d)))
    nabla = staticmethod(lambda d: T.DeviceTTO(T.Nabla(d)))
    delta = staticmethod(lambda d: T.DeviceTTO(T.Delta(d)))

    @staticmethod
    def diag_poly(coef, d, a, b):
        return T.DeviceTT.from_host(T.qtt_polynom(coef, d, a, b)).diag_tto()


RANKS_D8 = [1, 4, 6, 6, 6, 6, 6, 6, 4, 6, 6, 6, 6, 6, 6, 4, 1]


def test_ornstein_generator_dense_d4():
    d = 4
    ref = R.ornstein2d_coupled(d, R.HostOps)
    raw = R.ornstein2d_coupled(d, DeviceOps)
    assert raw.ranks() == ref.tto_rks
    rounded = raw.compress(truncerr=1e-6)
    assert rounded.ranks() == R.tto_compress(ref, truncerr=1e-6).tto_rks
    M = R.tto_matrix(ref)
    assert M.shape == (256, 256)
    e_raw, e_rounded = rel_max(R.tto_matrix(to_oracle(raw.download())), M), rel_max(R.tto_matrix(to_oracle(rounded.download())), M)
    print(f"d = 4 dense: raw {e_raw:.2e} rounded {e_rounded:.2e}")
    assert e_raw < 1e-9 and e_rounded < 1e-9
    D.status_all()


def _state(d, a=-6.0, b=6.0):
    gx = T.qtt_polynom([1.0, 0.3, -0.05], d, a, b)             # rank 3
    gy = T.qtt_exp(d, a, b, alpha=-0.3)                        # rank 1
    return gx, gy


def test_ornstein_generator_applied_d8():
    d = 8
    ref = R.ornstein2d_coupled(d, R.HostOps)
    raw = R.ornstein2d_coupled(d, DeviceOps)
    assert raw.ranks() == [1] + [28] * 7 + [6] + [28] * 7 + [1] == ref.tto_rks
    rounded = raw.compress(truncerr=1e-6)
    assert rounded.ranks() == RANKS_D8 == R.tto_compress(ref, truncerr=1e-6).tto_rks
    gx, gy = _state(d)
    u = T.DeviceTT.from_host(gx).kron(T.DeviceTT.from_host(gy))
    assert_same_train(u.download(), to_product(R.kron(to_oracle(gx), to_oracle(gy))))
    y = T.DeviceTT(u.dims, [p * q for p, q in zip(rounded.ranks(), u.max_ranks())])
    D.apply(rounded, u, y)
    got = R.ttv_vector(to_oracle(y.download()))
    want = R.ttv_vector(O.apply(ref, R.kron(to_oracle(gx), to_oracle(gy))))           # the unrounded operator, on the CPU
    assert got.shape == (2 ** 16,)
    err = rel_max(got, want)
    print(f"d = 8 applied: {err:.2e}")
    assert err < 1e-9
    D.status_all()


def _dense_rk4(M, v, steps):
    """rk4_method (src/solvers/euler.jl:193-209, normalised after every step) on a dense matrix."""
    for h in steps:
        k1 = M @ v
        k2 = M @ (v + h / 2 * k1)
        k3 = M @ (v + h / 2 * k2)
        k4 = M @ (v + h * k3)
        v = v + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        v = v / np.linalg.norm(v)
    return v


def test_rounded_operator_drives_rk4():
    """The device-rounded generator is accepted by an existing solver: three RK4 steps against the same chain with the host-assembled
    (unrounded, rank-28) operator, and against RK4 on the dense matrix, every entry at 1e-9 of the largest.

    The case is chosen so that the comparison is well posed.  A bond step of tt_compress! takes the SVD of the two-site block
    (n r_{k-1}) x (n r_{k+1}) as it lies, against right cores that are not orthogonal: a singular value of that block says nothing
    about the weight of its direction in the whole vector, so as soon as max_bond cuts a block the result depends on the
    representation of A * u (ranks 6 r or 28 r), not only on the vector.  (CPU oracle, LAPACK SVDs, rounded against unrounded operator,
    d = 4 per axis, three steps: 2.4e-3 at max_bond = 16, 1.3e-4 at 32, 2.0e-14 at 64; d = 8, max_bond = 8, two steps: 3.6e-2.)  On N
    binary sites a block in the left-to-right pass has at most min(2^k, 2 r_{k+1}) <= 2^(N-2) singular values, so with
    max_bond = 2^(N-2) no block is ever cut, every rounding of the chain is exact up to rounding errors and both operators must
    give the same vector.  d = 4 bits per axis (N = 8, max_bond = 64) keeps the rank-28 partner within the solver's limits; h = 1e-2
    is inside RK4's stability region (|A| < 40 at this grid).  At d = 8 the same freedom does not exist (2^14), so there the chain
    is only required to run: finite values, ranks within max_bond, no status."""
    from ttn_amd import solvers
    d, steps = 4, [1.0e-2] * 3
    N = 2 * d
    ref = R.ornstein2d_coupled(d, R.HostOps)
    rounded = R.ornstein2d_coupled(d, DeviceOps).compress(truncerr=1e-6)
    host = T.DeviceTTO(to_product(ref))                                              # assembled on the host, not rounded
    assert host.ranks() == [1, 28, 28, 28, 6, 28, 28, 28, 1] and rounded.ranks() == [1, 4, 6, 6, 4, 6, 6, 4, 1]
    gx, gy = _state(d)
    outs = []
    for A in (rounded, host):
        u0 = T.DeviceTT.from_host(gx).kron(T.DeviceTT.from_host(gy))
        outs.append(R.ttv_vector(to_oracle(solvers.rk4_method(A, u0, steps, max_bond=2 ** (N - 2)).download())))
    dense = _dense_rk4(R.tto_matrix(ref), R.ttv_vector(R.kron(to_oracle(gx), to_oracle(gy))), steps)
    e_host, e_dense = rel_max(outs[0], outs[1]), rel_max(outs[0], dense)
    print(f"rk4, 3 steps, d = 4: rounded vs host-assembled {e_host:.2e}, rounded vs dense RK4 {e_dense:.2e}")
    assert e_host < 1e-9 and e_dense < 1e-9
    # d = 8: accepted by the solver
    d = 8
    big = R.ornstein2d_coupled(d, DeviceOps).compress(truncerr=1e-6)
    assert big.ranks() == RANKS_D8
    gx, gy = _state(d)
    u = solvers.rk4_method(big, T.DeviceTT.from_host(gx).kron(T.DeviceTT.from_host(gy)), [1.0e-4] * 3, max_bond=8)
    assert max(u.max_ranks()) <= 8
    v = R.ttv_vector(to_oracle(u.download()))
    assert v.shape == (2 ** 16,) and np.isfinite(v).all() and abs(np.linalg.norm(v) - 1.0) < 1e-9
    D.status_all()


def test_deep_qtt_laplacian_squared():
    d = 30
    Dl = T.DeviceTTO(T.Delta(d))
    D2 = Dl.mul(Dl).compress(truncerr=1e-6)
    assert D2.ranks() == [1, 4] + [5] * (d - 3) + [4, 1]
    x = T.DeviceTT.from_host(T.qtt_sin(d, lam=math.pi))
    y1 = T.DeviceTT(x.dims, [p * q for p, q in zip(D2.ranks(), x.cap)])
    D.apply(D2, x, y1)
    t = T.DeviceTT(x.dims, [p * q for p, q in zip(Dl.rks, x.cap)])
    D.apply(Dl, x, t)
    y2 = T.DeviceTT(x.dims, [p * q for p, q in zip(Dl.rks, t.cap)])
    D.apply(Dl, t, y2)
    ny = float(D.norm(y2)[0])
    assert ny > 0
    for seed in range(5):
        p = T.DeviceTT.from_host(T.rand_tt((2,) * d, 4, seed=100 + seed))
        a, b, n_p = float(D.dot(p, y1)[0]), float(D.dot(p, y2)[0]), float(D.norm(p)[0])
        print(f"probe {seed}: {a:.15e} {b:.15e} scaled difference {abs(a - b) / (n_p * ny):.2e}")
        assert abs(a - b) <= 1e-9 * n_p * ny
    D.status_all()
