"""The pullback of <x, A y> on the GPU (csrc/ttn_expect_grad_kernels.h, include/ttn_expect_grad.h, ttn_amd.grad.sandwich_pullback) against
the NumPy restatement tests/expect_grad_reference.py (pinned by tests/test_cpu_expect_grad.py).

Tolerances are derived, not measured: every entry must agree with the restatement to 2 p eps S_abs (ER.sandwich_pullback_bound: p the
number of terms along the longest chain of the three-layer form, S_abs the same formula on absolute values).  Each case prints the largest
share of its bound it used (recorded in DESIGN.md 4.26).  Shapes: the smallest at which each piece can go wrong — d = 1 and 2, mixed dims
and a ragged batch on the general route, ranks off the 16 x 16 tile and different ranks on the two sides on the on-chip route, one case
just inside and one just outside each limit of the on-chip class, one batch whose trains take different routes."""
import ctypes as C

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import expect_grad_reference as ER
from tests import grad_reference as GR
from tests.helpers import to_oracle, to_product, worst_of
from tests.test_cpu_expect import mixed_case
from tests.test_cpu_expect_grad import mixed5_case
from tests.test_cpu_grad import _rand_op

pytestmark = pytest.mark.gpu
EPS = ER.EPS


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _up(T, trains, cap=None):
    dims = trains[0].ttv_dims
    if cap is None:
        cap = [max(t.ttv_rks[m] for t in trains) for m in range(len(dims) + 1)]
    h = T.DeviceTT(dims, cap, batch=len(trains))
    for b, t in enumerate(trains):
        h.upload(b, to_product(t))
    return h


def _same(h, trains):
    """The handle still holds, bit for bit, what was uploaded."""
    for b, t in enumerate(trains):
        got = h.download(b)
        assert got.ttv_rks == list(t.ttv_rks)
        assert all(np.array_equal(x, y) for x, y in zip(got.ttv_vec, t.ttv_vec))


def _share(got, ref, bound):
    """Largest |got - ref| / bound over the entries (0 / 0 counts as 0); asserts every entry is within its bound."""
    worst = 0.0
    for g, r, bd in zip(got, ref, bound):
        g, r, bd = np.asarray(g), np.asarray(r), np.asarray(bd)
        assert g.shape == r.shape, (g.shape, r.shape)
        err = np.abs(g - r)
        assert np.all(err <= bd), "entry beyond its bound: worst ratio %.3g" % float(np.max(err / np.maximum(bd, 1e-300)))
        nz = bd > 0
        if np.any(nz):
            worst = worst_of(worst, float(np.max(err[nz] / bd[nz])))
    return worst


def _free(*hs):
    for h in set(hs):
        h.free()


def _scale(x, A, y):
    return O.norm(x) * O.norm(O.apply(A, y))


def _check_abs(T, name, xs, A, ys, deltas, same):
    """The same call on |x|, |A|, |y|: every product is non-negative, S_abs is the value itself, and the bound 2 p eps S_abs is a
    relative one of a few 1e-13 per entry — on random signed trains of high rank S_abs exceeds the value by many orders."""
    axs, ays, aA = [ER._abs_tt(x) for x in xs], [ER._abs_tt(y) for y in ys], ER._abs_tto(A)
    hx = _up(T, axs)
    hy = hx if same else _up(T, ays)
    hA = T.DeviceTTO(to_product(aA))
    val, xbar, ybar = T.sandwich_pullback(hx, hA, hy, delta=deltas)
    worst = 0.0
    for t, (x, y) in enumerate(zip(axs, ays)):
        dl = 1.0 if deltas is None else float(np.broadcast_to(deltas, (len(xs),))[t])
        rv, rx, ry = ER.sandwich_pullback(x, aA, y, dl)
        bv, bx, by = ER.sandwich_pullback_bound(x, aA, y, dl)
        worst = worst_of(worst, _share(xbar.download(t).ttv_vec, rx, bx), _share(ybar.download(t).ttv_vec, ry, by))
        assert abs(val[t] - rv) <= bv
    print("sandwich_pullback %s, absolute values: largest share of the bound %.3g" % (name, worst))
    _free(hx, hy, hA, xbar, ybar)


def _check(T, name, xs, A, ys, deltas=None, same=False, capx=None, capy=None):
    """sandwich_pullback on a batch against the restatement, train by train: tangents entry by entry under the bound, ranks and gauge
    flags, the value (not scaled by delta) at the bar of test_gpu_expect.py, the Euler identity, operands untouched; then the same
    shapes on absolute values, where the bound is sharp."""
    # Do not drop _check_abs as redundant.  On signed random trains of high rank S_abs exceeds the entries by many orders (shares of
    # 1e-17 to 7e-19 in DESIGN.md 4.26), so the entry-wise comparison below cannot see a wrong contraction there: at those shapes the
    # signed pass checks only the ranks, the gauge flags, the value and the Euler identity.  The pass on |x|, |A|, |y| is the one that
    # checks the contraction.
    _check_abs(T, name, xs, A, ys, deltas, same)
    hx = _up(T, xs, capx)
    hy = hx if same else _up(T, ys, capy)
    hA = T.DeviceTTO(to_product(A))
    val, xbar, ybar = T.sandwich_pullback(hx, hA, hy, delta=deltas)
    sand = T.device.sandwich(hx, hA, hy)
    ex, ey = T.cores_dot(hx, xbar), T.cores_dot(hy, ybar)
    worst = 0.0
    for t, (x, y) in enumerate(zip(xs, ys)):
        dl = 1.0 if deltas is None else float(np.broadcast_to(deltas, (len(xs),))[t])
        rv, rx, ry = ER.sandwich_pullback(x, A, y, dl)
        _, bx, by = ER.sandwich_pullback_bound(x, A, y, dl)
        gx, gy = xbar.download(t), ybar.download(t)
        assert gx.ttv_rks == list(x.ttv_rks) and gy.ttv_rks == list(y.ttv_rks) and gx.ttv_ot == [0] * x.N and gy.ttv_ot == [0] * y.N
        worst = worst_of(worst, _share(gx.ttv_vec, rx, bx), _share(gy.ttv_vec, ry, by))
        sc = _scale(x, A, y)
        assert abs(val[t] - rv) <= 1e-12 * sc and abs(val[t] - sand[t]) <= 1e-12 * sc
        # Euler: N pairings, each another summation order of s
        assert abs(ex[t] - x.N * dl * rv) <= x.N * 1e-12 * abs(dl) * sc
        assert abs(ey[t] - x.N * dl * rv) <= x.N * 1e-12 * abs(dl) * sc
    print("sandwich_pullback %s: largest share of the bound %.3g" % (name, worst))
    _same(hx, xs)
    _same(hy, ys)
    return hx, hy, hA, xbar, ybar


def test_d1_and_d2(T):
    rng = np.random.default_rng(1)
    for dims, rx, ry, Ar in [((3,), [1, 1], [1, 1], [1, 1]), ((2, 3), [1, 2], [1, 3], [1, 2])]:
        d = len(dims)
        rx, ry, Ar = rx + [1] * (d + 1 - len(rx)), ry + [1] * (d + 1 - len(ry)), Ar + [1] * (d + 1 - len(Ar))
        x, y = O.rand_tt(dims, rx, rng), O.rand_tt(dims, ry, rng)
        _free(*_check(T, "d%d" % d, [x], _rand_op(dims, Ar, rng), [y], 0.7))
    # d = 1, n = 2: the on-chip class at its smallest
    x, y = O.rand_tt((2,), [1, 1], rng), O.rand_tt((2,), [1, 1], rng)
    _free(*_check(T, "d1 n2", [x], _rand_op((2,), [1, 1], rng), [y], -1.5))


@pytest.mark.parametrize("case", ["mixed", "mixed5"])
def test_general_route_mixed_dims(T, case):
    x, A, y = (mixed_case if case == "mixed" else mixed5_case)()
    _free(*_check(T, case, [x], A, [y], -0.75))


def test_general_route_ragged_batch_zero_train_and_single_outputs(T):
    x, A, y = mixed_case()
    rng = np.random.default_rng(21)
    x1 = O.rand_tt(x.ttv_dims, [1, 2, 3, 2, 1], rng)                 # below the handle's capacity [1, 2, 5, 3, 1]
    y1 = O.rand_tt(y.ttv_dims, [1, 2, 4, 1, 1], rng)
    x2 = O.TTvector(x.N, [np.zeros_like(c) for c in x.ttv_vec], x.ttv_dims, x.ttv_rks, x.ttv_ot)
    xs, ys, deltas = [x, x1, x2], [y, y1, y], np.array([0.5, -2.0, 3.0])
    hx, hy, hA, xbar, ybar = _check(T, "ragged batch", xs, A, ys, deltas)
    assert all(np.all(c == 0.0) for c in xbar.download(2).ttv_vec + ybar.download(2).ttv_vec)
    # xbar only, ybar only (into given destinations), and no value: the same bits as the full call
    _, x_only, none = T.sandwich_pullback(hx, hA, hy, delta=deltas, want_ybar=False)
    assert none is None
    dst = T.DeviceTT(y.ttv_dims, [1, 4, 6, 3, 1], batch=3)             # a destination with its own (larger) capacity
    v0, none, y_only = T.sandwich_pullback(hx, hA, hy, delta=deltas, ybar=dst, want_value=False, want_xbar=False)
    assert v0 is None and none is None and y_only is dst
    for t in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(x_only.download(t).ttv_vec, xbar.download(t).ttv_vec))
        assert all(np.array_equal(a, b) for a, b in zip(y_only.download(t).ttv_vec, ybar.download(t).ttv_vec))
    # out = NULL and delta = NULL through the C ABI: asynchronous, the same tangent as delta = 1
    L = T._lib.lib()
    T._lib.check(L.ttn_sandwich_pullback(hx.h, hA.h, hy.h, None, x_only.h, None, None))
    _, x1bar, _ = T.sandwich_pullback(hx, hA, hy, want_ybar=False)
    for t in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(x_only.download(t).ttv_vec, x1bar.download(t).ttv_vec))
    _free(hx, hy, hA, xbar, ybar, x_only, dst, x1bar)


@pytest.mark.parametrize("rx,ry", [(15, 16), (16, 17), (17, 15)])
def test_on_chip_tile_edges(T, rx, ry):
    dims = (2,) * 7
    rng = np.random.default_rng(10 * rx + ry)
    _free(*_check(T, "tile edges %d/%d" % (rx, ry), [O.rand_tt(dims, rx, rng)], O.rand_tto(dims, 1, rng), [O.rand_tt(dims, ry, rng)], 1.25))


QTT_CASES = [(9, 5, 13, 3), (12, 37, 64, 2), (14, 64, 21, 5), (14, 64, 64, 3)]


@pytest.mark.parametrize("d,rx,ry,R_", QTT_CASES)
def test_on_chip_different_ranks_on_the_two_sides(T, d, rx, ry, R_):
    rng = np.random.default_rng(100 * d + R_)
    dims = (2,) * d
    A = O.rand_tto(dims, R_, rng)
    assert max(A.tto_rks) == R_ <= T.device.EXPECT_QTT_MAX_OP_RANK and max(rx, ry) <= T.device.EXPECT_QTT_MAX_RANK
    _free(*_check(T, str((d, rx, ry, R_)), [O.rand_tt(dims, rx, rng)], A, [O.rand_tt(dims, ry, rng)], -0.3))


LIMIT_CASES = {"inside": (64, 64, 5), "x65": (65, 64, 2), "y65": (64, 65, 2), "R6": (20, 33, 6)}


@pytest.mark.parametrize("name", list(LIMIT_CASES))
def test_limits_of_the_on_chip_class_inside_and_outside(T, name):
    rx, ry, R_ = LIMIT_CASES[name]
    d = 14
    dims = (2,) * d
    rng = np.random.default_rng(3 + rx + ry + R_)
    A = O.rand_tto(dims, R_, rng)
    assert max(A.tto_rks) == R_
    _free(*_check(T, "limits " + name, [O.rand_tt(dims, rx, rng)], A, [O.rand_tt(dims, ry, rng)], 0.9))


def test_one_batch_two_routes(T):
    """Train 0 has a rank above the limit and takes the general route, train 1 fits the on-chip class: the decision is per train."""
    d = 10
    dims = (2,) * d
    rng = np.random.default_rng(5)
    xs = [O.rand_tt(dims, 32, rng), O.rand_tt(dims, 32, rng)]
    ys = [O.rand_tt(dims, 65, rng), O.rand_tt(dims, 64, rng)]
    _free(*_check(T, "two routes", xs, O.Delta(d), ys, np.array([1.0, -0.5])))


OPEN_CASES = {
    # on-chip class; Delta_NN's rank-4 ends are filled in row 1 / column 1 only, the trains' open ends are dense
    "Delta_NN": ((2,) * 6, [2, 4, 7, 8, 7, 4, 3], [3, 5, 8, 8, 6, 4, 2], None),
    # on-chip class, every boundary entry of operator and trains filled
    "chip dense ends": ((2,) * 6, [2, 4, 7, 17, 7, 4, 3], [3, 5, 8, 16, 6, 4, 2], [2, 3, 5, 4, 3, 3, 2]),
    # general route (mixed dims), end ranks 2
    "general dense ends": ((3, 2, 4, 2, 3), [2, 3, 5, 4, 2, 2], [2, 2, 4, 3, 3, 2], [2, 3, 3, 3, 3, 2]),
}


@pytest.mark.parametrize("name", list(OPEN_CASES))
def test_open_boundary_ranks(T, name):
    """Boundary ranks above 1 (a segment of a train, Delta_NN): the value and the tangents are those of the [1, 1, 1] boundary entry,
    L_1 = G_{N+1} = e_1 over the whole slot, as ER.environments states it.  The library workspace is first filled by another call, so
    that a boundary slot of which only entry [1, 1, 1] were written would hold that call's leftovers.  A batch of two, so that the
    second train's slots lie inside the workspace; signed trains, then their absolute values (the sharp bound)."""
    dims, rx, ry, Ar = OPEN_CASES[name]
    rng = np.random.default_rng(41)
    A = to_oracle(T.Delta_NN(len(dims))) if Ar is None else _rand_op(dims, Ar, rng)
    xs, ys = [O.rand_tt(dims, rx, rng) for _ in range(2)], [O.rand_tt(dims, ry, rng) for _ in range(2)]
    deltas = np.array([0.6, -1.1])
    # two trains of rank 32 at every bond, the ends included: every environment of their dot_pullback but its own two start states is
    # dense, 2 x 2 x 11 x 1024 doubles from the start of the workspace, which covers a boundary slot of every case here
    fill = _up(T, [O.rand_tt((2,) * 10, [32] * 11, rng) for _ in range(2)])
    worst = []
    for xs_, A_, ys_ in ((xs, A, ys), ([ER._abs_tt(x) for x in xs], ER._abs_tto(A), [ER._abs_tt(y) for y in ys])):
        _free(*T.dot_pullback(fill, fill, want_value=False)[1:])          # leaves its environments in the workspace
        hx, hy, hA = _up(T, xs_), _up(T, ys_), T.DeviceTTO(to_product(A_))
        val, xbar, ybar = T.sandwich_pullback(hx, hA, hy, delta=deltas)
        w = 0.0
        for t, (x, y) in enumerate(zip(xs_, ys_)):
            rv, rx_, ry_ = ER.sandwich_pullback(x, A_, y, deltas[t])
            bv, bx, by = ER.sandwich_pullback_bound(x, A_, y, deltas[t])
            gx, gy = xbar.download(t), ybar.download(t)
            assert gx.ttv_rks == list(x.ttv_rks) and gy.ttv_rks == list(y.ttv_rks)
            w = worst_of(w, _share(gx.ttv_vec, rx_, bx), _share(gy.ttv_vec, ry_, by))
            assert abs(val[t] - rv) <= bv
        worst.append(w)
        _same(hx, xs_)
        _same(hy, ys_)
        _free(hx, hy, hA, xbar, ybar)
    print("sandwich_pullback open ends, %s: largest share of the bound %.3g, on absolute values %.3g" % (name, worst[0], worst[1]))
    _free(fill)


def _named(T, name, d):
    return {"shift": lambda: O.shift(d), "Nabla": lambda: to_oracle(T.Nabla(d)), "Delta": lambda: O.Delta(d),
            "heisenberg": lambda: to_oracle(T.heisenberg_xyz_tto(d, jx=1.0, jy=0.7, jz=-1.2, lam=0.3, field="x"))}[name]()


@pytest.mark.parametrize("name", ["shift", "Nabla", "Delta", "heisenberg"])
def test_named_operators(T, name):
    d = 9
    rng = np.random.default_rng(7)
    A = _named(T, name, d)
    assert max(A.tto_rks) == (5 if name == "heisenberg" else 3)
    _free(*_check(T, name, [O.rand_tt((2,) * d, 11, rng)], A, [O.rand_tt((2,) * d, 16, rng)], 2.0))


def _transpose(A):
    return O.TToperator(A.N, [np.swapaxes(c, 0, 1).copy() for c in A.tto_vec], A.tto_dims, A.tto_rks, A.tto_ot)


def test_same_handle_for_x_and_y(T):
    d = 9
    dims = (2,) * d
    rng = np.random.default_rng(13)
    x = O.rand_tt(dims, 18, rng)
    # a symmetric operator: xbar and ybar agree within the sum of their bounds
    A = O.Delta(d)
    hx, _, hA, xbar, ybar = _check(T, "same handle, Delta", [x], A, [x], 0.4, same=True)
    _, bx, by = ER.sandwich_pullback_bound(x, A, x, 0.4)
    _share(xbar.download(0).ttv_vec, ybar.download(0).ttv_vec, [p + q for p, q in zip(bx, by)])
    _free(hx, hA, xbar, ybar)
    # any operator: xbar(A) = ybar(A^T), from <x, A x> = <x, A^T x>
    A = O.rand_tto(dims, 3, rng)
    At = _transpose(A)
    hx, _, hA, xbar, ybar = _check(T, "same handle, dense A", [x], A, [x], 0.4, same=True)
    hAt = T.DeviceTTO(to_product(At))
    _, xbar_t, ybar_t = T.sandwich_pullback(hx, hAt, hx, delta=0.4)
    _, bx, by = ER.sandwich_pullback_bound(x, A, x, 0.4)
    _, bxt, byt = ER.sandwich_pullback_bound(x, At, x, 0.4)
    w = max(_share(xbar.download(0).ttv_vec, ybar_t.download(0).ttv_vec, [p + q for p, q in zip(bx, byt)]),
            _share(ybar.download(0).ttv_vec, xbar_t.download(0).ttv_vec, [p + q for p, q in zip(by, bxt)]))
    print("xbar(A) against ybar(A^T): largest share of the summed bounds %.3g" % w)
    # and the two tangents of a non-symmetric operator are different
    assert max(float(np.max(np.abs(a - b))) for a, b in zip(xbar.download(0).ttv_vec, ybar.download(0).ttv_vec)) > 0.0
    _free(hx, hA, hAt, xbar, ybar, xbar_t, ybar_t)


def _rayleigh_case(case):
    rng = np.random.default_rng(70)
    if case == "mixed":
        dims = (3, 2, 4, 2, 3)
        return _rand_op(dims, [1, 3, 3, 3, 3, 1], rng), O.rand_tt(dims, [1, 3, 5, 4, 2, 1], rng)
    return O.Delta(6), O.rand_tt((2,) * 6, [1, 2, 4, 8, 4, 2, 1], rng)


@pytest.mark.parametrize("case", ["mixed", "delta6"])
def test_fused_rayleigh(T, case):
    """fused=True against the restatement under its derived bound, and against the composed fused=False within the bound of the two
    forms (tests/expect_grad_reference.py); the two cases of test_gpu_grad.py::test_rayleigh_gradient_device_finite_difference."""
    H, psi = _rayleigh_case(case)
    dH, x = T.DeviceTTO(to_product(H)), _up(T, [psi])
    E, g = T.rayleigh_value_and_grad(dH, x, fused=True)
    Er, gr = ER.rayleigh_value_and_grad(H, psi)
    sc = _scale(psi, H, psi) / O.dot(psi, psi)
    assert abs(E[0] - Er) <= 2e-12 * sc
    got = g.download(0).ttv_vec
    w1 = _share(got, gr, ER.rayleigh_fused_bound(H, psi))
    Ec, gc = T.rayleigh_value_and_grad(dH, x)
    assert abs(E[0] - Ec[0]) <= 2e-12 * sc
    w2 = _share(got, gc.download(0).ttv_vec, ER.rayleigh_composed_bound(H, psi))
    print("fused rayleigh %s: share of the fused bound %.3g, of the composed bound %.3g" % (case, w1, w2))
    _same(x, [psi])
    # expect_value_and_grad is xbar + ybar, and the host-train forms run the same kernels
    ev, eg = T.expect_value_and_grad(dH, x)
    sv, sg = ER.expect_value_and_grad(H, psi)
    _, bx, by = ER.sandwich_pullback_bound(psi, H, psi)
    assert abs(ev[0] - sv) <= 1e-12 * _scale(psi, H, psi)
    _share(eg.download(0).ttv_vec, sg, [p + q + 2 * EPS * np.abs(s) for p, q, s in zip(bx, by, sg)])
    Eh, gh = T.rayleigh_gradient(to_product(H), to_product(psi), fused=True)
    assert Eh == E[0] and all(np.array_equal(a, b) for a, b in zip(gh, got))
    val, pb = T.sandwich_rrule(to_product(psi), to_product(H), to_product(psi))
    xb, yb = pb(0.3)
    rv, rx, ry = ER.sandwich_pullback(psi, H, psi, 0.3)
    _, bx, by = ER.sandwich_pullback_bound(psi, H, psi, 0.3)
    assert abs(val - rv) <= 1e-12 * _scale(psi, H, psi)
    _share(xb, rx, bx)
    _share(yb, ry, by)
    _free(dH, x, g, gc, eg)


def _err(T, rc, code, word):
    assert rc == code, (rc, T._lib.last_error())
    assert word in T._lib.last_error(), T._lib.last_error()


def test_refusals_write_nothing(T):
    L, lib = T._lib.lib(), T._lib
    dims = (2, 3, 2)
    rng = np.random.default_rng(105)
    X, Y = O.rand_tt(dims, [1, 2, 3, 1], rng), O.rand_tt(dims, [1, 2, 2, 1], rng)
    keep, keep2, small_t = O.rand_tt(dims, [1, 2, 3, 1], rng), O.rand_tt(dims, [1, 2, 2, 1], rng), O.rand_tt(dims, [1, 1, 1, 1], rng)
    H = _rand_op(dims, [1, 2, 2, 1], rng)
    x, y, dst, dst2, small = _up(T, [X]), _up(T, [Y]), _up(T, [keep]), _up(T, [keep2]), _up(T, [small_t])
    other = _up(T, [O.rand_tt((2, 2, 2), [1, 2, 2, 1], rng)])
    two = _up(T, [X, X])
    zc = T.DeviceTT(dims, [1, 2, 3, 1], 1, dtype=np.complex128)
    dH = T.DeviceTTO(to_product(H))
    dHo = T.DeviceTTO(to_product(_rand_op((2, 2, 2), [1, 2, 2, 1], rng)))
    Hc = T.DeviceTTO(T.TToperator(3, [c.astype(np.complex128) for c in H.tto_vec], dims, H.tto_rks, [0] * 3))
    out = (C.c_double * 1)(7.0)
    f = L.ttn_sandwich_pullback

    def ok():
        val, xb, yb = T.sandwich_pullback(x, dH, y, delta=0.5)
        rv, rx, ry = ER.sandwich_pullback(X, H, Y, 0.5)
        _, bx, by = ER.sandwich_pullback_bound(X, H, Y, 0.5)
        assert abs(val[0] - rv) <= 1e-12 * _scale(X, H, Y)
        _share(xb.download(0).ttv_vec, rx, bx)
        _share(yb.download(0).ttv_vec, ry, by)
        _free(xb, yb)

    ok()
    # TTN_ERR_ARG
    for args in ((None, dH.h, y.h, None, dst.h, None), (x.h, None, y.h, None, dst.h, None), (x.h, dH.h, None, None, dst.h, None)):
        _err(T, f(*args, out), lib.TTN_ERR_ARG, "null")
    _err(T, f(x.h, dH.h, y.h, None, None, None, out), lib.TTN_ERR_ARG, "neither")
    for args in ((x.h, dH.h, y.h, None, x.h, None), (x.h, dH.h, y.h, None, y.h, None), (x.h, dH.h, y.h, None, None, x.h), (x.h, dH.h, y.h, None, None, y.h),
                 (x.h, dH.h, y.h, None, dst.h, dst.h)):
        _err(T, f(*args, out), lib.TTN_ERR_ARG, "alias")
    ok()
    # TTN_ERR_DIMS
    for args in ((other.h, dH.h, y.h, None, dst.h, None), (x.h, dH.h, other.h, None, dst.h, None), (x.h, dHo.h, y.h, None, dst.h, None),
                 (x.h, dH.h, y.h, None, other.h, None), (x.h, dH.h, y.h, None, None, other.h)):
        _err(T, f(*args, out), lib.TTN_ERR_DIMS, "dimensions")
    _err(T, f(x.h, dH.h, two.h, None, dst.h, None, out), lib.TTN_ERR_DIMS, "batch")
    _err(T, f(x.h, dH.h, y.h, None, two.h, None, out), lib.TTN_ERR_DIMS, "batch")
    ok()
    # TTN_ERR_CAPACITY: xbar against x's bounds, ybar against y's (dst2 has y's capacity: too small for x)
    _err(T, f(x.h, dH.h, y.h, None, small.h, None, out), lib.TTN_ERR_CAPACITY, "capacity")
    _err(T, f(x.h, dH.h, y.h, None, dst.h, small.h, out), lib.TTN_ERR_CAPACITY, "capacity")
    _err(T, f(x.h, dH.h, y.h, None, dst2.h, None, out), lib.TTN_ERR_CAPACITY, "capacity")
    ok()
    # TTN_ERR_UNSUPPORTED: a ComplexF64 handle in every position
    for args in ((zc.h, dH.h, y.h, None, dst.h, None), (x.h, Hc.h, y.h, None, dst.h, None), (x.h, dH.h, zc.h, None, dst.h, None),
                 (x.h, dH.h, y.h, None, zc.h, None), (x.h, dH.h, y.h, None, dst.h, zc.h)):
        _err(T, f(*args, out), lib.TTN_ERR_UNSUPPORTED, "Float64 only")
    # ... and the 480-site limit of ttn_sandwich
    dl = 481
    xl = T.DeviceTT((2,) * dl, [1] * (dl + 1), batch=1)
    xlb = T.DeviceTT((2,) * dl, [1] * (dl + 1), batch=1)
    Il = T.DeviceTTO(T.TToperator(dl, [np.eye(2).reshape(2, 2, 1, 1).copy() for _ in range(dl)], (2,) * dl, [1] * (dl + 1), [0] * dl))
    _err(T, f(xl.h, Il.h, xl.h, None, xlb.h, None, out), lib.TTN_ERR_UNSUPPORTED, "480")
    ok()
    # the Python wrapper raises what its siblings raise
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        T.sandwich_pullback(other, dH, y)
    with pytest.raises(T.TTNError, match="Float64 only"):
        T.sandwich_pullback(x, dH, zc, xbar=dst, want_ybar=False)
    # nothing was written
    assert out[0] == 7.0
    _same(dst, [keep])
    _same(dst2, [keep2])
    _same(small, [small_t])
    _same(x, [X])
    _same(y, [Y])
    ok()
    T.device.compress_status(dst)
    _free(x, y, dst, dst2, small, other, two, zc, dH, dHo, Hc, xl, xlb, Il)
