"""GPU checks of the core gradients (csrc/ttn_grad_kernels.h, ttn_amd.grad) against the NumPy restatement of the reference's
ChainRulesCore extension (tests/grad_reference.py, pinned to test/test_ad.jl by tests/test_cpu_grad.py).

Tolerances are derived, not measured: a nested sum of products computed in any order, FMA included, satisfies
|fl - exact| <= p eps S_abs with S_abs the same formula on the absolute values and p the number of terms along the longest chain; device
and restatement both round, so every entry must agree to 2 p eps S_abs (GR.dot_pullback_bound / GR.apply_pullback_bound).  Each case
prints the largest share of its bound it used (recorded in DESIGN.md 4.19)."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import grad_reference as GR
from tests.helpers import to_oracle, to_product, worst_of
from tests.test_cpu_grad import FD_EPS, _close, _dirs, _ising, _rand_op, check_descent, descent_setup

pytestmark = pytest.mark.gpu
EPS = GR.EPS


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _up(T, trains, cap=None, dims=None):
    """Oracle trains into one handle (capacity: the bondwise maximum unless given)."""
    dims = dims or trains[0].ttv_dims
    if cap is None:
        cap = [max(t.ttv_rks[m] for t in trains) for m in range(len(dims) + 1)]
    h = T.DeviceTT(dims, cap, batch=len(trains))
    for b, t in enumerate(trains):
        h.upload(b, to_product(t))
    return h


def _same(T, h, trains):
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
        assert np.all(err <= bd), "entry beyond 2 p eps S_abs: worst ratio %.3g" % float(np.max(err / np.maximum(bd, 1e-300)))
        nz = bd > 0
        if np.any(nz):
            worst = worst_of(worst, float(np.max(err[nz] / bd[nz])))
    return worst


def _check_dot_pullback(T, name, As, Bs, deltas, same_handle=False):
    a = _up(T, As)
    b = a if same_handle else _up(T, Bs)
    val, abar, bbar = T.dot_pullback(a, b, delta=deltas)
    worst = 0.0
    for t, (A, B) in enumerate(zip(As, Bs)):
        dl = 1.0 if deltas is None else float(np.broadcast_to(deltas, (len(As),))[t])
        rv, ra, rb = GR.dot_pullback(A, B, dl)
        _, ba, bb = GR.dot_pullback_bound(A, B, dl)
        ga, gb = abar.download(t), bbar.download(t)
        assert ga.ttv_rks == list(A.ttv_rks) and gb.ttv_rks == list(B.ttv_rks) and ga.ttv_ot == [0] * A.N
        worst = worst_of(worst, _share(ga.ttv_vec, ra, ba), _share(gb.ttv_vec, rb, bb))
        assert abs(val[t] - O.dot(A, B)) <= 1e-12 * O.norm(A) * O.norm(B)            # the tolerance of the dot parity tests
        assert abs(val[t] - rv) <= 1e-12 * O.norm(A) * O.norm(B)
    print("dot_pullback %s: largest share of the bound %.3g" % (name, worst))
    _same(T, a, As)
    _same(T, b, Bs)
    return a, b, abar, bbar


def _rt(dims, rks, seed):
    return O.rand_tt(dims, rks, np.random.default_rng(seed))


DOT_CASES = {
    "d1": ((3,), [1, 1], [1, 1]),
    "d2": ((2, 3), [1, 4, 1], [1, 2, 1]),
    "tile_edges": ((2,) * 8, [1, 2, 4, 15, 16, 17, 4, 2, 1], [1, 2, 3, 5, 5, 5, 3, 2, 1]),
    "lds_edge_rank5": ((2,) * 6, [1, 2, 63, 64, 65, 2, 1], [1, 2, 4, 5, 4, 2, 1]),
    "mixed_dims": ((3, 2, 4, 2, 3), [1, 3, 5, 4, 2, 1], [1, 2, 7, 3, 3, 1]),
}


@pytest.mark.parametrize("name", list(DOT_CASES))
def test_dot_pullback_shapes(T, name):
    dims, ra, rb = DOT_CASES[name]
    A, B = _rt(dims, ra, 11), _rt(dims, rb, 12)
    _check_dot_pullback(T, name, [A], [B], -0.75)


def test_dot_pullback_same_handle(T):
    """a and b the same handle, at the edge of the LDS-resident class (63 / 64 / 65)."""
    A = _rt((2,) * 6, [1, 2, 63, 64, 65, 2, 1], 13)
    _check_dot_pullback(T, "same handle", [A], [A], None, same_handle=True)


def test_dot_pullback_psi_and_H_psi(T):
    """(psi, Delta psi): ranks up to 64 against up to 192 — ramp sites on the LDS route, the body on the workgroup GEMM, one call."""
    psi = _rt((2,) * 10, [1, 2, 4, 16, 64, 64, 64, 64, 16, 4, 1], 14)
    Y = O.apply(O.Delta(10), psi)
    assert max(Y.ttv_rks) == 192
    _check_dot_pullback(T, "(psi, Delta psi)", [psi], [Y], 1.0 / O.dot(psi, psi))


def test_dot_pullback_ragged_batch_and_single_outputs(T):
    """Five trains with five rank vectors under one capacity, one cotangent each; then abar alone, bbar alone, and no value."""
    dims = (2,) * 6
    ras = [[1, 2, 4, 20, 4, 2, 1], [1, 1, 1, 1, 1, 1, 1], [1, 2, 3, 16, 3, 2, 1], [1, 2, 4, 17, 2, 1, 1], [1, 1, 2, 7, 4, 2, 1]]
    rbs = [[1, 2, 3, 5, 3, 2, 1], [1, 2, 4, 18, 4, 2, 1], [1, 1, 1, 1, 1, 1, 1], [1, 2, 4, 16, 4, 2, 1], [1, 2, 2, 2, 2, 2, 1]]
    As = [_rt(dims, r, 20 + i) for i, r in enumerate(ras)]
    Bs = [_rt(dims, r, 30 + i) for i, r in enumerate(rbs)]
    deltas = np.array([1.0, -2.0, 0.5, 3.0, -0.125])
    a, b, abar, bbar = _check_dot_pullback(T, "ragged batch", As, Bs, deltas)
    L = T._lib.lib()
    arr = (C.c_double * 5)(*deltas.tolist())
    a1, b1 = T.DeviceTT(dims, a.cap, 5), T.DeviceTT(dims, b.cap, 5)
    assert L.ttn_dot_pullback(a.h, b.h, arr, a1.h, None, None) == 0
    assert L.ttn_dot_pullback(a.h, b.h, arr, None, b1.h, None) == 0
    for t in range(5):
        _, ra_, rb_ = GR.dot_pullback(As[t], Bs[t], deltas[t])
        _, ba_, bb_ = GR.dot_pullback_bound(As[t], Bs[t], deltas[t])
        _share(a1.download(t).ttv_vec, ra_, ba_)
        _share(b1.download(t).ttv_vec, rb_, bb_)
    _same(T, a, As)
    _same(T, b, Bs)


def _check_apply_pullback(T, name, H, xs):
    rng = np.random.default_rng(50)
    yrks = [[R * r for R, r in zip(H.tto_rks, x.ttv_rks)] for x in xs]
    ybs = [O.rand_tt(H.tto_dims, rk, rng) for rk in yrks]
    dH = T.DeviceTTO(to_product(H))
    x, yb = _up(T, xs), _up(T, ybs)
    xb = T.apply_pullback(dH, x, yb)
    worst = 0.0
    for t, xt in enumerate(xs):
        ref = GR.apply_pullback(H, ybs[t].ttv_vec, xt.ttv_rks)
        got = xb.download(t)
        assert got.ttv_rks == list(xt.ttv_rks)
        worst = worst_of(worst, _share(got.ttv_vec, ref, GR.apply_pullback_bound(H, ybs[t].ttv_vec, xt.ttv_rks)))
    print("apply_pullback %s: largest share of the bound %.3g" % (name, worst))
    _same(T, x, xs)
    _same(T, yb, ybs)
    back = dH.download()
    assert all(np.array_equal(p, q) for p, q in zip(back.tto_vec, H.tto_vec))


@pytest.mark.parametrize("name", ["delta", "ising", "random", "ragged"])
def test_apply_pullback(T, name):
    if name == "delta":
        _check_apply_pullback(T, name, O.Delta(7), [_rt((2,) * 7, [1, 2, 4, 7, 9, 4, 2, 1], 60)])
    elif name == "ising":
        _check_apply_pullback(T, name, _ising(6), [_rt((2,) * 6, [1, 2, 3, 5, 4, 2, 1], 61)])
    elif name == "random":
        dims = (3, 2, 4, 2)
        _check_apply_pullback(T, name, _rand_op(dims, [1, 2, 3, 2, 1], np.random.default_rng(62)), [_rt(dims, [1, 3, 5, 2, 1], 63)])
    else:
        xs = [_rt((2,) * 6, r, 64 + i) for i, r in enumerate([[1, 2, 4, 8, 4, 2, 1], [1, 1, 2, 3, 2, 1, 1], [1, 2, 4, 5, 3, 2, 1]])]
        _check_apply_pullback(T, name, O.Delta(6), xs)


def _device_rayleigh(T, dH, psi, Y):
    T.device.apply(dH, psi, Y)
    return T.device.dot(psi, Y) / T.device.dot(psi, psi)


@pytest.mark.parametrize("case", ["mixed", "delta6"])
def test_rayleigh_gradient_device_finite_difference(T, case):
    """The directional derivative of rayleigh_value_and_grad against a central difference of device dot / apply at eps = 1e-6
    (rtol 1e-5, atol 1e-7: test_ad.jl:113), and the gradient itself against the restatement."""
    rng = np.random.default_rng(70)
    if case == "mixed":
        dims = (3, 2, 4, 2, 3)
        H, psi = _rand_op(dims, [1, 3, 3, 3, 3, 1], rng), O.rand_tt(dims, [1, 3, 5, 4, 2, 1], rng)
    else:
        H, psi = O.Delta(6), O.rand_tt((2,) * 6, [1, 2, 4, 8, 4, 2, 1], rng)
    dirs = _dirs(psi, rng)
    dH = T.DeviceTTO(to_product(H))
    x = _up(T, [psi])
    E, g = T.rayleigh_value_and_grad(dH, x)
    Er, gr = GR.rayleigh_value_and_grad(H, psi)
    assert abs(E[0] - Er) <= 1e-12 * max(1.0, abs(Er))
    got = g.download(0).ttv_vec
    scale = max(float(np.max(np.abs(c))) for c in gr)
    # (four pullbacks of a few hundred terms each, summed: 1e-11 of the largest entry is a hundred times their joint bound)
    assert all(np.allclose(a, b, rtol=0, atol=1e-11 * scale) for a, b in zip(got, gr))
    Y = T.DeviceTT(psi.ttv_dims, [R * r for R, r in zip(H.tto_rks, psi.ttv_rks)], 1)
    Ep = _device_rayleigh(T, dH, _up(T, [GR.shifted(psi, dirs, FD_EPS)]), Y)[0]
    Em = _device_rayleigh(T, dH, _up(T, [GR.shifted(psi, dirs, -FD_EPS)]), Y)[0]
    fd = (Ep - Em) / (2 * FD_EPS)
    print("device FD %s: AD %.12g FD %.12g" % (case, GR.ladot(got, dirs), fd))
    assert _close(GR.ladot(got, dirs), fd)
    _same(T, x, [psi])
    # the host-train forms run the same kernels
    Eh, gh = T.rayleigh_gradient(to_product(H), to_product(psi))
    assert Eh == E[0] and all(np.array_equal(a, b) for a, b in zip(gh, got))


def test_host_rrules(T):
    rng = np.random.default_rng(75)
    dims = (3, 2, 4, 2)
    A, B = O.rand_tt(dims, [1, 3, 4, 2, 1], rng), O.rand_tt(dims, [1, 2, 5, 3, 1], rng)
    val, pb = T.dot_rrule(to_product(A), to_product(B))
    ab, bb = pb(0.3)
    rv, ra, rb = GR.dot_pullback(A, B, 0.3)
    _, ba, bbd = GR.dot_pullback_bound(A, B, 0.3)
    assert abs(val - rv) <= 1e-12 * O.norm(A) * O.norm(B)
    _share(ab, ra, ba)
    _share(bb, rb, bbd)
    H = _rand_op(dims, [1, 2, 3, 2, 1], rng)
    Y, pb2 = T.apply_rrule(to_product(H), to_product(A))
    Yr = O.apply(H, A)
    assert Y.ttv_rks == Yr.ttv_rks
    ybar = [rng.standard_normal(c.shape) for c in Yr.ttv_vec]
    _share(pb2(ybar), GR.apply_pullback(H, ybar, A.ttv_rks), GR.apply_pullback_bound(H, ybar, A.ttv_rks))


def test_cores_axpby_and_dot(T):
    """Per-train alpha / beta on a ragged batch, x the same handle as y, against NumPy on downloaded cores.  Bounds: axpby is two
    products and a sum, each side rounding at most twice: 4 eps (|alpha x| + |beta y|); the pairing is a sum of m products:
    2 m eps sum |x| |y|."""
    dims = (2, 3, 2, 2)
    rks = [[1, 2, 6, 2, 1], [1, 1, 1, 1, 1], [1, 2, 5, 1, 1]]
    xs = [_rt(dims, r, 80 + i) for i, r in enumerate(rks)]
    ys = [_rt(dims, r, 90 + i) for i, r in enumerate(rks)]
    al, be = np.array([0.5, -2.0, 3.25]), np.array([1.5, 0.25, -1.0])
    x, y = _up(T, xs), _up(T, ys, cap=[1, 3, 8, 4, 1])                    # (different capacities: different slot offsets)
    pair = T.cores_dot(x, y)
    assert np.array_equal(pair, T.cores_dot(x, y))                        # fixed summation order: the same bits
    for t in range(3):
        m = sum(c.size for c in xs[t].ttv_vec)
        ref = GR.ladot(xs[t].ttv_vec, ys[t].ttv_vec)
        assert abs(pair[t] - ref) <= 2 * m * EPS * GR.ladot([np.abs(c) for c in xs[t].ttv_vec], [np.abs(c) for c in ys[t].ttv_vec])
    T.cores_axpby(al, x, be, y)
    _same(T, x, xs)
    now = []
    for t in range(3):
        got = y.download(t).ttv_vec
        ref = [al[t] * a + be[t] * b for a, b in zip(xs[t].ttv_vec, ys[t].ttv_vec)]
        _share(got, ref, [4 * EPS * (np.abs(al[t] * a) + np.abs(be[t] * b)) for a, b in zip(xs[t].ttv_vec, ys[t].ttv_vec)])
        now.append(got)
    T.cores_axpby(al, y, be, y)                                           # x is y
    for t in range(3):
        ref = [al[t] * a + be[t] * a for a in now[t]]
        _share(y.download(t).ttv_vec, ref, [4 * EPS * (np.abs(al[t] * a) + np.abs(be[t] * a)) for a in now[t]])
    last = [y.download(t).ttv_vec for t in range(3)]
    T.cores_axpby(None, x, None, y)                                       # NULL: 1 and 1
    for t in range(3):
        _share(y.download(t).ttv_vec, [a + b for a, b in zip(xs[t].ttv_vec, last[t])], [4 * EPS * (np.abs(a) + np.abs(b)) for a, b in zip(xs[t].ttv_vec, last[t])])
    T.device.compress_status(y)


def _err(T, rc, code, word):
    assert rc == code, (rc, T._lib.last_error())
    assert word in T._lib.last_error(), T._lib.last_error()


def test_refusals_write_nothing(T):
    L, lib = T._lib.lib(), T._lib
    dims = (2, 3, 2)
    A, B = _rt(dims, [1, 2, 3, 1], 100), _rt(dims, [1, 2, 2, 1], 101)
    keep = _rt(dims, [1, 2, 3, 1], 102)
    a, b = _up(T, [A]), _up(T, [B])
    dst = _up(T, [keep])
    out = (C.c_double * 1)(7.0)
    other = _up(T, [_rt((2, 2, 2), [1, 2, 2, 1], 103)])
    two = _up(T, [A, A])
    small = _up(T, [_rt(dims, [1, 1, 1, 1], 104)])
    zc = T.DeviceTT(dims, [1, 2, 3, 1], 1, dtype=np.complex128)
    H = _rand_op(dims, [1, 2, 2, 1], np.random.default_rng(105))
    dH = T.DeviceTTO(to_product(H))
    Hc = T.DeviceTTO(T.TToperator(3, [c.astype(np.complex128) for c in H.tto_vec], dims, H.tto_rks, [0] * 3))
    yb = _up(T, [_rt(dims, [1, 4, 6, 1], 106)])
    # dot_pullback
    _err(T, L.ttn_dot_pullback(a.h, b.h, None, None, None, out), lib.TTN_ERR_ARG, "neither")
    _err(T, L.ttn_dot_pullback(a.h, None, None, dst.h, None, out), lib.TTN_ERR_ARG, "null")
    _err(T, L.ttn_dot_pullback(a.h, other.h, None, dst.h, None, out), lib.TTN_ERR_DIMS, "dimensions")
    _err(T, L.ttn_dot_pullback(a.h, b.h, None, None, other.h, out), lib.TTN_ERR_DIMS, "dimensions")
    _err(T, L.ttn_dot_pullback(a.h, two.h, None, dst.h, None, out), lib.TTN_ERR_DIMS, "batch")
    _err(T, L.ttn_dot_pullback(a.h, b.h, None, small.h, None, out), lib.TTN_ERR_CAPACITY, "capacity")
    for args in ((zc.h, b.h, None, dst.h, None), (a.h, zc.h, None, dst.h, None), (a.h, b.h, None, zc.h, None), (a.h, b.h, None, dst.h, zc.h)):
        _err(T, L.ttn_dot_pullback(*args, out), lib.TTN_ERR_UNSUPPORTED, "ttn_dot_pullback")
    # apply_pullback
    _err(T, L.ttn_apply_pullback(dH.h, a.h, yb.h, None), lib.TTN_ERR_ARG, "null")
    _err(T, L.ttn_apply_pullback(dH.h, other.h, yb.h, dst.h), lib.TTN_ERR_DIMS, "dimensions")
    _err(T, L.ttn_apply_pullback(dH.h, two.h, yb.h, dst.h), lib.TTN_ERR_DIMS, "batch")
    _err(T, L.ttn_apply_pullback(dH.h, a.h, yb.h, small.h), lib.TTN_ERR_CAPACITY, "capacity")
    for args in ((Hc.h, a.h, yb.h, dst.h), (dH.h, zc.h, yb.h, dst.h), (dH.h, a.h, zc.h, dst.h), (dH.h, a.h, yb.h, zc.h)):
        _err(T, L.ttn_apply_pullback(*args), lib.TTN_ERR_UNSUPPORTED, "ttn_apply_pullback")
    # cores_axpby / cores_dot
    _err(T, L.ttn_tt_cores_axpby(None, other.h, None, dst.h), lib.TTN_ERR_DIMS, "dimensions")
    _err(T, L.ttn_tt_cores_axpby(None, two.h, None, dst.h), lib.TTN_ERR_DIMS, "batch")
    _err(T, L.ttn_tt_cores_axpby(None, a.h, None, small.h), lib.TTN_ERR_CAPACITY, "capacity")
    _err(T, L.ttn_tt_cores_axpby(None, zc.h, None, dst.h), lib.TTN_ERR_UNSUPPORTED, "ttn_tt_cores_axpby")
    _err(T, L.ttn_tt_cores_axpby(None, a.h, None, zc.h), lib.TTN_ERR_UNSUPPORTED, "ttn_tt_cores_axpby")
    _err(T, L.ttn_tt_cores_dot(a.h, dst.h, None), lib.TTN_ERR_ARG, "null")
    _err(T, L.ttn_tt_cores_dot(a.h, other.h, out), lib.TTN_ERR_DIMS, "dimensions")
    _err(T, L.ttn_tt_cores_dot(zc.h, a.h, out), lib.TTN_ERR_UNSUPPORTED, "ttn_tt_cores_dot")
    _err(T, L.ttn_tt_cores_dot(a.h, zc.h, out), lib.TTN_ERR_UNSUPPORTED, "ttn_tt_cores_dot")
    # nothing was written
    assert out[0] == 7.0
    _same(T, dst, [keep])
    _same(T, small, [_rt(dims, [1, 1, 1, 1], 104)])
    _same(T, a, [A])
    _same(T, b, [B])
    T.device.compress_status(dst)


def test_rank_mismatch_is_per_train(T):
    """Ranks live on the device: a ybar whose ranks are not R .* x marks that train alone (TTN_ST_RANKS_DIFFER through compress_status);
    its destination cores stay as they were and the other trains are computed.  The same for cores_axpby; cores_dot gives NaN."""
    H = O.Delta(5)
    dims = (2,) * 5
    xs = [_rt(dims, [1, 2, 3, 3, 2, 1], 110 + i) for i in range(3)]
    rng = np.random.default_rng(113)
    good = [3 * r for r in xs[0].ttv_rks]
    good[0] = good[-1] = 1
    bad = list(good)
    bad[2] -= 1
    ybs = [O.rand_tt(dims, good, rng), O.rand_tt(dims, bad, rng), O.rand_tt(dims, good, rng)]
    before = [_rt(dims, [1, 2, 3, 3, 2, 1], 120 + i) for i in range(3)]
    x, yb, xb = _up(T, xs), _up(T, ybs), _up(T, before)
    dH = T.DeviceTTO(to_product(H))
    T.apply_pullback(dH, x, yb, xb)
    with pytest.raises(AssertionError, match="ranks differ"):
        T.device.compress_status(xb)
    T.device.compress_status(xb)                                          # reported once, then cleared
    for t in (0, 2):
        _share(xb.download(t).ttv_vec, GR.apply_pullback(H, ybs[t].ttv_vec, xs[t].ttv_rks), GR.apply_pullback_bound(H, ybs[t].ttv_vec, xs[t].ttv_rks))
    assert all(np.array_equal(p, q) for p, q in zip(xb.download(1).ttv_vec, before[1].ttv_vec))
    # axpby / cores_dot: train 1 of u has other ranks than train 1 of v
    us = [xs[0], _rt(dims, [1, 2, 2, 3, 2, 1], 130), xs[2]]
    u, v = _up(T, us, cap=[1, 2, 3, 3, 2, 1]), _up(T, before)
    pair = T.cores_dot(u, v)
    assert math.isnan(pair[1])
    for t in (0, 2):
        m = sum(c.size for c in us[t].ttv_vec)
        assert abs(pair[t] - GR.ladot(us[t].ttv_vec, before[t].ttv_vec)) <= 2 * m * EPS * GR.ladot([np.abs(c) for c in us[t].ttv_vec], [np.abs(c) for c in before[t].ttv_vec])
    T.cores_axpby([2.0] * 3, u, [1.0] * 3, v)
    with pytest.raises(AssertionError, match="ranks differ"):
        T.device.compress_status(v)
    assert all(np.array_equal(p, q) for p, q in zip(v.download(1).ttv_vec, before[1].ttv_vec))
    for t in (0, 2):
        assert all(np.allclose(p, 2.0 * a + q, rtol=0, atol=8 * EPS * (np.abs(2 * a) + np.abs(q)).max())
                   for p, a, q in zip(v.download(t).ttv_vec, us[t].ttv_vec, before[t].ttv_vec))
    _same(T, u, us)


def test_descent_on_handles(T):
    """test_ad.jl:116-168 on a batch of three resident trains: 200 steps of backtracking gradient descent in which only energies cross
    to the host; per-train step sizes go through cores_axpby.  The four conditions of tests/test_cpu_grad.py per train, and the
    gradient at the train dmrg_eigsolve returns has sum_k ||g_k||^2 < (1e-4)^2."""
    H, starts, E_exact = descent_setup()
    dH = T.DeviceTTO(to_product(H))
    psi = _up(T, starts)
    cand, g = T.DeviceTT(psi.dims, psi.cap, 3), T.DeviceTT(psi.dims, psi.cap, 3)
    Y = T.DeviceTT(psi.dims, [R * c for R, c in zip(H.tto_rks, psi.cap)], 3)
    L = T._lib.lib()

    def step_to(alpha):
        T._lib.check(L.ttn_tt_copy(cand.h, psi.h))
        T.cores_axpby(-alpha, g, None, cand)
        return _device_rayleigh(T, dH, cand, Y)

    E = _device_rayleigh(T, dH, psi, Y)
    hist = [E.copy()]
    alpha = np.full(3, 0.05)
    for _ in range(200):
        T.rayleigh_value_and_grad(dH, psi, g)
        Etry = step_to(alpha)
        while True:
            back = (Etry > E) & (alpha > 1e-12)
            if not back.any():
                break
            alpha = np.where(back, alpha / 2, alpha)
            Etry = step_to(alpha)
        psi, cand = cand, psi
        E = Etry
        hist.append(E.copy())
        alpha = alpha * 1.5
    hist = np.array(hist)
    for t in range(3):
        print("device descent train %d: E0 %.4f -> %.6f, exact %.6f" % (t, hist[0, t], hist[-1, t], E_exact))
        check_descent(list(hist[:, t]), E_exact)
    # the gradient vanishes at an eigenvector
    _, xd, _ = T.dmrg_eigsolve(to_product(H), T.rand_tt((2,) * 10, 2, seed=9), sweep_schedule=[2, 4], rmax_schedule=[16, 16], tol=1e-10)
    dx = T.DeviceTT.from_host(xd)
    Ed, gd = T.rayleigh_value_and_grad(dH, dx)
    g2 = T.cores_dot(gd, gd)[0]
    print("gradient at the DMRG train: E %.8f, sum ||g_k||^2 %.3g" % (Ed[0], g2))
    assert abs(Ed[0] - E_exact) < 1e-6 and g2 < (1e-4) ** 2
