"""GPU checks of the fixed-rank manifold (csrc/ttn_tangent_kernels.h, ttn_amd.manifold) against the NumPy restatement
(tests/tangent_reference.py, pinned to a dense projector by tests/test_cpu_tangent.py).

The entrywise cases upload the ORACLE's gauges U and V, so both sides project in the same gauge and every entry of every dC_k must agree
to 2 p eps S_abs (R.project_bound: the formula on absolute values, |U_k| |L_{k+1}| included).  Each case prints the largest share of its
bound it used (recorded in DESIGN.md 4.33).  Ranks of x are feasible for orthonormal cores: r_k <= n_k r_{k-1} and r_{k-1} <= n_k r_k.

Tolerances that the bound does not cover:
  * <x, z>: 1e-12 ||x|| ||z||, the tolerance of the dot parity tests;
  * the gauge residual U_k^T dC_k: |U_k|^T bound_k for the error of dC_k, plus |I - U_k^T U_k| |U_k|^T S_abs for the orthogonality defect
    of the uploaded U_k itself (a property of the input, measured from it);
  * beta dC_d + alpha U_d: the device rounds alpha U and the fused sum, NumPy rounds both products and the sum — each side is within
    eps (|alpha U| + |beta dC|) of the exact value, so they agree to 2 eps (|alpha U| + |beta dC|);
  * dense tensors of trains that went through different gauges or an SVD: 1e-9 of the largest entry, the project's tensor parity."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import tangent_reference as R
from tests.helpers import to_oracle, to_product, worst_of

pytestmark = pytest.mark.gpu
EPS = R.EPS
QNAN = 0x7FF8000000000000
BIG = int(np.float64(1e300).view(np.uint64))


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _rt(dims, rks, seed):
    return O.rand_tt(dims, rks, np.random.default_rng(seed))


def _up(T, trains, cap=None):
    dims = trains[0].ttv_dims
    if cap is None:
        cap = [max(t.ttv_rks[m] for t in trains) for m in range(len(dims) + 1)]
    h = T.DeviceTT(dims, cap, batch=len(trains))
    for b, t in enumerate(trains):
        h.upload(b, to_product(t))
    return h


def _same(h, trains):
    for b, t in enumerate(trains):
        got = h.download(b)
        assert got.ttv_rks == list(t.ttv_rks)
        assert all(np.array_equal(x, y) for x, y in zip(got.ttv_vec, t.ttv_vec))


def _share(got, ref, bound):
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


# name -> (dims, x ranks, [z ranks per train] or "delta": z = Delta * w with w of x's ranks)
CASES = {
    "d1": ((3,), [1, 1], [[1, 1]]),
    "d2": ((2, 3), [1, 2, 1], [[1, 3, 1]]),
    "mixed_dims": ((3, 2, 4, 2, 3), [1, 3, 5, 4, 2, 1], [[1, 2, 5, 3, 3, 1]]),
    "tile_edges": ((2,) * 12, [1, 2, 4, 8, 15, 16, 17, 16, 8, 4, 4, 2, 1], [[1, 2, 3, 5, 5, 5, 5, 5, 5, 4, 3, 2, 1]]),
    "lds_edge": ((2,) * 15, [1, 2, 4, 8, 16, 32, 63, 64, 65, 64, 32, 16, 8, 4, 2, 1], [[1, 2, 3, 5, 5, 5, 5, 5, 5, 5, 5, 5, 4, 2, 2, 1]]),
    "x64_z192": ((2,) * 13, [1, 2, 4, 8, 16, 32, 64, 64, 32, 16, 8, 4, 2, 1], "delta"),
    "batch3": ((2,) * 6, [1, 2, 4, 4, 4, 2, 1], [[1, 2, 3, 5, 3, 2, 1], [1, 1, 1, 1, 1, 1, 1], [1, 2, 4, 17, 4, 2, 1]]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(xs, Us, Vs, zs, reference cores, reference values, bounds) of a case: computed once, shared, never modified."""
    dims, rx, rz = CASES[name]
    n = 1 if rz == "delta" else len(rz)
    xs = [_rt(dims, rx, 100 + 7 * b) for b in range(n)]
    if rz == "delta":
        zs = [O.apply(O.Delta(len(dims)), _rt(dims, rx, 55))]
        assert max(zs[0].ttv_rks) == 192 and max(rx) == 64
    else:
        zs = [_rt(dims, r, 200 + 7 * b) for b, r in enumerate(rz)]
    Us, Vs = zip(*(R.gauges(x) for x in xs))
    assert all(U.ttv_rks == rx and V.ttv_rks == rx for U, V in zip(Us, Vs))
    refs = [R.project(U, V, z) for U, V, z in zip(Us, Vs, zs)]
    bounds = [R.project_bound(U, V, z)[1] for U, V, z in zip(Us, Vs, zs)]
    return xs, list(Us), list(Vs), zs, [r[0] for r in refs], [r[1] for r in refs], bounds


def _project(T, U, V, z, xi=None, want=True):
    if xi is None:
        xi = T.DeviceTT(U.dims, U.cap, U.batch)
    out = (C.c_double * U.batch)() if want else None
    rc = T._lib.lib().ttn_tangent_project(U.h, V.h, z.h, xi.h, out)
    assert rc == 0, T._lib.last_error()
    return xi, (np.array(out[:]) if want else None)


def _gauge_tolerance(U, bound_k, k, p):
    """|U_k|^T bound_k + |I - U_k^T U_k| |U_k|^T S_abs, S_abs = bound_k / (2 p eps) (module docstring)."""
    n, rl, rr = U.ttv_vec[k].shape
    Um = np.abs(U.ttv_vec[k]).reshape(n * rl, rr, order="F")
    Uk = U.ttv_vec[k].reshape(n * rl, rr, order="F")
    Bm = bound_k.reshape(n * rl, rr, order="F")
    defect = np.abs(np.eye(rr) - Uk.T @ Uk)
    return Um.T @ Bm + defect @ (Um.T @ (Bm / (2.0 * p * EPS)))


def _check_project(T, name):
    xs, Us, Vs, zs, refs, vals, bounds = case(name)
    U, V, z = _up(T, Us), _up(T, Vs), _up(T, zs)
    xi, out = _project(T, U, V, z)
    worst, gworst, rel = 0.0, 0.0, 0.0
    for b in range(len(xs)):
        got = xi.download(b)
        assert got.ttv_rks == list(Us[b].ttv_rks) and got.ttv_ot == [0] * Us[b].N
        worst = worst_of(worst, _share(got.ttv_vec, refs[b], bounds[b]))
        # the bound on absolute values grows with the length of the chain far beyond what random signs let through: also hold every
        # entry to the project's tensor parity, 1e-9 of the largest entry of the tangent (not of its core: where U_k is square, on the
        # rank ramps, dC_k is zero up to rounding)
        top = max(float(np.max(np.abs(r))) for r in refs[b])
        for g, r in zip(got.ttv_vec, refs[b]):
            rel = worst_of(rel, float(np.max(np.abs(np.asarray(g) - r))) / top)
        scale = O.norm(xs[b]) * O.norm(zs[b])
        assert abs(out[b] - O.dot(xs[b], zs[b])) <= 1e-12 * scale and abs(out[b] - vals[b]) <= 1e-12 * scale
        d = Us[b].N
        p = sum(Us[b].ttv_dims[k] * Us[b].ttv_rks[k] * zs[b].ttv_rks[k] + Us[b].ttv_rks[k + 1] * zs[b].ttv_rks[k + 1] for k in range(d)) + max(Us[b].ttv_rks) + 1
        for k in range(d - 1):
            n, rl, rr = Us[b].ttv_vec[k].shape
            res = np.abs(Us[b].ttv_vec[k].reshape(n * rl, rr, order="F").T @ np.asarray(got.ttv_vec[k]).reshape(n * rl, rr, order="F"))
            tol = _gauge_tolerance(Us[b], bounds[b][k], k, p)
            assert np.all(res <= tol), "gauge residual beyond its bound at site %d" % k
            gworst = worst_of(gworst, float(np.max(res / np.maximum(tol, 1e-300))))
    print("tangent_project %s: largest share of the bound %.3g, of the gauge-residual bound %.3g; largest error / largest entry of the tangent %.2e"
          % (name, worst, gworst, rel))
    assert rel <= 1e-9
    _same(U, Us)
    _same(V, Vs)
    _same(z, zs)
    return U, V, z, xi


@pytest.mark.parametrize("name", list(CASES))
def test_project_entrywise(T, name):
    _check_project(T, name)


def test_project_without_value_is_the_same_tangent(T):
    xs, Us, Vs, zs, refs, vals, bounds = case("mixed_dims")
    U, V, z = _up(T, Us), _up(T, Vs), _up(T, zs)
    xi, _ = _project(T, U, V, z, want=False)
    _share(xi.download(0).ttv_vec, refs[0], bounds[0])


def test_project_with_slack_capacity(T):
    """Capacity above the ranks (slots larger than the cores) on every operand and on the destination, three trains."""
    xs, Us, Vs, zs, refs, vals, bounds = case("batch3")
    cap = [1, 3, 6, 20, 6, 3, 1]
    U, V, z = _up(T, Us, cap), _up(T, Vs, cap), _up(T, zs, cap)
    xi, out = _project(T, U, V, z, xi=T.DeviceTT(Us[0].ttv_dims, cap, 3))
    for b in range(3):
        _share(xi.download(b).ttv_vec, refs[b], bounds[b])


def test_gauge_independence(T):
    """The device's own gauges of x: the dense tangent equals the restatement's (which uses the oracle's gauges) at 1e-9 max|xi|."""
    xs, Us, Vs, zs, refs, vals, bounds = case("mixed_dims")
    x, z = _up(T, xs), _up(T, zs)
    M = T.ttvector_manifold(x)
    assert M.ranks == xs[0].ttv_rks
    pt = M.gauge(x)
    xi, val = M.project(pt, z)
    y = M.to_tt(pt, xi, alpha=0.0)
    got = O.ttv_to_tensor(to_oracle(y.download(0)))
    want = R.tangent_dense(Us[0], Vs[0], refs[0])
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("gauge independence: max |xi_dev - xi_ref| / max|xi| = %.2e" % err)
    assert err <= 1e-9
    assert abs(val[0] - vals[0]) <= 1e-12 * O.norm(xs[0]) * O.norm(zs[0])
    # the inner product of tangents is the tensors' and does not depend on the gauge either
    ip = float(M.tangent_inner(xi, xi)[0])
    assert abs(ip - R.tangent_inner(refs[0], refs[0])) <= 1e-9 * abs(ip)
    # transport to the same point is the identity on tangents
    xi2 = M.transport(pt, pt, xi)
    a, b = xi.download(0).ttv_vec, xi2.download(0).ttv_vec
    assert all(np.max(np.abs(p - q)) <= 1e-9 * max(np.max(np.abs(p)), 1e-300) + 1e-12 for p, q in zip(a, b))


# ---- to_tt ----------------------------------------------------------------------------------------------------------------------------------
def _check_to_tt(T, name, alphas, betas):
    xs, Us, Vs, zs, refs, vals, bounds = case(name)
    B, d, r = len(xs), Us[0].N, Us[0].ttv_rks
    U, V = _up(T, Us), _up(T, Vs)
    xis = [O.TTvector(d, [np.array(c) for c in refs[b]], Us[b].ttv_dims, list(r), [0] * d) for b in range(B)]
    xi = _up(T, xis)
    rk = [1] + [2 * v for v in r[1:d]] + [1] if d > 1 else [1, 1]
    y = T.DeviceTT(Us[0].ttv_dims, rk, B)
    arr = lambda v: None if v is None else (C.c_double * B)(*[float(q) for q in np.broadcast_to(v, (B,))])
    rc = T._lib.lib().ttn_tangent_to_tt(U.h, V.h, xi.h, arr(alphas), arr(betas), y.h)
    assert rc == 0, T._lib.last_error()
    for b in range(B):
        al = 1.0 if alphas is None else float(np.broadcast_to(alphas, (B,))[b])
        be = 1.0 if betas is None else float(np.broadcast_to(betas, (B,))[b])
        got = y.download(b)
        assert got.ttv_rks == rk and got.ttv_ot == [0] * d
        for k in range(d):
            W, rl, rr = np.asarray(got.ttv_vec[k]), r[k], r[k + 1]
            Uk, Vk, Xk = Us[b].ttv_vec[k], Vs[b].ttv_vec[k], refs[b][k]
            if k == d - 1:
                comb = W if d == 1 else W[:, rl:, :]
                assert np.all(np.abs(comb - (be * Xk + al * Uk)) <= 2 * EPS * (np.abs(al * Uk) + np.abs(be * Xk)))
                if d > 1:
                    assert np.array_equal(W[:, :rl, :], be * Vk)
            elif k == 0:
                assert np.array_equal(W[:, :, :rr], Xk) and np.array_equal(W[:, :, rr:], Uk)
            else:
                assert np.array_equal(W[:, :rl, :rr], Vk) and np.array_equal(W[:, rl:, :rr], Xk) and np.array_equal(W[:, rl:, rr:], Uk)
                zero = W[:, :rl, rr:]
                assert not zero.any() and not np.signbit(zero).any()          # explicit +0.0, whatever the slot held
    _same(U, Us)
    _same(V, Vs)
    _same(xi, xis)
    return y


@pytest.mark.parametrize("name", ["d1", "d2", "mixed_dims", "tile_edges"])
def test_to_tt_blocks(T, name):
    _check_to_tt(T, name, -0.75, 2.5)


def test_to_tt_batch_coefficients_and_defaults(T):
    _check_to_tt(T, "batch3", [1.0, -2.0, 0.5], [0.25, 0.0, -3.0])
    _check_to_tt(T, "batch3", None, None)
    _check_to_tt(T, "batch3", None, [0.5, 1.5, 2.5])


# ---- retract --------------------------------------------------------------------------------------------------------------------------------
def _dense(t):
    return O.ttv_to_tensor(to_oracle(t))


@pytest.mark.parametrize("name", ["mixed_dims", "tile_edges"])
def test_retract(T, name):
    xs, Us, Vs, zs, refs, vals, bounds = case(name)
    x, z = _up(T, xs), _up(T, zs)
    M = T.ttvector_manifold(x)
    pt = M.gauge(x)
    xi, _ = M.project(pt, z)
    nx, nxi = O.norm(xs[0]), np.sqrt(R.tangent_inner(refs[0], refs[0]))
    t = 0.3 * nx / nxi
    q = M.retract(pt, xi, t)
    assert q.ranks(0)[0] == M.ranks
    want = O.ttv_to_tensor(R.retract(Us[0], Vs[0], refs[0], t))
    got = _dense(q.download(0))
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("retract %s: tensor parity %.2e" % (name, err))
    assert err <= 1e-9
    # a zero step reproduces x
    q0 = M.retract(pt, xi, 0.0)
    assert q0.ranks(0)[0] == M.ranks
    xd = O.ttv_to_tensor(xs[0])
    err0 = float(np.linalg.norm(_dense(q0.download(0)) - xd) / np.linalg.norm(xd))
    print("retract %s: zero step reproduces x to %.2e" % (name, err0))
    assert err0 <= 1e-12
    _same(x, xs)


def test_host_forms(T):
    xs, Us, Vs, zs, refs, vals, bounds = case("mixed_dims")
    cores, val = T.tangent_project(to_product(xs[0]), to_product(zs[0]))
    assert abs(val - vals[0]) <= 1e-12 * O.norm(xs[0]) * O.norm(zs[0])
    ip = sum(float(np.vdot(c, c)) for c in cores)
    assert abs(ip - R.tangent_inner(refs[0], refs[0])) <= 1e-9 * ip
    y = T.manifold.retract(to_product(xs[0]), cores, 0.0)
    xd = O.ttv_to_tensor(xs[0])
    assert list(y.ttv_rks) == xs[0].ttv_rks and np.linalg.norm(_dense(y) - xd) <= 1e-12 * np.linalg.norm(xd)


def test_reference_surface_on_handles_and_host_trains(T):
    p, q = O.orthogonalize(O.qtt_sin(4)), O.orthogonalize(O.qtt_sin(4, lam=2 * np.pi))
    Mr = R.ttvector_manifold(p)
    for conv in (to_product, lambda t: T.DeviceTT.from_host(to_product(t))):
        P, Q = conv(p), conv(q)
        M = T.ttvector_manifold(P)
        assert M.dims == tuple(p.ttv_dims) and M.ranks == p.ttv_rks and M.representation_size() == tuple(p.ttv_dims)
        f = lambda v: float(np.asarray(v).reshape(-1)[0])
        assert abs(f(M.inner(P, P, Q)) - Mr.inner(p, p, q)) <= 1e-12 * O.norm(p) * O.norm(q)
        assert abs(f(M.norm(P, P)) - Mr.norm(p, p)) <= 1e-12 * O.norm(p)
        assert abs(f(M.distance(P, Q)) - Mr.distance(p, q)) <= 1e-7 * O.norm(p)          # a norm through dot: the floor is sqrt(eps)
        host = lambda h: to_oracle(h.download(0) if isinstance(h, T.DeviceTT) else h)
        z = host(M.zero_vector(P))
        assert z.ttv_rks == p.ttv_rks and not any(np.asarray(c).any() for c in z.ttv_vec)
        c = host(M.copy(P))
        assert all(np.array_equal(a, b) for a, b in zip(c.ttv_vec, p.ttv_vec))
        for t in (1.0, 0.5, 0.0):
            got = _dense(host(M.retract_project(P, Q, t)))
            want = O.ttv_to_tensor(Mr.retract_project(p, q, t))
            assert np.max(np.abs(got - want)) <= 1e-9 * np.max(np.abs(want))


def test_manifold_construction_refusals(T):
    a, b = _rt((2,) * 4, [1, 2, 3, 2, 1], 1), _rt((2,) * 4, [1, 2, 2, 2, 1], 2)
    with pytest.raises(T.TTNError, match="differ in their ranks"):
        T.ttvector_manifold(_up(T, [a, b]))
    with pytest.raises(T.TTNError, match="not feasible"):
        T.ttvector_manifold(_up(T, [_rt((2,) * 3, [1, 3, 2, 1], 3)]))
    with pytest.raises(T.TTNError, match="Float64 only"):
        T.ttvector_manifold(T.DeviceTT((2, 2), [1, 2, 1], 1, dtype=np.complex128))


# ---- drivers --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_fit_fixed_rank(T, seed):
    target = O.qtt_sin(6)
    x0 = O.rand_tt((2,) * 6, target.ttv_rks, np.random.default_rng(seed))
    tg, xh = _up(T, [target]), _up(T, [x0])
    x, errs = T.fit_fixed_rank(tg, xh, 12)
    print("fit_fixed_rank seed %d: " % seed + " ".join("%.1e" % e[0] for e in errs))
    assert x.ranks(0)[0] == target.ttv_rks and len(errs) == 12
    assert errs[-1][0] < 1e-6
    _same(xh, [x0])
    _same(tg, [target])


@functools.lru_cache(maxsize=None)
def _descent_start():
    x0 = O.rand_tt((2,) * 5, 2, np.random.default_rng(5))
    return O.scale(1.0 / O.norm(x0), x0)


def test_rayleigh_descent_fixed_step(T):
    x0 = _descent_start()
    A = T.DeviceTTO(to_product(O.Delta(5)))
    x, en = T.rayleigh_descent(A, _up(T, [x0]), 6, 0.1, backtrack=False)
    _, ref = R.rayleigh_descent(O.Delta(5), x0, 6, 0.1, backtrack=False)
    en = [float(e[0]) for e in en]
    print("rayleigh_descent fixed step: " + " ".join("%.10f" % e for e in en))
    assert len(en) == len(ref) == 7
    assert all(abs(a - b) <= 1e-9 * abs(ref[0]) for a, b in zip(en, ref))
    assert x.ranks(0)[0] == x0.ttv_rks


def test_rayleigh_descent_backtracking(T):
    x0 = _descent_start()
    A = T.DeviceTTO(to_product(O.Delta(5)))
    x, en = T.rayleigh_descent(A, _up(T, [x0]), 20, 0.25, backtrack=True)
    en = [float(e[0]) for e in en]
    print("rayleigh_descent backtracking: " + " ".join("%.6f" % e for e in en))
    assert len(en) == 21 and all(b <= a for a, b in zip(en, en[1:])) and en[-1] < en[0]
    assert x.ranks(0)[0] == x0.ttv_rks
    assert abs(float(T.device.norm(x)[0]) - 1.0) <= 1e-12


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def _refused(T, rc, code, who):
    assert rc == code, (rc, T._lib.last_error())
    assert who in T._lib.last_error(), T._lib.last_error()


def test_refusals_leave_the_destination_alone(T):
    L = T._lib.lib()
    E = T._lib
    dims, r = (2,) * 4, [1, 2, 3, 2, 1]
    x = _rt(dims, r, 1)
    Uo, Vo = R.gauges(x)
    keep = _rt(dims, r, 2)                                            # what the destinations hold before the refused calls
    keep2 = _rt(dims, [1, 4, 6, 4, 1], 3)
    U, V, z, xi, y = _up(T, [Uo]), _up(T, [Vo]), _up(T, [_rt(dims, [1, 2, 2, 2, 1], 4)]), _up(T, [keep]), _up(T, [keep2])
    other_dims = _up(T, [_rt((2, 2, 2, 3), r, 5)])
    two = _up(T, [Uo, Uo])
    small = _up(T, [_rt(dims, [1, 2, 2, 2, 1], 6)])
    small_keep = small.download(0)
    cplx = T.DeviceTT(dims, r, 1, dtype=np.complex128)
    P, W = "ttn_tangent_project", "ttn_tangent_to_tt"
    _refused(T, L.ttn_tangent_project(None, V.h, z.h, xi.h, None), E.TTN_ERR_ARG, P)
    _refused(T, L.ttn_tangent_project(U.h, V.h, z.h, None, None), E.TTN_ERR_ARG, P)
    _refused(T, L.ttn_tangent_project(U.h, V.h, xi.h, xi.h, None), E.TTN_ERR_ARG, P)
    _refused(T, L.ttn_tangent_project(xi.h, V.h, z.h, xi.h, None), E.TTN_ERR_ARG, P)
    _refused(T, L.ttn_tangent_project(U.h, V.h, other_dims.h, xi.h, None), E.TTN_ERR_DIMS, P)
    _refused(T, L.ttn_tangent_project(U.h, two.h, z.h, xi.h, None), E.TTN_ERR_DIMS, P)
    _refused(T, L.ttn_tangent_project(U.h, V.h, z.h, small.h, None), E.TTN_ERR_CAPACITY, P)
    _refused(T, L.ttn_tangent_project(U.h, V.h, cplx.h, xi.h, None), E.TTN_ERR_UNSUPPORTED, P)
    _refused(T, L.ttn_tangent_to_tt(U.h, None, xi.h, None, None, y.h), E.TTN_ERR_ARG, W)
    _refused(T, L.ttn_tangent_to_tt(U.h, V.h, xi.h, None, None, xi.h), E.TTN_ERR_ARG, W)
    _refused(T, L.ttn_tangent_to_tt(U.h, V.h, y.h, None, None, y.h), E.TTN_ERR_ARG, W)
    _refused(T, L.ttn_tangent_to_tt(U.h, V.h, other_dims.h, None, None, y.h), E.TTN_ERR_DIMS, W)
    _refused(T, L.ttn_tangent_to_tt(U.h, V.h, two.h, None, None, y.h), E.TTN_ERR_DIMS, W)
    _refused(T, L.ttn_tangent_to_tt(U.h, V.h, z.h, None, None, xi.h), E.TTN_ERR_CAPACITY, W)
    _refused(T, L.ttn_tangent_to_tt(U.h, cplx.h, xi.h, None, None, y.h), E.TTN_ERR_UNSUPPORTED, W)
    _same(xi, [keep])
    _same(y, [keep2])
    _same(small, [to_oracle(small_keep)])
    # more than 480 sites; more than 65535 trains in the assembly
    long_dims = (2,) * 481
    hs = [T.DeviceTT(long_dims, [1] * 482, 1) for _ in range(4)]
    _refused(T, L.ttn_tangent_project(hs[0].h, hs[1].h, hs[2].h, hs[3].h, None), E.TTN_ERR_UNSUPPORTED, P)
    many = [T.DeviceTT((2,), [1, 1], 65536) for _ in range(4)]
    _refused(T, L.ttn_tangent_to_tt(many[0].h, many[1].h, many[2].h, None, None, many[3].h), E.TTN_ERR_UNSUPPORTED, W)
    # valid calls afterwards succeed
    xi2, out = _project(T, U, V, z, xi=xi)
    assert np.isfinite(out).all()
    assert L.ttn_tangent_to_tt(U.h, V.h, xi.h, None, None, y.h) == 0
    assert y.ranks(0)[0] == [1, 4, 6, 4, 1]


def test_per_train_rank_mismatch(T):
    """U and V of train 1 differ in a rank: that train is left alone and flagged on the destination, train 0 is computed."""
    L = T._lib.lib()
    xs, Us, Vs, zs, refs, vals, bounds = case("batch3")
    odd = R.gauges(_rt(Us[0].ttv_dims, [1, 2, 3, 4, 4, 2, 1], 9))[1]
    cap = [1, 2, 4, 17, 4, 2, 1]
    U, V, z = _up(T, Us[:2], cap), _up(T, [Vs[0], odd], cap), _up(T, zs[:2], cap)
    keep = [_rt(Us[0].ttv_dims, Us[0].ttv_rks, 70), _rt(Us[0].ttv_dims, Us[0].ttv_rks, 71)]
    xi = _up(T, keep, cap)
    xi, out = _project(T, U, V, z, xi=xi)
    _share(xi.download(0).ttv_vec, refs[0], bounds[0])
    assert np.isnan(out[1]) and abs(out[0] - vals[0]) <= 1e-12 * O.norm(xs[0]) * O.norm(zs[0])
    assert all(np.array_equal(a, b) for a, b in zip(xi.download(1).ttv_vec, keep[1].ttv_vec))
    assert L.ttn_compress_status(xi.h, None) == T._lib.TTN_ERR_DIMS and "ranks differ" in T._lib.last_error()
    assert L.ttn_compress_status(xi.h, None) == 0
    # the assembly: xi of train 0 is a tangent now, train 1 still mismatches
    y = T.DeviceTT(Us[0].ttv_dims, [1, 4, 8, 8, 8, 4, 1], 2)
    assert L.ttn_tangent_to_tt(U.h, V.h, xi.h, None, None, y.h) == 0
    assert y.ranks(0)[0] == [1, 4, 8, 8, 8, 4, 1] and y.ranks(1)[0] != [1, 4, 8, 8, 8, 4, 1]
    assert L.ttn_compress_status(y.h, None) == T._lib.TTN_ERR_DIMS
    assert L.ttn_compress_status(y.h, None) == 0


# ---- poison ---------------------------------------------------------------------------------------------------------------------------------
def _mode(T, on, pattern=0):
    assert T._lib.lib().ttn_selftest_poison(int(on), C.c_uint64(pattern)) == 0


def test_project_and_to_tt_under_poison(T):
    """The two smallest entrywise cases and two to_tt cases with the workspace and the new handles' slack poisoned (quiet NaN, then 1e300): the
    two runs of project agree bit for bit with the clean run, and to_tt's explicit zeros are zeros."""
    cleans = {}
    for name in ("d1", "d2"):
        xs, Us, Vs, zs, refs, vals, bounds = case(name)
        xi, val = _project(T, _up(T, Us), _up(T, Vs), _up(T, zs))
        cleans[name] = (xi.download(0).ttv_vec, val[0])
    for pattern in (QNAN, BIG):
        _mode(T, 1, pattern)
        try:
            for name in ("d1", "d2"):
                xs, Us, Vs, zs, refs, vals, bounds = case(name)
                got, val = _project(T, _up(T, Us), _up(T, Vs), _up(T, zs))
                assert all(np.array_equal(a, b) for a, b in zip(got.download(0).ttv_vec, cleans[name][0]))
                assert val[0] == cleans[name][1]
                _check_project(T, name)
            _check_to_tt(T, "mixed_dims", -0.75, 2.5)
            _check_to_tt(T, "tile_edges", None, 0.0)
        finally:
            _mode(T, 0)
