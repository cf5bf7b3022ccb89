"""GPU tests of contract_sites (include/ttn_contract.h) and of the QTT layer on top of it (marginal, slice_dim, moments).

Reference and tolerance (tests/contract_reference.py): the device result is compared entrywise with the NumPy contraction of the dense
tensor, or, where the train is too long for that, core by core with the core chain in the other association order.  The bound is
derived: 2 * sum_k (r_{k-1} + n_k) * eps * S, S the same contraction of |X_k| with |w_k|.  Every test prints its worst err / S."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import contract_reference as R
from tests.helpers import worst_of

pytestmark = pytest.mark.gpu

QNAN = 0x7FF8000000000000
BIG = int(np.float64(1e300).view(np.uint64))


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def rand_train(T, rng, dims, rks):
    cores = [np.asfortranarray(rng.standard_normal((dims[k], rks[k], rks[k + 1]))) for k in range(len(dims))]
    return T.TTvector(len(dims), cores, tuple(dims), list(rks), [0] * len(dims))


def upload(T, trains, cap=None):
    """the trains (common dims) as one resident batch; cap: the handle's rank capacity (default: the largest rank per bond)"""
    N = trains[0].N
    if cap is None:
        cap = [max(t.ttv_rks[m] for t in trains) for m in range(N + 1)]
    h = T.DeviceTT(trains[0].ttv_dims, cap, batch=len(trains))
    for b, t in enumerate(trains):
        h.upload(b, t)
    return h


def rand_weights(rng, dims, contracted, batch=None):
    """{1-based site: vector} for the 0-based contracted sites"""
    return {k + 1: rng.standard_normal(dims[k] if batch is None else (batch, dims[k])) for k in contracted}


def weights_of(w, b):
    """0-based site -> the vector train b sees"""
    return {s - 1: (np.asarray(v)[b] if np.asarray(v).ndim == 2 else np.asarray(v)) for s, v in w.items()}


def check_dense(T, x_trains, w, y, what):
    """y (resident) against the dense reference, train by train: ranks as specified, err <= bound * S entrywise.  Returns worst err / (eps S)
    relative to the bound."""
    worst = 0.0
    for b, x in enumerate(x_trains):
        wb = weights_of(w, b)
        kept, start = R.kept_and_start(x.N, wb.keys())
        got = y.download(b)
        assert list(got.ttv_rks) == [x.ttv_rks[s] for s in start] + [1], (what, b, got.ttv_rks)
        assert got.ttv_rks[0] == 1 and got.ttv_rks[-1] == 1
        assert list(got.ttv_ot) == [0] * len(kept)
        ref = R.contract_dense(x.ttv_vec, wb)
        S = R.contract_dense(*R.abs_inputs(x.ttv_vec, wb))
        err = np.abs(R.dense(got.ttv_vec) - ref)
        bound = R.bound_factor(x.ttv_vec) * R.EPS
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(S > 0, err / np.where(S > 0, S, 1.0), np.where(err == 0, 0.0, np.inf))
        worst = worst_of(worst, float(np.max(rel)) / bound)
        assert np.all(err <= bound * S), (what, b, float(np.max(rel)), bound)
    return worst


def untouched_are_bit_equal(x_trains, w, y):
    """every kept core with no run next to it is x's core, bit for bit"""
    n = 0
    for b, x in enumerate(x_trains):
        kept, start = R.kept_and_start(x.N, weights_of(w, b).keys())
        got = y.download(b)
        for m, k in enumerate(kept):
            if start[m] == k and not (m == len(kept) - 1 and k < x.N - 1):
                assert np.array_equal(np.asarray(got.ttv_vec[m]).view(np.uint64), np.asarray(x.ttv_vec[k]).view(np.uint64)), (b, k)
                n += 1
    return n


# ---- 1. every pattern, on-chip route ---------------------------------------------------------------------------------------------------
def test_every_pattern_on_chip(T):
    """d = 6, n = 2, ranks [1, 2, 3, 4, 3, 2, 1], two trains: all 62 proper non-empty kept sets."""
    rng = np.random.default_rng(10)
    dims, rks = (2,) * 6, [1, 2, 3, 4, 3, 2, 1]
    xs = [rand_train(T, rng, dims, rks) for _ in range(2)]
    x = upload(T, xs)
    worst, copies, count = 0.0, 0, 0
    for nk in range(1, 6):
        for kept in itertools.combinations(range(6), nk):
            con = [k for k in range(6) if k not in kept]
            w = rand_weights(rng, dims, con)
            y = T.device.contract_sites(x, w)
            assert y.dims == tuple(dims[k] for k in kept)
            worst = worst_of(worst, check_dense(T, xs, w, y, kept))
            copies += untouched_are_bit_equal(xs, w, y)
            y.free()
            count += 1
    x.free()
    assert count == 62 and copies > 0
    print("on-chip, 62 kept sets: worst err / (bound S) = %.3f, %d cores copied bit for bit" % (worst, copies))


# ---- 2. tile edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [15, 16, 17, 31, 33, 63, 64])
def test_tile_edges(T, r):
    """d = 5, ranks [1, r, r, r, r, 1] (over-parametrised: legal), kept sets {1,3,5}, {2,4}, {3}, {1}, {5} (1-based)."""
    rng = np.random.default_rng(20 + r)
    dims, rks = (2,) * 5, [1, r, r, r, r, 1]
    xs = [rand_train(T, rng, dims, rks)]
    x = upload(T, xs)
    worst = 0.0
    for kept in ((0, 2, 4), (1, 3), (2,), (0,), (4,)):
        w = rand_weights(rng, dims, [k for k in range(5) if k not in kept])
        y = T.device.contract_sites(x, w)
        worst = worst_of(worst, check_dense(T, xs, w, y, kept))
        y.free()
    x.free()
    print("r = %d: worst err / (bound S) = %.3f" % (r, worst))


# ---- 3. general route ------------------------------------------------------------------------------------------------------------------
GENERAL = [
    ((3, 2, 4, 1, 5), [1, 3, 5, 4, 2, 1], [(1, 4), (0, 2, 3), (0, 3), (2, 4), (1,), (0, 1, 2, 3), (3,), (0, 1, 3, 4), (4,)]),
    ((2, 2, 2, 2), [1, 65, 65, 65, 1], [(0, 2), (0, 3), (1, 3), (2,), (0, 1, 3), (0,), (3,)]),
]


@pytest.mark.parametrize("dims, rks, kept_sets", GENERAL, ids=["mixed-dims", "rank65"])
def test_general_route(T, dims, rks, kept_sets):
    """n_k != 2 (n_k = 1 included) and ranks above 64: runs at the left end, in the middle (lengths 1 and 2) and at the right end, alone
    and combined at one kept site."""
    rng = np.random.default_rng(30 + len(dims))
    d = len(dims)
    xs = [rand_train(T, rng, dims, rks), rand_train(T, rng, dims, rks)]
    x = upload(T, xs)
    worst = 0.0
    for kept in kept_sets:
        w = rand_weights(rng, dims, [k for k in range(d) if k not in kept])
        y = T.device.contract_sites(x, w)
        worst = worst_of(worst, check_dense(T, xs, w, y, kept))
        untouched_are_bit_equal(xs, w, y)
        y.free()
    x.free()
    print("general route %s: worst err / (bound S) = %.3f" % (dims, worst))


# ---- 4. ragged batch and slack, plain and on poisoned memory ---------------------------------------------------------------------------
RAGGED = [
    ((2,) * 5, [[1, 2, 4, 3, 2, 1], [1, 1, 2, 2, 1, 1], [1, 2, 3, 5, 2, 1]], [1, 6, 6, 6, 6, 1]),
    ((3, 2, 4, 1, 5), [[1, 3, 5, 4, 2, 1], [1, 2, 2, 2, 1, 1], [1, 3, 6, 4, 4, 1]], [1, 7, 8, 8, 5, 1]),
]


@pytest.mark.parametrize("pattern", [None, QNAN, BIG], ids=["plain", "qnan", "1e300"])
@pytest.mark.parametrize("dims, ranks, cap", RAGGED, ids=["on-chip", "general"])
def test_ragged_batch_and_slack(T, dims, ranks, cap, pattern):
    """Three trains of different ranks and a rank-1 zero train in handles whose capacity exceeds them, on x and on y; with the library's
    poison mode on, slack and workspace hold the pattern and no result may change."""
    lib = T._lib.lib()
    if pattern is not None:
        assert lib.ttn_selftest_poison(1, C.c_uint64(pattern)) == 0
    try:
        rng = np.random.default_rng(40)
        d = len(dims)
        xs = [rand_train(T, rng, dims, r) for r in ranks]
        xs.append(T.TTvector(d, [np.zeros((n, 1, 1), order="F") for n in dims], tuple(dims), [1] * (d + 1), [0] * d))
        x = upload(T, xs, cap)
        worst = 0.0
        for kept in ((0, 2, 4), (1, 3), (2,), (0, 3), (0, 1), (3, 4), (1, 2, 3)):
            con = [k for k in range(d) if k not in kept]
            w = rand_weights(rng, dims, con, batch=len(xs))
            ycap = [c + 2 for c in T.device.contract_rank_capacity(cap, [k + 1 for k in con])]
            y = T.DeviceTT([dims[k] for k in kept], ycap, batch=len(xs))
            T.device.contract_sites(x, w, y)
            worst = worst_of(worst, check_dense(T, xs, w, y, kept))
            zero = y.download(len(xs) - 1)
            assert list(zero.ttv_rks) == [1] * (len(kept) + 1) and all(not np.asarray(c).any() for c in zero.ttv_vec)
            y.free()
        x.free()
        T.device.status_all()
    finally:
        if pattern is not None:
            assert lib.ttn_selftest_poison(0, C.c_uint64(0)) == 0
    print("ragged %s: worst err / (bound S) = %.3f" % (dims, worst))


# ---- 5. long runs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kept", [(0, 1, 2), (37, 38, 39)], ids=["trailing-37", "leading-37"])
def test_long_runs(T, kept):
    """d = 40, n = 2, rank 4: a run of 37 sites behind, or in front of, three kept sites, core by core against the core chain."""
    rng = np.random.default_rng(50)
    d = 40
    dims, rks = (2,) * d, [1] + [4] * (d - 1) + [1]
    x_host = rand_train(T, rng, dims, rks)
    x_host.ttv_vec = [np.asfortranarray(c * 0.7) for c in x_host.ttv_vec]        # keeps the product of 37 matrices in range
    con = [k for k in range(d) if k not in kept]
    w = rand_weights(rng, dims, con)
    wb = weights_of(w, 0)
    x = upload(T, [x_host])
    y = T.device.contract_sites(x, w)
    got = y.download(0)
    ref = R.contract_chain(x_host.ttv_vec, wb)
    S = R.contract_chain(*R.abs_inputs(x_host.ttv_vec, wb))
    bound = R.bound_factor(x_host.ttv_vec) * R.EPS
    worst = 0.0
    for m in range(3):
        assert np.asarray(got.ttv_vec[m]).shape == ref[m].shape
        err = np.abs(np.asarray(got.ttv_vec[m]) - ref[m])
        worst = worst_of(worst, float(np.max(err / S[m])) / bound)
        assert np.all(err <= bound * S[m])
    x.free(); y.free()
    print("long run %s: worst err / (bound S) = %.3f" % (kept, worst))


# ---- 6. bits ---------------------------------------------------------------------------------------------------------------------------
def _bits(y, b):
    t = y.download(b)
    return list(t.ttv_rks), [np.asarray(c).view(np.uint64).copy() for c in t.ttv_vec]


def _same(a, b):
    return a[0] == b[0] and all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))


@pytest.mark.parametrize("dims, rks", [((2,) * 6, [1, 2, 4, 8, 4, 2, 1]), ((2, 3, 2, 2, 3, 2), [1, 2, 4, 5, 4, 2, 1])], ids=["on-chip", "general"])
def test_bits(T, dims, rks):
    """The call twice gives identical bits; a batch of 3 with per-train weights equals the three single-train calls; a shared table equals
    the same table repeated per train."""
    rng = np.random.default_rng(60)
    d = len(dims)
    xs = [rand_train(T, rng, dims, rks) for _ in range(3)]
    x = upload(T, xs)
    for kept in ((1, 4), (0, 3), (2,), (0, 1, 5)):
        con = [k for k in range(d) if k not in kept]
        w = rand_weights(rng, dims, con, batch=3)
        y1, y2 = T.device.contract_sites(x, w), T.device.contract_sites(x, w)
        for b in range(3):
            assert _same(_bits(y1, b), _bits(y2, b)), ("twice", kept, b)
            xb = upload(T, [xs[b]], x.cap)
            yb = T.device.contract_sites(xb, {s: v[b] for s, v in w.items()})
            assert _same(_bits(y1, b), _bits(yb, 0)), ("alone", kept, b)
            xb.free(); yb.free()
        shared = {s: v[0] for s, v in w.items()}
        ys, yr = T.device.contract_sites(x, shared), T.device.contract_sites(x, {s: np.tile(v, (3, 1)) for s, v in shared.items()})
        for b in range(3):
            assert _same(_bits(ys, b), _bits(yr, b)), ("shared", kept, b)
        for h in (y1, y2, ys, yr):
            h.free()
    x.free()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(T):
    """Every row of the list in ttn_contract.h: its code, a message, y untouched; a correct call afterwards still passes."""
    L, lib = T._lib, T._lib.lib()
    rng = np.random.default_rng(70)
    dims, rks = (2, 3, 2, 2), [1, 2, 3, 2, 1]
    xs = [rand_train(T, rng, dims, rks) for _ in range(3)]
    x = upload(T, xs)
    good = {2: rng.standard_normal(3), 4: rng.standard_normal(2)}
    y = T.device.contract_sites(x, good)                                  # kept sites 1 and 3: dims (2, 2), ranks [1, 2, 1]
    before = [_bits(y, b) for b in range(3)]
    i64 = lambda v: (C.c_int64 * len(v))(*v)                               # noqa: E731
    f64 = lambda v: (C.c_double * len(v))(*v)                              # noqa: E731
    wtab = f64([1.0] * 16)

    def refused(code, x_h, sites, wbatch, w, y_h, what):
        rc = lib.ttn_tt_contract_sites(x_h, len(sites), i64(sites) if sites is not None else None, wbatch, w, y_h)
        assert rc == code, (what, rc, L.last_error())
        assert L.last_error(), what
        for b in range(3):
            assert _same(_bits(y, b), before[b]), what

    refused(L.TTN_ERR_ARG, None, [2, 4], 1, wtab, y.h, "null x")
    refused(L.TTN_ERR_ARG, x.h, [2, 4], 1, wtab, None, "null y")
    refused(L.TTN_ERR_ARG, x.h, [2, 4], 1, None, y.h, "null weights")
    rc = lib.ttn_tt_contract_sites(x.h, 2, None, 1, wtab, y.h)
    assert rc == L.TTN_ERR_ARG and L.last_error()
    refused(L.TTN_ERR_ARG, x.h, [2, 4], 1, wtab, x.h, "y == x")
    refused(L.TTN_ERR_ARG, x.h, [0, 4], 1, wtab, y.h, "site 0")
    refused(L.TTN_ERR_ARG, x.h, [2, 5], 1, wtab, y.h, "site d + 1")
    refused(L.TTN_ERR_ARG, x.h, [2, 2], 1, wtab, y.h, "repeated")
    refused(L.TTN_ERR_ARG, x.h, [4, 2], 1, wtab, y.h, "unsorted")
    refused(L.TTN_ERR_ARG, x.h, [1, 2, 3, 4], 1, wtab, y.h, "no kept site")
    refused(L.TTN_ERR_ARG, x.h, [2, 4], 2, wtab, y.h, "wbatch")
    refused(L.TTN_ERR_ARG, x.h, [2, 4], 0, wtab, y.h, "wbatch 0")
    refused(L.TTN_ERR_DIMS, x.h, [1, 4], 1, wtab, y.h, "y's dims")          # keeps sites 2, 3: dims (3, 2)
    refused(L.TTN_ERR_DIMS, x.h, [4], 1, wtab, y.h, "y's number of sites")
    y1 = T.DeviceTT((2, 2), [1, 3, 1], batch=1)
    refused(L.TTN_ERR_DIMS, x.h, [2, 4], 1, wtab, y1.h, "y's batch")
    ysmall = T.DeviceTT((2, 2), [1, 1, 1], batch=3)
    refused(L.TTN_ERR_CAPACITY, x.h, [2, 4], 1, wtab, ysmall.h, "y's capacity")
    assert ysmall.ranks(0)[0] == [1, 1, 1]
    xc = T.DeviceTT(dims, rks, batch=3, dtype=np.complex128)
    yc = T.DeviceTT((2, 2), [1, 3, 1], batch=3, dtype=np.complex128)
    refused(L.TTN_ERR_UNSUPPORTED, xc.h, [2, 4], 1, wtab, y.h, "complex x")
    refused(L.TTN_ERR_UNSUPPORTED, x.h, [2, 4], 1, wtab, yc.h, "complex y")
    for h in (y1, ysmall, xc, yc):
        h.free()
    # a core of 2^31 doubles: dims (2, 2, 2) with capacity 32768 on both inner bonds (one train, 16 GiB, freed at once)
    xbig = T.DeviceTT((2, 2, 2), [1, 32768, 32768, 1], batch=1)
    ybig = T.DeviceTT((2, 2), [1, 4, 1], batch=1)
    try:
        rc = lib.ttn_tt_contract_sites(xbig.h, 1, i64([2]), 1, wtab, ybig.h)
        assert rc == L.TTN_ERR_UNSUPPORTED and "2^31" in L.last_error(), (rc, L.last_error())
    finally:
        xbig.free(); ybig.free()
    # the Python layer refuses with the library's exception
    with pytest.raises(T.TTNError, match="capacity"):
        T.device.contract_sites(x, good, T.DeviceTT((2, 2), [1, 1, 1], batch=3))
    with pytest.raises(T.TTNError, match="no kept site"):
        T.device.contract_sites(x, {s: np.ones(n) for s, n in zip((1, 2, 3, 4), dims)})
    # ... and a correct call still passes, into the handle that saw every refusal
    T.device.contract_sites(x, good, y)
    for b in range(3):
        assert _same(_bits(y, b), before[b])
    print("refusals: worst err / (bound S) = %.3f" % check_dense(T, xs, good, y, "after the refusals"))
    x.free(); y.free()
    T.device.status_all()


# ---- 8. the QTT layer ------------------------------------------------------------------------------------------------------------------
A, B = -1.0, 2.0


def _density(n_dims):
    """a product of different Gaussians plus a rank-2 coupling term, on [A, B]^n"""
    import torch
    mu, var = (0.3, 0.9, -0.2), (0.08, 0.2, 0.15)

    def f(X):
        g = torch.ones(X.shape[0], dtype=torch.float64, device=X.device)
        for m in range(n_dims):
            g = g * torch.exp(-(X[:, m] - mu[m]) ** 2 / (2 * var[m]))
        return g + 0.05 * (torch.sin(3.0 * X[:, 0]) * torch.cos(2.0 * X[:, -1]) + X[:, 0] * X[:, -1])
    return f


@pytest.fixture(scope="module", params=[(2, 5, "interleaved"), (2, 5, "serial"), (3, 3, "interleaved"), (3, 3, "serial")],
                ids=lambda p: "%dx%d-%s" % p)
def qcase(T, request):
    """(q, its dense array, meta): computed once per layout and left unchanged"""
    n_dims, bits, ordering = request.param
    q = T.function_to_qttv(_density(n_dims), n_dims, bits, ordering=ordering, a=A, b=B)
    arr = T.qttv_to_array(q)
    return q, arr, (n_dims, bits, ordering)


def _grid_S(q, vectors):
    """S on the grid of the kept dimensions: the contraction of |cores| with |weights| (0-based sites), mapped by the bit rule"""
    kept_dims = sorted({q_dim for s in range(q.N) if s not in vectors for q_dim in [_dim_of(q, s)]})
    S = R.contract_dense(*R.abs_inputs(q.ttv_vec, vectors))
    return R.site_to_grid(S, len(kept_dims), q.bits_per_dim, q.ordering)


def _dim_of(q, s):
    from ttn_amd import qttnd
    return qttnd.site_dim_level(s, q.n_dims, q.bits_per_dim, q.ordering)[0]


def test_site_to_grid_matches_qttv_to_array(T, qcase):
    """the reference's bit rule against the library's dense export"""
    q, arr, (n_dims, bits, ordering) = qcase
    mine = R.site_to_grid(R.dense(q.ttv_vec), n_dims, bits, ordering)
    S = R.site_to_grid(R.dense([np.abs(c) for c in q.ttv_vec]), n_dims, bits, ordering)
    assert np.all(np.abs(mine - arr) <= R.bound_factor(q.ttv_vec) * R.EPS * S)


def test_marginal(T, qcase):
    """marginal against qttv_to_array(q).sum(axis) * h for every non-empty proper kept set, host and resident; metadata of every result"""
    from ttn_amd import qttnd
    q, arr, (n_dims, bits, ordering) = qcase
    h = (B - A) / (2 ** bits - 1)
    bound = R.bound_factor(q.ttv_vec) * R.EPS
    dx = T.DeviceTT.from_host(q.ttvector(), batch=2)
    worst = 0.0
    for nk in range(1, n_dims):
        for keep in itertools.combinations(range(n_dims), nk):
            summed = tuple(m for m in range(n_dims) if m not in keep)
            ref = arr.sum(axis=summed) * h ** len(summed)
            vectors = {s: np.full(2, h if lvl == 0 else 1.0) for m in summed for lvl, s in enumerate(qttnd.dim_sites(m, n_dims, bits, ordering))}
            S = _grid_S(q, vectors)
            m_host = T.marginal(q, keep, h)
            assert isinstance(m_host, T.QTTvector) and (m_host.n_dims, m_host.bits_per_dim, m_host.ordering) == (nk, bits, ordering)
            assert m_host.N == nk * bits
            err = np.abs(T.qttv_to_array(m_host) - ref)
            worst = worst_of(worst, float(np.max(err / S)) / bound)
            assert np.all(err <= bound * S), (keep, float(np.max(err / S)), bound)
            my, meta = T.marginal((dx, (n_dims, bits, ordering)), keep, h)
            assert meta == (nk, bits, ordering) and my.batch == 2 and my.N == nk * bits
            for b in range(2):
                res = T.qttv_to_array(T.QTTvector(my.download(b), *meta))
                assert np.all(np.abs(res - ref) <= bound * S), (keep, b)
            my.free()
    # without h: the plain sums; keep = () is the mass, through dot
    m0 = T.marginal(q, (0,))
    ref0 = arr.sum(axis=tuple(range(1, n_dims)))
    S0 = _grid_S(q, {s: np.ones(2) for m in range(1, n_dims) for s in qttnd.dim_sites(m, n_dims, bits, ordering)})
    assert np.all(np.abs(T.qttv_to_array(m0) - ref0) <= bound * S0)
    mass = T.marginal(q, (), h)
    S_all = float(np.abs(arr).sum()) * h ** n_dims
    assert abs(mass - arr.sum() * h ** n_dims) <= 1e-12 * S_all
    masses = T.marginal((dx, (n_dims, bits, ordering)), (), h)
    assert masses.shape == (2,) and np.all(np.abs(masses - arr.sum() * h ** n_dims) <= 1e-12 * S_all)
    full = T.marginal(q, tuple(range(n_dims)))
    assert all(np.array_equal(a_, b_) for a_, b_ in zip(full.ttv_vec, q.ttv_vec))
    dx.free()
    print("marginal %s: worst err / (bound S) = %.3f" % ((n_dims, bits, ordering), worst))


def test_slice_dim(T, qcase):
    """slice_dim against the array's slice at the first, the last and a middle index, in every dimension; one index per train on a
    resident batch; metadata of every result"""
    q, arr, (n_dims, bits, ordering) = qcase
    from ttn_amd import qttnd
    bound = R.bound_factor(q.ttv_vec) * R.EPS
    G = 2 ** bits
    picks = [0, G - 1, G // 2 - 3]
    dx = T.DeviceTT.from_host(q.ttvector(), batch=3)
    worst = 0.0
    for dim in range(n_dims):
        sites = qttnd.dim_sites(dim, n_dims, bits, ordering)
        cuts, meta = T.slice_dim((dx, (n_dims, bits, ordering)), dim, np.array(picks))
        assert meta == (n_dims - 1, bits, ordering) and cuts.batch == 3
        for b, g in enumerate(picks):
            ref = np.take(arr, g, axis=dim)
            vectors = {s: np.eye(2)[(g >> (bits - 1 - lvl)) & 1] for lvl, s in enumerate(sites)}
            S = _grid_S(q, vectors)
            sl = T.slice_dim(q, dim, g)
            assert (sl.n_dims, sl.bits_per_dim, sl.ordering, sl.N) == (n_dims - 1, bits, ordering, (n_dims - 1) * bits)
            err = np.abs(T.qttv_to_array(sl) - ref)
            worst = worst_of(worst, float(np.max(err / np.where(S > 0, S, np.inf))) / bound)
            assert np.all(err <= bound * S), (dim, g)
            res = T.qttv_to_array(T.QTTvector(cuts.download(b), *meta))
            assert np.all(np.abs(res - ref) <= bound * S), (dim, g, "resident")
        cuts.free()
    dx.free()
    print("slice_dim %s: worst err / (bound S) = %.3f" % ((n_dims, bits, ordering), worst))


def test_moments(T, qcase):
    """moments against the dense formulas of the reference's Ornstein2D example (lines 63-70): 1e-12 of the absolute-value scale of each
    sum, the bound dot is tested with"""
    q, arr, (n_dims, bits, ordering) = qcase
    G = 2 ** bits
    h = (B - A) / (G - 1)
    xes = np.linspace(A, B, G)
    hn = h ** n_dims

    def along(v, m):
        return v.reshape([G if k == m else 1 for k in range(n_dims)])

    mass_ref = arr.sum() * hn
    mean_ref = np.array([(along(xes, m) * arr).sum() * hn for m in range(n_dims)])
    cov_ref = np.array([[(along(xes - mean_ref[i], i) * along(xes - mean_ref[j], j) * arr).sum() * hn for j in range(n_dims)] for i in range(n_dims)])
    absarr = np.abs(arr)
    mean_S = np.array([(along(np.abs(xes), m) * absarr).sum() * hn for m in range(n_dims)])
    cov_S = np.array([[(along(np.abs(xes - mean_ref[i]), i) * along(np.abs(xes - mean_ref[j]), j) * absarr).sum() * hn for j in range(n_dims)]
                      for i in range(n_dims)])
    mass, mean, cov = T.moments(q, A, B)
    worst = worst_of(abs(mass - mass_ref) / (absarr.sum() * hn), np.max(np.abs(mean - mean_ref) / mean_S), np.max(np.abs(cov - cov_ref) / cov_S))
    print("moments %s: worst err / S = %.2e" % ((n_dims, bits, ordering), worst))
    assert abs(mass - mass_ref) <= 1e-12 * absarr.sum() * hn
    assert np.all(np.abs(mean - mean_ref) <= 1e-12 * mean_S)
    assert np.all(np.abs(cov - cov_ref) <= 1e-12 * cov_S)
    assert np.array_equal(cov, cov.T)
    dx = T.DeviceTT.from_host(q.ttvector(), batch=2)
    masses, means, covs = T.moments((dx, (n_dims, bits, ordering)), A, B)
    dx.free()
    assert masses.shape == (2,) and means.shape == (2, n_dims) and covs.shape == (2, n_dims, n_dims)
    for b in range(2):
        assert abs(masses[b] - mass_ref) <= 1e-12 * absarr.sum() * hn
        assert np.all(np.abs(means[b] - mean_ref) <= 1e-12 * mean_S)
        assert np.all(np.abs(covs[b] - cov_ref) <= 1e-12 * cov_S)
