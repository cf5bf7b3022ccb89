"""tt_cross_batch on the device (tensortrainnumerics.jl_amd/cross.py, csrc/ttn_cross_batch_kernels.h) against the NumPy restatement
(tests/cross_reference.py) run once per function, against tt_cross per function, closed forms and the refusals."""
import numpy as np
import pytest

import ttn_amd as T
from tests import cross_reference as R
from tests.test_cpu_cross_batch import MIXED, MIXED_ALG, MIXED_DOMAIN, MIXED_KW, MIXED_SWEEPS, PARITY, table_family

pytestmark = pytest.mark.gpu
X = T.cross


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    T.ensure_init(0)
    T.tdvp._dev()
    return _t


def batch_f(fs, seen=None):
    """NumPy functions f_b of the (P, N) coordinate matrix as the f(X, which) tt_cross_batch calls; `seen` records every `which`"""
    def f(Xd, which):
        Xh, w = Xd.cpu().numpy(), which.cpu().tolist()
        if seen is not None:
            seen.append(w)
        return np.stack([fs[b](Xh[a]) for a, b in enumerate(w)])
    return f


def dev_f(g):
    return lambda Xd: g(Xd.cpu().numpy())


def _up_sets(torch, S):
    """host sets (A, rows, cols) -> device (A, cols, rows)"""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(S, (0, 2, 1)))).to("cuda")


# ---- the site kernel -----------------------------------------------------------------------------------------------------------------
# (m, r, rank index extent, n): m = extent * n.  Square; small; across a wave; more than one pass of 1024 threads; above the LDS budget
# (workspace route); and 96 x 96, the largest matrix of the LDS route (2 * 8 * m * r = 144 KiB exactly).
SITE = [(4, 4, 2, 2), (6, 2, 2, 3), (65, 3, 5, 13), (1030, 5, 10, 103), (400, 24, 20, 20), (96, 96, 8, 12)]


def _site_reference(M, n, other, r, direction, set_in):
    piv, Cm, swaps = R.maxvol(R._qr(M), 1.05, 100)
    li, lr = (piv - 1) % n + 1, (piv - 1) // n
    if direction == 0:
        core = Cm.reshape(-1, order="F")
        nxt = np.hstack([set_in[lr], li.reshape(-1, 1)])
    else:
        core = np.transpose(Cm.reshape((n, other, r), order="F"), (0, 2, 1)).reshape(-1, order="F")
        nxt = np.hstack([li.reshape(-1, 1), set_in[lr]])
    return piv, Cm, swaps, core, nxt


@pytest.mark.parametrize("direction", [0, 1], ids=["l2r", "r2l"])
@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("m,r,ext,n", SITE, ids=[f"{m}x{r}" for m, r, _, _ in SITE])
def test_site_kernel_matches_restatement(torch, m, r, ext, n, A, direction):
    rng = np.random.default_rng(100 * m + 10 * r + 2 * A + direction)
    Ms = [rng.standard_normal((m, r)) * 2.0 ** rng.integers(-30, 30) for _ in range(A)]
    zero = 1 if A == 3 else None                                       # one all-zero fibre among the three
    if zero is not None:
        Ms[zero] = np.zeros((m, r))
    set_in = rng.integers(1, 6, (A, ext, 1))
    if direction == 0:                                                 # site 2 of 3: rl = ext, rr = r
        rl, rr = ext, r
        V = np.stack([M.reshape(-1, order="F") for M in Ms])
    else:                                                              # site 2 of 3: rl = r, rr = ext; V[i, a, b] = M[i + n b, a]
        rl, rr = r, ext
        V = np.stack([np.transpose(M.reshape((n, ext, r), order="F"), (0, 2, 1)).reshape(-1, order="F") for M in Ms])
    with torch.cuda.stream(T.tdvp._dev()[1]):
        info = torch.full((A, 2), 7, dtype=torch.int64, device="cuda")
        core, nxt, piv = X._d_batch_site(direction, 3, 2, n, rl, rr, torch.from_numpy(V).to("cuda"), 1.05, 100, _up_sets(torch, set_in), info)
        core, nxt, piv, info = core.cpu().numpy().reshape(A, -1), np.transpose(nxt.cpu().numpy(), (0, 2, 1)), piv.cpu().numpy(), info.cpu().numpy()
    for a in range(A):
        if a == zero:
            assert info[a, 0] == T._lib.TTN_ERR_SINGULAR and np.all(core[a] == 0.0)
            assert np.all((piv[a] >= 1) & (piv[a] <= m))
            continue
        rp, Cm, swaps, rcore, rnxt = _site_reference(Ms[a], n, ext, r, direction, set_in[a])
        assert info[a].tolist() == [0, swaps] and np.array_equal(piv[a], rp)
        assert np.max(np.abs(core[a] - rcore)) <= 1e-10 * np.max(np.abs(Cm))
        assert np.array_equal(nxt[a], rnxt)


def test_site_kernel_at_the_first_and_last_site_and_refusals(torch):
    rng = np.random.default_rng(8)
    L = T._lib.lib()
    with torch.cuda.stream(T.tdvp._dev()[1]):
        for direction in (0, 1):
            Ms = rng.standard_normal((2, 7, 1))                                 # site 1 (left-to-right) / site N (right-to-left): m = n, r = 1
            info = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
            core, nxt, piv = X._d_batch_site(direction, 2, 1 if direction == 0 else 2, 7, 1, 1, torch.from_numpy(Ms.reshape(2, 7)).to("cuda"),
                                             1.05, 100, None, info)
            for a in range(2):
                rp, Cm, swaps = R.maxvol(R._qr(Ms[a]), 1.05, 100)
                assert np.array_equal(piv[a].cpu().numpy(), rp) and nxt[a].cpu().numpy().reshape(-1).tolist() == list(rp)
                assert np.max(np.abs(core[a].cpu().numpy().reshape(-1) - Cm.reshape(-1))) <= 1e-12
        V = torch.zeros((1, 16), dtype=torch.float64, device="cuda")
        out = torch.zeros((1, 64), dtype=torch.int64, device="cuda")
        p = X._p
        bad = [(1, 0, 3, 2, 2, 1, 4), (1, 0, 3, 3, 2, 2, 2), (1, 1, 3, 1, 2, 2, 2), (0, 0, 3, 2, 2, 2, 2), (1, 2, 3, 2, 2, 2, 2)]   # m < r, bad sites, A, dir
        for A, d, N, site, n, rl, rr in bad:
            assert L.ttn_cross_batch_site(A, d, N, site, n, rl, rr, p(V), 1.05, 10, p(out), p(out), p(V), p(out), p(out)) == T._lib.TTN_ERR_ARG
        assert L.ttn_cross_batch_site(1, 0, 3, 2, 2, 1025, 1025, p(V), 1.05, 10, p(out), p(out), p(V), p(out), p(out)) == T._lib.TTN_ERR_UNSUPPORTED
        assert L.ttn_cross_batch_site(1, 1, 3, 2, (1 << 20) + 1, 1, 1, p(V), 1.05, 10, p(out), p(out), p(V), p(out), p(out)) == T._lib.TTN_ERR_UNSUPPORTED
        assert L.ttn_cross_batch_site(70000, 0, 3, 2, 2, 2, 2, p(V), 1.05, 10, p(out), p(out), p(V), p(out), p(out)) == T._lib.TTN_ERR_UNSUPPORTED
        assert L.ttn_cross_batch_site(1, 0, 3, 2, 2, 2, 2, p(V), 1.05, 10, None, p(out), p(V), p(out), p(out)) == T._lib.TTN_ERR_ARG


# ---- points and evaluation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 3])
def test_points_equal_restatement(torch, A):
    rng = np.random.default_rng(20 + A)
    N, Is = 4, [None, 3, 4, 2, 5]
    Rs = [None, 1, 3, 4, 2, 1]
    domain = [np.linspace(0.1, 1.0, Is[k]) ** 2 for k in range(1, N + 1)]
    with torch.cuda.stream(T.tdvp._dev()[1]):
        pb = X._BatchProblem(lambda Xd, which: Xd[:, :, 0], domain, A)
        for j in (1, 2, N):                                                              # site 1, an inner site, site N
            ls = [[None, np.ones((1, 0), np.int64)] + [np.stack([rng.integers(1, Is[c + 1] + 1, Rs[k]) for c in range(k - 1)], 1) for k in range(2, N + 1)]
                  for _ in range(A)]
            rs = [[None] + [np.stack([rng.integers(1, Is[c] + 1, Rs[k + 1]) for c in range(k + 1, N + 1)], 1) for k in range(1, N)] + [np.ones((1, 0), np.int64)]
                  for _ in range(A)]
            Ld = None if j == 1 else _up_sets(torch, np.stack([l[j] for l in ls]))
            Rd = None if j == N else _up_sets(torch, np.stack([r_[j] for r_ in rs]))
            Xd = pb.fibre_points(j, Is[j], Rs[j], Rs[j + 1], Ld, Rd).cpu().numpy()
            for a in range(A):
                ref = R._build_fiber_indices(ls[a], rs[a], j, Is, Rs, N)
                assert np.array_equal(Xd[a].T, np.stack([domain[d][ref[:, d] - 1] for d in range(N)], 1))
        idx = np.stack([rng.integers(1, Is[k] + 1, 37) for k in range(1, N + 1)], 1)
        Xd = pb.shared_points(torch.from_numpy(np.ascontiguousarray(idx.T)).to("cuda")).cpu().numpy()
        for a in range(A):
            assert np.array_equal(Xd[a].T, np.stack([domain[d][idx[:, d] - 1] for d in range(N)], 1))
        pb1 = X._BatchProblem(lambda Xd, which: Xd[:, :, 0], [domain[3]], A)              # N = 1: the fibre is the axis
        X1 = pb1.fibre_points(1, 5, 1, 1, None, None).cpu().numpy()
        assert X1.shape == (A, 1, 5) and all(np.array_equal(X1[a, 0], domain[3]) for a in range(A))


@pytest.mark.parametrize("A", [1, 3])
def test_evaluation_point_weight_and_error_forms(torch, A):
    rng = np.random.default_rng(30 + A)
    for dims, rks in [((3,), (1, 1)), ((2, 5, 3, 4), (1, 2, 7, 3, 1)), ((4, 2, 3), (1, 4, 70, 1))]:
        N = len(dims)
        trains = [[rng.standard_normal((n, a, b)) for n, a, b in zip(dims, rks[:-1], rks[1:])] for _ in range(A)]
        idx = np.stack([rng.integers(1, n + 1, 130) for n in dims], axis=1)
        w = [rng.standard_normal(n) for n in dims]
        scales = [1e-200, 1e200, 1.0][:A] if A == 3 else [1.0]
        for a in range(A):
            trains[a][0] = trains[a][0] * scales[a]
        with torch.cuda.stream(T.tdvp._dev()[1]):
            cores = [torch.from_numpy(np.stack([np.ascontiguousarray(np.transpose(t[k])) for t in trains])).to("cuda") for k in range(N)]
            it = torch.from_numpy(np.ascontiguousarray(idx.T)).to("cuda")
            ref = np.stack([R._evaluate_tt(t, idx, N) for t in trains])
            yref = ref * (1.0 + 1e-3 * rng.standard_normal(ref.shape))
            out, err = X._d_batch_eval(cores, rks, dims, idx=it, yref=torch.from_numpy(yref).to("cuda"), tol=1e-10)
            outw, _ = X._d_batch_eval(cores, rks, dims, w=torch.from_numpy(np.concatenate(w)).to("cuda"))
            out, err, outw = out.cpu().numpy(), err.cpu().numpy(), outw.cpu().numpy().reshape(-1)
        for a in range(A):
            # a value is a sum of products; its rounding error is below (operations) eps (the sum of the moduli), under 4500 operations
            mag = [np.abs(c) for c in trains[a]]
            assert np.all(np.abs(out[a] - ref[a]) <= 1e-12 * R._evaluate_tt(mag, idx, N))
            rw = R._contract_with_weights(trains[a], w)
            assert abs(outw[a] - rw) <= 1e-12 * R._contract_with_weights(mag, [np.abs(x) for x in w])
            s = scales[a]                                                  # the error in units where nothing under- or overflows
            want = np.linalg.norm(yref[a] / s - out[a] / s) / max(np.linalg.norm(yref[a] / s), 1e-10 / s)
            assert abs(err[a] - want) <= 1e-8 * want


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def _check_function(b, tt, g, domain, akw, kw):
    """function b of the last batched run against the restatement and against tt_cross with the same seed"""
    N = len(domain)
    cores, rks, tr = R.cross_maxvol(g, domain, **akw, **kw)
    last = X._LAST_BATCH
    assert tt.ttv_rks == rks and last["sweeps"][b] == tr["sweeps"]
    ls, rs = X.last_batch_sets(b)
    for k in range(2, N + 1):
        assert np.array_equal(ls[k], tr["lsets"][k]), ("lsets", b, k)
    for k in range(1, N):
        assert np.array_equal(rs[k], tr["rsets"][k]), ("rsets", b, k)
    eps_b = list(last["eps"][b])
    for x, y in zip(eps_b, tr["eps"]):
        assert abs(x - y) <= max(1e-8 * abs(y), 1e-13), (b, eps_b, tr["eps"])
    dense, rdense = R.full_tensor(tt.ttv_vec), R.full_tensor(cores)
    assert np.linalg.norm(dense - rdense) <= 1e-10 * np.linalg.norm(rdense)
    one = T.tt_cross(dev_f(g), domain, T.MaxVol(verbose=False, **akw), **kw)
    l1 = X._LAST
    assert one.ttv_rks == tt.ttv_rks and l1["sweeps"] == len(eps_b)
    for k in range(2, N + 1):
        assert np.array_equal(ls[k], l1["lsets"][k])
    for k in range(1, N):
        assert np.array_equal(rs[k], l1["rsets"][k])
    for x, y in zip(eps_b, l1["eps"]):
        assert abs(x - y) <= max(1e-8 * abs(y), 1e-13)
    assert np.linalg.norm(dense - R.full_tensor(one.ttv_vec)) <= 1e-10 * np.linalg.norm(rdense)


@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_driver_parity_per_function(torch, case):
    name, dims, batch, ranks, akw, seed = case
    domain = [np.arange(1.0, n + 1.0) for n in dims]
    fs = table_family(dims, batch, seed)
    kw = dict(ranks=ranks, val_size=50, seed=seed)
    tts = T.tt_cross_batch(batch_f(fs), dims, batch, T.MaxVol(verbose=False, **akw), **kw)
    assert len(tts) == batch
    for b in range(batch):
        _check_function(b, tts[b], fs[b], domain, akw, kw)


def test_mixed_family_active_set(torch):
    seen = []
    tts = T.tt_cross_batch(batch_f(MIXED, seen), MIXED_DOMAIN, 3, T.MaxVol(verbose=False, **MIXED_ALG), **MIXED_KW)
    last = dict(X._LAST_BATCH)
    assert last["sweeps"] == MIXED_SWEEPS
    # the probe, the validation points and the 2 (N - 1) + 1 = 5 fibres of sweep 1 see all three; sweep 2 only the two still running
    assert seen == [[0, 1, 2]] * 7 + [[1, 2]] * 5
    assert [t.ttv_rks for t in tts] == [[1, 1, 1, 1], [1, 2, 2, 1], [1, 2, 2, 1]]
    assert last["eps"][0][-1] < 1e-10 and last["eps"][1][-1] < 1e-10 and last["eps"][2][-1] > 1e-10
    for b in range(3):
        _check_function(b, tts[b], MIXED[b], MIXED_DOMAIN, MIXED_ALG, MIXED_KW)


def test_resident_handle_equals_host_result(torch):
    alg = T.MaxVol(verbose=False, **MIXED_ALG)
    host = T.tt_cross_batch(batch_f(MIXED), MIXED_DOMAIN, 3, alg, **MIXED_KW)
    dev = T.tt_cross_batch(batch_f(MIXED), MIXED_DOMAIN, 3, alg, resident=True, **MIXED_KW)
    assert isinstance(dev, T.DeviceTT) and dev.batch == 3 and dev.cap == [1, 2, 2, 1]
    for b in range(3):
        got = dev.download(b)
        assert dev.ranks(b)[0] == host[b].ttv_rks == got.ttv_rks
        assert all(np.array_equal(x, y) for x, y in zip(got.ttv_vec, host[b].ttv_vec))
    d = T.device.dot(dev, dev)
    for b in range(3):
        want = T.dot(host[b], host[b])
        assert abs(d[b] - want) <= 1e-12 * abs(want)
    dev.free()


def test_integrate_batch_closed_form_and_per_function(torch):
    cs = [0.3, -0.7, 1.1, 2.0]
    ct = torch.tensor(cs, dtype=torch.float64, device="cuda")
    f = lambda Xd, which: torch.exp(ct[which][:, None] * Xd.sum(dim=2))       # noqa: E731
    alg = T.MaxVol(verbose=False, tol=1e-12)
    got = T.tt_integrate_batch(f, 3, 4, alg=alg, ranks=1)
    assert got.shape == (4,)
    for b, c in enumerate(cs):
        exact = ((np.exp(c) - 1.0) / c) ** 3
        assert abs(got[b] - exact) <= 1e-10 * exact
        one = T.tt_integrate(lambda Xd, c=c: torch.exp(c * Xd.sum(dim=1)), 3, alg=alg, ranks=1)
        assert abs(got[b] - one) <= 1e-12 * abs(one)
    got2 = T.tt_integrate_batch(f, [0.0] * 3, [1.0] * 3, batch=4, alg=alg, ranks=1)
    assert np.array_equal(got, got2)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_library_usable(torch):
    dom = [np.linspace(0.1, 1, 5), np.linspace(0.2, 1.3, 4), np.linspace(0.1, 0.9, 6)]
    ok = lambda Xd, which: torch.exp(Xd.sum(dim=2) * (1.0 + which[:, None]))       # noqa: E731
    alg = T.MaxVol(verbose=False)

    def fine():
        tts = T.tt_cross_batch(ok, dom, 2, alg, ranks=1, val_size=20)
        assert [t.ttv_rks for t in tts] == [[1, 1, 1, 1]] * 2

    cases = [
        (lambda: T.tt_cross_batch(ok, dom, 2, T.DMRG(verbose=False)), "DMRG"),
        (lambda: T.tt_cross_batch(ok, dom, 2, T.Greedy(verbose=False)), "Greedy"),
        (lambda: T.tt_cross_batch(ok, dom, 2, T.MaxVol(verbose=False, pivot=T.RandomPivot())), "MaxVolPivot"),
        (lambda: T.tt_cross_batch(lambda Xd, which: Xd.sum(dim=2).to(torch.complex128), dom, 2, alg), "complex"),
        (lambda: T.tt_cross_batch(ok, [d + 0.1j for d in dom], 2, alg), "real domain"),
        (lambda: T.tt_cross_batch(ok, dom, 0, alg), "batch"),
        (lambda: T.tt_cross_batch(lambda Xd, which: torch.ones(Xd.shape[0] * Xd.shape[1] + (Xd.shape[1] == 20), device="cuda"), dom, 2, alg,
                                  val_size=20), "values for .*validation"),
        (lambda: T.tt_cross_batch(lambda Xd, which: Xd[:, :, 0] / ((which[:, None] != 1) | (Xd[:, :, 1] < 1.2)), dom, 3, alg, val_size=3),
         r"non-finite value for function 1 \((the validation points|iteration 1, )"),
        (lambda: T.tt_cross_batch(lambda Xd, which: (which[:, None] != 2) * torch.exp(Xd.sum(dim=2)), dom, 3, alg, ranks=1, val_size=20),
         "zero pivot for function 2"),
    ]
    for call, word in cases:
        with pytest.raises(T.TTNError, match=word):
            call()
        fine()
