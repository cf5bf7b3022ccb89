"""GPU checks of the penalised two-site eigensolvers (csrc/ttn_eig_ortho_kernels.h, include/ttn_eig_ortho.h): parity with the NumPy
restatement (tests/eig_ortho_reference.py) on the dense branch, n_ortho = 0 against the plain entry points bitwise, the lowest levels
against the dense spectrum, Lanczos against dense, batch = single calls bitwise (per-train and shared penalty trains, operator
batches), the first excited level of the d = 32 Ising chain against free fermions, and the refusals of the C layer."""
import ctypes as C

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import eig_ortho_reference as EO
from tests.helpers import to_oracle, to_product

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _lap(d, shift=0.5):
    return O.tto_add(O.Delta(d), O.tto_scale(shift, O.id_tto(d)))


def _sym_rand(dims, R, rng):
    B = O.rand_tto(dims, R, rng)
    Bt = O.TToperator(B.N, [np.ascontiguousarray(np.swapaxes(c, 0, 1)) for c in B.tto_vec], tuple(B.tto_dims), list(B.tto_rks), [0] * B.N)
    return O.tto_add(B, Bt)


def _fn(T, mode):
    return T.solvers.dmrg_eigsolve_ if mode == 1 else T.solvers.mals_eigsolve_


def _solve_dev(T, mode, A, x0, phis, weight, rmax_schedule, **kw):
    """One penalised solve through the device form, host trains in and out: (E, x, r_hist, overlaps)."""
    dims = tuple(x0.ttv_dims)
    dA = T.DeviceTTO(to_product(A))
    dx0 = T.DeviceTT.from_host(to_product(x0))
    dx = T.DeviceTT(dims, T.solvers.dmrg_capacity(dims, x0.ttv_rks, max(rmax_schedule)))
    dphi = [T.DeviceTT.from_host(to_product(p)) for p in phis]
    E, R, ovl = _fn(T, mode)(dA, dx0, dx, rmax_schedule=rmax_schedule, ortho_to=dphi, weight=weight, **kw)
    dx.max_ranks()
    x = to_oracle(dx.download(0))
    for h in [dA, dx0, dx] + dphi:
        h.free()
    return E[0], x, R[0], ovl[0]


def _phis(dims, n_ortho, rmax, rng):
    """The two ends of the chain-slot indexing: a rank-1 train (every bond 1) and trains whose ranks lie above the rmax of x."""
    d = len(dims)
    out = [O.rand_tt(dims, [1] * (d + 1), rng)]
    for k in range(1, n_ortho):
        out.append(O.rand_tt(dims, [1] + [rmax + k] * (d - 1) + [1], rng))
    return out


PARITY = [((2,) * 3, [2], [4]), ((2,) * 4, [3], [4]), ((3, 2, 4, 2), [2], [8]), ((2,) * 8, [2, 3], [4, 8])]


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("n_ortho", [1, 3])
@pytest.mark.parametrize("dims,sched,rmaxs", PARITY)
def test_parity_dense(T, mode, n_ortho, dims, sched, rmaxs):
    """Against the restatement, the same host trains on both sides, weight 10, tol 1e-10: the bars of test_gpu_eigsolve's
    test_parity_dense plus the returned overlaps.  Operators: Delta + 0.5 I and Ising (h = 1.5) on dims of 2, a random symmetric
    operator on the mixed dims (neither constructor exists there).  The tensor comparison holds for every case: no K_eff of a
    restatement run has its two lowest eigenvalues within 1e-6 (asserted)."""
    d = len(dims)
    rng = np.random.default_rng(1000 * d + 10 * n_ortho + mode)
    if all(n == 2 for n in dims):
        ops = [("lap", _lap(d)), ("ising", to_oracle(T.ising_tto(d, J=1.0, h=1.5)))]
    else:
        ops = [("symrand", _sym_rand(dims, 3, rng))]
    for name, A in ops:
        x0 = O.rand_tt(dims, 2, rng)
        phis = _phis(dims, n_ortho, max(rmaxs), rng)
        kw = dict(tol=1e-10, sweep_schedule=sched)
        info = {}
        Er, xr, rr, ovr = EO.two_site_eigsolve_ortho(mode, A, x0, phis, 10.0, rmax_schedule=rmaxs, info=info, **kw)
        Eg, xg, rg, ovg = _solve_dev(T, mode, A, x0, phis, 10.0, rmaxs, **kw)
        assert info["min_gap"] > 1e-6, (name, info)
        assert rg == rr, name
        assert list(xg.ttv_rks) == list(xr.ttv_rks), name
        assert list(xg.ttv_ot) == list(xr.ttv_ot), name
        scale = max(1.0, max(abs(v) for v in Er))
        print(name, "max |E - E_ref| %.2e" % np.max(np.abs(np.array(Eg) - np.array(Er))), "min gap %.2e" % info["min_gap"])
        assert np.max(np.abs(np.array(Eg) - np.array(Er))) <= 1e-10 * scale, name
        vg, vr = O.ttv_to_tensor(xg).ravel(), O.ttv_to_tensor(xr).ravel()
        s = 1.0 if float(vg @ vr) >= 0 else -1.0
        assert np.max(np.abs(s * vg - vr)) <= 1e-8 * np.max(np.abs(vr)), name
        assert abs(np.linalg.norm(vg) - 1.0) <= 1e-12, name
        for p, o in zip(phis, ovg):
            assert abs(o - float(O.dot(p, xg)) / O.norm(p)) <= 1e-10, name


@pytest.mark.parametrize("mode,it_solver", [(1, False), (0, False), (0, True)])
def test_no_penalty_is_the_plain_entry_point(T, mode, it_solver):
    """n_ortho = 0 through ttn_*_eigsolve_ortho: E, r_hist and the cores of ttn_*_eigsolve bit for bit.  DMRG at rank 16, d = 10, runs
    both the dense and the Lanczos branch.  MALS truncates by sv_trunc and at tol 1e-10 its windows stay within the 256 unknowns of the
    dense branch, so it runs a second time with it_solver: every window matrix-free."""
    d = 10
    A = to_oracle(T.ising_tto(d, J=1.0, h=1.5))
    x0 = O.rand_tt((2,) * d, 2, np.random.default_rng(21 + mode))
    dA = T.DeviceTTO(to_product(A))
    dx0 = T.DeviceTT.from_host(to_product(x0))
    cap = T.solvers.dmrg_capacity((2,) * d, x0.ttv_rks, 16)
    a, b = T.DeviceTT((2,) * d, cap), T.DeviceTT((2,) * d, cap)
    E0, R0 = _fn(T, mode)(dA, dx0, a, 1e-10, [2, 3], [4, 16], it_solver, 200, 1e-10)
    it0, _ = T.solvers.eigsolve_stats(1)
    E1, R1, ovl = _fn(T, mode)(dA, dx0, b, 1e-10, [2, 3], [4, 16], it_solver, 200, 1e-10, ortho_to=[])
    it1, _ = T.solvers.eigsolve_stats(1)
    assert ovl.shape == (1, 0)
    if mode == 1 or it_solver:
        assert it0[0] > 0
    assert it1 == it0
    assert E1 == E0 and R1 == R0
    xa, xb = a.download(0), b.download(0)
    assert list(xa.ttv_rks) == list(xb.ttv_rks)
    for ca, cb in zip(xa.ttv_vec, xb.ttv_vec):
        assert np.array_equal(np.asarray(ca), np.asarray(cb))


@pytest.mark.parametrize("mode", ["dmrg", "mals"])
@pytest.mark.parametrize("case", [0, 1, 2])
def test_levels_against_dense_spectrum(T, mode, case):
    """The cases of the CPU test through lowest_states (host form): levels 0..3 within 1e-8 of eigvalsh, overlaps with the earlier
    states <= 1e-8.  XXX at d = 6: levels 1..3 are the triplet and their overlap matrix is the identity."""
    name, A, seed, kw = EO.level_cases()[case]
    ev = np.linalg.eigvalsh(O.qtto_to_matrix(A))
    starts = [to_product(s) for s in EO.level_starts(A, seed + (1 if mode == "dmrg" else 0))]
    E, xs, S = T.lowest_states(to_product(A), starts, 4, 10.0, mode=mode, **kw)
    print(name, mode, "energy errors", np.abs(E - ev[:4]), "overlaps", np.max(np.abs(S - np.eye(4))))
    assert np.max(np.abs(E - ev[:4])) <= 1e-8
    assert np.max(np.abs(S - np.eye(4))) <= 1e-8
    xo = [to_oracle(x) for x in xs]
    for k in range(4):
        for j in range(k):
            assert abs(float(O.dot(xo[j], xo[k]))) / O.norm(xo[j]) <= 1e-8
    if name == "xxx":
        assert np.max(np.abs(E[1:] - ev[1])) <= 1e-8 and np.max(np.abs(S[1:, 1:] - np.eye(3))) <= 1e-8


@pytest.mark.parametrize("mode", [1, 0])
def test_lanczos_vs_dense(T, mode):
    d = 8
    rng = np.random.default_rng(41 + mode)
    for A in (_lap(d), to_oracle(T.ising_tto(d, J=1.0, h=1.5))):
        x0 = O.rand_tt((2,) * d, 2, rng)
        phis = [O.rand_tt((2,) * d, 2, rng), O.rand_tt((2,) * d, 3, rng)]
        kw = dict(tol=1e-10, sweep_schedule=[3])
        Ed, _, _, _ = _solve_dev(T, mode, A, x0, phis, 10.0, [8], **kw)
        El, _, _, _ = _solve_dev(T, mode, A, x0, phis, 10.0, [8], it_solver=True, itslv_thresh=1, linsolv_tol=1e-10, **kw)
        it, res = T.solvers.eigsolve_stats(1)
        print("|E_l - E_d| %.2e" % abs(El[-1] - Ed[-1]), "residual %.2e" % res[0], "applications", it[0])
        assert abs(El[-1] - Ed[-1]) <= 1e-9
        assert res[0] <= 1e-10 and it[0] > 0


def _upload_batch(T, dims, trains):
    top = [max(int(t.ttv_rks[k]) for t in trains) for k in range(len(dims) + 1)]
    h = T.DeviceTT(dims, top, batch=len(trains))
    for i, t in enumerate(trains):
        h.upload(i, to_product(t))
    return h


def _same_train(a, b):
    assert list(a.ttv_rks) == list(b.ttv_rks)
    for ca, cb in zip(a.ttv_vec, b.ttv_vec):
        assert np.array_equal(np.asarray(ca), np.asarray(cb))


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("form", ["per_train", "shared", "operator_batch"])
def test_batch_equals_single_calls(T, mode, form):
    """d = 10, B = 8, two penalty trains, rank 16 (dense and Lanczos windows): every train of the batch is bitwise its single call.
    per_train: phi batches of 8 whose trains have different ranks; shared: phi batches of 1; operator_batch: eight fields h."""
    d, B = 10, 8
    dims = (2,) * d
    rng = np.random.default_rng(83 + mode)
    x0s = [O.rand_tt(dims, 2, rng) for _ in range(B)]
    sched, rmaxs = [2, 3], [4, 16]
    hs = [1.5] * B
    if form == "operator_batch":
        hs = list(np.linspace(0.7, 2.1, B))
        ZZ, X = T.DeviceTTO(T.ising_tto(d, J=1.0, h=0.0)), T.DeviceTTO(T.ising_tto(d, J=0.0, h=1.0))
        dA = T.DeviceTTO.lincomb([ZZ, X], np.array([[1.0, h] for h in hs]))
        singles = [dA.select(i) for i in range(B)]
    else:
        dA = T.DeviceTTO(T.ising_tto(d, J=1.0, h=1.5))
        singles = [dA] * B
    if form == "shared":
        phis = [[O.rand_tt(dims, 3, rng)] * B, [O.rand_tt(dims, 1, rng)] * B]
        dphi = [T.DeviceTT.from_host(to_product(p[0])) for p in phis]
    else:
        phis = [[O.rand_tt(dims, 1 + (i + j) % 4, rng) for i in range(B)] for j in range(2)]
        dphi = [_upload_batch(T, dims, p) for p in phis]
    w = 5.0 + rng.random((B, 2)) * 10.0
    cap = T.solvers.dmrg_capacity(dims, x0s[0].ttv_rks, max(rmaxs))
    dx0 = _upload_batch(T, dims, x0s)
    dx = T.DeviceTT(dims, cap, batch=B)
    Eb, Rb, Ob = _fn(T, mode)(dA, dx0, dx, 1e-10, sched, rmaxs, ortho_to=dphi, weight=w)
    for i in range(B):
        s0 = T.DeviceTT.from_host(to_product(x0s[i]))
        s = T.DeviceTT(dims, cap)
        sp = [T.DeviceTT.from_host(to_product(phis[j][i])) for j in range(2)]
        Es, Rs, Os = _fn(T, mode)(singles[i], s0, s, 1e-10, sched, rmaxs, ortho_to=sp, weight=w[i])
        assert Es[0] == Eb[i] and Rs[0] == Rb[i], i
        assert np.array_equal(Os[0], Ob[i]), i
        _same_train(dx.download(i), s.download(0))
        for h in [s0, s] + sp:
            h.free()


REF_REL_ERR = 5.97e-13     # two_site_eigsolve_ortho(1, ...) on the CPU, same schedule, starts and weight: |rayleigh - E1| / |E1|


def test_ising_d32_first_excited(T):
    """Transverse-field Ising, d = 32, J = 1, h = 1.5, matrix-free, schedule [2, 3] / [8, 16], linsolv_tol 1e-10, weight 10: the ground
    state, then level 1 against it.  rayleigh(level 1) against E0 + eps_min of the free fermions; the bar is ten times the relative
    error of the restatement on the CPU with this schedule and these starts, REF_REL_ERR above, and never looser than 1e-6.
    Overlap with the ground state <= 1e-8.  Measured on the device: relative error 5.98e-13, overlap 6.2e-14."""
    d = 32
    A = to_oracle(T.ising_tto(d, J=1.0, h=1.5))
    rng = np.random.default_rng(5)
    x0 = O.rand_tt((2,) * d, [1] + [2] * (d - 1) + [1], rng)
    x1 = O.rand_tt((2,) * d, [1] + [2] * (d - 1) + [1], rng)
    kw = dict(tol=1e-12, sweep_schedule=[2, 3], rmax_schedule=[8, 16], linsolv_tol=1e-10)
    _, g, _ = T.dmrg_eigsolve(to_product(A), to_product(x0), **kw)
    _, x, _ = T.dmrg_eigsolve(to_product(A), to_product(x1), ortho_to=[g], weight=10.0, **kw)
    it, res = T.solvers.eigsolve_stats(1)
    _, e1, _ = EO.free_fermion_levels(d, 1.0, 1.5)
    ray = float(T.rayleigh(to_product(A), x))
    rel = abs(ray - e1) / abs(e1)
    ovl = abs(float(T.dot(g, x))) / float(T.norm(g))
    print("level 1: rayleigh %.12f exact %.12f relative error %.3e overlap %.3e Lanczos applications %d" % (ray, e1, rel, ovl, it[0]))
    assert rel <= min(10.0 * REF_REL_ERR, 1e-6)
    assert ovl <= 1e-8
    assert it[0] > 0 and res[0] <= 1e-10


def _cores(h, b=0):
    t = h.download(b)
    return [np.array(c, copy=True) for c in t.ttv_vec], list(t.ttv_rks)


def test_refusals(T):
    """Every refusal of include/ttn_eig_ortho.h returns its code, names the call and leaves x as it was; a valid call on the same
    handles succeeds afterwards.  (The workspace refusal TTN_ERR_CAPACITY: test_capacity_refusal.)"""
    E_ = T._lib
    L = E_.lib()
    d, B = 4, 2
    dims = (2,) * d
    rng = np.random.default_rng(3)
    dA = T.DeviceTTO(T.Delta(d))
    dx0 = _upload_batch(T, dims, [O.rand_tt(dims, 2, rng) for _ in range(B)])
    dx = _upload_batch(T, dims, [O.rand_tt(dims, [1, 2, 4, 2, 1], rng) for _ in range(B)])
    phi = _upload_batch(T, dims, [O.rand_tt(dims, 2, rng) for _ in range(B)])
    phi1 = T.DeviceTT.from_host(to_product(O.rand_tt(dims, 3, rng)))
    phi3 = _upload_batch(T, dims, [O.rand_tt(dims, 2, rng) for _ in range(3)])
    zero = T.DeviceTT.from_host(to_product(O.zeros_tt(dims, [1, 2, 2, 2, 1])), batch=B)
    other = T.DeviceTT.from_host(to_product(O.rand_tt((2, 3, 2, 2), 2, rng)), batch=B)
    cplx = T.DeviceTT(dims, [1, 2, 2, 2, 1], batch=B, dtype=np.complex128)
    before = [_cores(dx, b) for b in range(B)]
    arr = C.c_int64 * 1
    hl = T.solvers.eigsolve_history_len(1, d, [2])
    Eh, Rh, ov = (C.c_double * (B * hl))(), (C.c_int64 * (B * hl))(), (C.c_double * (B * 8))()

    def call(fn, handles, weights, n=None, x=dx, x0=dx0):
        n = len(handles) if n is None else n
        ph = (C.c_void_p * max(len(handles), 1))(*[h.h if h is not None else None for h in handles])
        w = (C.c_double * max(len(weights), 1))(*weights)
        return fn(dA.h, x0.h, x.h, n, ph, w, 1e-10, 1, arr(2), arr(4), 0, 200, 1e-8, 256, hl, Eh, Rh, ov)

    ok_w = [10.0] * 16
    for fn, who in ((L.ttn_dmrg_eigsolve_ortho, "ttn_dmrg_eigsolve_ortho"), (L.ttn_mals_eigsolve_ortho, "ttn_mals_eigsolve_ortho")):
        if fn is L.ttn_mals_eigsolve_ortho:
            hl = T.solvers.eigsolve_history_len(0, d, [2])
            Eh, Rh = (C.c_double * (B * hl))(), (C.c_int64 * (B * hl))()
        cases = [
            (call(fn, [phi] * 9, ok_w + [10.0] * 2), E_.TTN_ERR_ARG),                   # n_ortho = 9
            (call(fn, [phi], ok_w, n=-1), E_.TTN_ERR_ARG),
            (call(fn, [phi, None], ok_w), E_.TTN_ERR_ARG),                              # a null handle
            (call(fn, [dx], ok_w), E_.TTN_ERR_ARG),                                     # phi is x
            (call(fn, [phi, dx0], ok_w), E_.TTN_ERR_ARG),                               # phi is x0
            (call(fn, [phi3], ok_w), E_.TTN_ERR_ARG),                                   # batch 3 against 2
            (call(fn, [phi], [10.0, float("nan")]), E_.TTN_ERR_ARG),
            (call(fn, [phi], [0.0, 10.0]), E_.TTN_ERR_ARG),
            (call(fn, [phi], [10.0, -1.0]), E_.TTN_ERR_ARG),
            (call(fn, [phi, zero], ok_w), E_.TTN_ERR_ARG),                              # ||phi|| = 0
            (call(fn, [other], ok_w), E_.TTN_ERR_DIMS),
            (call(fn, [cplx], ok_w), E_.TTN_ERR_UNSUPPORTED),
        ]
        for k, (rc, want) in enumerate(cases):
            assert rc == want, (who, k, rc, E_.last_error())
        assert call(fn, [phi, None], ok_w) == E_.TTN_ERR_ARG and who in E_.last_error()
        for b in range(B):
            cores, rks = _cores(dx, b)
            assert rks == before[b][1]
            for ca, cb in zip(cores, before[b][0]):
                assert np.array_equal(ca, cb)
    # an operator batch is refused by the C entry points (solvers.py serves one through select(b), test_batch_equals_single_calls)
    dAb = T.DeviceTTO.stack([T.Delta(d), T.Delta(d)])
    ph = (C.c_void_p * 1)(phi.h)
    rc = L.ttn_dmrg_eigsolve_ortho(dAb.h, dx0.h, dx.h, 1, ph, (C.c_double * 2)(10.0, 10.0), 1e-10, 1, arr(2), arr(4), 0, 200, 1e-8, 256,
                                   T.solvers.eigsolve_history_len(1, d, [2]), Eh, Rh, ov)
    assert rc == E_.TTN_ERR_UNSUPPORTED and "operator batch" in E_.last_error()
    out = T.DeviceTT(dims, [1, 2, 4, 2, 1], batch=B)
    E, R, ovl = T.solvers.dmrg_eigsolve_(dA, dx0, out, 1e-10, [2], [4], ortho_to=[phi, phi1], weight=10.0)
    assert np.all(np.isfinite(E)) and ovl.shape == (B, 2)
    for b in range(B):
        xb = to_oracle(out.download(b))
        pb, p1 = to_oracle(phi.download(b)), to_oracle(phi1.download(0))
        assert abs(ovl[b, 0] - float(O.dot(pb, xb)) / O.norm(pb)) <= 1e-10
        assert abs(ovl[b, 1] - float(O.dot(p1, xb)) / O.norm(p1)) <= 1e-10


@pytest.mark.parametrize("mode", [1, 0])
def test_capacity_refusal(T, mode):
    """The workspace refusal, reached with small handles: a result handle with the capacities [1, 128, 1, 128, 1] has cores of 8 KB per
    train, but its window (1, 2) is a two-site problem of 65 536 unknowns at capacity, whose Lanczos area alone is (30 + 1 + 10 + R)
    x 65 536 doubles per train (about 25 MB, with the G / H slots about 30 MB): 32 768 trains ask for about a terabyte, more than any
    device holds, and the call returns TTN_ERR_CAPACITY from its size check, before the workspace is grown, before the norms of phi are
    taken and before x is written.  The overlap chains and projected vectors of the penalty are part of that sum.  x (two trains
    compared) is unchanged; the same operator, starts and phi then solve into a handle of small capacity."""
    E_ = T._lib
    L = E_.lib()
    d, B = 4, 32768
    dims = (2,) * d
    rng = np.random.default_rng(13 + mode)
    dA = T.DeviceTTO(T.Delta(d))
    dx0 = T.DeviceTT.from_host(to_product(O.rand_tt(dims, 1, rng)), batch=B)
    big = T.DeviceTT.from_host(to_product(O.rand_tt(dims, [1, 2, 1, 2, 1], rng)), batch=B, cap_rks=[1, 128, 1, 128, 1])
    phi = T.DeviceTT.from_host(to_product(O.rand_tt(dims, 2, rng)))          # batch 1: shared
    before = [_cores(big, b) for b in (0, B - 1)]
    hl = T.solvers.eigsolve_history_len(mode, d, [2])
    Eh, Rh, ov = np.zeros(B * hl), np.zeros(B * hl, dtype=np.int64), np.zeros(B)
    w = np.full(B, 10.0)
    arr = C.c_int64 * 1
    fn, who = (L.ttn_dmrg_eigsolve_ortho, "ttn_dmrg_eigsolve_ortho") if mode == 1 else (L.ttn_mals_eigsolve_ortho, "ttn_mals_eigsolve_ortho")
    rc = fn(dA.h, dx0.h, big.h, 1, (C.c_void_p * 1)(phi.h), w.ctypes.data_as(E_.p_f64), 1e-10, 1, arr(2), arr(128), 0, 200, 1e-8, 256, hl,
            Eh.ctypes.data_as(E_.p_f64), Rh.ctypes.data_as(E_.p_i64), ov.ctypes.data_as(E_.p_f64))
    assert rc == E_.TTN_ERR_CAPACITY, (rc, E_.last_error())
    assert who in E_.last_error() and "workspace" in E_.last_error()
    for b, (cores0, rks0) in zip((0, B - 1), before):
        cores, rks = _cores(big, b)
        assert rks == rks0
        for ca, cb in zip(cores, cores0):
            assert np.array_equal(ca, cb)
    out = T.DeviceTT(dims, [1, 2, 4, 2, 1], batch=B)
    E, R, ovl = _fn(T, mode)(dA, dx0, out, 1e-10, [2], [4], ortho_to=[phi], weight=10.0)
    assert len(E) == B and np.all(np.isfinite(np.array(E))) and ovl.shape == (B, 1)
    for h in (dA, dx0, big, phi, out):
        h.free()
