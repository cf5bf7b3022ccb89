"""GPU checks of dmrg_eigsolve / mals_eigsolve (csrc/ttn_eigsolve_kernels.h): the reference's assertions (test/test_dmrg.jl:100-171,
test/test_mals.jl:79-160) through the device, parity with the NumPy restatement (tests/eig_reference.py) on the dense local branch,
oracle-free exact answers (the QTT Laplacian, the free-fermion transverse-field Ising chain at d = 32 on the matrix-free branch), Lanczos
against the dense branch, batch = single calls bitwise, and the refusals."""
import math

import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator, eigsh

from oracle import tt_oracle as O
from tests import eig_reference as ER
from tests.helpers import to_oracle, to_product

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _spd(d, shift=3.0):
    return O.tto_add(O.Delta(d), O.tto_scale(shift, O.id_tto(d)))


def _solve(T, mode, A, x0, **kw):
    fn = T.dmrg_eigsolve if mode == 1 else T.mals_eigsolve
    E, x, r = fn(to_product(A), to_product(x0), **kw)
    return E, to_oracle(x), r


@pytest.mark.parametrize("mode", [1, 0])
def test_reference_cases(T, mode):
    """test/test_dmrg.jl:100-171 (N = 2) and test/test_mals.jl:79-160 through the device."""
    rng = np.random.default_rng(11 + mode)
    d = 4
    x0 = O.rand_tt((2,) * d, [1, 2, 2, 2, 1], rng)
    E, x, r = _solve(T, mode, _spd(d), x0, sweep_schedule=[2], rmax_schedule=[4])
    assert all(isinstance(v, float) for v in E) and all(isinstance(v, int) for v in r) and len(E) == len(r)
    assert x.N == d and tuple(x.ttv_dims) == (2,) * d
    A = _spd(d, 3.0)
    E, x, _ = _solve(T, mode, A, x0, sweep_schedule=[4], rmax_schedule=[4])
    rq = O.dot(x, O.apply(A, x)) / O.dot(x, x)
    assert E[-1] > 0 and math.isclose(rq, E[-1], rel_tol=0.1)
    E, _, _ = _solve(T, mode, _spd(d, 2.0), x0, sweep_schedule=[4], rmax_schedule=[4])
    assert E[-1] <= E[0] + 1e-8
    x1 = O.rand_tt((2,) * d, [1] * 5, rng)
    E, x, r = _solve(T, mode, _spd(d, 2.0), x1, sweep_schedule=[2, 4], rmax_schedule=[2, 4])
    assert len(E) >= 2 and max(x.ttv_rks) <= 4 and all(v > 0 for v in r)
    E, _, _ = _solve(T, mode, _spd(d, 1.0), x0, sweep_schedule=[2], rmax_schedule=[4])
    assert all(np.isfinite(E))
    if mode == 1:                                        # test_dmrg.jl:154-171
        x3 = O.rand_tt((2,) * 3, [1, 2, 2, 1], rng)
        E, x, r = _solve(T, mode, _spd(3, 2.0), x3, sweep_schedule=[1], rmax_schedule=[2], it_solver=True, itslv_thresh=1, linsolv_maxiter=20)
    else:                                                # test_mals.jl:146-160
        E, x, r = _solve(T, mode, _spd(d, 2.0), x0, sweep_schedule=[2], rmax_schedule=[4], it_solver=True, itslv_thresh=1)
    assert len(E) > 0 and all(np.isfinite(E)) and len(r) == len(E)


def _ops(T, d):
    ops = [("lap", _spd(d, 0.5)), ("ising", to_oracle(T.ising_tto(d, J=1.0, h=1.5)))]
    if d % 2 == 0 and d <= 6:
        ops.append(("xxx", to_oracle(T.xxx_tto(d))))
    return ops


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("d,sched,rmaxs,tol", [(3, [2], [4], 1e-10), (4, [3], [4], 1e-10), (6, [1, 3], [4, 8], 1e-10),
                                               (8, [2, 3], [4, 8], 1e-10), (10, [2], [4], 1e-10)])
def test_parity_dense(T, mode, d, sched, rmaxs, tol):
    rng = np.random.default_rng(100 * d + mode)
    for name, A in _ops(T, d):
        x0 = O.rand_tt((2,) * d, 2, rng)
        Eg, xg, rg = _solve(T, mode, A, x0, tol=tol, sweep_schedule=sched, rmax_schedule=rmaxs)
        Er, xr, rr = ER.two_site_eigsolve(mode, A, x0, tol=tol, sweep_schedule=sched, rmax_schedule=rmaxs)
        assert rg == rr, name
        assert list(xg.ttv_rks) == list(xr.ttv_rks), name
        assert list(xg.ttv_ot) == list(xr.ttv_ot), name
        scale = max(1.0, max(abs(v) for v in Er))
        assert np.max(np.abs(np.array(Eg) - np.array(Er))) <= 1e-10 * scale, name
        vg, vr = O.ttv_to_tensor(xg).ravel(), O.ttv_to_tensor(xr).ravel()
        s = 1.0 if float(vg @ vr) >= 0 else -1.0
        assert np.max(np.abs(s * vg - vr)) <= 1e-8 * np.max(np.abs(vr)), name
        assert abs(np.linalg.norm(vg) - 1.0) <= 1e-12, name


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("d", [3, 5, 8])
def test_laplacian_exact(T, mode, d):
    """The smallest eigenvalue of tridiag(-1, 2, -1) + s I of size 2^d, 2 - 2 cos(pi / (2^d + 1)) + s: its vector is a QTT sine (rank 2)."""
    s = 1.0
    x0 = O.rand_tt((2,) * d, 2, np.random.default_rng(d))
    E, x, _ = _solve(T, mode, _spd(d, s), x0, tol=1e-12, sweep_schedule=[3], rmax_schedule=[4])
    assert abs(E[-1] - (2.0 - 2.0 * math.cos(math.pi / (2 ** d + 1)) + s)) <= 1e-11


@pytest.mark.parametrize("rmax", [16, 32])
def test_ising_d32_free_fermions(T, rmax):
    """Transverse-field Ising, d = 32, J = 1, h = 1.5, matrix-free branch (local problems up to 1024 / 4096 unknowns): E[end] within 1e-8
    relative of the free-fermion ground energy.  Schedule: sweeps 1-2 at rank rmax / 2, sweep 3 at rank rmax, then the closing solve
    (the restatement reaches 4e-15 with it at rmax 16)."""
    d = 32
    x0 = O.rand_tt((2,) * d, [1] + [2] * (d - 1) + [1], np.random.default_rng(5))
    E, x, r = _solve(T, 1, to_oracle(T.ising_tto(d, J=1.0, h=1.5)), x0, tol=1e-12, sweep_schedule=[2, 3], rmax_schedule=[rmax // 2, rmax],
                     linsolv_tol=1e-10)
    ex = ER.free_fermion_ground_energy(d, 1.0, 1.5)
    assert abs(E[-1] - ex) <= 1e-8 * abs(ex)
    assert max(r) == rmax
    it, res = T.solvers.eigsolve_stats(1)
    assert it[0] > 0 and res[0] <= 1e-10


@pytest.mark.parametrize("mode", [1, 0])
def test_lanczos_vs_dense(T, mode):
    d = 8
    rng = np.random.default_rng(31 + mode)
    for A in (_spd(d, 0.5), to_oracle(T.ising_tto(d, J=1.0, h=1.5))):
        x0 = O.rand_tt((2,) * d, 2, rng)
        Ed, _, rd = _solve(T, mode, A, x0, tol=1e-10, sweep_schedule=[3], rmax_schedule=[8])
        El, xl, rl = _solve(T, mode, A, x0, tol=1e-10, sweep_schedule=[3], rmax_schedule=[8], it_solver=True, itslv_thresh=1,
                            linsolv_tol=1e-10)
        assert abs(El[-1] - Ed[-1]) <= 1e-9
        it, res = T.solvers.eigsolve_stats(1)
        assert res[0] <= 1e-10
        assert 0 < it[0] < len(El) * 200 * 30            # below the cap: linsolv_maxiter restarts of 30 applications per solve


@pytest.mark.parametrize("mode", [1, 0])
def test_batch_equals_single_calls(T, mode):
    d, B = 10, 8
    rng = np.random.default_rng(77 + mode)
    A = to_oracle(T.ising_tto(d, J=1.0, h=1.5))
    x0s = [O.rand_tt((2,) * d, 2, rng) for _ in range(B)]
    sched, rmaxs = [2, 3], [4, 16]                       # rank 16: the middle windows (512 unknowns) take the matrix-free branch
    dA = T.DeviceTTO(to_product(A))
    cap = T.solvers.dmrg_capacity((2,) * d, x0s[0].ttv_rks, max(rmaxs))
    dx0 = T.DeviceTT((2,) * d, x0s[0].ttv_rks, batch=B)
    for i in range(B):
        dx0.upload(i, to_product(x0s[i]))
    dx = T.DeviceTT((2,) * d, cap, batch=B)
    fn = T.solvers.dmrg_eigsolve_ if mode == 1 else T.solvers.mals_eigsolve_
    Eb, Rb = fn(dA, dx0, dx, 1e-10, sched, rmaxs)
    for i in range(B):
        s0 = T.DeviceTT.from_host(to_product(x0s[i]))
        s = T.DeviceTT((2,) * d, cap)
        Es, Rs = fn(dA, s0, s, 1e-10, sched, rmaxs)
        assert Es[0] == Eb[i] and Rs[0] == Rb[i]
        a, b = dx.download(i), s.download(0)
        assert list(a.ttv_rks) == list(b.ttv_rks)
        for ca, cb in zip(a.ttv_vec, b.ttv_vec):
            assert np.array_equal(np.asarray(ca), np.asarray(cb))
        s0.free(); s.free()


def test_refusals(T):
    d = 4
    A = T.Delta(d)
    x0 = to_product(O.rand_tt((2,) * d, 2, np.random.default_rng(1)))
    with pytest.raises(T.TTNError):
        T.dmrg_eigsolve(A, x0, N=1)
    with pytest.raises(T.TTNError):
        T.mals_eigsolve(A, x0, sweep_schedule=[3, 2], rmax_schedule=[2, 4])
    with pytest.raises(T.TTNError):
        T.heisenberg_xyz_tto(d, lam=1.0, field="y")
    # the C entry point refuses a wrong history length and an oversized capacity before it launches anything
    dA = T.DeviceTTO(A)
    dx0 = T.DeviceTT.from_host(x0)
    dx = T.DeviceTT((2,) * d, [1, 2, 4, 2, 1])
    import ctypes as C
    arr = C.c_int64 * 1
    E = (C.c_double * 64)()
    R = (C.c_int64 * 64)()
    L = T._lib.lib()
    rc = L.ttn_dmrg_eigsolve(dA.h, dx0.h, dx.h, 1e-12, 1, arr(2), arr(4), 0, 200, 1e-8, 256, 3, E, R)
    assert rc == T._lib.TTN_ERR_ARG
    big = T.DeviceTT((2,) * 16, [1, 2, 4, 8, 16, 32, 64, 128, 200, 128, 64, 32, 16, 8, 4, 2, 1])   # n * cap = 400 > 256
    b0 = T.DeviceTT((2,) * 16, [1] * 17)
    dA16 = T.DeviceTTO(T.Delta(16))
    rc = L.ttn_dmrg_eigsolve(dA16.h, b0.h, big.h, 1e-12, 1, arr(2), arr(4), 0, 200, 1e-8, 256, 2 * 14 + 1, E, R)
    assert rc == T._lib.TTN_ERR_UNSUPPORTED


# ---- mixed local dimensions, hard spectra, the dense branch above 256 unknowns, Lanczos edges, ragged batches, scale and shift ----

MIXED = [(3, 2, 4, 2, 3), (2, 3, 3, 2, 2, 3), (3,) * 6]


def _sym_rand(dims, R, rng):
    """S = B + B^T with B = rand_tto(dims, R) (operator rank up to 2R): B^T swaps axes 0 and 1 of every core."""
    B = O.rand_tto(dims, R, rng)
    Bt = O.TToperator(B.N, [np.ascontiguousarray(np.swapaxes(c, 0, 1)) for c in B.tto_vec], tuple(B.tto_dims), list(B.tto_rks), [0] * B.N)
    return O.tto_add(B, Bt)


def _dense(A):
    P = int(np.prod(A.tto_dims))
    return O.tto_to_tensor(A).reshape(P, P)


def _id_tto(dims):
    return O.TToperator(len(dims), [np.eye(n)[:, :, None, None].copy() for n in dims], tuple(dims), [1] * (len(dims) + 1), [0] * len(dims))


def _full_rank(dims):
    return max(min(int(np.prod(dims[:k])), int(np.prod(dims[k:]))) for k in range(1, len(dims)))


def _residual(A, x, E):
    """||A x - E x|| / ||x|| through the oracle."""
    r = O.sub(O.apply(A, x), O.scale(E, x))
    return O.norm(r) / O.norm(x)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("dims", MIXED)
def test_mixed_dims_parity_dense(T, mode, dims):
    """Mixed local dimensions (n_i != n_{i+1} in every window) with random symmetric operators of rank 16 on the dense branch: bitwise
    rank history, energies to 1e-10 and vectors to 1e-8 against the restatement; then the Lanczos branch on the same problem, E[end]
    within 1e-9 of the dense one."""
    rng = np.random.default_rng(sum(dims) + 7 * mode)
    A = _sym_rand(dims, 8, rng)
    assert max(A.tto_rks) > 5                            # operator ranks above the spin chains' 5
    x0 = O.rand_tt(dims, 2, rng)
    kw = dict(tol=1e-10, sweep_schedule=[1, 3], rmax_schedule=[3, 4])       # every local problem <= 256 unknowns: dense in both modes
    Eg, xg, rg = _solve(T, mode, A, x0, **kw)
    Er, xr, rr = ER.two_site_eigsolve(mode, A, x0, **kw)
    assert rg == rr
    assert list(xg.ttv_rks) == list(xr.ttv_rks)
    scale = max(1.0, max(abs(v) for v in Er))
    assert np.max(np.abs(np.array(Eg) - np.array(Er))) <= 1e-10 * scale
    vg, vr = O.ttv_to_tensor(xg).ravel(), O.ttv_to_tensor(xr).ravel()
    s = 1.0 if float(vg @ vr) >= 0 else -1.0
    assert np.max(np.abs(s * vg - vr)) <= 1e-8 * np.max(np.abs(vr))
    El, _, _ = _solve(T, mode, A, x0, it_solver=True, linsolv_tol=1e-12, **kw)
    assert abs(El[-1] - Eg[-1]) <= 1e-9 * scale


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("dims", MIXED)
def test_mixed_dims_full_rank_exact(T, mode, dims):
    """At full rank the two-site problems span the whole space: E[end] is the smallest eigenvalue of the densified operator (1e-10 ||S||).
    DMRG takes the dense branch up to 2048 unknowns (itslv_thresh = 2048); MALS keeps its threshold 256, so (3,)^6 runs Lanczos there."""
    rng = np.random.default_rng(31 * len(dims) + mode)
    A = _sym_rand(dims, 8, rng)
    w = np.linalg.eigvalsh(_dense(A))
    x0 = O.rand_tt(dims, 1, rng)
    E, x, _ = _solve(T, mode, A, x0, tol=1e-13, sweep_schedule=[3], rmax_schedule=[_full_rank(dims)], itslv_thresh=2048,
                     linsolv_tol=1e-12)
    nrm = float(np.max(np.abs(w)))
    assert abs(E[-1] - w[0]) <= 1e-10 * nrm
    assert _residual(A, x, E[-1]) <= 1e-6 * nrm


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("h", [0.5, 1.0])
def test_ising_d32_ordered_and_critical(T, mode, h):
    """Transverse-field Ising, d = 32, J = 1, rank up to 16: h = 0.5 is ordered (a doublet split by about h^d, the local problems
    near-degenerate), h = 1.0 critical.  The schedule of test_ising_d32_free_fermions at rmax 16; local problems above 256 unknowns take
    the matrix-free branch.  Tolerance against the free-fermion energy: 1e-10 relative.  The restatement (tests/eig_reference.py) at this
    schedule and start is off by 5.3e-12 (DMRG, both fields), 6.4e-12 (MALS, h = 0.5) and 6.7e-12 (MALS, h = 1.0)."""
    d = 32
    x0 = O.rand_tt((2,) * d, [1] + [2] * (d - 1) + [1], np.random.default_rng(5))
    E, x, r = _solve(T, mode, to_oracle(T.ising_tto(d, J=1.0, h=h)), x0, tol=1e-12, sweep_schedule=[2, 3], rmax_schedule=[8, 16],
                     linsolv_tol=1e-10)
    ex = ER.free_fermion_ground_energy(d, 1.0, h)
    assert abs(E[-1] - ex) <= 1e-10 * abs(ex)
    assert E[-1] >= ex - 1e-12 * abs(ex)                 # variational: not below the ground state beyond rounding
    it, res = T.solvers.eigsolve_stats(1)
    assert res[0] <= 1e-10


@pytest.mark.parametrize("mode,it_solver", [(1, False), (0, False), (0, True)])
@pytest.mark.parametrize("d", [8, 16])
def test_classical_ising_degenerate(T, mode, d, it_solver):
    """h = 0: E = -(d - 1)|J| exactly, doubly degenerate (the two Neel states); the local problems are diagonal with repeated smallest
    entries.  Energy and eigen-residual only: the vector is any state of the doublet.  Not DMRG with Lanczos: once the train is a
    product of basis states, the swapped start block of a left move is itself an eigenvector of the diagonal K (an excited one), Lanczos
    breaks down on it at j = 0, as KrylovKit does from an exact eigenvector, and the sweep stays there (E = -3 at d = 8)."""
    A = to_oracle(T.ising_tto(d, J=1.0, h=0.0))
    x0 = O.rand_tt((2,) * d, 2, np.random.default_rng(40 + d + mode))
    E, x, _ = _solve(T, mode, A, x0, tol=1e-12, sweep_schedule=[2], rmax_schedule=[4], it_solver=it_solver, linsolv_tol=1e-12)
    assert abs(E[-1] + (d - 1)) <= 1e-12 * d
    assert _residual(A, x, E[-1]) <= 1e-9


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("d", [3, 5, 7, 9, 11])
def test_xxx_odd(T, mode, d):
    """The XXX chain at odd d has a degenerate ground state (total spin 1/2): at full rank, E[end] against eigvalsh to 1e-11 and the
    eigen-residual to 1e-6, about sqrt(linsolv_tol) (any vector of the doublet passes, a vector partly outside it does not).  The device
    reaches 2e-8 to 2e-7, the restatement (LAPACK SVD in the core moves) 1e-13: the device's SVD core moves, not the local eigensolver,
    set that floor.  MALS runs with tol = 0: its sv_trunc drops a tail of squared weight up to tol ||s||^2, which at tol = 1e-13 leaves
    a residual of 1e-5 at d = 11 (the restatement too)."""
    A = to_oracle(T.xxx_tto(d))
    ev = np.linalg.eigvalsh(O.qtto_to_matrix(A))[0]
    x0 = O.rand_tt((2,) * d, 2, np.random.default_rng(60 + d + mode))
    E, x, _ = _solve(T, mode, A, x0, tol=1e-13 if mode == 1 else 0.0, sweep_schedule=[2, 4], rmax_schedule=[8, 2 ** (d // 2)],
                     linsolv_tol=1e-12)
    assert abs(E[-1] - ev) <= 1e-11 * max(1.0, abs(ev))
    assert _residual(A, x, E[-1]) <= 1e-6


def test_dense_above_256(T):
    """DMRG with itslv_thresh = 2048: Ising d = 10 at rank 16 has local problems of 1024 unknowns on the dense branch.  Parity with the
    restatement, and the Lanczos branch within 1e-9."""
    d = 10
    A = to_oracle(T.ising_tto(d, J=1.0, h=1.5))
    x0 = O.rand_tt((2,) * d, 2, np.random.default_rng(10))
    kw = dict(tol=1e-10, sweep_schedule=[2, 3], rmax_schedule=[8, 16], itslv_thresh=2048)
    Eg, xg, rg = _solve(T, 1, A, x0, **kw)
    Er, xr, rr = ER.two_site_eigsolve(1, A, x0, **kw)
    assert max(rg) >= 12 and rg == rr                    # rank 12 or more: windows of 2 * 12 * 2 * 12 > 256 unknowns
    assert np.max(np.abs(np.array(Eg) - np.array(Er))) <= 1e-10 * max(abs(v) for v in Er)
    vg, vr = O.ttv_to_tensor(xg).ravel(), O.ttv_to_tensor(xr).ravel()
    s = 1.0 if float(vg @ vr) >= 0 else -1.0
    assert np.max(np.abs(s * vg - vr)) <= 1e-8 * np.max(np.abs(vr))
    El, _, _ = _solve(T, 1, A, x0, it_solver=True, linsolv_tol=1e-12, **kw)
    assert abs(El[-1] - Eg[-1]) <= 1e-9


def _tto_matvec(A, v):
    """A v for a dense vector v (C-order over the sites, as _dense), core by core without forming the matrix."""
    t = np.reshape(v, tuple(A.tto_dims) + (1,))         # (y_1 .. y_d, R_0)
    for G in A.tto_vec:                                 # G (x, y, R_l, R_r): contract y_k and R_l, append x_k, carry R_r last
        t = np.moveaxis(np.moveaxis(np.tensordot(G, t, axes=([1, 2], [0, t.ndim - 1])), 0, -1), 0, -1)
    return t.reshape(-1)


def _dmrg_walk(dims, start_rks, rmax):
    """(window sizes, max-rank history, final ranks) of one DMRG sweep plus the closing solve at rank rmax when every core move keeps
    min(rmax, n_i r_i, n_{i+1} r_{i+2}), i.e. no singular value falls below tol (the kernel's walk: windows 0..d-3, d-2..1, then 0)."""
    d = len(dims)
    r = list(start_rks)
    sizes, hist = [], []
    windows = list(range(d - 2)) + list(range(d - 2, 0, -1)) + [0]
    for t, i in enumerate(windows):
        na, nb = dims[i] * r[i], dims[i + 1] * r[i + 2]
        sizes.append(na * nb)
        if t == len(windows) - 1:
            hist.append(max(r))                         # the closing entry comes before its move
        r[i + 1] = min(rmax, na, nb)
        if t < len(windows) - 1:
            hist.append(max(r))
    return sizes, hist, r


def test_dense_near_limit(T):
    """d = 12 at rank 22 from a rank-16 start, random symmetric operator (its ground state keeps every rank the bounds allow): the backward
    half sweep meets a window of 2 * 22 * 2 * 22 = 1936 unknowns on the dense branch.  The window sizes follow from the rank history,
    which the test pins step by step.  Against the Lanczos branch (1e-9 ||S||) and the dense spectrum: not below its smallest eigenvalue,
    and above it by no more than the rank-22 truncation (the restatement: 1.7e-5 ||S||)."""
    d = 12
    dims = (2,) * d
    rng = np.random.default_rng(12)
    A = _sym_rand(dims, 3, rng)
    x0 = O.rand_tt(dims, 16, rng)
    sizes, hist, final = _dmrg_walk(dims, x0.ttv_rks, 22)
    assert max(sizes) == 1936
    kw = dict(tol=1e-12, sweep_schedule=[2], rmax_schedule=[22], itslv_thresh=2048)
    Eg, xg, rg = _solve(T, 1, A, x0, **kw)
    assert rg == hist and list(xg.ttv_rks) == final
    P = 2 ** d
    op = LinearOperator((P, P), matvec=lambda v: _tto_matvec(A, v), dtype=np.float64)
    w0 = float(eigsh(op, k=1, which="SA", tol=1e-14, v0=np.ones(P))[0][0])
    nrm = float(abs(eigsh(op, k=1, which="LM", tol=1e-8, v0=np.ones(P))[0][0]))
    El, _, _ = _solve(T, 1, A, x0, it_solver=True, linsolv_tol=1e-12, **kw)
    assert abs(El[-1] - Eg[-1]) <= 1e-9 * nrm
    assert w0 - 1e-10 * nrm <= Eg[-1] <= w0 + 1e-4 * nrm


@pytest.mark.parametrize("mode", [1, 0])
def test_lanczos_small_n(T, mode):
    """it_solver at d = 3 with rank 2: every local problem has fewer than 30 unknowns, so Lanczos stops at j + 1 == N with the exact
    projected problem."""
    A = _spd(3, 0.5)
    x0 = O.rand_tt((2,) * 3, 2, np.random.default_rng(3))
    E, _, _ = _solve(T, mode, A, x0, tol=1e-12, sweep_schedule=[2], rmax_schedule=[2], it_solver=True, linsolv_tol=1e-12)
    ev = np.linalg.eigvalsh(O.qtto_to_matrix(A))[0]
    assert abs(E[-1] - ev) <= 1e-12
    it, res = T.solvers.eigsolve_stats(1)
    assert res[0] <= 1e-14 and 0 < it[0] <= 8 * len(E)      # 0 at j + 1 == N, rounding where an invariant subspace came first


def test_lanczos_converged_start(T):
    """Started from an exact ground state (the Neel product state of the classical Ising chain, whose local blocks are basis vectors of
    the diagonal K), the first Lanczos vector is invariant: the breakdown exit at j = 0, one operator application per local solve, and
    E = -(d - 1) at every step.  MALS: the DMRG mode starts Lanczos from the swapped block after a left move, which is an eigenvector too
    but not the lowest one."""
    d = 6
    A = to_oracle(T.ising_tto(d, J=1.0, h=0.0))
    x0 = O.rand_tt((2,) * d, 1, np.random.default_rng(0))
    x0.ttv_vec = [np.eye(2)[:, k % 2].reshape(2, 1, 1).copy() for k in range(d)]
    E, _, _ = _solve(T, 0, A, x0, tol=1e-12, sweep_schedule=[2], rmax_schedule=[2], it_solver=True, linsolv_tol=1e-12)
    assert all(abs(e + (d - 1)) <= 1e-13 for e in E)
    it, res = T.solvers.eigsolve_stats(1)
    assert it[0] == len(E) and res[0] <= 1e-13


def test_lanczos_exhaustion(T):
    """linsolv_maxiter = 1 with linsolv_tol = 1e-15 on Ising d = 32 from a rank-16 start: TTN_ERR_NO_CONVERGENCE, and the same handles
    serve a normal call afterwards."""
    d = 32
    dA = T.DeviceTTO(to_product(to_oracle(T.ising_tto(d, J=1.0, h=1.5))))
    x0 = O.rand_tt((2,) * d, 16, np.random.default_rng(5))           # 1024 unknowns from the first windows on: 60 applications do not converge
    dx0 = T.DeviceTT.from_host(to_product(x0))
    cap = T.solvers.dmrg_capacity((2,) * d, x0.ttv_rks, 16)
    dx = T.DeviceTT((2,) * d, cap)
    with pytest.raises(T.TTNError, match="ttn error %d" % T._lib.TTN_ERR_NO_CONVERGENCE):
        T.solvers.dmrg_eigsolve_(dA, dx0, dx, 1e-12, [2], [16], True, 1, 1e-15)
    E, _ = T.solvers.dmrg_eigsolve_(dA, dx0, dx, 1e-12, [2], [16], True, 200, 1e-10)
    ex = ER.free_fermion_ground_energy(d, 1.0, 1.5)
    assert abs(E[0][-1] - ex) <= 1e-6 * abs(ex)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("it_solver", [False, True])
def test_ragged_batch_equals_single_calls(T, mode, it_solver):
    """Six trains with different start ranks and start vectors, mixed dims: each train of the batch is bitwise equal to its single call."""
    dims = (2, 3, 3, 2, 2, 3)
    rng = np.random.default_rng(90 + mode + 2 * it_solver)
    A = _sym_rand(dims, 4, rng)
    starts = [[1, 1, 1, 1, 1, 1, 1], [1, 2, 2, 2, 2, 2, 1], [1, 2, 3, 2, 3, 3, 1], [1, 2, 6, 4, 2, 3, 1], [1, 1, 2, 1, 2, 1, 1],
              [1, 2, 4, 6, 4, 3, 1]]
    x0s = [O.rand_tt(dims, rk, rng) for rk in starts]
    top = [max(rk[k] for rk in starts) for k in range(len(dims) + 1)]
    sched, rmaxs = [2, 3], [4, 6]
    dA = T.DeviceTTO(to_product(A))
    cap = T.solvers.dmrg_capacity(dims, top, max(rmaxs))
    B = len(x0s)
    dx0 = T.DeviceTT(dims, top, batch=B)
    for i in range(B):
        dx0.upload(i, to_product(x0s[i]))
    dx = T.DeviceTT(dims, cap, batch=B)
    fn = T.solvers.dmrg_eigsolve_ if mode == 1 else T.solvers.mals_eigsolve_
    Eb, Rb = fn(dA, dx0, dx, 1e-10, sched, rmaxs, it_solver, 200, 1e-12)
    for i in range(B):
        s0 = T.DeviceTT.from_host(to_product(x0s[i]))
        s = T.DeviceTT(dims, cap)
        Es, Rs = fn(dA, s0, s, 1e-10, sched, rmaxs, it_solver, 200, 1e-12)
        assert Es[0] == Eb[i] and Rs[0] == Rb[i], i
        a, b = dx.download(i), s.download(0)
        assert list(a.ttv_rks) == list(b.ttv_rks), i
        for ca, cb in zip(a.ttv_vec, b.ttv_vec):
            assert np.array_equal(np.asarray(ca), np.asarray(cb)), i
        s0.free(); s.free()


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("c", [1e-8, 1e8])
def test_scale_and_shift(T, mode, c):
    """E(c S + s I) = c E(S) + s to 1e-12 relative on the dense branch (full rank: both solves are exact)."""
    dims = (3, 2, 4, 2, 3)
    rng = np.random.default_rng(5 + mode)
    S = _sym_rand(dims, 4, rng)
    s = 2.0 * c
    As = O.tto_add(O.tto_scale(c, S), O.tto_scale(s, _id_tto(dims)))
    x0 = O.rand_tt(dims, 2, rng)
    kw = dict(tol=1e-13, sweep_schedule=[3], rmax_schedule=[_full_rank(dims)])
    E1, _, _ = _solve(T, mode, S, x0, **kw)
    E2, _, _ = _solve(T, mode, As, x0, **kw)
    want = c * E1[-1] + s
    assert abs(E2[-1] - want) <= 1e-12 * abs(want)
