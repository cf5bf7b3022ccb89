"""GPU checks of dmrg_eigsolve / mals_eigsolve (csrc/ttn_eigsolve_kernels.h): the reference's assertions (test/test_dmrg.jl:100-171,
test/test_mals.jl:79-160) through the device, parity with the NumPy restatement (tests/eig_reference.py) on the dense local branch,
oracle-free exact answers (the QTT Laplacian, the free-fermion transverse-field Ising chain at d = 32 on the matrix-free branch), Lanczos
against the dense branch, batch = single calls bitwise, and the refusals."""
import math

import numpy as np
import pytest

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
