"""The stepper family on the GPU: the fused update z = alpha x + beta (A y) (csrc/ttn_step_kernels.h, include/ttn_step.h) against the
four-launch composition it replaces — every bit —, the implicit steppers on the ALS / MALS / DMRG solvers against the NumPy restatement
(tests/stepper_reference.py), the reference's own known answers through the public host-level calls (test/test_euler.jl), and the public
increase_ranks (test/test_tt_tools.jl:949-967).

Bars.  Kernel: np.array_equal.  Steppers: tt_rel_diff <= 1e-9 per step for als (the per-solve bar of test_gpu_als.py), 1e-8 per step
for mals and dmrg (test_gpu_mals.py); s steps: s times that, because the step map LHS^-1 (I + (h/2) A) has norm within 1e-3 of 1 for the
test operator (||(h/2) A|| < 4e-4): per-step errors add and are not amplified.  Ranks equal the restatement's."""
import math

import numpy as np
import pytest

import ttn_amd as T
from oracle import tt_oracle as O
from tests import opalg_reference as OR
from tests import stepper_reference as R
from tests.helpers import to_oracle, to_product, tt_rel_diff, worst_of
from tests.test_gpu_opalg import CASES
from ttn_amd import device as D
from ttn_amd import solvers as S

pytestmark = pytest.mark.gpu

ONE_STEP = {"als": 1.0e-9, "mals": 1.0e-8, "dmrg": 1.0e-8}


def upload_batch(trains, cap=None):
    """Trains of common dims, possibly different ranks, into one handle (capacity: the per-bond maximum)."""
    dims = trains[0].ttv_dims
    if cap is None:
        cap = [max(t.ttv_rks[m] for t in trains) for m in range(len(dims) + 1)]
    h = T.DeviceTT(dims, cap, batch=len(trains))
    for b, t in enumerate(trains):
        h.upload(b, to_product(t))
    return h


def factors(a, B):
    return [1.0] * B if a is None else [float(v) for v in np.broadcast_to(np.asarray(a, dtype=float), (B,))]


def compose(alpha, x, beta, A, y):
    """ttn_apply -> ttn_scale_batch -> ttn_scale_batch -> ttn_add: what ttn_apply_axpby must reproduce in every bit."""
    B = x.batch
    tcap = [a * c for a, c in zip(A.rks, y.cap)]
    t, t2, x2 = T.DeviceTT(x.dims, tcap, B), T.DeviceTT(x.dims, tcap, B), T.DeviceTT(x.dims, x.cap, B)
    D.apply(A, y, t)
    D.scale_batch(factors(beta, B), t, t2)
    D.scale_batch(factors(alpha, B), x, x2)
    zcap = [1] + [p + q for p, q in zip(x.cap[1:-1], tcap[1:-1])] + [1]
    z = T.DeviceTT(x.dims, zcap, B)
    D.add(x2, t2, z)
    for h in (t, t2, x2):
        h.free()
    return z


def fused(alpha, x, beta, A, y):
    zcap = [1] + [p + a * q for p, a, q in zip(x.cap[1:-1], A.rks[1:-1], y.cap[1:-1])] + [1]
    return D.apply_axpby(alpha, x, beta, A, y, T.DeviceTT(x.dims, zcap, x.batch))


def assert_same_bits(got, ref):
    assert got.batch == ref.batch
    for b in range(got.batch):
        assert got.ranks(b) == ref.ranks(b), (b, got.ranks(b), ref.ranks(b))
        g, r = got.download(b), ref.download(b)
        for k, (cg, cr) in enumerate(zip(g.ttv_vec, r.ttv_vec)):
            assert cg.shape == cr.shape, (b, k, cg.shape, cr.shape)
            assert np.array_equal(cg, cr), (b, k, float(np.abs(cg - cr).max()))


def ragged(rks, b):
    """Ranks of train b of a batch: the interior ranks lowered by b (at least 1)."""
    return [1] + [max(1, r - b) for r in rks[1:-1]] + [1]


VARIANTS = [                                     # (alpha, beta) for a batch of 3
    (None, None),
    (None, 0.025),
    (-1.0, None),
    ([0.5, -2.0, 1.0 / 3.0], [3.0, 1.0, -0.125]),
    (0.0, 1.5),
    ([1.0, 0.0, 2.0], [0.0, 7.0, 0.0]),
]


# ---- 1. the kernel, bitwise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,ra,rb", CASES)
def test_apply_axpby_equals_the_composition_in_every_bit(dims, ra, rb):
    """The ragged shapes of the operator-algebra tests (n = 2, 3, 4, 5; an operator core beyond the LDS staging; more tiles than blocks),
    a batch of 3 with different ranks per train, x != y and x = y, every kind of factor."""
    rng = np.random.default_rng(21)
    big = max(ra) * max(rb) >= 1000                          # (a 2352 x 2352 middle core: one train, one pair of factors)
    B = 1 if big else 3
    dA = T.DeviceTTO(to_product(OR.rand_tto(dims, ra, rng)))
    y = upload_batch([OR.rand_ttv(dims, ragged(rb, b), rng) for b in range(B)])
    x = upload_batch([OR.rand_ttv(dims, ragged(rb[::-1], b), rng) for b in range(B)])
    for alpha, beta in ([(0.5, -2.0)] if big else VARIANTS):
        for xx in ((x,) if big else (x, y)):                 # x != y, then x = y (the steppers' case)
            got, ref = fused(alpha, xx, beta, dA, y), compose(alpha, xx, beta, dA, y)
            assert_same_bits(got, ref)
            got.free(); ref.free()
    for h in (dA, x, y):
        h.free()


def test_apply_axpby_scales_the_core_the_gauge_flags_name():
    """x from orthogonalize(x, 3, .): its first core with flag 0 is core 3, which is where alpha lands; per-train flags differ when one
    train of the batch was zeroed by scale_batch (flags all 0 -> core 1)."""
    rng = np.random.default_rng(22)
    dims, B = (2, 3, 2, 2, 2), 3
    dA = T.DeviceTTO(to_product(OR.rand_tto(dims, [1, 3, 2, 4, 2, 1], rng)))
    y = upload_batch([OR.rand_ttv(dims, [1, 2, 5, 4, 2, 1], rng) for _ in range(B)])
    x0 = upload_batch([OR.rand_ttv(dims, [1, 2, 6, 4, 2, 1], rng) for _ in range(B)])
    x = T.DeviceTT(dims, x0.cap, B)
    D.orthogonalize(x0, 3, x)
    assert x.ranks(0)[1].index(0) == 2
    for alpha, beta in VARIANTS[2:5]:
        got, ref = fused(alpha, x, beta, dA, y), compose(alpha, x, beta, dA, y)
        assert_same_bits(got, ref)
    xm = T.DeviceTT(dims, x0.cap, B)
    D.scale_batch([1.0, 0.0, 1.0], x, xm)                    # train 1: zeros, flags 0; trains 0 and 2 keep the flag on core 3
    assert [xm.ranks(b)[1].index(0) for b in range(B)] == [2, 0, 2]
    assert_same_bits(fused([2.0, 3.0, -4.0], xm, 0.5, dA, y), compose([2.0, 3.0, -4.0], xm, 0.5, dA, y))


def test_apply_axpby_one_site_is_refused_like_add():
    rng = np.random.default_rng(23)
    A = T.DeviceTTO(to_product(OR.rand_tto((3,), [1, 1], rng)))
    x = upload_batch([OR.rand_ttv((3,), [1, 1], rng)])
    z = T.DeviceTT((3,), [1, 1])
    with pytest.raises(T.TTNError, match="d >= 2"):
        D.add(x, x, T.DeviceTT((3,), [1, 1]))
    with pytest.raises(T.TTNError, match="d >= 2"):
        D.apply_axpby(1.0, x, 1.0, A, x, z)


def test_apply_axpby_refusals_leave_the_library_usable():
    rng = np.random.default_rng(24)
    dims = (2, 2, 3)
    A = T.DeviceTTO(to_product(OR.rand_tto(dims, [1, 2, 3, 1], rng)))
    x = upload_batch([OR.rand_ttv(dims, [1, 2, 2, 1], rng)])
    y = upload_batch([OR.rand_ttv(dims, [1, 2, 3, 1], rng)])
    ref = compose(-1.0, x, 0.5, A, y)

    def ok():
        got = fused(-1.0, x, 0.5, A, y)
        assert_same_bits(got, ref)
        got.free()

    with pytest.raises(T.TTNError, match="alias"):
        D.apply_axpby(1.0, x, 1.0, A, y, x)
    ok()
    with pytest.raises(T.TTNError, match="alias"):
        D.apply_axpby(1.0, x, 1.0, A, y, y)
    ok()
    with pytest.raises(T.TTNError, match="capacity too small"):
        D.apply_axpby(1.0, x, 1.0, A, y, T.DeviceTT(dims, [1, 5, 11, 1]))       # needs [1, 6, 11, 1]
    ok()
    with pytest.raises(T.TTNError, match="ttn_apply_axpby.*ComplexF64"):
        D.apply_axpby(1.0, x, 1.0, A, y, T.DeviceTT(dims, [1, 6, 11, 1], dtype=np.complex128))
    ok()
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        D.apply_axpby(1.0, x, 1.0, A, y, T.DeviceTT((2, 2, 2), [1, 6, 11, 1]))
    with pytest.raises(AssertionError, match="batch sizes differ"):
        D.apply_axpby(1.0, x, 1.0, A, y, T.DeviceTT(dims, [1, 6, 11, 1], batch=2))
    ok()


# ---- 2. the steppers against the restatement ---------------------------------------------------------------------------------------------
START = {(4, "als"): [1, 2, 4, 2, 1], (4, "mals"): [1, 2, 2, 2, 1], (4, "dmrg"): [1, 2, 2, 2, 1],
         (6, "als"): [1, 2, 4, 8, 4, 2, 1], (6, "mals"): [1, 2, 3, 3, 3, 2, 1], (6, "dmrg"): [1, 2, 3, 3, 3, 2, 1]}
CONFIGS = [                                      # d, steps, normalize, max_bond, solver keywords
    (4, 1, False, 0, {}),
    (4, 3, True, 4, {}),
    (6, 3, False, 0, {}),
    (6, 2, True, 4, {}),
]


def run_both(method, solver, d, nsteps, normalize, max_bond, kw, seed):
    rng = np.random.default_rng(seed)
    A = R.heat_operator(d)
    u0s = [O.rand_tt((2,) * d, START[(d, solver)], rng) for _ in range(3)]
    steps = [0.05] * nsteps
    du = upload_batch(u0s)
    f = S.crank_nicholson_method if method == "cn" else S.implicit_euler_method
    g = R.crank_nicholson_method if method == "cn" else R.implicit_euler_method
    sol = f(T.DeviceTTO(to_product(A)), du, du, steps, normalize=normalize, tt_solver=solver, max_bond=max_bond, **kw)
    worst = 0.0
    for b, u0 in enumerate(u0s):
        ref = g(A, u0, u0, steps, normalize=normalize, tt_solver=solver, max_bond=max_bond, **kw)
        got = to_oracle(sol.download(b))
        assert got.ttv_rks == ref.ttv_rks, (b, got.ttv_rks, ref.ttv_rks)
        worst = worst_of(worst, tt_rel_diff(got, ref))
    print(f"{method} {solver} d={d} steps={nsteps} normalize={normalize} max_bond={max_bond} {kw}: worst tt_rel_diff {worst:.2e}")
    assert worst <= nsteps * ONE_STEP[solver], worst
    sol.free(); du.free()


@pytest.mark.parametrize("d,nsteps,normalize,max_bond,kw", CONFIGS)
@pytest.mark.parametrize("solver", ["als", "mals", "dmrg"])
@pytest.mark.parametrize("method", ["ie", "cn"])
def test_implicit_steppers_match_the_restatement(method, solver, d, nsteps, normalize, max_bond, kw):
    run_both(method, solver, d, nsteps, normalize, max_bond, kw, seed=31)


@pytest.mark.parametrize("method", ["ie", "cn"])
def test_als_stepper_forwards_sweep_count(method):
    run_both(method, "als", 4, 2, False, 0, {"sweep_count": 4}, seed=32)
    run_both(method, "als", 4, 1, False, 0, {"sweep_count": 4, "it_solver": True, "r_itsolver": 10}, seed=33)     # accepted and ignored


def test_operator_handles_and_host_operators_give_the_same_steps():
    """A as a TToperator or as a DeviceTTO; two distinct step sizes in one call (the left-hand operator is built once per size)."""
    rng = np.random.default_rng(34)
    A = R.heat_operator(4)
    u0 = O.rand_tt((2,) * 4, START[(4, "als")], rng)
    steps = [0.05, 0.02, 0.05]
    ref = R.crank_nicholson_method(A, u0, u0, steps, normalize=False, tt_solver="als")
    for op in (to_product(A), T.DeviceTTO(to_product(A))):
        du = upload_batch([u0])
        sol = S.crank_nicholson_method(op, du, du, steps, normalize=False, tt_solver="als")
        assert tt_rel_diff(to_oracle(sol.download(0)), ref) <= 3 * ONE_STEP["als"]
    with pytest.raises(T.TTNError, match="N = 2"):
        S.implicit_euler_method(op, du, du, steps, tt_solver="dmrg", N=3)


# ---- 3. the reference's known answers through the public host-level calls ----------------------------------------------------------------
def test_host_level_known_answers():
    """test/test_euler.jl:34-58 (implicit Euler + dmrg), :87-110 (Crank-Nicolson + mals): dense solves, 1e-5."""
    A = R.heat_operator(4)
    Ap = to_product(A)
    u0 = T.rand_tt((2,) * 4, [1, 2, 2, 2, 1], seed=41)
    sol = T.implicit_euler_method(Ap, u0, u0, [0.05], normalize=False, tt_solver="dmrg")
    assert isinstance(sol, T.TTvector)
    err = R.rel(O.qtt_to_vector(to_oracle(sol)), R.dense_implicit_euler(A, to_oracle(u0), [0.05]))
    print(f"implicit Euler + dmrg vs dense: {err:.2e}")
    assert err < 1.0e-5
    sol = T.crank_nicholson_method(Ap, u0, u0, [0.05], normalize=False, tt_solver="mals")
    err = R.rel(O.qtt_to_vector(to_oracle(sol)), R.dense_crank_nicholson(A, to_oracle(u0), [0.05]))
    print(f"Crank-Nicolson + mals vs dense: {err:.2e}")
    assert err < 1.0e-5
    sol = T.euler_method(Ap, u0, [0.05], normalize=False)
    ud = O.qtt_to_vector(to_oracle(u0))
    assert R.rel(O.qtt_to_vector(to_oracle(sol)), ud + 0.05 * (R.dense(A) @ ud)) < 1.0e-6          # :5-31


def test_host_level_normalize_and_return_error():
    """:237-266: normalize = true gives norm 1 (1e-10) and a finite error for every method; the errors equal the restatement's (1e-8
    absolute); :300-313: RK4's return_error < 1e-10."""
    A = R.heat_operator(3)
    Ap = to_product(A)
    u0 = T.rand_tt((2,) * 3, [1, 2, 2, 1], seed=42)
    uo = to_oracle(u0)
    steps = [0.02]

    def check(sol, err, ref_err, what):
        assert isinstance(sol, T.TTvector) and isinstance(err, float) and math.isfinite(err)
        nrm = float(np.linalg.norm(O.qtt_to_vector(to_oracle(sol))))
        print(f"{what}: norm {nrm:.15f}, rel_error {err:.6e}" + ("" if ref_err is None else f", restatement {ref_err:.6e}"))
        assert abs(nrm - 1.0) < 1.0e-10
        if ref_err is not None:
            assert abs(err - ref_err) <= 1.0e-8

    sol, err = T.euler_method(Ap, u0, steps, normalize=True, return_error=True)
    check(sol, err, R.euler_method(A, uo, steps, normalize=True, return_error=True)[1], "euler")
    for solver in ("als", "mals", "dmrg"):
        sol, err = T.implicit_euler_method(Ap, u0, u0, steps, normalize=True, return_error=True, tt_solver=solver)
        check(sol, err, R.implicit_euler_method(A, uo, uo, steps, normalize=True, return_error=True, tt_solver=solver)[1], "ie " + solver)
        sol, err = T.crank_nicholson_method(Ap, u0, u0, steps, normalize=True, return_error=True, tt_solver=solver)
        check(sol, err, R.crank_nicholson_method(A, uo, uo, steps, normalize=True, return_error=True, tt_solver=solver)[1], "cn " + solver)
    sol, err = T.implicit_euler_method(Ap, u0, u0, steps, normalize=True, return_error=True, tt_solver="krylov", tol=1.0e-10)
    check(sol, err, None, "ie krylov")
    sol, err = T.crank_nicholson_method(Ap, u0, u0, steps, normalize=True, return_error=True, tt_solver="krylov", tol=1.0e-10)
    check(sol, err, None, "cn krylov")
    sol, err = T.rk4_method(Ap, u0, steps, 6, normalize=True, return_error=True)
    check(sol, err, R.rk4_method(A, uo, steps, 6, normalize=True, return_error=True)[1], "rk4")
    # :300-313
    A4, u4 = R.heat_operator(4), T.rand_tt((2,) * 4, [1, 2, 2, 2, 1], seed=43)
    sol, err = T.rk4_method(to_product(A4), u4, [0.05], 8, normalize=False, return_error=True)
    ref_err = R.rk4_method(A4, to_oracle(u4), [0.05], 8, normalize=False, return_error=True)[1]
    print(f"rk4 return_error {err:.3e} (restatement {ref_err:.3e})")
    assert err < 1.0e-10 and abs(err - ref_err) <= 1.0e-8


def test_return_error_on_a_batch_is_one_value_per_train():
    rng = np.random.default_rng(44)
    A = R.heat_operator(4)
    u0s = [O.rand_tt((2,) * 4, START[(4, "als")], rng) for _ in range(3)]
    du = upload_batch(u0s)
    sol, err = S.crank_nicholson_method(to_product(A), du, du, [0.05, 0.05], normalize=True, return_error=True, tt_solver="als")
    assert isinstance(err, np.ndarray) and err.dtype == np.float64 and err.shape == (3,)
    for b, u0 in enumerate(u0s):
        ref = R.crank_nicholson_method(A, u0, u0, [0.05, 0.05], normalize=True, return_error=True, tt_solver="als")[1]
        assert abs(err[b] - ref) <= 1.0e-8, (b, err[b], ref)


# ---- 4. DeviceTT.increase_ranks ----------------------------------------------------------------------------------------------------------
def test_device_increase_ranks_zero_noise():
    rng = np.random.default_rng(51)
    dims = (2, 3, 2, 2)
    trains = [O.rand_tt(dims, ragged([1, 2, 3, 2, 1], b), rng) for b in range(3)]
    x = upload_batch(trains)
    y = x.increase_ranks(5)
    want = T.r_and_d_to_rks([1, 5, 5, 5, 1], dims, rmax=5)
    for b, t in enumerate(trains):
        rks, ot = y.ranks(b)
        assert rks == want == [1, 2, 4, 2, 1] and ot == [0] * 4
        got = to_oracle(y.download(b))
        assert np.array_equal(R.dense_sequential(got), R.dense_sequential(t))
        for g, r in zip(got.ttv_vec, R.increase_ranks(t, 5).ttv_vec):
            assert np.array_equal(g, r)
    z = x.increase_ranks(7, rks=[1, 2, 3, 2, 1], cap_rks=[1, 4, 6, 4, 1])
    assert z.ranks(2)[0] == [1, 2, 3, 2, 1] and z.cap == [1, 4, 6, 4, 1]
    assert np.array_equal(R.dense_sequential(to_oracle(z.download(2))), R.dense_sequential(trains[2]))


def test_device_increase_ranks_with_noise():
    """test/test_tt_tools.jl:960-964 on [1, 1, 1, 1] -> [1, 2, 2, 1]: the named blocks are non-zero, the old block is kept bit for bit,
    and the new block is noise * Q with Q orthonormal, so ||new - old||_F = noise * sqrt(min(rows, columns) of Q): the number of new
    columns (cores 1 and 2) or new rows (core 3); 1e-10 relative slack for the rounding of the Householder QR."""
    rng = np.random.default_rng(52)
    noise = 1.0e-3
    trains = [O.rand_tt((2, 2, 2), [1, 1, 1, 1], rng) for _ in range(3)]
    x = upload_batch(trains)
    y = x.increase_ranks(2, noise=noise, seed=5)
    y2 = x.increase_ranks(2, noise=noise, seed=6)
    for b, t in enumerate(trains):
        rks, ot = y.ranks(b)
        assert rks == [1, 2, 2, 1] and ot == [0, 0, 0]
        c = y.download(b).ttv_vec
        assert np.any(c[0][:, :, 1] != 0) and np.any(c[1][:, 1, 1] != 0) and np.any(c[2][:, 1, :] != 0)
        pad = R.increase_ranks(t, 2).ttv_vec
        for k in range(3):
            assert np.array_equal(c[k][:, : t.ttv_vec[k].shape[1], : t.ttv_vec[k].shape[2]], t.ttv_vec[k])
            diff = float(np.linalg.norm(c[k] - pad[k]))
            print(f"train {b} core {k + 1}: ||new - old|| = {diff:.6e} (noise {noise:g})")
            assert 0.0 < diff <= noise * math.sqrt(1.0) * (1.0 + 1.0e-10)      # one new column (cores 1, 2) / one new row (core 3)
        assert not np.array_equal(c[1], y2.download(b).ttv_vec[1])              # another seed, another block
    # the noise does not depend on the train: the batch gives the trains of single calls
    assert np.array_equal(y.download(0).ttv_vec[0][:, :, 1], y.download(2).ttv_vec[0][:, :, 1])
    # the host function goes through the same kernel
    h = T.increase_ranks(to_product(trains[1]), 2, noise=noise, seed=5)
    assert h.ttv_rks == [1, 2, 2, 1] and h.ttv_ot == [0, 0, 0]
    for g, r in zip(h.ttv_vec, y.download(1).ttv_vec):
        assert np.array_equal(g, r)


def test_device_increase_ranks_refusals():
    rng = np.random.default_rng(53)
    dims = (2, 2, 2, 2)
    x = upload_batch([O.rand_tt(dims, [1, 2, 2, 2, 1], rng), O.rand_tt(dims, [1, 2, 3, 2, 1], rng)])
    L = T._lib.lib()

    def call(new, y, noise=0.0):
        T._lib.check(L.ttn_tt_increase_ranks(x.h, (T._lib.i64 * 5)(*new), noise, 0, y.h))

    y = T.DeviceTT(dims, [1, 2, 4, 2, 1], batch=2)
    with pytest.raises(AssertionError, match="New bond dimension too low"):
        x.increase_ranks(3)                                                     # train 1 already has rank 3
    with pytest.raises(T.TTNError, match="below a current rank"):
        call([1, 2, 2, 2, 1], y)                                                # ... below train 1's rank 3
    with pytest.raises(T.TTNError, match="above the destination's capacity"):
        call([1, 2, 4, 3, 1], y)
    with pytest.raises(T.TTNError, match="end ranks"):
        call([2, 2, 4, 2, 1], y)
    with pytest.raises(T.TTNError, match="alias"):
        T._lib.check(L.ttn_tt_increase_ranks(x.h, (T._lib.i64 * 5)(1, 2, 3, 2, 1), 0.0, 0, x.h))
    with pytest.raises(T.TTNError, match="ComplexF64"):
        call([1, 2, 4, 2, 1], T.DeviceTT(dims, [1, 2, 4, 2, 1], batch=2, dtype=np.complex128))
    call([1, 2, 4, 2, 1], y)                                                    # and the library is still usable
    assert y.ranks(1)[0] == [1, 2, 4, 2, 1]


# ---- 5. one example-shaped run -------------------------------------------------------------------------------------------------------------
def test_example_shaped_crank_nicholson_als_run():
    """As examples/Schrodinger_groundstate.jl and Ornstein.jl start: a QTT Gaussian enriched by increase_ranks(., 6; noise = 1e-3), then
    Crank-Nicolson steps on the ALS solver, which keeps the ranks it is given."""
    d = 8
    g = T.tt_compress_(T.function_to_qtt(lambda t: math.exp(-0.5 * (-5.0 + 10.0 * t) ** 2), d), 3)
    assert max(g.ttv_rks) <= 3
    u0 = T.increase_ranks(g, 6, noise=1.0e-3, seed=1)
    want = [1, 2, 4, 6, 6, 6, 4, 2, 1]
    assert u0.ttv_rks == want
    A = R.heat_operator(d)
    steps = [0.05] * 5
    sol = T.crank_nicholson_method(to_product(A), u0, u0, steps, normalize=False, tt_solver="als")
    assert sol.ttv_rks == want
    ref = R.crank_nicholson_method(A, to_oracle(u0), to_oracle(u0), steps, normalize=False, tt_solver="als")
    err = tt_rel_diff(to_oracle(sol), ref)
    print(f"example-shaped run, 5 steps: tt_rel_diff {err:.2e}")
    assert ref.ttv_rks == want and err <= 5 * ONE_STEP["als"]
