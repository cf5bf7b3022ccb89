"""Operator batches on the GPU (include/ttn_opbatch.h, csrc/ttn_opbatch_kernels.h): one TT operator per train.

The bar is BITWISE equality with the single-operator path: a kernel that takes a batch runs the same instructions on the same data, only
the operator's address moves by train * stride.  So for every consumer the batch call with ``DeviceTTO.stack([A_0 .. A_{B-1}])`` is
compared with B calls of the same function with ``DeviceTTO(A_b)`` on the SAME B-train handle (same launch geometry, same workspace
layout), keeping train b of run b: cores, ranks, gauge flags, scalars and histories must be ``np.array_equal``.  One case per consumer is
also held against the oracle with the bar the consumer's own test file uses.  Shapes: the smallest at which each piece can go wrong."""
import numpy as np
import pytest

import ttn_amd as T
from oracle import tt_oracle as O
from tests import eig_reference as ER
from tests.helpers import to_oracle, to_product, worst_of
from tests.test_cpu_expect import mixed_case
from ttn_amd import device as D
from ttn_amd import grad as G
from ttn_amd import solvers as S
from ttn_amd._lib import TTNError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    T.ensure_init(0)


def rand_op(dims, rks, rng):
    d = len(dims)
    return O.TToperator(d, [rng.standard_normal((dims[k], dims[k], rks[k], rks[k + 1])) for k in range(d)], tuple(dims), list(rks), [0] * d)


def upload_batch(trains, cap=None):
    dims = trains[0].ttv_dims
    if cap is None:
        cap = [max(t.ttv_rks[m] for t in trains) for m in range(len(dims) + 1)]
    h = T.DeviceTT(dims, cap, batch=len(trains))
    for b, t in enumerate(trains):
        h.upload(b, to_product(t))
    return h


def stack(ops):
    return T.DeviceTTO.stack([to_product(A) for A in ops])


def singles(ops):
    return [T.DeviceTTO(to_product(A)) for A in ops]


def train_bits(h, b):
    """Everything train b of a handle holds: (ranks, gauge flags, cores)."""
    rks, ot = h.ranks(b)
    return rks, ot, [np.asarray(c) for c in h.download(b).ttv_vec]


def assert_train_equal(got, ref, what):
    assert got[0] == ref[0], (what, "ranks", got[0], ref[0])
    assert got[1] == ref[1], (what, "gauge flags", got[1], ref[1])
    for k, (cg, cr) in enumerate(zip(got[2], ref[2])):
        assert np.array_equal(cg, cr), (what, "core", k, float(np.max(np.abs(cg - cr))))


def free(*hs):
    for h in hs:
        if h is not None:
            h.free()


def ragged(rng, d, rmax):
    return [1] + [int(rng.integers(1, rmax + 1)) for _ in range(d - 1)] + [1]


# the three mappings of k_apply: n = 2 with the core in LDS (rows x K columns), mixed dims (input fibres), operator core beyond the LDS
def apply_case(name):
    if name == "qtt_lds":
        rng = np.random.default_rng(501)
        dims, Ar, B = (2,) * 5, [1, 3, 2, 3, 2, 1], 5
        xs = [O.rand_tt(dims, ragged(rng, 5, 6), rng) for _ in range(B)]
        cap = [1, 6, 6, 6, 6, 1]
    elif name == "mixed":
        rng = np.random.default_rng(502)
        dims, Ar, B = (3, 2, 4), [1, 2, 3, 1], 3
        xs = [O.rand_tt(dims, r, rng) for r in ([1, 3, 2, 1], [1, 2, 4, 1], [1, 1, 3, 1])]
        cap = [1, 3, 4, 1]
    else:
        rng = np.random.default_rng(503)
        dims, Ar, B = (4, 4, 4), [1, 17, 17, 1], 2
        assert 16 * 17 * 17 > 4096                          # TTN_APPLY_LDS_DOUBLES: the operator is read through the caches
        xs = [O.rand_tt(dims, r, rng) for r in ([1, 3, 2, 1], [1, 2, 3, 1])]
        cap = [1, 3, 3, 1]
    ops = [rand_op(dims, Ar, rng) for _ in range(B)]
    return dims, Ar, ops, xs, cap


@pytest.mark.parametrize("name", ["qtt_lds", "mixed", "no_lds"])
def test_apply(name):
    dims, Ar, ops, xs, cap = apply_case(name)
    B = len(ops)
    hx = upload_batch(xs, cap)
    ycap = [a * c for a, c in zip(Ar, cap)]
    hA = stack(ops)
    assert hA.batch == B and hA.ranks() == Ar
    y = D.apply(hA, hx, T.DeviceTT(dims, ycap, B))
    got = [train_bits(y, b) for b in range(B)]
    y2 = T.DeviceTT(dims, ycap, B)
    for b, A1 in enumerate(singles(ops)):
        D.apply(A1, hx, y2)
        assert_train_equal(got[b], train_bits(y2, b), (name, b))
        A1.free()
    # the oracle, with the bar of test_gpu_parity.py (cores of A * x, 1e-12 of the largest entry), every train
    for b in range(B):
        ref = O.apply(ops[b], xs[b])
        assert got[b][0] == list(ref.ttv_rks)
        err = worst_of(*(np.max(np.abs(a - r)) for a, r in zip(got[b][2], ref.ttv_vec)))
        scale = max(np.max(np.abs(r)) for r in ref.ttv_vec)
        print(f"{name} train {b}: core error {err:.2e}, scale {scale:.2e}")
        assert err <= 1e-12 * scale
    free(hx, y, y2, hA)


@pytest.mark.parametrize("name", ["qtt_lds", "mixed"])
def test_apply_axpby(name):
    dims, Ar, ops, xs, cap = apply_case(name)
    B, d = len(ops), len(dims)
    rng = np.random.default_rng(7)
    alpha, beta = rng.standard_normal(B), rng.standard_normal(B)
    ys = [O.rand_tt(dims, x.ttv_rks[::-1] if name == "qtt_lds" else x.ttv_rks, rng) for x in xs]
    hx, hy = upload_batch(xs, cap), upload_batch(ys, cap)
    zcap = [1] + [c + a * c for a, c in zip(Ar[1:-1], cap[1:-1])] + [1]
    hA = stack(ops)
    for xx in (hx, hy):                                       # x != y, then x = y (the steppers' case)
        z = D.apply_axpby(alpha, xx, beta, hA, hy, T.DeviceTT(dims, zcap, B))
        got = [train_bits(z, b) for b in range(B)]
        z2 = T.DeviceTT(dims, zcap, B)
        for b, A1 in enumerate(singles(ops)):
            D.apply_axpby(alpha, xx, beta, A1, hy, z2)
            assert_train_equal(got[b], train_bits(z2, b), (name, b))
            A1.free()
        free(z, z2)
        # the oracle: alpha x + beta A y as a tensor, 1e-12 of its largest entry
        for b in range(B):
            x = xs[b] if xx is hx else ys[b]
            ref = alpha[b] * O.ttv_to_tensor(x) + beta[b] * O.ttv_to_tensor(O.apply(ops[b], ys[b]))
            t = O.ttv_to_tensor(O.TTvector(d, got[b][2], dims, got[b][0], got[b][1]))
            assert np.max(np.abs(t - ref)) <= 1e-12 * np.max(np.abs(ref))
    free(hx, hy, hA)


# ---- <x, A y>: both routes of k_expect ------------------------------------------------------------------------------------------------
def sandwich_case(route):
    if route == "qtt":
        rng = np.random.default_rng(601)
        dims, B = (2,) * 6, 3
        ops = [O.rand_tto(dims, 3, rng) for _ in range(B)]
        assert max(ops[0].tto_rks) == 3 and all(A.tto_rks == ops[0].tto_rks for A in ops)
        xs = [O.rand_tt(dims, 5, rng) for _ in range(B)]
        ys = [O.rand_tt(dims, 13, rng) for _ in range(B)]
    else:
        x, A, y = mixed_case()
        rng = np.random.default_rng(602)
        dims, B = x.ttv_dims, 3
        ops = [A] + [rand_op(dims, A.tto_rks, rng) for _ in range(B - 1)]
        xs = [x] + [O.rand_tt(dims, x.ttv_rks, rng) for _ in range(B - 1)]
        ys = [y] + [O.rand_tt(dims, y.ttv_rks, rng) for _ in range(B - 1)]
    return ops, xs, ys


@pytest.mark.parametrize("route", ["qtt", "general"])
def test_sandwich_expect_rayleigh(route):
    ops, xs, ys = sandwich_case(route)
    B = len(ops)
    hx, hy, hA = upload_batch(xs), upload_batch(ys), stack(ops)
    got = D.sandwich(hx, hA, hy)
    got_dev = D.sandwich_dev(hx, hA, hy)
    D.sync()
    assert np.array_equal(got_dev.cpu().numpy(), got)
    ex, ray = D.expect(hA, hy), D.rayleigh(hA, hy)
    for b, A1 in enumerate(singles(ops)):
        assert D.sandwich(hx, A1, hy)[b] == got[b]
        assert D.expect(A1, hy)[b] == ex[b] and D.rayleigh(A1, hy)[b] == ray[b]
        A1.free()
    # the oracle, bar of test_gpu_expect.py
    for b in range(B):
        Ay = O.apply(ops[b], ys[b])
        ref, scale = O.dot(xs[b], Ay), O.norm(xs[b]) * O.norm(Ay)
        print(f"{route} train {b}: got {got[b]:.17e} ref {ref:.17e} err/scale {abs(got[b] - ref) / scale:.2e}")
        assert abs(got[b] - ref) <= 1e-12 * scale
    free(hx, hy, hA)


@pytest.mark.parametrize("route", ["qtt", "general"])
def test_sandwich_swapped_operators_give_swapped_numbers(route):
    """Trains 0 and 2 are the same train; the operators at 0 and 2 trade places: a kernel that read operator 0 everywhere would not notice."""
    ops, xs, ys = sandwich_case(route)
    xs[2], ys[2] = xs[0], ys[0]
    hx, hy = upload_batch(xs), upload_batch(ys)
    hA, hS = stack(ops), stack([ops[2], ops[1], ops[0]])
    a, s = D.sandwich(hx, hA, hy), D.sandwich(hx, hS, hy)
    assert a[0] != a[2]
    assert s[0] == a[2] and s[2] == a[0] and s[1] == a[1]
    free(hx, hy, hA, hS)


@pytest.mark.parametrize("route", ["qtt", "general"])
def test_sandwich_pullback(route):
    ops, xs, ys = sandwich_case(route)
    B, d = len(ops), xs[0].N
    delta = np.array([0.5, -2.0, 1.25])
    hx, hy, hA = upload_batch(xs), upload_batch(ys), stack(ops)
    val, xb, yb = G.sandwich_pullback(hx, hA, hy, delta=delta)
    gx, gy = [train_bits(xb, b) for b in range(B)], [train_bits(yb, b) for b in range(B)]
    ev, eg = G.expect_value_and_grad(hA, hy)
    rv, rg = G.rayleigh_value_and_grad(hA, hy, fused=True)
    ge, gr = [train_bits(eg, b) for b in range(B)], [train_bits(rg, b) for b in range(B)]
    # the oracle: the value with the bar of test_gpu_expect.py, the gradients through Euler's identity sum_k <xbar_k, x_k> = N delta value
    # with the bar of test_gpu_expect_grad.py
    sx, sy = G.cores_dot(xb, hx), G.cores_dot(yb, hy)
    for b in range(B):
        Ay = O.apply(ops[b], ys[b])
        ref, scale = O.dot(xs[b], Ay), O.norm(xs[b]) * O.norm(Ay)
        assert abs(val[b] - ref) <= 1e-12 * scale
        assert abs(sx[b] - d * delta[b] * ref) <= d * 1e-12 * abs(delta[b]) * scale
        assert abs(sy[b] - d * delta[b] * ref) <= d * 1e-12 * abs(delta[b]) * scale
    for b, A1 in enumerate(singles(ops)):
        v1, x1, y1 = G.sandwich_pullback(hx, A1, hy, delta=delta)
        assert v1[b] == val[b]
        assert_train_equal(gx[b], train_bits(x1, b), (route, "xbar", b))
        assert_train_equal(gy[b], train_bits(y1, b), (route, "ybar", b))
        e1, g1 = G.expect_value_and_grad(A1, hy)
        assert e1[b] == ev[b]
        assert_train_equal(ge[b], train_bits(g1, b), (route, "expect grad", b))
        r1, h1 = G.rayleigh_value_and_grad(A1, hy, fused=True)
        assert r1[b] == rv[b]
        assert_train_equal(gr[b], train_bits(h1, b), (route, "rayleigh grad", b))
        free(x1, y1, g1, h1, A1)
    free(hx, hy, hA, xb, yb, eg, rg)


# ---- the two-site eigensolvers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 0])
def test_two_site_eigensolvers(mode):
    d, hs = 6, [0.5, 1.0, 1.5, 2.5]
    B = len(hs)
    dims = (2,) * d
    ops = [to_oracle(T.ising_tto(d, J=1.0, h=h)) for h in hs]
    x0s = [to_oracle(T.rand_tt(dims, 2, seed=10 + b)) for b in range(B)]
    sched, rmaxs, tol = (2,), (4,), 1e-10
    cap = S.dmrg_capacity(dims, x0s[0].ttv_rks, max(rmaxs))
    fn = S.dmrg_eigsolve_ if mode == 1 else S.mals_eigsolve_
    hx0, hA = upload_batch(x0s), stack(ops)
    x = T.DeviceTT(dims, cap, B)
    E, R = fn(hA, hx0, x, tol, sched, rmaxs)
    got = [train_bits(x, b) for b in range(B)]
    x2 = T.DeviceTT(dims, cap, B)
    for b, A1 in enumerate(singles(ops)):
        E1, R1 = fn(A1, hx0, x2, tol, sched, rmaxs)
        assert np.array_equal(np.array(E1[b]), np.array(E[b])) and R1[b] == R[b], (b, E1[b], E[b])
        assert_train_equal(got[b], train_bits(x2, b), (mode, b))
        A1.free()
    final = [E[b][-1] for b in range(B)]
    assert len(set(final)) == B and all(final[b] > final[b + 1] for b in range(B - 1)), final      # a stronger field lowers the ground energy
    # the restatement of the reference, bar of test_gpu_eigsolve.py
    for b in range(B):
        Er, xr, rr = ER.two_site_eigsolve(mode, ops[b], x0s[b], tol=tol, sweep_schedule=list(sched), rmax_schedule=list(rmaxs))
        assert R[b] == rr and got[b][0] == list(xr.ttv_rks) and got[b][1] == list(xr.ttv_ot)
        scale = max(1.0, max(abs(v) for v in Er))
        assert np.max(np.abs(np.array(E[b]) - np.array(Er))) <= 1e-10 * scale
    free(hx0, hA, x, x2)


# ---- the explicit steppers: only apply, apply_axpby, add, scale and tt_compress_ --------------------------------------------------------
@pytest.mark.parametrize("stepper", ["rk4", "euler"])
def test_explicit_steppers(stepper):
    d, cs = 4, [1.0, -0.5, 2.0]
    B = len(cs)
    dims = (2,) * d
    ops = [O.tto_scale(c, O.Delta(d)) for c in cs]
    assert all(A.tto_rks == ops[0].tto_rks for A in ops)
    u0s = [to_oracle(T.rand_tt(dims, 2, seed=30 + b)) for b in range(B)]
    steps = [0.01, 0.02]

    def run(A):
        if stepper == "rk4":
            return S.rk4_method(A, hu, steps, max_bond=4)
        return S.euler_method(A, hu, steps)
    hu, hA = upload_batch(u0s), stack(ops)
    u = run(hA)
    got = [train_bits(u, b) for b in range(B)]
    for b, A1 in enumerate(singles(ops)):
        u1 = run(A1)
        assert_train_equal(got[b], train_bits(u1, b), (stepper, b))
        free(u1, A1)
    assert not np.array_equal(got[0][2][0], got[1][2][0])
    free(hu, hA, u)


# ---- construction ---------------------------------------------------------------------------------------------------------------------------
def assert_ops_equal(a, b):
    assert list(a.tto_rks) == list(b.tto_rks) and tuple(a.tto_dims) == tuple(b.tto_dims)
    for ca, cb in zip(a.tto_vec, b.tto_vec):
        assert np.array_equal(np.asarray(ca), np.asarray(cb))


def test_stack_download_select():
    rng = np.random.default_rng(701)
    dims, Ar, B = (3, 2, 3), [1, 3, 2, 1], 4                  # cores of 27 (odd), 24 and 18 doubles
    ops = [to_product(rand_op(dims, Ar, rng)) for _ in range(B)]
    hA = T.DeviceTTO.stack(ops)
    assert hA.batch == B and hA.ranks() == Ar and hA.dims == dims
    for b in range(B):
        assert_ops_equal(hA.download(b), ops[b])
        s = hA.select(b)
        assert s.batch == 1
        assert_ops_equal(s.download(), ops[b])
        s.free()
    one = T.DeviceTTO.stack(ops[:1])                           # a batch of one is an ordinary operator
    assert one.batch == 1
    assert_ops_equal(one.mul(one).download(), T.DeviceTTO(ops[0]).mul(T.DeviceTTO(ops[0])).download())
    with pytest.raises(TTNError):
        hA.select(B)
    free(hA, one)


@pytest.mark.parametrize("cap", [None, [1, 5, 4, 1]])
def test_from_tt_batch_packs_capacity_strided_slots(cap):
    rng = np.random.default_rng(702)
    dims, Ar, B = (3, 2, 3), [1, 3, 2, 1], 3
    A = to_product(rand_op(dims, Ar, rng))
    hA = T.DeviceTTO(A)
    t = hA.to_tt(B, cap_rks=cap)
    hB = T.DeviceTTO.from_tt_batch(t)
    assert hB.batch == B and hB.ranks() == Ar and hB.dims == dims
    for b in range(B):
        assert_ops_equal(hB.download(b), A)
    free(hA, t, hB)


def test_from_tt_batch_refuses_unequal_ranks():
    rng = np.random.default_rng(703)
    dims = (4, 4, 4)
    h = upload_batch([O.rand_tt(dims, [1, 2, 3, 1], rng), O.rand_tt(dims, [1, 2, 2, 1], rng)])
    with pytest.raises(TTNError, match="ranks of train 1 .* bond 2"):
        T.DeviceTTO.from_tt_batch(h)
    h.free()


def test_lincomb():
    rng = np.random.default_rng(704)
    d, B = 4, 4
    dims = (2,) * d
    T0, T1 = T.DeviceTTO(T.Delta(d)), T.DeviceTTO(to_product(rand_op(dims, [1, 2, 2, 2, 1], rng)))
    c = rng.standard_normal((B, 2))
    c[1, 0] = 0.0                                             # scale_batch writes a zero train for a zero factor
    H = T.DeviceTTO.lincomb([T0, T1], c)
    assert H.batch == B
    assert H.ranks() == [1] + [a + b for a, b in zip(T0.rks[1:-1], T1.rks[1:-1])] + [1]
    D0, D1 = T0.to_dense().cpu().numpy(), T1.to_dense().cpu().numpy()
    eps = np.finfo(np.float64).eps
    for b in range(B):
        s = H.select(b)
        got = s.to_dense().cpu().numpy()
        ref = c[b, 0] * D0 + c[b, 1] * D1
        bound = 64 * eps * (abs(c[b, 0]) * np.max(np.abs(D0)) + abs(c[b, 1]) * np.max(np.abs(D1)))
        print(f"lincomb {b}: error {np.max(np.abs(got - ref)):.2e}, bound {bound:.2e}")
        assert np.max(np.abs(got - ref)) <= bound
        s.free()
    free(T0, T1, H)


# ---- everything else refuses ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refusal_handles(_init):
    rng = np.random.default_rng(801)
    d, B = 4, 3
    dims = (2,) * d
    Ar = [1, 2, 2, 2, 1]
    ops = [to_product(rand_op(dims, Ar, rng)) for _ in range(B)]
    h = {"Ab": T.DeviceTTO.stack(ops), "A1": T.DeviceTTO(ops[0]),
         "x": upload_batch([O.rand_tt(dims, 2, rng) for _ in range(B)]),
         "x2": upload_batch([O.rand_tt(dims, 2, rng) for _ in range(2)]),
         "out": T.DeviceTT(dims, [1, 4, 8, 4, 1], B), "dims": dims, "B": B}
    yield h
    free(h["Ab"], h["A1"], h["x"], h["x2"], h["out"])


REFUSALS = {
    "apply_compress": lambda h: D.apply_compress(h["Ab"], h["x"], h["out"], 4),
    "mul": lambda h: h["Ab"].mul(h["A1"]),
    "mul_right": lambda h: h["A1"].mul(h["Ab"]),
    "add": lambda h: h["Ab"].add(h["A1"]),
    "scale": lambda h: h["Ab"].scale(2.0),
    "kron": lambda h: h["A1"].kron(h["Ab"]),
    "inner": lambda h: h["Ab"].inner(h["A1"]),
    "to_tt": lambda h: h["Ab"].to_tt(h["B"]),
    "compress": lambda h: h["Ab"].compress(2),
    "to_dense": lambda h: h["Ab"].to_dense(),
    "als_linsolve_": lambda h: S.als_linsolve_(h["Ab"], h["x"], h["x"], h["out"]),
    "mals_linsolve_": lambda h: S.mals_linsolve_(h["Ab"], h["x"], h["x"], h["out"]),
    "dmrg_linsolve_": lambda h: S.dmrg_linsolve_(h["Ab"], h["x"], h["x"], h["out"]),
    "krylov_linsolve": lambda h: S.krylov_linsolve(h["Ab"], h["x"], h["x"]),
    "implicit_euler_method": lambda h: S.implicit_euler_method(h["Ab"], h["x"], h["x"], [0.1]),
    "als_eigsolve_": lambda h: S.als_eigsolve_(h["Ab"], h["x"], h["out"]),
    "als_gen_eigsolv_A": lambda h: S.als_gen_eigsolv_(h["Ab"], h["A1"], h["x"], h["out"]),
    "als_gen_eigsolv_S": lambda h: S.als_gen_eigsolv_(h["A1"], h["Ab"], h["x"], h["out"]),
    "apply_pullback": lambda h: G.apply_pullback(h["Ab"], h["x"], h["out"]),
    "rayleigh_value_and_grad_unfused": lambda h: G.rayleigh_value_and_grad(h["Ab"], h["x"], fused=False),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(refusal_handles, name):
    with pytest.raises(TTNError, match="operator batch"):
        REFUSALS[name](refusal_handles)


BATCH_MISMATCH = {
    "apply": lambda h: D.apply(h["Ab"], h["x2"], T.DeviceTT(h["dims"], [1, 4, 4, 4, 1], 2)),
    "apply_axpby": lambda h: D.apply_axpby(None, h["x2"], None, h["Ab"], h["x2"], T.DeviceTT(h["dims"], [1, 6, 6, 6, 1], 2)),
    "sandwich": lambda h: D.sandwich(h["x2"], h["Ab"], h["x2"]),
    "sandwich_pullback": lambda h: G.sandwich_pullback(h["x2"], h["Ab"], h["x2"]),
    "dmrg_eigsolve_": lambda h: S.dmrg_eigsolve_(h["Ab"], h["x2"], T.DeviceTT(h["dims"], [1, 2, 4, 2, 1], 2)),
    "mals_eigsolve_": lambda h: S.mals_eigsolve_(h["Ab"], h["x2"], T.DeviceTT(h["dims"], [1, 2, 4, 2, 1], 2)),
}


@pytest.mark.parametrize("name", sorted(BATCH_MISMATCH))
def test_batch_mismatch(refusal_handles, name):
    """Operator batch 3, trains 2: TTN_ERR_DIMS, which the binding raises as the reference's assertion."""
    with pytest.raises(AssertionError, match="batch sizes differ"):
        BATCH_MISMATCH[name](refusal_handles)


def test_stack_refuses_complex_and_unequal_operators():
    rng = np.random.default_rng(802)
    dims = (2, 2, 2)
    A = to_product(rand_op(dims, [1, 2, 2, 1], rng))
    Z = T.TToperator(A.N, [np.asfortranarray(c.astype(np.complex128)) for c in A.tto_vec], A.tto_dims, A.tto_rks, A.tto_ot)
    with pytest.raises(TTNError, match="operator batch is Float64 only"):
        T.DeviceTTO.stack([A, Z])
    with pytest.raises(TTNError, match="ranks"):
        T.DeviceTTO.stack([A, to_product(rand_op(dims, [1, 2, 3, 1], rng))])
    with pytest.raises(TTNError, match="dims"):
        T.DeviceTTO.stack([A, to_product(rand_op((2, 3, 2), [1, 2, 2, 1], rng))])
    with pytest.raises(TTNError):
        T.DeviceTTO.stack([])
