"""GPU parity tests: the HIP path (through the C ABI of include/ttn.h) against the CPU oracle and
the committed golden fixtures.  Tolerances (fp64):
  layout / ranks / ot flags / rank decisions ........ bit-exact
  apply, hadamard, +, scalar* ....................... bit-exact for {0,±1,2}-valued operators and pure
                                                      copies/products; rtol 4 ulp for general operators
  dot / norm ........................................ rtol 1e-12
  orthogonalize ..................................... reconstruction 1e-12 rel, ||QᵀQ − I||_max 1e-12
  tt_compress! ...................................... singular values rtol 1e-10 (atol 1e-13·σ₁),
                                                      ||y_gpu − y_cpu|| / ||y_cpu|| ≤ 1e-9
"""
import math

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests.helpers import (load_golden, sign_fix_compare, to_oracle, to_product, tt_from_golden, tt_rel_diff,
                           tto_from_golden, worst_of)

pytestmark = pytest.mark.gpu

ULP4 = 4 * np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _cores_equal(a, b, rtol=0.0):
    assert list(a.ttv_rks) == list(b.ttv_rks)
    assert list(a.ttv_ot) == list(b.ttv_ot)
    for ca, cb in zip(a.ttv_vec, b.ttv_vec):
        ca, cb = np.asarray(ca), np.asarray(cb)
        assert ca.shape == cb.shape
        if rtol == 0.0:
            assert np.array_equal(ca, cb)
        else:
            assert np.allclose(ca, cb, rtol=rtol, atol=rtol * np.max(np.abs(cb)))


# ------------------------------------------------------------------------------------------------
# golden fixtures
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list("abce"))
def test_golden_random_small(T, name):
    g = load_golden("random_small.npz")
    x, y, A = tt_from_golden(g, f"{name}_x"), tt_from_golden(g, f"{name}_y"), tto_from_golden(g, f"{name}_A")
    px, py, pA = to_product(x), to_product(y), to_product(A)
    _cores_equal(T.apply(pA, px), tt_from_golden(g, f"{name}_apply"), rtol=ULP4)
    _cores_equal(T.hadamard(px, py), tt_from_golden(g, f"{name}_hadamard"))
    _cores_equal(T.add(px, py), tt_from_golden(g, f"{name}_add"))
    _cores_equal(T.scale(-2.5, px), tt_from_golden(g, f"{name}_scale"))
    assert math.isclose(T.dot(px, py), float(g[f"{name}_dot"]), rel_tol=1e-12)
    assert math.isclose(T.norm(px), float(g[f"{name}_norm_x"]), rel_tol=1e-12)
    dense = g[f"{name}_x_dense"]
    for c in range(1, x.N + 1):
        o = T.orthogonalize(px, i=c)
        assert o.ttv_rks == list(g[f"{name}_orth{c}_rks"]) and o.ttv_ot == list(g[f"{name}_orth{c}_ot"])
        assert np.allclose(O.ttv_to_tensor(to_oracle(o)), dense, atol=1e-12 * np.max(np.abs(dense)))
    # apply + round with per-bond singular values
    mb, te = int(g[f"{name}_max_bond"]), float(g[f"{name}_truncerr"])
    dA = T.DeviceTTO(pA)
    dx = T.DeviceTT.from_host(px)
    dy = T.DeviceTT(px.ttv_dims, [a * b for a, b in zip(pA.tto_rks, px.ttv_rks)])
    dy.capture_singular_values(True)
    T.device.apply_compress(dA, dx, dy, mb, te, 1)
    T.device.compress_status(dy)
    z = dy.download()
    assert z.ttv_rks == list(g[f"{name}_compress_rks"])
    ref = g[f"{name}_compress_dense"]
    assert np.allclose(O.ttv_to_tensor(to_oracle(z)), ref, atol=1e-10 * np.max(np.abs(ref)))
    for i in range(int(g[f"{name}_compress_nsv"])):
        sv_ref = g[f"{name}_compress_sv{i}"]
        sv = dy.singular_values(0, i)
        assert len(sv) >= len(sv_ref)
        assert np.allclose(sv[: len(sv_ref)], sv_ref, rtol=1e-10, atol=1e-13 * sv_ref[0])


def test_golden_config1(T):
    """BASELINE.json config 1: tt_compress!(id_tto(6) * qtt_sin(6, λ=π), 2) — README.md:84-103 inputs."""
    g = load_golden("closed_forms.npz")
    y = T.id_tto(6) * T.qtt_sin(6, lam=math.pi)
    _cores_equal(y, tt_from_golden(g, "c1_applied"))
    r = T.tt_compress_(y, 2)
    assert r is y and y.ttv_rks == [1, 2, 2, 2, 2, 2, 1]
    assert np.allclose(T.qtt_to_vector(y), g["c1_dense"], atol=1e-12)
    assert np.allclose(T.qtt_to_vector(y), np.sin(math.pi ** 2 * np.linspace(0, 1, 64)), atol=1e-12)
    for k, c in enumerate(y.ttv_vec):
        assert c.shape == (2, y.ttv_rks[k], y.ttv_rks[k + 1])


# ------------------------------------------------------------------------------------------------
# apply
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,r", [(4, 3), (12, 16), (20, 32)])
def test_apply_laplacian_bit_exact(T, d, r):
    x = T.rand_tt((2,) * d, r, seed=d)
    got = T.Delta(d) * x
    ref = O.apply(O.Delta(d), to_oracle(x))
    _cores_equal(got, ref)                 # entries of Δ are in {0,±1,2}: products exact, one rounding per sum
    assert got.ttv_rks == [a * b for a, b in zip(T.Delta(d).tto_rks, x.ttv_rks)] and got.ttv_ot == [0] * d


def test_apply_general_dims_and_callable(T):
    rng = np.random.default_rng(21)
    dims = (2, 3, 4, 3)
    A = O.rand_tto(dims, 3, rng)
    v = O.rand_tt(dims, [1, 2, 4, 3, 1], rng)
    pA, pv = to_product(A), to_product(v)
    ref = O.apply(A, v)
    _cores_equal(pA * pv, ref, rtol=ULP4)
    _cores_equal(pA(pv), ref, rtol=ULP4)   # test/test_tt_operations.jl:116-122
    TA = O.tto_to_tensor(A)
    dense = np.einsum("abcdefgh,efgh->abcd", TA, O.ttv_to_tensor(v))
    assert np.allclose(O.ttv_to_tensor(to_oracle(pA * pv)), dense, atol=1e-12)


def test_apply_full_size_linearity(T):
    """C3-sized property test: A(x + 2y) == A x + 2 A y as tensors (TT inner products)."""
    d = 30
    x = T.rand_tt((2,) * d, 16, seed=1)
    y = T.rand_tt((2,) * d, 16, seed=2)
    A = T.Delta(d)
    lhs = A * (x + 2.0 * y)
    rhs = (A * x) + 2.0 * (A * y)
    assert T.euclidean_distance(lhs, rhs) <= 1e-12 * T.norm(rhs)


# ------------------------------------------------------------------------------------------------
# dot / norm / hadamard / + / scalar
# ------------------------------------------------------------------------------------------------
def test_dot_norm_closed_forms(T):
    d = 8                                   # test/test_tt_operations.jl:303-320
    A1, A2 = T.qtt_exp(d), T.qtt_sin(d, lam=math.pi)
    S1, S2 = T.qtt_to_vector(A1), T.qtt_to_vector(A2)
    assert T.euclidean_distance(A1, A1) == 0.0
    assert math.isclose(T.dot(A1, A2), float(S1 @ S2), rel_tol=1e-10)
    assert math.isclose(T.norm(A2), float(np.linalg.norm(S2)), rel_tol=1e-10)
    assert abs(math.sqrt(S1 @ S1 - 2 * (S1 @ S2) + S2 @ S2) - T.euclidean_distance(A1, A2)) < 1e-10


@pytest.mark.parametrize("d,ra,rb", [(20, 32, 96), (30, 64, 192)])
def test_dot_full_size_vs_oracle(T, d, ra, rb):
    a = T.rand_tt((2,) * d, ra, seed=5)
    b = T.rand_tt((2,) * d, rb, seed=6)
    ref = O.dot(to_oracle(a), to_oracle(b))
    assert math.isclose(T.dot(a, b), ref, rel_tol=1e-12, abs_tol=1e-12 * O.norm(to_oracle(a)) * O.norm(to_oracle(b)))
    assert math.isclose(T.norm(a), O.norm(to_oracle(a)), rel_tol=1e-12)


@pytest.mark.parametrize("d,ra,rb,seed", [(9, 5, 13, 0), (12, 37, 64, 1), (14, 64, 21, 2), (30, 64, 64, 3), (7, 16, 17, 4), (2, 2, 2, 5)])
def test_dot_lds_resident_path_odd_ranks(T, d, ra, rb, seed):
    """The LDS-resident form of k_dot (n = 2, every rank <= 64; csrc/ttn_dot_kernels.h) on ranks that are NOT multiples of the 16 x 16
    MFMA tile and differ between the two trains — masked fragments, partially filled tile grids, rank ramps at both ends — against
    the oracle (src/tt_operations.jl:239-250) to 1e-12, plus a batch whose trains carry different ranks."""
    rng = np.random.default_rng(100 + seed)
    a = to_product(O.rand_tt((2,) * d, ra, rng))
    b = to_product(O.rand_tt((2,) * d, rb, rng))
    ref = O.dot(to_oracle(a), to_oracle(b))
    scale = O.norm(to_oracle(a)) * O.norm(to_oracle(b))
    assert abs(T.dot(a, b) - ref) <= 1e-12 * scale
    assert abs(T.dot(b, a) - ref) <= 1e-12 * scale
    # ragged batch: train 1 has smaller ranks than the handle's capacity
    a2 = to_product(O.rand_tt((2,) * d, max(1, ra // 2), rng))
    b2 = to_product(O.rand_tt((2,) * d, max(1, rb // 3), rng))
    da, db = T.DeviceTT(a.ttv_dims, a.ttv_rks, batch=2), T.DeviceTT(b.ttv_dims, b.ttv_rks, batch=2)
    da.upload(0, a); da.upload(1, a2); db.upload(0, b); db.upload(1, b2)
    got = T.device.dot(da, db)
    assert abs(got[0] - ref) <= 1e-12 * scale
    ref2 = O.dot(to_oracle(a2), to_oracle(b2))
    assert abs(got[1] - ref2) <= 1e-12 * O.norm(to_oracle(a2)) * O.norm(to_oracle(b2))


def test_hadamard_closed_forms(T):
    d = 8                                   # test/test_tt_operations.jl:41-71
    x = np.linspace(0, 1, 2 ** d)
    A1, A2, A3 = T.qtt_exp(d), T.qtt_sin(d, lam=math.pi), T.qtt_cos(d, lam=math.pi)
    assert np.allclose(T.qtt_to_vector(T.hadamard(A2, A3)), np.cos(math.pi ** 2 * x) * np.sin(math.pi ** 2 * x), atol=1e-12, rtol=0)
    assert np.allclose(T.qtt_to_vector(T.hadamard(A1, A2)), np.exp(x) * np.sin(math.pi ** 2 * x), atol=1e-12, rtol=0)
    big = T.hadamard(T.rand_tt((2,) * 10, 8, seed=1), T.rand_tt((2,) * 10, 12, seed=2))
    ref = O.hadamard(to_oracle(T.rand_tt((2,) * 10, 8, seed=1)), to_oracle(T.rand_tt((2,) * 10, 12, seed=2)))
    _cores_equal(big, ref)


def test_add_and_inplace_add(T):
    rng = np.random.default_rng(1)          # test/test_tt_operations.jl:106-114
    x = to_product(O.rand_tt((2, 3), [1, 2, 1], rng))
    y = to_product(O.rand_tt((2, 3), [1, 3, 1], rng))
    expected = O.ttv_to_tensor(to_oracle(x + y))
    assert np.allclose(expected, O.ttv_to_tensor(to_oracle(x)) + O.ttv_to_tensor(to_oracle(y)), atol=1e-12)
    r = T.add_(x, y)
    assert r is x and x.ttv_rks == [1, 5, 1] and all(o == 0 for o in x.ttv_ot)
    assert np.allclose(O.ttv_to_tensor(to_oracle(x)), expected, atol=1e-12)


def test_scale_semantics(T):
    x = T.rand_tt((2,) * 5, 3, seed=9)
    x.ttv_ot = [1, 1, 0, -1, -1]
    y = 3.0 * x
    ref = O.scale(3.0, to_oracle(x))
    _cores_equal(y, ref)                    # scales the first core with ot == 0 (site 3); ot copied
    z = 0.0 * x
    assert z.ttv_ot == [0] * 5 and all(np.all(c == 0) for c in z.ttv_vec) and z.ttv_rks == x.ttv_rks
    w = x - x                                   # (-1.0) * x + x: a rank-2r train that represents exactly zero
    assert np.max(np.abs(O.ttv_to_tensor(to_oracle(w)))) <= 1e-14 * np.max(np.abs(O.ttv_to_tensor(to_oracle(x))))
    # dot(w, w) is a sum of terms of size ||x||^2 that cancel: zero to the parity bar of dot (1e-12 of that size) — the norm, its
    # square root, is then zero to sqrt(eps) ||x|| only (the left-to-right order of round 2 happened to cancel exactly)
    assert abs(T.dot(w, w)) <= 1e-12 * T.dot(x, x)
    _cores_equal(x / 4.0, O.div(to_oracle(x), 4.0))


# ------------------------------------------------------------------------------------------------
# orthogonalize
# ------------------------------------------------------------------------------------------------
def test_orthogonalize_reference_properties(T):
    rng = np.random.default_rng(3)          # test/test_tt_tools.jl:981-1017
    dims = (2, 3, 4)
    tt = to_product(O.rand_tt(dims, [1, 2, 3, 1], rng))
    T0 = O.ttv_to_tensor(to_oracle(tt))
    for center in (1, 2, 3):
        orth = T.orthogonalize(tt, i=center)
        assert np.allclose(O.ttv_to_tensor(to_oracle(orth)), T0, atol=1e-12)
        assert orth.ttv_ot[center - 1] == 0
        assert all(orth.ttv_ot[j] == 1 for j in range(center - 1))
        assert all(orth.ttv_ot[j] == -1 for j in range(center, 3))
        for j in range(center - 1):
            G = np.asarray(orth.ttv_vec[j])
            n, rl, rr = G.shape
            A = G.transpose(1, 0, 2).reshape(rl * n, rr, order="F")
            assert np.allclose(A.T @ A, np.eye(rr), atol=1e-12)
        for j in range(center, 3):
            G = np.asarray(orth.ttv_vec[j])
            n, rl, rr = G.shape
            A = G.transpose(1, 2, 0).reshape(rl, rr * n, order="F")
            assert np.allclose(A @ A.T, np.eye(rl), atol=1e-12)


@pytest.mark.parametrize("d,r,center", [(12, 20, 1), (12, 20, 7), (12, 20, 12), (16, 48, 1)])
def test_orthogonalize_vs_oracle(T, d, r, center):
    x = T.Delta(d) * T.rand_tt((2,) * d, r // 3 + 1, seed=d + center)      # rank-deficient-ish input, ranks 3*(...)
    got = T.orthogonalize(x, i=center)
    ref = O.orthogonalize(to_oracle(x), i=center)
    assert got.ttv_rks == ref.ttv_rks and got.ttv_ot == ref.ttv_ot
    assert tt_rel_diff(to_oracle(got), to_oracle(x)) < 1e-12
    for j, G in enumerate(got.ttv_vec):
        G = np.asarray(G)
        n, rl, rr = G.shape
        if j < center - 1:
            A = G.transpose(1, 0, 2).reshape(rl * n, rr, order="F")
            assert np.max(np.abs(A.T @ A - np.eye(rr))) < 1e-12
        elif j > center - 1:
            A = G.transpose(1, 2, 0).reshape(rl, rr * n, order="F")
            assert np.max(np.abs(A @ A.T - np.eye(rl))) < 1e-12


@pytest.mark.parametrize("center", [1, 15, 30])
def test_orthogonalize_full_size_vs_oracle(T, center):
    """SURVEY 8 row a6 at ITS size: y = Delta(30) * rand_tt(rank 64) (ranks up to 192: the 192 x 384 LQ / 384 x 192 QR steps of C3),
    centres at both ends and in the middle.  Ranks and gauge flags exact vs the oracle (src/tt_tools.jl:511-543), the tensor
    unchanged to 1e-12, every non-centre core orthonormal to 1e-12 (test/test_tt_tools.jl:981-1017 at the headline size)."""
    d, r = 30, 64
    x = T.Delta(d) * T.rand_tt((2,) * d, r, seed=30)
    assert max(x.ttv_rks) == 192
    got = T.orthogonalize(x, i=center)
    ref = O.orthogonalize(to_oracle(x), i=center)
    assert got.ttv_rks == ref.ttv_rks and got.ttv_ot == ref.ttv_ot
    assert tt_rel_diff(to_oracle(got), to_oracle(x)) < 1e-12
    worst = 0.0
    for j, G in enumerate(got.ttv_vec):
        G = np.asarray(G)
        n, rl, rr = G.shape
        if j < center - 1:
            Amat = G.transpose(1, 0, 2).reshape(rl * n, rr, order="F")
            worst = worst_of(worst, float(np.max(np.abs(Amat.T @ Amat - np.eye(rr)))))
        elif j > center - 1:
            Amat = G.transpose(1, 2, 0).reshape(rl, rr * n, order="F")
            worst = worst_of(worst, float(np.max(np.abs(Amat @ Amat.T - np.eye(rl)))))
    assert worst < 1e-12, worst
    # the centre core carries the norm: same as the oracle's (gauge invariant)
    assert math.isclose(np.linalg.norm(np.asarray(got.ttv_vec[center - 1])), np.linalg.norm(ref.ttv_vec[center - 1]), rel_tol=1e-12)


@pytest.mark.parametrize("d,r,center,seed", [(30, 64, 1, 0), (30, 64, 12, 1), (16, 37, 1, 2), (12, 20, 5, 3), (30, 64, 30, 4), (9, 5, 2, 5)])
def test_orthogonalize_three_launch_form(T, monkeypatch, d, r, center, seed):
    """The form rank <= 64 QTT trains take: one wave per train over the ramp sites at the right end (csrc/ttn_ortho_ramp.h), the
    512-thread Cholesky-QR kernel (two workgroups per CU, csrc/ttn_ortho512.h) over the tall sites and the centre core, the
    1024-thread kernel for the left sweep and for whatever the other two refuse — and the single 1024-thread launch (TTN_ORTHO512=0),
    both compared with the oracle: ranks / gauge flags exact, tensor unchanged to 1e-12, every non-centre core orthonormal to 1e-12
    (src/tt_tools.jl:511-543); plus a batch of 300 trains through the default dispatch."""
    rng = np.random.default_rng(500 + seed)
    x = to_product(O.rand_tt((2,) * d, r, rng))
    ref = O.orthogonalize(to_oracle(x), i=center)
    for form in ("1", "0"):                 # the multi-launch form (the default for these trains), then the single 1024-thread launch
        monkeypatch.setenv("TTN_ORTHO512", form)
        got = T.orthogonalize(x, i=center)
        assert got.ttv_rks == ref.ttv_rks and got.ttv_ot == ref.ttv_ot
        assert tt_rel_diff(to_oracle(got), to_oracle(x)) < 1e-12
        worst = 0.0
        for j, G in enumerate(got.ttv_vec):
            G = np.asarray(G)
            n, rl, rr = G.shape
            if j < center - 1:
                Amat = G.transpose(1, 0, 2).reshape(rl * n, rr, order="F")
                worst = worst_of(worst, float(np.max(np.abs(Amat.T @ Amat - np.eye(rr)))))
            elif j > center - 1:
                Amat = G.transpose(1, 2, 0).reshape(rl, rr * n, order="F")
                worst = worst_of(worst, float(np.max(np.abs(Amat @ Amat.T - np.eye(rl)))))
        assert worst < 1e-12, (form, worst)
    monkeypatch.delenv("TTN_ORTHO512")
    if seed == 2:
        B = 300
        dx = T.DeviceTT((2,) * d, x.ttv_rks, batch=B)
        xs = [to_product(O.rand_tt((2,) * d, r, rng)) for _ in range(4)]
        for b in range(B):
            dx.upload(b, xs[b % 4])
        dy = T.DeviceTT((2,) * d, x.ttv_rks, batch=B)
        T.device.orthogonalize(dx, center, dy)
        for b in (0, 1, 150, 299):
            yb = dy.download(b)
            assert tt_rel_diff(to_oracle(yb), to_oracle(xs[b % 4])) < 1e-12
            assert yb.ttv_rks == O.orthogonalize(to_oracle(xs[b % 4]), i=center).ttv_rks


def _ortho_checks(O_, got, x, center, tol=1e-12):
    ref = O_.orthogonalize(to_oracle(x), i=center)
    assert got.ttv_rks == ref.ttv_rks and got.ttv_ot == ref.ttv_ot
    assert tt_rel_diff(to_oracle(got), to_oracle(x)) < tol
    worst = 0.0
    for j, G in enumerate(got.ttv_vec):
        G = np.asarray(G)
        n, rl, rr = G.shape
        if j < center - 1:
            Amat = G.transpose(1, 0, 2).reshape(rl * n, rr, order="F")
            worst = worst_of(worst, float(np.max(np.abs(Amat.T @ Amat - np.eye(rr)))))
        elif j > center - 1:
            Amat = G.transpose(1, 2, 0).reshape(rl, rr * n, order="F")
            worst = worst_of(worst, float(np.max(np.abs(Amat @ Amat.T - np.eye(rl)))))
    assert worst < tol, worst


def test_dot_and_streaming_ops_fuzz(T):
    """Sixty random pairs of trains (2..14 sites of size 2, every fifth trial of size 3; independent ragged bond ranks) through dot,
    +, hadamard, scalar * and tto * ttv with a random operator: the kernels rewritten in round 3 (K fibres per thread in add / hadamard /
    apply, the LDS-resident dot) on shapes where nothing is a multiple of anything.  Ranks exact; cores of the HBM-bound ops entrywise
    1e-13 / 1e-12 (they are copies and short sums), dot to 1e-12 of ||x|| ||y||."""
    rng = np.random.default_rng(99)
    for trial in range(60):
        d = int(rng.integers(2, 15))
        n = 2 if trial % 5 else 3
        dims = (n,) * d
        x = O.rand_tt(dims, [1] + [int(rng.integers(1, 40)) for _ in range(d - 1)] + [1], rng)
        y = O.rand_tt(dims, [1] + [int(rng.integers(1, 40)) for _ in range(d - 1)] + [1], rng)
        xp, yp = to_product(x), to_product(y)
        assert abs(T.dot(xp, yp) - O.dot(x, y)) <= 1e-12 * math.sqrt(abs(O.dot(x, x)) * abs(O.dot(y, y)))
        z, zref = T.add(xp, yp), O.add(x, y)
        assert list(z.ttv_rks) == zref.ttv_rks and tt_rel_diff(to_oracle(z), zref) < 1e-13
        xs = O.rand_tt(dims, [1] + [int(rng.integers(1, 9)) for _ in range(d - 1)] + [1], rng)
        ys = O.rand_tt(dims, [1] + [int(rng.integers(1, 9)) for _ in range(d - 1)] + [1], rng)
        h, href = T.hadamard(to_product(xs), to_product(ys)), O.hadamard(xs, ys)
        assert list(h.ttv_rks) == href.ttv_rks
        assert max(np.max(np.abs(np.asarray(a) - b)) for a, b in zip(h.ttv_vec, href.ttv_vec)) <= 1e-13 * max(np.max(np.abs(b)) for b in href.ttv_vec)
        A = O.rand_tto(dims, int(rng.integers(1, 5)), rng)
        ya, yref = T.apply(to_product(A), xp), O.apply(A, x)
        assert list(ya.ttv_rks) == yref.ttv_rks
        assert max(np.max(np.abs(np.asarray(a) - b)) for a, b in zip(ya.ttv_vec, yref.ttv_vec)) <= 1e-12 * max(np.max(np.abs(b)) for b in yref.ttv_vec)
        assert tt_rel_diff(to_oracle(T.scale(-1.75, xp)), O.scale(-1.75, x)) < 1e-13


@pytest.mark.parametrize("eps", [1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 1e-5])
def test_orthogonalize_moderately_ill_conditioned_sites(T, eps):
    """Trains whose tall sites have pairs of columns that agree up to eps (cond of the site matrices ~ 1 / eps): the range in which the
    512-thread kernel accepts a Cholesky-QR step as it is (measured defect <= 2e-13), repairs it by a first-order second pass (<= 1e-9)
    or refuses it and hands the train to the Householder route.  Whatever route a site takes, the TENSOR must stay within 1e-12 and
    the cores orthonormal to 1e-12 — the first version multiplied by an explicitly assembled inverse of L and kept the orthogonality
    defect (eps cond^2, up to 1e-10) as an error of Q R = W after the repair; found by sweeping eps, fixed by blocked substitution."""
    rng = np.random.default_rng(11)
    d, r = 14, 48
    x = O.rand_tt((2,) * d, r, rng)
    for k in (6, 7, 8):
        c = x.ttv_vec[k]
        c[:, 1::2, :] = c[:, 0::2, :][:, : c[:, 1::2, :].shape[1], :] + eps * c[:, 1::2, :]
    xp = to_product(x)
    _ortho_checks(O, T.orthogonalize(xp, i=1), xp, 1)
    _ortho_checks(O, T.orthogonalize(xp, i=5), xp, 5)


def test_apply_with_operator_cores_beyond_the_lds_staging_and_long_ragged_dots(T):
    """tto * ttv with operator cores too large for k_apply's LDS staging (rank 40: 6400 doubles per core; the kernel's other mappings)
    and dot on chains of up to 30 sites with independent ragged ranks up to 64 (the LDS-resident path) and up to 99 (the generic path),
    singly and as one ragged batch."""
    rng = np.random.default_rng(123)
    for d, n, ro, rx in [(5, 2, 40, 9), (4, 2, 33, 64), (4, 3, 20, 7), (6, 2, 24, 16)]:
        dims = (n,) * d
        A, x = O.rand_tto(dims, ro, rng), O.rand_tt(dims, rx, rng)
        ya, yref = T.apply(to_product(A), to_product(x)), O.apply(A, x)
        assert list(ya.ttv_rks) == yref.ttv_rks
        assert max(np.max(np.abs(np.asarray(a) - b)) for a, b in zip(ya.ttv_vec, yref.ttv_vec)) <= 1e-12 * max(np.max(np.abs(b)) for b in yref.ttv_vec)
    for trial in range(30):
        d = int(rng.integers(2, 31))
        hi = 65 if trial % 3 else 100
        x = O.rand_tt((2,) * d, [1] + [int(rng.integers(1, hi)) for _ in range(d - 1)] + [1], rng)
        y = O.rand_tt((2,) * d, [1] + [int(rng.integers(1, hi)) for _ in range(d - 1)] + [1], rng)
        x, y = O.scale(1 / O.norm(x), x), O.scale(1 / O.norm(y), y)
        assert abs(T.dot(to_product(x), to_product(y)) - O.dot(x, y)) <= 1e-12
    B, d = 40, 12
    cap = [1] + [64] * (d - 1) + [1]
    xs = [O.rand_tt((2,) * d, [1] + [int(rng.integers(1, 65)) for _ in range(d - 1)] + [1], rng) for _ in range(B)]
    ys = [O.rand_tt((2,) * d, [1] + [int(rng.integers(1, 65)) for _ in range(d - 1)] + [1], rng) for _ in range(B)]
    dx, dy = T.DeviceTT((2,) * d, cap, batch=B), T.DeviceTT((2,) * d, cap, batch=B)
    for b in range(B):
        dx.upload(b, to_product(xs[b]))
        dy.upload(b, to_product(ys[b]))
    got = T.device.dot(dx, dy)
    for b in range(B):
        assert abs(got[b] - O.dot(xs[b], ys[b])) <= 1e-12 * O.norm(xs[b]) * O.norm(ys[b])


@pytest.mark.parametrize("d,r,mb,seed", [(10, 8, 8, 0), (12, 16, 9, 1), (30, 64, 64, 2), (8, 5, 100, 3)])
def test_stateless_apply_compress_is_compress_of_apply(T, d, r, mb, seed):
    """ttn_apply_compress_f64 — op = x -> tt_compress!(A * x, max_bond) of src/solvers/euler.jl:55 as one stateless call — against the
    oracle's tt_compress_(apply(A, x)) and against the two-call form of this library: ranks exact, tensor 1e-9 (typically 1e-13),
    singular-value gauge as everywhere."""
    rng = np.random.default_rng(900 + seed)
    A = O.Delta(d)
    x = O.rand_tt((2,) * d, r, rng)
    ref = O.tt_compress_(O.apply(A, x), mb)
    got = T.apply_compress(to_product(A), to_product(x), mb)
    two = T.tt_compress_(T.apply(to_product(A), to_product(x)), mb)
    assert list(got.ttv_rks) == ref.ttv_rks == list(two.ttv_rks)
    assert tt_rel_diff(to_oracle(got), ref) < 1e-9 and tt_rel_diff(to_oracle(got), to_oracle(two)) < 1e-9


def test_orthogonalize_benchmark_trains_stay_in_the_fast_kernels(T):
    """A guard on the dispatch, not on numbers: 128 of the benchmark's trains (d = 30, rank 64, seeds 30 ...) are all FINISHED by the
    512-thread kernel — none is refused at its first tall site (cond 150 ... 2e3) and left to the third launch, where a single train's
    remaining sweep costs as much as the whole batch's (seen as a bimodal 3.5 / 4.7 ms per 1024 trains while the repair bound was
    1e-9) — and they pass the usual checks."""
    import ctypes as C
    d, r, B = 30, 64, 128
    x0 = T.rand_tt((2,) * d, r, seed=30)
    dx = T.DeviceTT((2,) * d, x0.ttv_rks, batch=B)
    xs = [T.rand_tt((2,) * d, r, seed=30 + b) for b in range(B)]
    for b in range(B):
        dx.upload(b, xs[b])
    dy = T.DeviceTT((2,) * d, x0.ttv_rks, batch=B)
    T.device.orthogonalize(dx, 1, dy)
    st = (C.c_int64 * 4)()
    unfinished = []
    for b in range(B):
        T._lib.check(T._lib.lib().ttn_debug_ortho_state(b, st))
        if int(st[3]) != 1:
            unfinished.append((b, int(st[0])))
    assert not unfinished, unfinished
    for b in (0, 17, 127):
        _ortho_checks(O, dy.download(b), xs[b], 1)


def test_compress_fuzz_ragged_ranks(T):
    """120 random trains (2..12 sites of size 2 or 3, independent bond ranks 2..40, max_bond 1..29, truncerr 0 / 1e-8 / 1e-4, one or
    two sweeps) through tt_compress! and through the stateless fused apply + compress with a random operator: ranks exact always.
    The tensor is compared at 1e-9 whenever the problem is well posed.  It is NOT well posed when a bond of the input is rank deficient
    relative to its neighbours and max_bond: the reference keeps min(length(s), max_bond) singular values, i.e. it GROWS such a bond by
    singular vectors of (numerically) zero singular values — arbitrary vectors, LAPACK's choice in the reference, Jacobi's here —, the
    sqrt(S) split hands each factor sqrt(1e-16) = 1e-8 of them, and the lossy truncations of the following bonds mix that differently
    (seen: 2e-2 between two results of EQUAL quality).  Detected from the oracle's own kept singular values (one below 1e-10 of the
    largest of its step); those cases are held to the approximation error against the input instead: not worse than 1.5 x the oracle's."""
    rng = np.random.default_rng(2024)
    ill = 0
    for trial in range(120):
        d = int(rng.integers(2, 13))
        n = 2 if trial % 4 else 3
        dims = (n,) * d
        x = O.rand_tt(dims, [1] + [int(rng.integers(2, 41)) for _ in range(d - 1)] + [1], rng)
        mb = int(rng.integers(1, 30))
        te = [0.0, 0.0, 1e-8, 1e-4][trial % 4]
        sw = 1 if trial % 7 else 2
        A = O.rand_tto(dims, int(rng.integers(1, 4)), rng)
        for fused in (False, True):
            src = O.apply(A, x) if fused else x
            sv = []
            ref = O.tt_compress_(O.copy_tt(src), mb, truncerr=te, sweeps=sw, svals_out=sv)
            got = T.apply_compress(to_product(A), to_product(x), mb, truncerr=te, sweeps=sw) if fused \
                else T.tt_compress_(to_product(O.copy_tt(x)), mb, truncerr=te, sweeps=sw)
            assert list(got.ttv_rks) == ref.ttv_rks, (trial, fused)
            grown = any(len(v) and float(np.min(v)) < 1e-10 * float(np.max(v)) for v in sv)
            if not grown:
                assert tt_rel_diff(to_oracle(got), ref) < 1e-9, (trial, fused)
            else:
                ill += 1
                e_dev, e_ref = tt_rel_diff(to_oracle(got), src), tt_rel_diff(ref, src)
                assert e_dev <= 1.5 * e_ref + 1e-9, (trial, fused, e_dev, e_ref)        # (seen: 1.5e-3 against the oracle's 1.9e-3, and the reverse)
    assert ill < 80                                            # (41 of the 240 runs with this seed: the classifier must not swallow the test)


def test_orthogonalize_fuzz_ragged_ranks(T):
    """Forty QTT trains with random lengths (3..16), random bond ranks in 1..64 (wide, square and tall sites in any order, ranks that
    are no multiples of anything) and random centres through the default dispatch (ramp kernel / 512-thread kernel / general route,
    whichever each site belongs to), singly and as one ragged batch: ranks and gauge flags exact, tensor 1e-12, orthonormality 1e-12."""
    rng = np.random.default_rng(4242)
    for trial in range(40):
        d = int(rng.integers(3, 17))
        rks = [1] + [int(rng.integers(1, 65)) for _ in range(d - 1)] + [1]
        x = O.rand_tt((2,) * d, rks, rng)                      # (rand_tt caps the ranks at what the dimensions allow)
        center = int(rng.integers(1, d + 1))
        xp = to_product(x)
        _ortho_checks(O, T.orthogonalize(xp, i=center), xp, center)
    # one batch, all trains with the same declared rank bound but different actual ranks (ragged)
    d, B = 12, 24
    bound = [1] + [64] * (d - 1) + [1]
    trains = []
    for b in range(B):
        rks = [1] + [int(rng.integers(1, 65)) for _ in range(d - 1)] + [1]
        trains.append(to_product(O.rand_tt((2,) * d, rks, rng)))
    cap = bound                                                # (a capacity, not a rank profile: larger than any train's ranks)
    dx = T.DeviceTT((2,) * d, cap, batch=B)
    for b in range(B):
        dx.upload(b, trains[b])
    dy = T.DeviceTT((2,) * d, cap, batch=B)
    for center in (1, 7):
        T.device.orthogonalize(dx, center, dy)
        for b in range(B):
            _ortho_checks(O, dy.download(b), trains[b], center)


def test_orthogonalize_hand_over_between_the_kernels(T, monkeypatch):
    """The rarely taken paths of the multi-launch form: (a) the 512-thread kernel takes nothing (TTN_ORTHO_CHOLQR=1 forbids its
    Cholesky-QR steps): the 1024-thread kernel resumes every train right behind the ramp kernel, from the compacted list; (b) a train
    whose tall sites are numerically rank deficient (pairs of columns equal to 1e-9: cond ~ 1e9, a Cholesky pivot fails or the measured
    orthogonality is far above the bar): the step is REFUSED in the middle of the sweep and the general route (Householder) finishes
    that train, while its neighbours in the batch finish in the 512-thread kernel.  Same checks as everywhere: ranks / gauge flags
    exact, tensor unchanged, every non-centre core orthonormal to 1e-12 (src/tt_tools.jl:511-543)."""
    rng = np.random.default_rng(77)
    d, r = 14, 24
    x = to_product(O.rand_tt((2,) * d, r, rng))
    monkeypatch.setenv("TTN_ORTHO512", "1")
    monkeypatch.setenv("TTN_ORTHO_CHOLQR", "1")
    for center in (1, 6):
        _ortho_checks(O, T.orthogonalize(x, i=center), x, center)
    monkeypatch.delenv("TTN_ORTHO_CHOLQR")
    # (b) ill-conditioned tall sites: column al' of core 7 and 8 nearly equal to column al' - 1
    bad = to_oracle(x)
    for k in (6, 7):
        c = bad.ttv_vec[k]
        c[:, 1::2, :] = c[:, 0::2, :][:, : c[:, 1::2, :].shape[1], :] + 1e-9 * c[:, 1::2, :]
    bad = to_product(bad)
    B = 20
    good = [to_product(O.rand_tt((2,) * d, r, rng)) for _ in range(3)]
    dx = T.DeviceTT((2,) * d, x.ttv_rks, batch=B)
    for b in range(B):
        dx.upload(b, bad if b in (3, 11) else good[b % 3])
    dy = T.DeviceTT((2,) * d, x.ttv_rks, batch=B)
    T.device.orthogonalize(dx, 1, dy)
    # the state words of the launch (diagnostic hook of the library): [next site, right buffer, left buffer, finished by k_ortho512]
    import ctypes as C
    finished = []
    for b in range(B):
        st = (C.c_int64 * 4)()
        T._lib.check(T._lib.lib().ttn_debug_ortho_state(b, st))
        finished.append(int(st[3]))
    assert [b for b in range(B) if not finished[b]] == [3, 11], finished        # refused exactly where the sites are rank deficient
    for b in (0, 3, 4, 11, 19):
        src = bad if b in (3, 11) else good[b % 3]
        _ortho_checks(O, dy.download(b), src, 1, tol=1e-11 if b in (3, 11) else 1e-12)
    monkeypatch.delenv("TTN_ORTHO512")


# ------------------------------------------------------------------------------------------------
# _tt_bond_truncate! / tt_compress!
# ------------------------------------------------------------------------------------------------
def test_bond_truncate_reference_cases(T):
    rng = np.random.default_rng(5)          # test/test_tt_tools.jl:433-498
    tt = T.TTvector(3, [rng.standard_normal((2, 1, 4)), rng.standard_normal((2, 4, 4)), rng.standard_normal((2, 4, 1))],
                    (2, 2, 2), [1, 4, 4, 1], [0, 0, 0])
    ref = to_oracle(tt)
    y = T._tt_bond_truncate_(tt, 1, max_bond=2, truncerr=0.0)
    O.tt_bond_truncate_(ref, 1, max_bond=2)
    assert tt.ttv_rks[1] <= 2 and tt.ttv_rks == ref.ttv_rks
    r = tt.ttv_rks[1]
    assert tt.ttv_vec[0].shape == (2, 1, r) and tt.ttv_vec[1].shape == (2, r, 4)
    assert y.ttv_rks[1] == tt.ttv_rks[1] and y.ttv_vec[0].shape == tt.ttv_vec[0].shape
    assert np.allclose(O.ttv_to_tensor(to_oracle(tt)), O.ttv_to_tensor(ref), atol=1e-12)

    u, v, p, q = [1.2, -0.5], [0.7, 0.3], [2.0, 3.0], [4.0, 5.0]
    c1, c2 = np.zeros((2, 1, 2)), np.zeros((2, 2, 1))
    for s in range(2):
        for g in range(2):
            c1[s, 0, g] = p[g] * u[s]
            c2[s, g, 0] = q[g] * v[s]
    tt2 = T.TTvector(2, [c1, c2], (2, 2), [1, 2, 1], [0, 0])
    T0 = O.ttv_to_tensor(to_oracle(tt2))
    y2 = T._tt_bond_truncate_(tt2, 1, max_bond=1)
    assert tt2.ttv_rks[1] == 1 and tt2.ttv_vec[0].shape == (2, 1, 1) and tt2.ttv_vec[1].shape == (2, 1, 1) and y2.ttv_rks[1] == 1
    assert np.allclose(O.ttv_to_tensor(to_oracle(tt2)), T0, atol=1e-12)
    tt3 = T.rand_tt((2, 2, 2), [1, 2, 2, 1], seed=4)
    with pytest.raises(AssertionError):
        T._tt_bond_truncate_(tt3, 0)
    with pytest.raises(AssertionError):
        T._tt_bond_truncate_(tt3, tt3.N)


def test_tt_compress_reference_behaviour(T, caplog):
    tt = T.rand_tt((2, 2, 2), [1, 2, 2, 1], seed=6)                     # test/test_tt_tools.jl:500-574
    before, T0 = list(tt.ttv_rks), O.ttv_to_tensor(to_oracle(tt))
    y = T.tt_compress_(tt, 10, sweeps=1)
    assert y is tt and tt.ttv_rks == before
    assert np.allclose(O.ttv_to_tensor(to_oracle(tt)), T0, atol=1e-12)
    tt = T.rand_tt((2, 2, 2, 2), [1, 4, 4, 4, 1], seed=7)
    y = T.tt_compress_(tt, 2, sweeps=1)
    assert y is tt and max(tt.ttv_rks) <= 2
    for i in range(4):
        assert tt.ttv_vec[i].shape == (2, tt.ttv_rks[i], tt.ttv_rks[i + 1])
    with pytest.raises(AssertionError):
        T.tt_compress_(T.rand_tt((2, 2, 2), [1, 2, 2, 1], seed=8), 2, sweeps=0)
    tt = T.rand_tt((2, 2, 2), [1, 3, 3, 1], seed=9)
    ref = to_oracle(tt)
    assert T.tt_compress_(tt, 3, sweeps=2, truncerr=0.0) is tt
    O.tt_compress_(ref, 3, sweeps=2)
    assert np.allclose(O.ttv_to_tensor(to_oracle(tt)), O.ttv_to_tensor(ref), atol=1e-12)
    import logging
    with caplog.at_level(logging.INFO, logger="TensorTrainNumerics"):
        T.tt_compress_(T.rand_tt((2, 2, 2), [1, 2, 2, 1], seed=10), 2, verbose=True)
    msgs = [r.getMessage() for r in caplog.records]
    assert any("TT compress: sweep 1 (L→R)" in m for m in msgs) and any("TT compress: sweep 1 (R→L)" in m for m in msgs)


def test_compress_rank_growth_like_reference(T):
    """The reference keeps min(length(s), max_bond) singular values, so the rank of a rank-deficient bond GROWS
    (zero singular values are kept): ranks [1,1,1,1] with max_bond 10 become [1,2,2,1]."""
    x = T.rand_tt((2, 2, 2), [1, 1, 1, 1], seed=3)
    ref = O.tt_compress_(to_oracle(x), 10)
    assert ref.ttv_rks == [1, 2, 2, 1]
    dense = O.ttv_to_tensor(to_oracle(x))
    got = T.tt_compress_(x, 10)
    assert got.ttv_rks == ref.ttv_rks
    for k, c in enumerate(got.ttv_vec):
        assert c.shape == (2, got.ttv_rks[k], got.ttv_rks[k + 1])
    assert np.allclose(O.ttv_to_tensor(to_oracle(got)), dense, atol=1e-14)
    need, fin = T.device.compress_rank_bound((2, 2, 2), [1, 1, 1, 1], 10)
    assert need == [1, 2, 2, 1] and fin == [1, 2, 2, 1]
    # a handle whose capacity cannot hold the grown rank is refused instead of overflowing
    dx = T.DeviceTT.from_host(T.rand_tt((2, 2, 2), [1, 1, 1, 1], seed=3))
    with pytest.raises(T.TTNError):
        T.device.tt_compress_(dx, 10)
    # a wider example: random rank-2 train inside rank-5 capacity, no truncation
    y = T.rand_tt((2,) * 6, [1, 2, 2, 2, 2, 2, 1], seed=5)
    refy = O.tt_compress_(to_oracle(y), 50)
    goty = T.tt_compress_(y, 50)
    assert goty.ttv_rks == refy.ttv_rks
    assert tt_rel_diff(to_oracle(goty), refy) < 1e-12


def test_compress_compressible_inputs(T):
    """Restates test/test_qtt_multidim.jl:577-614 with closed-form inputs (truncerr = 1e-12)."""
    d = 12
    e = T.qtt_exp(d, alpha=-1.0)
    padded = (e + 0.5 * e) + ((-0.25) * e + e)
    assert max(padded.ttv_rks) == 4
    ref = to_oracle(padded)
    T.tt_compress_(padded, 10, truncerr=1e-12)
    O.tt_compress_(ref, 10, truncerr=1e-12)
    assert padded.ttv_rks == ref.ttv_rks and max(padded.ttv_rks) == 1
    x = np.linspace(0, 1, 2 ** d)
    assert np.max(np.abs(T.qtt_to_vector(padded) - 2.25 * np.exp(-x))) < 1e-10
    d = 10
    s = T.qtt_sin(d, lam=2.0)
    big = T.hadamard(s, T.qtt_cos(d, lam=3.0)) + 1e-3 * T.hadamard(s, s)
    dense = T.qtt_to_vector(big)
    refb = to_oracle(big)
    T.tt_compress_(big, 8, truncerr=1e-12)
    O.tt_compress_(refb, 8, truncerr=1e-12)
    assert big.ttv_rks == refb.ttv_rks and max(big.ttv_rks) <= 8
    assert np.max(np.abs(T.qtt_to_vector(big) - dense)) < 1e-8


@pytest.mark.parametrize("d,r,seed", [(8, 6, 1), (12, 16, 2), (20, 32, 20)])
def test_apply_compress_vs_oracle(T, d, r, seed):
    """Δ(d) * random rank-r train, then tt_compress!(·, r): ranks exact, per-bond singular values 1e-10,
    cores equal up to one sign per bond, tensor difference ≤ 1e-9 (config 2 is d=20, r=32)."""
    x = T.rand_tt((2,) * d, r, seed=seed)
    A = T.Delta(d)
    dA, dx = T.DeviceTTO(A), T.DeviceTT.from_host(x)
    dy = T.DeviceTT(x.ttv_dims, [a * b for a, b in zip(A.tto_rks, x.ttv_rks)])
    dy.capture_singular_values(True)
    T.device.apply_compress(dA, dx, dy, r, 0.0, 1)
    T.device.compress_status(dy)
    got = dy.download()
    sv = []
    ref = O.tt_compress_(O.apply(O.Delta(d), to_oracle(x)), r, svals_out=sv)
    assert got.ttv_rks == ref.ttv_rks
    for i, s_ref in enumerate(sv):
        s = dy.singular_values(0, i)            # the device captures ALL singular values, the oracle the kept ones
        assert len(s) >= len(s_ref)
        assert np.allclose(s[: len(s_ref)], s_ref, rtol=1e-10, atol=1e-13 * s_ref[0]), f"bond step {i}"
    assert tt_rel_diff(to_oracle(got), ref) <= 1e-9
    assert sign_fix_compare(to_oracle(got), ref) <= 1e-7


def test_rk4_step_from_apply_round(T):
    """test/test_euler.jl:269-298: one RK4 step assembled from apply, +, scalar*, tt_compress! vs dense RK4."""
    rng = np.random.default_rng(7)
    d = 4
    hh = 1 / d ** 2
    A = T.toeplitz_to_qtto(-2.0, 1.0, 1.0, d)
    A.tto_vec[0] = (-hh ** 2) * A.tto_vec[0]
    u0 = to_product(O.rand_tt((2,) * d, [1, 2, 2, 2, 1], rng))
    h, mb = 0.05, 8
    k1 = A * u0
    k2 = A * T.tt_compress_(u0 + (h / 2) * k1, mb)
    k3 = A * T.tt_compress_(u0 + (h / 2) * k2, mb)
    k4 = A * T.tt_compress_(u0 + h * k3, mb)
    incr = (h / 6) * T.tt_compress_(k1 + 2 * k2 + 2 * k3 + k4, mb)
    sol = T.tt_compress_(u0 + incr, mb)
    Ad, ud = O.qtto_to_matrix(to_oracle(A)), T.qtt_to_vector(u0)
    K1 = Ad @ ud
    K2 = Ad @ (ud + h / 2 * K1)
    K3 = Ad @ (ud + h / 2 * K2)
    K4 = Ad @ (ud + h * K3)
    refv = ud + h / 6 * (K1 + 2 * K2 + 2 * K3 + K4)
    assert np.linalg.norm(T.qtt_to_vector(sol) - refv) / np.linalg.norm(refv) < 1e-6


def test_batched_handles_independent_trains(T):
    """A batch of different trains through apply + round: every train equals its own oracle result."""
    d, r, B = 10, 8, 5
    A = T.Delta(d)
    xs = [T.rand_tt((2,) * d, r, seed=100 + b) for b in range(B)]
    dA = T.DeviceTTO(A)
    dx = T.DeviceTT((2,) * d, xs[0].ttv_rks, batch=B)
    for b, x in enumerate(xs):
        dx.upload(b, x)
    dy = T.DeviceTT((2,) * d, [a * c for a, c in zip(A.tto_rks, xs[0].ttv_rks)], batch=B)
    T.device.apply_compress(dA, dx, dy, r, 0.0, 1)
    T.device.compress_status(dy)
    nrm = T.device.norm(dy)
    for b, x in enumerate(xs):
        ref = O.tt_compress_(O.apply(O.Delta(d), to_oracle(x)), r)
        got = dy.download(b)
        assert got.ttv_rks == ref.ttv_rks
        assert tt_rel_diff(to_oracle(got), ref) <= 1e-9
        assert math.isclose(nrm[b], O.norm(ref), rel_tol=1e-9)


def test_headline_config_properties(T):
    """C3 (d=30, rank 64): the oracle needs ~0.2 s here, so compare directly AND check size-independent
    properties: ranks, idempotence of a second round at the same max_bond, norm never increases."""
    d, r = 30, 64
    x = T.rand_tt((2,) * d, r, seed=30)
    A = T.Delta(d)
    dA, dx = T.DeviceTTO(A), T.DeviceTT.from_host(x)
    dy = T.DeviceTT(x.ttv_dims, [a * b for a, b in zip(A.tto_rks, x.ttv_rks)])
    T.device.apply(dA, dx, dy)
    n_before = T.device.norm(dy)[0]
    T.device.tt_compress_(dy, r)
    T.device.compress_status(dy)
    got = dy.download()
    assert got.ttv_rks == x.ttv_rks
    ref = O.tt_compress_(O.apply(O.Delta(d), to_oracle(x)), r)
    assert got.ttv_rks == ref.ttv_rks
    assert tt_rel_diff(to_oracle(got), ref) <= 1e-9
    n_after = T.device.norm(dy)[0]
    assert n_after <= n_before * (1 + 1e-12)
    # second round at the same rank: every merged matrix already has rank <= r, so the tensor is unchanged
    T.device.tt_compress_(dy, r)
    again = dy.download()
    assert again.ttv_rks == got.ttv_rks
    assert tt_rel_diff(to_oracle(again), to_oracle(got)) <= 1e-10


@pytest.mark.parametrize("seed", [30, 192, 210])
def test_headline_config_singular_values(T, seed):
    """C3 through the fused op with every bond step's singular values captured.  The 96-row step at the right end of the L->R
    half (128 x 96, 64 kept) has a kept-block conditioning of 1.4e2 / 2.4e3 / 5e3 for these seeds: it takes the zero-padded
    Gram + eigensolver route finished by the Jacobi polish of U^T M; the R->L half takes the
    diagonal-left form of route F.  Same bar as everywhere: ranks exact, kept singular values rtol 1e-10 (atol 1e-13 sigma_1,
    which is where LAPACK's own accuracy for the small values of the ill-conditioned ramp steps ends), tensor 1e-9."""
    d, r = 30, 64
    x = T.rand_tt((2,) * d, r, seed=seed)
    A = T.Delta(d)
    dA, dx = T.DeviceTTO(A), T.DeviceTT.from_host(x)
    dy = T.DeviceTT(x.ttv_dims, [a * b for a, b in zip(A.tto_rks, x.ttv_rks)])
    dy.capture_singular_values(True)
    T.device.apply_compress(dA, dx, dy, r, 0.0, 1)
    T.device.compress_status(dy)
    sv = []
    ref = O.tt_compress_(O.apply(O.Delta(d), to_oracle(x)), r, svals_out=sv)
    got = dy.download()
    assert got.ttv_rks == ref.ttv_rks
    for i, s_ref in enumerate(sv):
        s = dy.singular_values(0, i)
        assert np.allclose(s[: len(s_ref)], s_ref, rtol=1e-10, atol=1e-13 * s_ref[0]), f"bond step {i}"
    assert tt_rel_diff(to_oracle(got), ref) <= 1e-9


# The seeds bench.py times are 30 .. 1053.  The 96-row step at the right end of the L->R half (bond step 24) takes the Gram route
# finished by the Jacobi polish up to a kept-block conditioning of FAST_KAPPA_POLISH = 32768; over those 1024 seeds the
# conditioning of that step reaches 4.45e4 (tools/diag_kappa_batch.py 1024 24, round 2).  The 16 worst seeds — two beyond the
# limit (Householder route), the others between 6.8e3 and 3.0e4 (polish route AT its acceptance limit) — lead the list; the
# rest are a spread of ordinary seeds of the same batch.
BENCH_WORST_KAPPA_SEEDS = [490, 1004, 82, 243, 371, 274, 646, 294, 153, 857, 963, 726, 212, 90, 962, 422]
BENCH_PARITY_SEEDS = BENCH_WORST_KAPPA_SEEDS + [30 + 21 * i for i in range(48)]


def test_bench_batch_parity(T):
    """ONE ttn_apply_compress launch over 64 of the trains bench.py times (same seeds, same fused op, same batch layout), every
    bond step's singular values captured: per train ranks exact, kept singular values rtol 1e-10, tensor difference to the oracle
    <= 1e-9.  This pins the route the headline number is measured on, at its acceptance limit.
    Absolute floor of the singular-value comparison: 2e-12 sigma_1 up to and including the first step that keeps an ill-conditioned
    block (kappa > 1e9), 2e-11 sigma_1 downstream of it.  The 64-row ramp step of the R->L half (bond step 34) keeps ALL singular
    values of a merged matrix with a conditioning of 5e7 ... 5e10; two backward-stable SVDs of it (LAPACK gesdd here, Householder +
    one-sided Jacobi on the device) agree on its small values to c * K * eps * sigma_1 in ABSOLUTE terms only (measured: up to
    1.2e-12 sigma_1), and they leave DIFFERENT (equally valid) cores in the directions of those values; the next steps' merged
    matrices — formed from these non-orthogonal U sqrt(S) cores — inherit that: measured over these trains with three builds
    (tools/diag_sv_batch.py), the smallest kept value of step 35 (4e-2 sigma_1, conditioning 25) deviates by 1.7e-12 ... 6.6e-12 sigma_1
    and the deviation decays over the following steps (3e-12, 1e-12, 5e-13), while the tensors agree to 1e-13.  Before step 34
    nothing exceeds 1e-13 sigma_1."""
    d, r = 30, 64
    seeds = BENCH_PARITY_SEEDS
    assert len(seeds) == 64 and len(set(seeds)) == 64 and all(30 <= s_ <= 1053 for s_ in seeds)
    A = T.Delta(d)
    dA = T.DeviceTTO(A)
    x0 = T.rand_tt((2,) * d, r, seed=seeds[0])
    dx = T.DeviceTT((2,) * d, x0.ttv_rks, batch=len(seeds))
    xs = []
    for b, sd in enumerate(seeds):
        xs.append(T.rand_tt((2,) * d, r, seed=sd))
        dx.upload(b, xs[-1])
    dy = T.DeviceTT((2,) * d, [a * c for a, c in zip(A.tto_rks, x0.ttv_rks)], batch=len(seeds))
    dy.capture_singular_values(True)
    T.device.apply_compress(dA, dx, dy, r, 0.0, 1)
    T.device.compress_status(dy)
    OA = O.Delta(d)
    worst_sv, worst_abs, worst_t, kappa24 = 0.0, 0.0, 0.0, []
    for b, sd in enumerate(seeds):
        sv = []
        ref = O.tt_compress_(O.apply(OA, to_oracle(xs[b])), r, svals_out=sv)
        got = dy.download(b)
        assert got.ttv_rks == ref.ttv_rks, f"seed {sd}"
        ill = False                                              # an ill-conditioned kept block upstream
        for i, s_ref in enumerate(sv):
            s = dy.singular_values(b, i)[: len(s_ref)]
            atol = (2e-11 if ill else 2e-12) * s_ref[0]
            ill = ill or s_ref[0] > 1e9 * s_ref[min(len(s_ref), r) - 1]
            assert np.allclose(s, s_ref, rtol=1e-10, atol=atol), f"seed {sd} bond step {i}: max abs/sigma_1 {np.max(np.abs(s - s_ref) / s_ref[0]):.2e}"
            big = s_ref >= 2e-2 * s_ref[0]                        # where the relative bar is the binding one
            worst_sv = worst_of(worst_sv, float(np.max(np.abs(s[big] - s_ref[big]) / s_ref[big])))
            worst_abs = worst_of(worst_abs, float(np.max(np.abs(s - s_ref)) / s_ref[0]))
        kappa24.append(sv[24][0] / sv[24][min(len(sv[24]), r) - 1])
        err = tt_rel_diff(to_oracle(got), ref)
        worst_t = worst_of(worst_t, err)
        assert err <= 1e-9, f"seed {sd}: tensor rel. diff {err:.2e}"
    # the list really contains the acceptance limit of the polish route (and trains beyond it)
    assert max(kappa24[:16]) > 32768.0 and sum(1 for k_ in kappa24[:16] if 2.0e4 < k_ <= 32768.0) >= 4, kappa24[:16]
    print(f"bench-batch parity: worst rel. error of singular values >= 2e-2 sigma_1 {worst_sv:.2e}, worst abs. error / sigma_1 {worst_abs:.2e}, worst tensor rel. diff {worst_t:.2e}")


def test_bench_batch_singular_values_against_extended_precision(T):
    """The arbiter behind test_bench_batch_parity's absolute floors (2e-12 / 2e-11 sigma_1 between the device and LAPACK downstream
    of the kappa ~ 5e10 ramp step, bond step 34).  Two fp64 SVDs cannot arbitrate each other there, so every bond step from 33 to
    40 of 16 bench trains (the 8 worst-kappa seeds + 8 ordinary ones) is run ALONE on the device (ttn_bond_truncate) from the
    device's own upstream state, and its captured singular values are compared with the singular values of THE SAME merged matrix
    computed in extended precision on the host (numpy.longdouble, eps 1.1e-19: QR of the left core + one-sided Jacobi, the product
    never rounded to fp64; tests/helpers.py).  Bar for the device: rtol 1e-10 with an absolute floor of 1e-13 sigma_1
    — the fp64 backward-error level p * eps of ANY stable SVD of a 128-row matrix, 20x / 200x below the floors of the
    device-vs-LAPACK comparison.  The gap between the two floors is therefore not device error: it is the difference of the INPUTS
    of those steps (two valid gauges of the ill-conditioned step 34), which this test takes out by construction.  LAPACK's gesdd
    on the same fp64 matrices is measured alongside (printed) and held to the same bar."""
    import scipy.linalg as sla
    from tests.helpers import ext_svdvals_product
    d, r = 30, 64
    seeds = BENCH_WORST_KAPPA_SEEDS[:8] + [30 + 21 * i for i in range(8)]
    A = T.Delta(d)
    dA = T.DeviceTTO(A)
    x0 = T.rand_tt((2,) * d, r, seed=seeds[0])
    dx = T.DeviceTT((2,) * d, x0.ttv_rks, batch=len(seeds))
    for b, sd in enumerate(seeds):
        dx.upload(b, T.rand_tt((2,) * d, r, seed=sd))
    ycap = [a * c for a, c in zip(A.tto_rks, x0.ttv_rks)]
    # the one-launch run the bench times, singular values captured: the step-by-step run below must reproduce it
    dy1 = T.DeviceTT((2,) * d, ycap, batch=len(seeds))
    dy1.capture_singular_values(True)
    T.device.apply_compress(dA, dx, dy1, r, 0.0, 1)
    T.device.compress_status(dy1)
    # the same sweep cut into pieces: fused L->R pass, R->L bonds d-1 .. k0+1 in one call, then bond by bond
    dy = T.DeviceTT((2,) * d, ycap, batch=len(seeds))
    L = T._lib.lib()
    T._lib.check(L.ttn_apply_begin(dA.h, dx.h, dy.h))
    T._lib.check(L.ttn_apply_sweep(dA.h, dx.h, dy.h, 1, d - 1, r, 0.0, 0))
    first_step, last_step = 33, 40
    k_of = lambda step: (d - 1) - (step - (d - 1))            # noqa: E731   1-based bond of R->L bond step `step`
    T._lib.check(L.ttn_sweep(dy.h, d - 1, k_of(first_step) + 1, r, 0.0))
    dy.capture_singular_values(True)
    worst_dev_rel, worst_dev_abs, worst_lap_rel, worst_lap_abs, worst_vs_launch = 0.0, 0.0, 0.0, 0.0, 0.0
    for step in range(first_step, last_step + 1):
        k = k_of(step)
        before = [dy.download(b) for b in range(len(seeds))]
        T._lib.check(L.ttn_bond_truncate(dy.h, k, r, 0.0))
        T.device.compress_status(dy)
        for b, sd in enumerate(seeds):
            ck, ck1 = np.asarray(before[b].ttv_vec[k - 1]), np.asarray(before[b].ttv_vec[k])
            n1, Dl, rm = ck.shape
            n2, _, Dr = ck1.shape
            Am = ck.transpose(1, 0, 2).reshape(Dl * n1, rm, order="F")              # [(alpha + Dl s1), gamma]   (tt_tools.jl:746-749)
            Bm = ck1.transpose(1, 0, 2).reshape(rm, n2 * Dr, order="F")             # [gamma, (s2 + n2 beta)]
            keep = min(Dl * n1, n2 * Dr, r)
            s_ext = ext_svdvals_product(Am, Bm)[:keep]
            s_dev = dy.singular_values(b, 0)[:keep]
            s_lap = sla.svdvals(Am @ Bm)[:keep]
            s1 = float(s_ext[0])
            e_dev = np.abs(s_dev - s_ext).astype(float)
            e_lap = np.abs(s_lap - s_ext).astype(float)
            tol = 1e-10 * s_ext.astype(float) + 1e-13 * s1
            assert np.all(e_dev <= tol), (f"seed {sd} bond step {step}: device vs extended precision: max abs/sigma_1 {e_dev.max() / s1:.2e}, "
                                          f"max (err - 1e-13 sigma_1)/s {np.max((e_dev - 1e-13 * s1) / s_ext.astype(float)):.2e}")
            big = s_ext.astype(float) >= 2e-2 * s1
            worst_dev_rel = worst_of(worst_dev_rel, float(np.max(e_dev[big] / s_ext.astype(float)[big])))
            worst_lap_rel = worst_of(worst_lap_rel, float(np.max(e_lap[big] / s_ext.astype(float)[big])))
            worst_dev_abs, worst_lap_abs = worst_of(worst_dev_abs, e_dev.max() / s1), worst_of(worst_lap_abs, e_lap.max() / s1)
            s_launch = dy1.singular_values(b, step)[:keep]
            worst_vs_launch = worst_of(worst_vs_launch, float(np.max(np.abs(s_launch - s_dev)) / s1))
    print(f"sv arbiter (longdouble): device rel (>= 2e-2 sigma_1) {worst_dev_rel:.2e} abs/sigma_1 {worst_dev_abs:.2e}; LAPACK gesdd rel {worst_lap_rel:.2e} "
          f"abs/sigma_1 {worst_lap_abs:.2e}; step-by-step vs one launch abs/sigma_1 {worst_vs_launch:.2e}")
    # the pieces reproduce the one-launch sweep (same kernels, same order): identical up to the gauge noise of step 34
    assert worst_vs_launch <= 2e-11


# ------------------------------------------------------------------------------------------------
# edge cases: general physical dimensions, short sides > 128 (global-memory Jacobi fallback), truncerr > 0 on
# incompressible input, several sweeps, single bonds, ragged batches
# ------------------------------------------------------------------------------------------------
def _check_compress(T, x_prod, max_bond, truncerr=0.0, sweeps=1, tol=1e-9):
    ref = O.tt_compress_(to_oracle(x_prod), max_bond, truncerr=truncerr, sweeps=sweeps)
    got = T.tt_compress_(x_prod.copy(), max_bond, truncerr=truncerr, sweeps=sweeps)
    assert got.ttv_rks == ref.ttv_rks
    assert tt_rel_diff(to_oracle(got), ref) <= tol
    return got


def test_compress_general_dims_and_odd_sizes(T):
    rng = np.random.default_rng(31)
    x = to_product(O.rand_tt((3, 2, 5, 2, 3, 4), [1, 3, 5, 7, 6, 3, 1], rng))
    _check_compress(T, x, 4)
    _check_compress(T, x, 100)                      # nothing to truncate, ranks may be capped by min(rows, cols)
    y = to_product(O.rand_tt((2, 2), [1, 2, 1], rng))
    _check_compress(T, y, 1)
    z = to_product(O.rand_tt((4,), [1, 1], rng))    # d = 1: no bond at all
    got = T.tt_compress_(z.copy(), 3)
    assert got.ttv_rks == [1, 1] and np.array_equal(got.ttv_vec[0], z.ttv_vec[0])


def test_compress_short_side_above_128_uses_fallback(T):
    """x ranks 70 -> y ranks 210, max_bond 100: merged matrices have a short side of 200 > 128, so the LDS-resident
    Jacobi does not apply and the global-memory Jacobi + Householder route must give the oracle's answer."""
    d = 16
    x = T.Delta(d) * T.rand_tt((2,) * d, 70, seed=77)
    assert max(x.ttv_rks) == 210
    got = _check_compress(T, x, 100)
    assert max(got.ttv_rks) == 100


def test_compress_long_panel_householder(T):
    """A 140 x 900 merged matrix (dims (140, 3, 300), ranks [1, 140, 300, 1]): the blocked Householder LQ gets panels too long for
    its LDS form (16 x 900) and forms V V^T outside the workgroup GEMM (that GEMM call wrote an LDS matrix through a global pointer:
    a GPU fault on the first matrix wide enough to reach it — found by the 512-thread build, whose LDS panel is shorter)."""
    rng = np.random.default_rng(140)
    x = to_product(O.rand_tt((140, 3, 300), [1, 140, 300, 1], rng))
    _check_compress(T, x, 90)


@pytest.mark.parametrize("d,r,mb", [(14, 100, 100), (16, 128, 128)])
def test_compress_ranks_up_to_128_blocked_jacobi(T, d, r, mb):
    """Merged short side 128 < p <= 256 (ranks 65..128): Householder LQ + the blocked LDS Jacobi (column blocks of 32 of a
    matrix that lives in global memory).  Ranks exact, tensor 1e-9 against the oracle; per-bond singular values rtol 1e-10
    with atol 1e-12*sigma_1: at these sizes (256 x 512 merged matrices, 30 un-gauged steps each feeding the next) device and
    LAPACK trajectories drift apart by a few 1e-13*sigma_1 (measured 2e-13..7e-13, tools/diag_sv_err.py), the same size for the
    blocked and the in-LDS Householder — the 1e-13 of the rank-64 tests is too tight here."""
    x = T.rand_tt((2,) * d, r, seed=4)
    A = T.Delta(d)
    dA, dx = T.DeviceTTO(A), T.DeviceTT.from_host(x)
    dy = T.DeviceTT(x.ttv_dims, [a * b for a, b in zip(A.tto_rks, x.ttv_rks)])
    dy.capture_singular_values(True)
    T.device.apply_compress(dA, dx, dy, mb)
    T.device.compress_status(dy)
    got = dy.download()
    sv = []
    ref = O.tt_compress_(O.apply(O.Delta(d), to_oracle(x)), mb, svals_out=sv)
    assert got.ttv_rks == ref.ttv_rks and max(got.ttv_rks) > 64
    for i, s_ref in enumerate(sv):
        s = dy.singular_values(0, i)
        assert np.allclose(s[: len(s_ref)], s_ref, rtol=1e-10, atol=1e-12 * s_ref[0]), f"bond step {i}"
    assert tt_rel_diff(to_oracle(got), ref) <= 1e-9


def test_compress_truncerr_on_incompressible_input(T):
    d = 10
    x = T.Delta(d) * T.rand_tt((2,) * d, 8, seed=5)
    for te in (1e-1, 1e-2, 1e-6):
        _check_compress(T, x, 1000, truncerr=te)
    _check_compress(T, x, 6, truncerr=1e-3, sweeps=2)


def test_bond_truncate_every_bond(T):
    d = 7
    x = T.Delta(d) * T.rand_tt((2,) * d, 4, seed=9)
    for k in range(1, d):
        ref = to_oracle(x)
        O.tt_bond_truncate_(ref, k, max_bond=5)
        got = x.copy()
        y = T._tt_bond_truncate_(got, k, max_bond=5)
        assert got.ttv_rks == ref.ttv_rks
        assert tt_rel_diff(to_oracle(got), ref) <= 1e-9
        assert y.ttv_ot[k - 1] == 0 and tt_rel_diff(to_oracle(y), ref) <= 1e-9      # the returned orthogonalize(psi; i=k)


def test_ragged_batch_different_ranks_per_train(T):
    d = 8
    A = T.Delta(d)
    rks = [[1, 2, 3, 3, 3, 3, 3, 2, 1], [1, 2, 4, 8, 8, 8, 4, 2, 1], [1, 1, 1, 1, 1, 1, 1, 1, 1]]
    xs = [T.rand_tt((2,) * d, r, seed=40 + i) for i, r in enumerate(rks)]
    cap = [max(r[m] for r in rks) for m in range(d + 1)]
    dx = T.DeviceTT((2,) * d, cap, batch=3)
    for b, x in enumerate(xs):
        dx.upload(b, x)
    need, _ = T.device.compress_rank_bound((2,) * d, [a * c for a, c in zip(A.tto_rks, cap)], 6)
    dy = T.DeviceTT((2,) * d, need, batch=3)
    T.device.apply_compress(T.DeviceTTO(A), dx, dy, 6, 0.0, 1)
    T.device.compress_status(dy)
    for b, x in enumerate(xs):
        ref = O.tt_compress_(O.apply(O.Delta(d), to_oracle(x)), 6)
        got = dy.download(b)
        assert got.ttv_rks == ref.ttv_rks
        assert tt_rel_diff(to_oracle(got), ref) <= 1e-9


def test_fast_routes_agree_with_robust_route(T, monkeypatch):
    """Routes F/G (Gram/Cholesky) against route H (Householder) on the same input: TTN_FAST=0 forces H."""
    d, r = 14, 24
    x = T.Delta(d) * T.rand_tt((2,) * d, r, seed=3)
    fast = T.tt_compress_(x.copy(), r)
    monkeypatch.setenv("TTN_FAST", "0")
    robust = T.tt_compress_(x.copy(), r)
    assert fast.ttv_rks == robust.ttv_rks
    assert tt_rel_diff(to_oracle(fast), to_oracle(robust)) <= 1e-10


@pytest.mark.parametrize("seed", [3, 192])
def test_rank64_route_variants_agree(T, monkeypatch, seed):
    """The rank-64 sweep (128-row Gram steps, the zero-padded 96-row Gram step with or without its Jacobi polish, the
    diagonal-left form of route F) against the same sweep with each shortcut switched off through the diagnostic bits of
    TTN_FAST (csrc/ttn_dense_kernels.h, CompressArgs.fast) and against the all-Householder route: same ranks, tensors to 1e-10."""
    d, r = 16, 64
    A = T.Delta(d)
    x = T.rand_tt((2,) * d, r, seed=seed)
    dA, dx = T.DeviceTTO(A), T.DeviceTT.from_host(x)

    def run():
        dy = T.DeviceTT(x.ttv_dims, [a * b for a, b in zip(A.tto_rks, x.ttv_rks)])
        T.device.apply_compress(dA, dx, dy, r, 0.0, 1)
        T.device.compress_status(dy)
        return dy.download()

    base = run()
    for bits in ("9", "17", "25", "31", "0"):          # 1|8, 1|16, 1|8|16, every eigensolver shortcut off, Householder only
        monkeypatch.setenv("TTN_FAST", bits)
        other = run()
        assert other.ttv_rks == base.ttv_rks, bits
        assert tt_rel_diff(to_oracle(other), to_oracle(base)) <= 1e-10, bits


@pytest.mark.parametrize("dims,oprks,xr,mb", [((2,) * 30, None, 64, 64), ((2, 3, 2, 2, 3, 2, 2), [1, 2, 3, 2, 4, 2, 3, 1], 5, 6),
                                              ((4, 2, 3, 4, 2), [1, 3, 2, 2, 3, 1], 7, 9)])
def test_fused_apply_compress_equals_apply_then_compress(T, monkeypatch, dims, oprks, xr, mb):
    """ttn_apply_compress never writes A*x (the first L->R sweep builds each merged matrix from core k, x_{k+1}, A_{k+1});
    TTN_NOFUSE=1 runs apply and compress separately.  Same ranks, tensors to 1e-10; general dims / operator ranks too,
    and the unfused result is pinned to the oracle."""
    d = len(dims)
    rng = np.random.default_rng(7)
    if oprks is None:
        A = T.Delta(d)
    else:
        A = T.TToperator(d, [np.asfortranarray(rng.standard_normal((dims[k], dims[k], oprks[k], oprks[k + 1]))) for k in range(d)],
                         dims, oprks, [0] * d)
    x = T.rand_tt(dims, xr, seed=11)
    B = 3
    dA, dx = T.DeviceTTO(A), T.DeviceTT.from_host(x, batch=B)
    cap = [a * c for a, c in zip(A.tto_rks, x.ttv_rks)]
    y1, y2 = T.DeviceTT(dims, cap, batch=B), T.DeviceTT(dims, cap, batch=B)
    T.device.apply_compress(dA, dx, y1, mb)
    T.device.compress_status(y1)
    monkeypatch.setenv("TTN_NOFUSE", "1")
    T.device.apply_compress(dA, dx, y2, mb)
    T.device.compress_status(y2)
    monkeypatch.delenv("TTN_NOFUSE")
    ref = O.tt_compress_(O.apply(to_oracle(A), to_oracle(x)), mb) if d <= 12 else None
    for b in (0, B - 1):
        f, u = y1.download(b), y2.download(b)
        assert f.ttv_rks == u.ttv_rks
        assert tt_rel_diff(to_oracle(f), to_oracle(u)) <= 1e-10
        if ref is not None:
            assert u.ttv_rks == ref.ttv_rks and tt_rel_diff(to_oracle(u), ref) <= 1e-9


def test_sweep_ranges_and_core_handoff_reproduce_compress(T):
    """ttn_sweep over 1..d-1 then d-1..1 is tt_compress! (same bond steps, same order: identical cores); cutting the chain at
    a bond and moving the boundary core through ttn_tt_core_export / _import (what pipeline.py sends over RCCL) too."""
    import ctypes as C
    import torch
    d, r, B = 12, 16, 3
    A = T.Delta(d)
    x = T.rand_tt((2,) * d, r, seed=9)
    dA, dx = T.DeviceTTO(A), T.DeviceTT.from_host(x, batch=B)
    cap = [a * c for a, c in zip(A.tto_rks, x.ttv_rks)]
    ref, two = T.DeviceTT((2,) * d, cap, batch=B), T.DeviceTT((2,) * d, cap, batch=B)
    T.device.apply(dA, dx, ref); T.device.tt_compress_(ref, r)
    T.device.apply(dA, dx, two)
    L = T._lib.lib()
    T._lib.check(L.ttn_sweep(two.h, 1, d - 1, r, 0.0))
    # round trip of core 5 through a dense device buffer between the two sweep directions
    n, bl, br = C.c_int64(), C.c_int64(), C.c_int64()
    T._lib.check(L.ttn_tt_core_extent(two.h, 5, C.byref(n), C.byref(bl), C.byref(br)))
    buf = torch.empty((B, n.value), dtype=torch.float64, device="cuda")
    rk2 = torch.empty((B, 2), dtype=torch.int64, device="cuda")
    T._lib.check(L.ttn_tt_core_export(two.h, 5, buf.data_ptr(), rk2.data_ptr()))
    T.device.sync()
    assert rk2.cpu().tolist() == [[int(bl.value), int(br.value)]] * B or all(a <= bl.value and c <= br.value for a, c in rk2.cpu().tolist())
    T._lib.check(L.ttn_tt_core_import(two.h, 5, buf.data_ptr(), rk2.data_ptr(), bl.value, br.value))
    T._lib.check(L.ttn_sweep(two.h, d - 1, 1, r, 0.0))
    T.device.sync()
    for b in range(B):
        a_, b_ = ref.download(b), two.download(b)
        assert a_.ttv_rks == b_.ttv_rks
        for k in range(d):
            assert np.array_equal(a_.ttv_vec[k], b_.ttv_vec[k])
    # argument checking: bond indices are 1-based in 1:(N-1); an import that does not fit the slot is refused
    with pytest.raises(AssertionError):                      # like the reference's @assert 1 <= k < N (tt_tools.jl:744)
        T._lib.check(L.ttn_sweep(two.h, 0, 3, r, 0.0))
    with pytest.raises(T.TTNError):
        T._lib.check(L.ttn_tt_core_import(two.h, 5, buf.data_ptr(), rk2.data_ptr(), 10 ** 6, 1))


# ------------------------------------------------------------------------------------------------
# device-resident caller chains: rk4_method / euler_method of src/solvers/euler.jl on handles
# ------------------------------------------------------------------------------------------------
def test_rk4_and_euler_device_chains(T):
    d, B = 8, 3
    hh = 1 / d ** 2
    A = T.toeplitz_to_qtto(-2.0, 1.0, 1.0, d)
    A.tto_vec[0] = (-hh ** 2) * A.tto_vec[0]
    us = [T.rand_tt((2,) * d, [1, 2, 3, 3, 3, 3, 3, 2, 1], seed=70 + b) for b in range(B)]
    du = T.DeviceTT((2,) * d, us[0].ttv_rks, batch=B)
    for b, u in enumerate(us):
        du.upload(b, u)
    dA = T.DeviceTTO(A)
    steps = [0.05, 0.05, 0.1]
    out = T.solvers.rk4_method(dA, du, steps, 6, normalize=True)
    eul = T.solvers.euler_method(dA, du, steps, normalize=True)
    for b, u in enumerate(us):
        ref = O.rk4_method(to_oracle(A), to_oracle(u), steps, 6, normalize=True)
        got = out.download(b)
        assert got.ttv_rks == ref.ttv_rks
        assert tt_rel_diff(to_oracle(got), ref) <= 1e-9
        assert abs(T.norm(got) - 1.0) < 1e-10
        refe = O.euler_method(to_oracle(A), to_oracle(u), steps, normalize=True)
        gote = eul.download(b)
        assert gote.ttv_rks == refe.ttv_rks and gote.ttv_ot == refe.ttv_ot
        assert tt_rel_diff(to_oracle(gote), refe) <= 1e-10
    # dense check of the RK4 chain for one train and one step, as test/test_euler.jl:269-298 does
    one = T.solvers.rk4_method(dA, T.DeviceTT.from_host(us[0]), [0.05], 8, normalize=False).download(0)
    Ad, ud = O.qtto_to_matrix(to_oracle(A)), T.qtt_to_vector(us[0])
    h = 0.05
    K1 = Ad @ ud; K2 = Ad @ (ud + h / 2 * K1); K3 = Ad @ (ud + h / 2 * K2); K4 = Ad @ (ud + h * K3)
    refv = ud + h / 6 * (K1 + 2 * K2 + 2 * K3 + K4)
    assert np.linalg.norm(T.qtt_to_vector(one) - refv) / np.linalg.norm(refv) < 1e-6


def _dense_op(A):
    return O.qtto_to_matrix(to_oracle(A))


def _nabla(T, d):
    return T.toeplitz_to_qtto(1.0, 0.0, -1.0, d)            # src/tt_operators.jl:276-278


@pytest.mark.parametrize("case", ["cn_gmres_default", "cn_nonsymmetric", "cn_bicgstab_bounded", "ie_cg"])
def test_krylov_linsolve_steppers_match_dense_solves(T, case):
    """krylov_linsolve + crank_nicholson_method / implicit_euler_method with tt_solver="krylov" on handles
    (src/solvers/euler.jl:34-190), checked the way the reference checks them: against the dense solve
    (test/test_euler.jl:105-240: rel error 1e-8, 1e-7 for the bounded BiCGStab case, rank bound).  KrylovKit itself is a
    third-party dependency outside the reference tree: iterates are parity-unpinned, the solution is pinned."""
    from ttn_amd import solvers as S
    rng_seed = {"cn_gmres_default": 1, "cn_nonsymmetric": 2, "cn_bicgstab_bounded": 3, "ie_cg": 4}[case]
    steps = [0.05]
    if case == "cn_gmres_default":
        d, A, kw, bound, tol_err = 4, None, dict(tol=1.0e-12), 0, 1.0e-8
        A = S._tto_scale(0.1, T.Delta(d))
    elif case == "cn_nonsymmetric":
        d = 4
        A, kw, bound, tol_err = S._tto_scale(0.1, _nabla(T, d)), dict(tol=1.0e-12), 0, 1.0e-8
        assert not np.allclose(_dense_op(A), _dense_op(A).T)
    elif case == "cn_bicgstab_bounded":
        d = 5
        A, bound, tol_err = S._tto_scale(0.1, _nabla(T, d)), 8, 1.0e-7
        kw = dict(krylov_solver="bicgstab", maxiter=30, rtol=1.0e-10, atol=1.0e-12)
    else:
        d = 3
        A, bound, tol_err = S._tto_scale(0.1, T.id_tto(d)), 0, 1.0e-8
        kw = dict(isposdef=True, issymmetric=True, tol=1.0e-12)
    B = 2
    u0s = [T.rand_tt((2,) * d, 2, seed=rng_seed * 10 + b) for b in range(B)]
    du = T.DeviceTT((2,) * d, u0s[0].ttv_rks, batch=B)
    for b in range(B):
        du.upload(b, u0s[b])
    if case == "ie_cg":
        sol = S.implicit_euler_method(A, du, du, steps, normalize=False, tt_solver="krylov", **kw)
    else:
        sol = S.crank_nicholson_method(A, du, du, steps, normalize=False, tt_solver="krylov", max_bond=bound, **kw)
    Ad = _dense_op(A)
    I = np.eye(Ad.shape[0])
    for b in range(B):
        ud = O.qtt_to_vector(to_oracle(u0s[b]))
        ref = np.linalg.solve(I - steps[0] * Ad, ud) if case == "ie_cg" else np.linalg.solve(I - 0.5 * steps[0] * Ad, (I + 0.5 * steps[0] * Ad) @ ud)
        got = sol.download(b)
        err = np.linalg.norm(T.qtt_to_vector(got) - ref) / np.linalg.norm(ref)
        assert err < tol_err, (case, b, err)
        if bound:
            assert max(got.ttv_rks) <= bound
    with pytest.raises(ValueError):                              # ArgumentError in the reference (euler.jl:31)
        S.implicit_euler_method(A, du, du, steps, normalize=False, tt_solver="krylov", krylov_solver="unknown")


def test_randomized_apply_compress_parity(T):
    """60 random problems (d 2..10, dims 2..4, x ranks 1..19, operator ranks 1..3, max_bond 1..23, truncerr in {0, 1e-10, 1e-6,
    1e-3}) through the fused ttn_apply_compress: ranks exact, tensor 1e-9 against the oracle.  (tools/diag_fuzz.py runs the
    same generator for any count; 400 cases were clean on the round-1 build.)"""
    rng = np.random.default_rng(1)
    for it in range(60):
        d = int(rng.integers(2, 11))
        dims = tuple(int(v) for v in rng.integers(2, 5, size=d))
        xr = int(rng.integers(1, 20))
        oprks = [1] + [int(v) for v in rng.integers(1, 4, size=d - 1)] + [1]
        A = T.TToperator(d, [np.asfortranarray(rng.standard_normal((dims[k], dims[k], oprks[k], oprks[k + 1]))) for k in range(d)],
                         dims, oprks, [0] * d)
        x = T.rand_tt(dims, xr, seed=int(rng.integers(1, 10 ** 6)))
        mb = int(rng.integers(1, 24))
        te = float(rng.choice([0.0, 0.0, 1e-10, 1e-6, 1e-3]))
        ref = O.tt_compress_(O.apply(to_oracle(A), to_oracle(x)), mb, truncerr=te)
        cap = [a * c for a, c in zip(A.tto_rks, x.ttv_rks)]
        need, _ = T.device.compress_rank_bound(dims, cap, mb)
        dy = T.DeviceTT(dims, [max(a, b) for a, b in zip(cap, need)])
        T.device.apply_compress(T.DeviceTTO(A), T.DeviceTT.from_host(x), dy, mb, te)
        T.device.compress_status(dy)
        got = dy.download()
        assert got.ttv_rks == ref.ttv_rks, (it, dims, xr, oprks, mb, te)
        assert tt_rel_diff(to_oracle(got), ref) <= 1e-9, (it, dims, xr, oprks, mb, te)


# ---- steps that take the symmetric-eigensolver routes (128-row Gram steps keeping <= 64 vectors, 64 x 64 route-F cores) ----------
@pytest.mark.parametrize("d,kind,xr,max_bond,truncerr,seed", [(12, 0, 64, 64, 0.0, 0), (13, 0, 64, 50, 0.0, 1), (12, 1, 64, 33, 0.0, 2),
                                                              (12, 2, 64, 64, 1e-8, 3), (14, 2, 48, 64, 0.0, 4), (12, 0, 64, 20, 1e-12, 5),
                                                              (12, 0, 32, 32, 0.0, 6), (13, 2, 32, 20, 1e-8, 7), (12, 1, 32, 31, 0.0, 8)])
def test_apply_compress_eigen_routes_vs_oracle(T, d, kind, xr, max_bond, truncerr, seed):
    """n = 2, rank-64 inputs: the L->R steps merge to 128 x 384 (Gram + eigensolver, csrc/ttn_eig_kernels.h), the R->L steps are
    route F with a 64 x 64 core (N = 64 eigensolver); rank-32 inputs: 64 x 192 Gram steps on the N = 64 eigensolver.  Same tolerances as the other tt_compress! tests: ranks exact, tensors 1e-9."""
    rng = np.random.default_rng(seed)
    if kind == 0:
        A = O.Delta(d)
    elif kind == 1:
        A = O.tto_add(O.Delta(d), O.tto_scale(0.7, O.shift(d)))
    else:
        A = O.rand_tto((2,) * d, 3, rng)
    x = O.rand_tt((2,) * d, xr, rng)
    ref = O.tt_compress_(O.apply(A, x), max_bond, truncerr=truncerr)
    cap = [a * c for a, c in zip(A.tto_rks, x.ttv_rks)]
    need, _ = T.device.compress_rank_bound((2,) * d, cap, max_bond)
    dy = T.DeviceTT((2,) * d, [max(a, b) for a, b in zip(cap, need)])
    T.device.apply_compress(T.DeviceTTO(to_product(A)), T.DeviceTT.from_host(to_product(x)), dy, max_bond, truncerr)
    T.device.compress_status(dy)
    got = dy.download()
    assert list(got.ttv_rks) == list(ref.ttv_rks)
    assert tt_rel_diff(to_oracle(got), ref) <= 1e-9
