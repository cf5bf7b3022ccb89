"""CPU tests of the fixed-rank manifold layer (no GPU): the NumPy restatement (tests/tangent_reference.py) — the yardstick of
tests/test_gpu_tangent.py — against a dense projector built from the Jacobian of the train map, the algebraic properties of an orthogonal
projector, the reference's Manopt extension pinned to the assertions of test/test_manopt.jl, and the entry points' header, ctypes table,
exports and refusals that need no device.

Tolerances: every quantity below is a sum of at most a few hundred products of O(1) numbers in Float64, compared with another
evaluation order of the same sum: 1e-12 of the scale of the operands leaves three decimal digits over p eps (p < 1e3)."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import tangent_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, RANKS = (2, 3, 2, 2), [1, 2, 3, 2, 1]
TOL = 1e-12


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    return ttn_amd


@pytest.fixture(scope="module")
def setup():
    rng = np.random.default_rng(11)
    x = O.rand_tt(DIMS, RANKS, rng)
    U, V = R.gauges(x)
    assert U.ttv_rks == RANKS and V.ttv_rks == RANKS
    z = O.rand_tt(DIMS, [1, 2, 5, 2, 1], rng)
    w = O.rand_tt(DIMS, [1, 1, 2, 2, 1], rng)
    return x, U, V, z, w, R.dense_projector(x)


def vec(t):
    return O.ttv_to_tensor(t).reshape(-1)


def test_gauges_reproduce_the_point(setup):
    x, U, V, *_ = setup
    xv = vec(x)
    assert np.max(np.abs(vec(U) - xv)) <= TOL * np.max(np.abs(xv))
    assert np.max(np.abs(vec(V) - xv)) <= TOL * np.max(np.abs(xv))
    for k in range(x.N - 1):                              # U_k^T U_k = 1 in the left unfolding, V_k V_k^T = 1 in the right one
        Uk = U.ttv_vec[k].reshape(-1, RANKS[k + 1])
        assert np.max(np.abs(Uk.T @ Uk - np.eye(RANKS[k + 1]))) <= TOL
        Vk = V.ttv_vec[k + 1]
        gram = np.einsum("zxa,zya->xy", Vk, Vk)
        assert np.max(np.abs(gram - np.eye(RANKS[k + 1]))) <= TOL


def test_dense_projector_is_a_projector_of_the_manifold_dimension(setup):
    x, *_, P = setup
    assert np.max(np.abs(P @ P - P)) <= TOL and np.max(np.abs(P - P.T)) <= TOL
    assert round(np.trace(P)) == R.manifold_dimension(DIMS, RANKS)


def test_restatement_against_the_dense_projector(setup):
    x, U, V, z, w, P = setup
    for t in (z, w, x):
        cores, val = R.project(U, V, t)
        want = P @ vec(t)
        got = R.tangent_dense(U, V, cores).reshape(-1)
        scale = np.max(np.abs(vec(t)))
        err = np.max(np.abs(got - want))
        print(f"ranks {t.ttv_rks}: |P z - dense| / max|z| {err / scale:.2e}")
        assert err <= TOL * scale
        assert abs(val - float(np.dot(vec(x), vec(t)))) <= TOL * np.linalg.norm(vec(x)) * np.linalg.norm(vec(t))
        for k in range(x.N - 1):                          # the gauge condition
            g = np.einsum("zxa,zxb->ab", U.ttv_vec[k], cores[k])
            assert np.max(np.abs(g)) <= TOL * scale * np.max(np.abs(vec(x)))


def test_projection_is_idempotent_and_fixes_the_point(setup):
    x, U, V, z, _, _ = setup
    c1, _ = R.project(U, V, z)
    c2, _ = R.project(U, V, R.to_tt(U, V, c1, 0.0, 1.0))
    scale = max(np.max(np.abs(c)) for c in c1)
    assert all(np.max(np.abs(a - b)) <= TOL * scale for a, b in zip(c1, c2))
    cx, val = R.project(U, V, x)                          # P x = x: dC_d = U_d, the rest zero
    sx = np.max(np.abs(U.ttv_vec[-1]))
    assert np.max(np.abs(cx[-1] - U.ttv_vec[-1])) <= TOL * sx
    assert all(np.max(np.abs(c)) <= TOL * sx for c in cx[:-1])
    assert abs(val - O.dot(x, x)) <= TOL * O.dot(x, x)


def test_projection_is_self_adjoint_and_cores_dot_is_the_inner_product(setup):
    x, U, V, z, w, P = setup
    cz, _ = R.project(U, V, z)
    cw, _ = R.project(U, V, w)
    zv, wv = vec(z), vec(w)
    scale = np.linalg.norm(zv) * np.linalg.norm(wv)
    pz, pw = R.tangent_dense(U, V, cz).reshape(-1), R.tangent_dense(U, V, cw).reshape(-1)
    assert abs(np.dot(pz, wv) - np.dot(zv, pw)) <= TOL * scale
    assert abs(R.tangent_inner(cz, cw) - np.dot(pz, pw)) <= TOL * scale
    assert abs(R.tangent_inner(cz, cw) - np.dot(P @ zv, P @ wv)) <= TOL * scale


@pytest.mark.parametrize("alpha,beta", [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (-0.75, 2.5)])
def test_to_tt_against_dense(setup, alpha, beta):
    x, U, V, z, _, P = setup
    cz, _ = R.project(U, V, z)
    y = R.to_tt(U, V, cz, alpha, beta)
    assert y.ttv_rks == [1, 4, 6, 4, 1]
    want = alpha * vec(x) + beta * (P @ vec(z))
    assert np.max(np.abs(vec(y) - want)) <= TOL * (abs(alpha) * np.max(np.abs(vec(x))) + abs(beta) * np.max(np.abs(vec(z))))
    # the off-diagonal block is an explicit zero, the copies are copies
    for k in (1, 2):
        rl, rr = RANKS[k], RANKS[k + 1]
        W = y.ttv_vec[k]
        assert not W[:, :rl, rr:].any()
        assert np.array_equal(W[:, :rl, :rr], V.ttv_vec[k]) and np.array_equal(W[:, rl:, rr:], U.ttv_vec[k]) and np.array_equal(W[:, rl:, :rr], cz[k])


def test_to_tt_and_project_at_one_site():
    rng = np.random.default_rng(3)
    x, z = O.rand_tt((5,), [1, 1], rng), O.rand_tt((5,), [1, 1], rng)
    U, V = R.gauges(x)
    c, val = R.project(U, V, z)                           # the tangent space of a one-site train is the whole space
    assert np.max(np.abs(c[0] - z.ttv_vec[0])) <= TOL * np.max(np.abs(z.ttv_vec[0]))
    assert abs(val - O.dot(x, z)) <= TOL * O.norm(x) * O.norm(z)
    y = R.to_tt(U, V, c, 2.0, -3.0)
    assert y.ttv_rks == [1, 1] and np.max(np.abs(y.ttv_vec[0] - (2.0 * x.ttv_vec[0] - 3.0 * z.ttv_vec[0]))) <= 1e-14 * 25


def test_retract_restatement(setup):
    x, U, V, z, _, _ = setup
    cz, _ = R.project(U, V, z)
    y = R.retract(U, V, cz, 0.0)
    assert y.ttv_rks == RANKS
    assert np.max(np.abs(vec(y) - vec(x))) <= TOL * np.max(np.abs(vec(x)))
    y = R.retract(U, V, cz, 1e-3)
    assert y.ttv_rks == RANKS
    # a retraction agrees with x + t xi to first order: the remainder is O(t^2)
    lin = vec(x) + 1e-3 * R.tangent_dense(U, V, cz).reshape(-1)
    assert np.max(np.abs(vec(y) - lin)) <= 1e-4 * np.max(np.abs(vec(x)))


def test_project_bound_covers_a_perturbed_evaluation(setup):
    """The bound is 2 p eps times the formula on absolute values: it is positive wherever the projection can be non-zero and far above
    the difference of two evaluation orders of the same sums."""
    x, U, V, z, _, _ = setup
    cz, val = R.project(U, V, z)
    vb, cb = R.project_bound(U, V, z)
    zz = O.TTvector(z.N, [np.asfortranarray(c) for c in z.ttv_vec], z.ttv_dims, z.ttv_rks, z.ttv_ot)
    L, G = R.chains(U, V, zz)
    for k in range(x.N):                                  # another order: G first
        M = np.einsum("zyb,ab->zya", z.ttv_vec[k], G[k + 1])
        o = np.einsum("xy,zya->zxa", L[k], M)
        if k < x.N - 1:
            o = o - np.einsum("zxa,ac->zxc", U.ttv_vec[k], L[k + 1] @ G[k + 1].T)
        assert np.all(np.abs(o - cz[k]) <= cb[k])
        assert cb[k].shape == cz[k].shape and np.all(cb[k] > 0)
    assert vb > 0


# ---- the reference's Manopt extension: test/test_manopt.jl ------------------------------------------------------------------------------
def test_reference_surface_pinned_to_test_manopt():
    target = O.orthogonalize(O.qtt_sin(4))
    M = R.ttvector_manifold(target)
    assert M.dims == tuple(target.ttv_dims) and M.ranks == target.ttv_rks and M.ranks is not target.ttv_rks       # :8-10
    t3 = O.orthogonalize(O.qtt_sin(3))
    assert R.ttvector_manifold(t3).representation_size() == tuple(t3.ttv_dims)                                      # :16
    z = M.zero_vector(target)                                                                                        # :29-35
    assert tuple(z.ttv_dims) == tuple(target.ttv_dims) and z.ttv_rks == target.ttv_rks and not any(c.any() for c in z.ttv_vec)
    assert O.norm(O.sub(M.copy(target), target)) < 1e-14                                                              # :52-54
    p, q = target, O.orthogonalize(O.qtt_sin(4, lam=2 * np.pi))                                                       # :66-82
    inner = M.inner(p, p, p)
    assert np.isclose(inner, O.dot(p, p)) and inner >= 0
    assert np.isclose(M.norm(p, p), np.sqrt(inner))
    dist = M.distance(p, q)
    assert np.isclose(dist, M.norm(p, O.sub(p, q))) and dist >= 0
    assert M.distance(p, p) < 1e-14
    X = O.copy_tt(p)                                                                                                  # :86-104
    assert O.norm(O.sub(M.retract_project(p, X), O.orthogonalize(O.add(p, X)))) < 1e-12
    assert O.norm(O.sub(M.retract_project(p, X, 0.5), O.orthogonalize(O.add(p, O.scale(0.5, X))))) < 1e-12
    assert O.norm(O.sub(M.retract_project(p, X, 0.0), O.orthogonalize(p))) < 1e-12


def test_reference_gradient_descent_case():
    """test_manopt.jl:107-129: three steps x <- retract_project(x, -(x - target)) from the zero train reach the target at < 1e-6."""
    target = O.orthogonalize(O.qtt_sin(4))
    M = R.ttvector_manifold(target)
    x = O.zeros_tt(target.ttv_dims, target.ttv_rks)
    for _ in range(3):
        x = M.retract_project(x, O.sub(x, target), -1.0)
    err = O.norm(O.sub(x, target)) / O.norm(target)
    print(f"gradient descent: ||x - target|| / ||target|| = {err:.2e}")
    assert err < 1e-6


def test_restated_drivers_reach_their_ends():
    """The two drivers as tests/test_gpu_tangent.py runs them: the fixed point reaches the target, the descent is monotone at fixed ranks."""
    target = O.qtt_sin(6)
    for seed in (1, 2):
        x0 = O.rand_tt((2,) * 6, target.ttv_rks, np.random.default_rng(seed))
        x, errs = R.fit_fixed_rank(target, x0, 12)
        print(f"fit_fixed_rank seed {seed}: " + " ".join(f"{e:.1e}" for e in errs))
        assert x.ttv_rks == target.ttv_rks and errs[-1] < 1e-6
    A = O.Delta(5)
    x0 = O.rand_tt((2,) * 5, 2, np.random.default_rng(5))
    x0 = O.scale(1.0 / O.norm(x0), x0)
    x, en = R.rayleigh_descent(A, x0, 20, 0.25, backtrack=True)
    assert x.ttv_rks == x0.ttv_rks and len(en) == 21
    assert all(b <= a for a, b in zip(en, en[1:])) and en[-1] < en[0]


# ---- header, ctypes table, exports, refusals --------------------------------------------------------------------------------------------
def test_tangent_header_and_ctypes_table_agree(T):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttn_tangent.h")).read(), flags=re.S)
    protos = re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert {n for n, _ in protos} == set(T._lib.TANGENT_SIGNATURES) == {"ttn_tangent_project", "ttn_tangent_to_tt"}
    others = set()
    for name in dir(T._lib):
        if name.endswith("SIGNATURES") and name != "TANGENT_SIGNATURES":
            others |= set(getattr(T._lib, name))
    assert "ttn_dot_pullback" in others and not set(T._lib.TANGENT_SIGNATURES) & others
    lib = T._lib.lib()
    for name, args in protos:
        res, argt = T._lib.TANGENT_SIGNATURES[name]
        assert res is ctypes.c_int and hasattr(lib, name)
        assert len(args.split(",")) == len(argt) == {"ttn_tangent_project": 5, "ttn_tangent_to_tt": 6}[name]
    assert '#include "ttn_tangent.h"' in open(os.path.join(ROOT, "include", "ttn.h")).read()
    api = open(os.path.join(ROOT, "tensortrainnumerics.jl_amd", "csrc", "ttn_api.hip")).read()
    assert '#include "ttn_host_tangent.h"' in api and '#include "ttn_tangent_kernels.h"' in api


def test_exports_and_host_side_refusals(T):
    for name in ("ttvector_manifold", "TTManifold", "TTPoint", "fit_fixed_rank", "rayleigh_descent", "tangent_project"):
        assert name in T.__all__ and callable(getattr(T, name))
    assert callable(T.manifold.retract)
    x = T.qtt_sin(4)
    M = T.ttvector_manifold(x)
    assert M.dims == tuple(x.ttv_dims) and M.ranks == list(x.ttv_rks) and M.ranks is not x.ttv_rks
    assert M.representation_size() == (2, 2, 2, 2)
    z = M.zero_vector(x)
    assert list(z.ttv_rks) == list(x.ttv_rks) and not any(c.any() for c in z.ttv_vec)
    with pytest.raises(T.TTNError, match="not feasible"):
        T.TTManifold((2, 2, 2), [1, 3, 2, 1])
    with pytest.raises(T.TTNError, match="not compatible"):
        T.TTManifold((2, 2, 2), [1, 2, 1])
    with pytest.raises(TypeError):
        T.ttvector_manifold(np.zeros(3))
    with pytest.raises(TypeError):
        M.gauge(x)                                         # a host train: the fixed-rank surface works on handles
    import torch
    if torch.cuda.is_available():
        cores, val = T.tangent_project(x, x)
        assert abs(val - float(T.dot(x, x))) <= 1e-12 * float(T.dot(x, x))
        return
    for call in (lambda: T.tangent_project(x, x), lambda: T.manifold.retract(x, x.ttv_vec, 0.5), lambda: M.inner(x, x, x)):
        with pytest.raises(T.TTNError):                    # no device: a loud failure, never a CPU fallback
            call()
