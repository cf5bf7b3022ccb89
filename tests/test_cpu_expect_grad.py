"""The NumPy restatement of the three-layer pullback of <x, A y> (tests/expect_grad_reference.py) — the yardstick of
tests/test_gpu_expect_grad.py — pinned without a GPU: against the composition of the two existing rules through H * psi
(tests/grad_reference.py), against central differences at the tolerance of tests/test_cpu_grad.py, the Euler identity of a multilinear
form, and the fused Rayleigh gradient against the composed one.  Also the exports, the header and the loud failure of the host wrappers."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import expect_grad_reference as ER
from tests import grad_reference as GR
from tests.test_cpu_expect import mixed_case
from tests.test_cpu_grad import _close, _dirs, _fd, _rand_op, _rayleigh_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = ER.EPS


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    return ttn_amd


def mixed5_case():
    """dims (3, 2, 4, 2, 3) with a non-symmetric operator."""
    rng = np.random.default_rng(30)
    dims = (3, 2, 4, 2, 3)
    return O.rand_tt(dims, [1, 3, 5, 4, 2, 1], rng), _rand_op(dims, [1, 2, 3, 3, 2, 1], rng), O.rand_tt(dims, [1, 2, 7, 3, 3, 1], rng)


def qtt_case():
    rng = np.random.default_rng(31)
    dims = (2,) * 7
    return O.rand_tt(dims, 5, rng), O.rand_tto(dims, 3, rng), O.rand_tt(dims, 6, rng)


CASES = {"mixed": mixed_case, "mixed5": mixed5_case, "qtt": qtt_case}


def _within(got, ref, bound):
    for g, r, b in zip(got, ref, bound):
        assert g.shape == r.shape
        assert np.all(np.abs(g - r) <= b), float(np.max(np.abs(g - r) / np.maximum(b, 1e-300)))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_composition_through_apply(name):
    """xbar is Abar of the dot pullback on (x, A y); ybar is the apply pullback of its Bbar — each within the sum of the bounds: the
    three-layer bound, the dot pullback's, the apply pullback's, and the dot pullback's bound on Bbar carried through |A|."""
    x, A, y = CASES[name]()
    delta = -0.6
    s, xb, yb = ER.sandwich_pullback(x, A, y, delta)
    bs, bx, by = ER.sandwich_pullback_bound(x, A, y, delta)
    Ay = O.apply(A, y)
    v, abar, bbar = GR.dot_pullback(x, Ay, delta)
    bv, ba, bbb = GR.dot_pullback_bound(x, Ay, delta)
    assert abs(s - v) <= bs + bv
    _within(xb, abar, [p + q for p, q in zip(bx, ba)])
    yref = GR.apply_pullback(A, bbar, y.ttv_rks)
    carried = GR.apply_pullback(ER._abs_tto(A), bbb, y.ttv_rks)
    own = GR.apply_pullback_bound(A, bbar, y.ttv_rks)
    _within(yb, yref, [p + q + r for p, q, r in zip(by, own, carried)])
    # the tangents have the shapes of the cores and the environments meet in s at every bond
    assert [c.shape for c in xb] == [c.shape for c in x.ttv_vec] and [c.shape for c in yb] == [c.shape for c in y.ttv_vec]
    L, G = ER.environments(x, A, y)
    for k in range(x.N + 1):
        assert abs(float(np.sum(L[k] * G[k])) - s) <= 2 * bs


@pytest.mark.parametrize("name", list(CASES))
def test_central_differences(name):
    x, A, y = CASES[name]()
    rng = np.random.default_rng(41)
    _, xb, yb = ER.sandwich_pullback(x, A, y, 1.0)
    dx, dy = _dirs(x, rng), _dirs(y, rng)
    fx = _fd(lambda t: O.dot(t, O.apply(A, y)), x, dx)
    fy = _fd(lambda t: O.dot(x, O.apply(A, t)), y, dy)
    print(name, "AD", GR.ladot(xb, dx), "FD", fx, "| AD", GR.ladot(yb, dy), "FD", fy)
    assert _close(GR.ladot(xb, dx), fx) and _close(GR.ladot(yb, dy), fy)
    # the cotangent scales both
    _, x2, y2 = ER.sandwich_pullback(x, A, y, -0.37)
    assert all(np.allclose(a, -0.37 * b, rtol=1e-14, atol=0) for a, b in zip(x2 + y2, xb + yb))


@pytest.mark.parametrize("name", list(CASES))
def test_euler_identity(name):
    """s is linear in every core: sum_k <x_k, xbar_k> = N delta s, and the same for y — N pairings, each another order of the sum s."""
    x, A, y = CASES[name]()
    delta = 0.8
    s, xb, yb = ER.sandwich_pullback(x, A, y, delta)
    bs = ER.sandwich_pullback_bound(x, A, y, delta)[0]
    for cores, bar in ((x.ttv_vec, xb), (y.ttv_vec, yb)):
        assert abs(GR.ladot(cores, bar) - x.N * delta * s) <= x.N * abs(delta) * 2 * bs


@pytest.mark.parametrize("case", [0, 1, 2])
def test_fused_rayleigh_equals_the_composed_one(case):
    name, H, psi = list(_rayleigh_cases())[case]
    E, g = ER.rayleigh_value_and_grad(H, psi)
    Er, gr = GR.rayleigh_value_and_grad(H, psi)
    assert abs(E - Er) <= 1e-13 * max(1.0, abs(Er))
    bound = ER.rayleigh_composed_bound(H, psi)
    _within(g, gr, [2 * b for b in bound])                # both sides are restatements here: each side of each form rounds
    share = max(float(np.max(np.abs(a - b)[c > 0] / c[c > 0])) for a, b, c in zip(g, gr, bound))
    print(name, "largest share of the composed bound", share)
    ev, eg = ER.expect_value_and_grad(H, psi)
    assert abs(ev - O.dot(psi, O.apply(H, psi))) <= 1e-13 * O.norm(psi) * O.norm(O.apply(H, psi))
    _, xb, yb = ER.sandwich_pullback(psi, H, psi)
    assert all(np.array_equal(a, b + c) for a, b, c in zip(eg, xb, yb))


def test_exports_header_and_loud_failure_without_gpu(T):
    for name in ("sandwich_pullback", "expect_value_and_grad", "sandwich_rrule", "rayleigh_value_and_grad", "rayleigh_gradient"):
        assert name in T.__all__ and callable(getattr(T, name)) and getattr(T, name) is getattr(T.grad, name)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttn_expect_grad.h")).read(), flags=re.S)
    protos = re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert {n for n, _ in protos} == set(T._lib.EXPECT_GRAD_SIGNATURES) == {"ttn_sandwich_pullback"}
    others = set(T._lib.SIGNATURES) | set(T._lib.RECT_SIGNATURES) | set(T._lib.DENSE_SIGNATURES) | set(T._lib.STEP_SIGNATURES)\
        | set(T._lib.CROSS_BATCH_SIGNATURES) | set(T._lib.EXPECT_SIGNATURES)
    assert not set(T._lib.EXPECT_GRAD_SIGNATURES) & others
    lib = T._lib.lib()
    for name, args in protos:
        res, argt = T._lib.EXPECT_GRAD_SIGNATURES[name]
        assert res is ctypes.c_int and hasattr(lib, name) and len(args.split(",")) == len(argt) == 7
    assert '#include "ttn_expect_grad.h"' in open(os.path.join(ROOT, "include", "ttn.h")).read()
    import torch
    if torch.cuda.is_available():
        return
    x, A = T.rand_tt((2,) * 4, 3, seed=1), T.Delta(4)
    for call in (lambda: T.sandwich_rrule(x, A, x), lambda: T.rayleigh_gradient(A, x, fused=True)):
        with pytest.raises(T.TTNError):
            call()
