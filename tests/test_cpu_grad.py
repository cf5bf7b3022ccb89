"""The NumPy restatement of the core gradients (tests/grad_reference.py) against the reference's own AD tests (test/test_ad.jl): directional
central finite differences at eps = 1e-6 with rtol 1e-5, atol 1e-7 (test_ad.jl:39, :113), the N = 1 closed form (:89-101) and the fixed-rank
gradient descent (:116-156) at 200 steps.  No GPU: this pins the yardstick the device tests (tests/test_gpu_grad.py) compare against."""
import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import grad_reference as GR
from tests.helpers import to_oracle

FD_EPS, RTOL, ATOL = 1.0e-6, 1.0e-5, 1.0e-7


def _close(a, b):
    return abs(a - b) <= ATOL + RTOL * abs(b)


def _fd(f, x, dirs):
    return (f(GR.shifted(x, dirs, FD_EPS)) - f(GR.shifted(x, dirs, -FD_EPS))) / (2 * FD_EPS)


def _dirs(x, rng):
    return [rng.standard_normal(c.shape) for c in x.ttv_vec]


def _rand_op(dims, rks, rng):
    return O.TToperator(len(dims), [rng.standard_normal((dims[k], dims[k], rks[k], rks[k + 1])) for k in range(len(dims))], tuple(dims),
                        list(rks), [0] * len(dims))


def _ising(d):
    import ttn_amd as T
    return to_oracle(T.ising_tto(d, J=-1.0, h=-0.5, interaction="z", field="x"))


def test_dot_rule_vs_finite_difference():
    rng = np.random.default_rng(1)
    dims = (3, 2, 4, 2, 3)
    A = O.rand_tt(dims, [1, 3, 5, 4, 2, 1], rng)
    B = O.rand_tt(dims, [1, 2, 7, 3, 3, 1], rng)
    val, abar, bbar = GR.dot_pullback(A, B, 1.0)
    assert abs(val - O.dot(A, B)) <= 1e-12 * O.norm(A) * O.norm(B)
    da, db = _dirs(A, rng), _dirs(B, rng)
    fa, fb = _fd(lambda a: O.dot(a, B), A, da), _fd(lambda b: O.dot(A, b), B, db)
    print("dot rule: rel", abs(GR.ladot(abar, da) - fa) / abs(fa), abs(GR.ladot(bbar, db) - fb) / abs(fb))
    assert _close(GR.ladot(abar, da), fa) and _close(GR.ladot(bbar, db), fb)
    # the cotangent scales both
    _, a2, b2 = GR.dot_pullback(A, B, -0.37)
    assert all(np.allclose(x, -0.37 * y, rtol=1e-14, atol=0) for x, y in zip(a2 + b2, abar + bbar))


def test_dot_of_apply_vs_finite_difference():
    """dot(c, H * psi) with respect to psi: the two rules chained."""
    rng = np.random.default_rng(2)
    dims = (3, 2, 4, 2)
    H = _rand_op(dims, [1, 2, 3, 2, 1], rng)
    psi = O.rand_tt(dims, [1, 3, 4, 2, 1], rng)
    c = O.rand_tt(dims, [1, 2, 5, 3, 1], rng)
    _, _, ybar = GR.dot_pullback(c, O.apply(H, psi), 1.0)
    g = GR.apply_pullback(H, ybar, psi.ttv_rks)
    dirs = _dirs(psi, rng)
    fd = _fd(lambda x: O.dot(c, O.apply(H, x)), psi, dirs)
    print("dot(c, H psi): rel", abs(GR.ladot(g, dirs) - fd) / abs(fd))
    assert _close(GR.ladot(g, dirs), fd)


def _rayleigh_cases():
    rng = np.random.default_rng(3)
    yield "ising4", _ising(4), O.rand_tt((2,) * 4, [1, 2, 2, 2, 1], rng)
    dims = (3, 2, 4, 2, 3)
    yield "mixed", _rand_op(dims, [1, 3, 3, 3, 3, 1], rng), O.rand_tt(dims, [1, 3, 5, 4, 2, 1], rng)
    yield "delta6", O.Delta(6), O.rand_tt((2,) * 6, [1, 2, 4, 8, 4, 2, 1], rng)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_rayleigh_gradient_vs_finite_difference(case):
    name, H, psi = list(_rayleigh_cases())[case]
    rng = np.random.default_rng(40 + case)
    E, g = GR.rayleigh_value_and_grad(H, psi)
    assert abs(E - GR.rayleigh(H, psi)) <= 1e-13 * max(1.0, abs(E))
    dirs = _dirs(psi, rng)
    fd = _fd(lambda x: GR.rayleigh(H, x), psi, dirs)
    print(name, "rel", abs(GR.ladot(g, dirs) - fd) / abs(fd))
    assert _close(GR.ladot(g, dirs), fd)


def test_n1_closed_form():
    """test_ad.jl:89-101: for one site the per-core gradient is the Hilbert gradient (2 / <psi, psi>) (H psi - E psi)."""
    rng = np.random.default_rng(5)
    X = np.array([[0.0, 1.0], [1.0, 0.0]])
    H = O.TToperator(1, [(-0.5 * X).reshape(2, 2, 1, 1)], (2,), [1, 1], [0])
    psi = O.rand_tt((2,), [1, 1], rng)
    E, g = GR.rayleigh_value_and_grad(H, psi)
    nn = O.dot(psi, psi)
    ana = (2 / nn) * (O.apply(H, psi).ttv_vec[0] - E * psi.ttv_vec[0])
    assert np.allclose(g[0].ravel(), ana.ravel(), rtol=1e-8, atol=1e-10)


def descent_setup():
    """Ising n = 10, J = -1, h = -0.5, three rank-6 starts, and the exact ground energy of the 1024 x 1024 Hamiltonian."""
    H = _ising(10)
    starts = [O.rand_tt((2,) * 10, 6, np.random.default_rng(700 + s)) for s in range(3)]
    E_exact = float(np.linalg.eigvalsh(O.qtto_to_matrix(H))[0])
    return H, starts, E_exact


def check_descent(hist, E_exact):
    assert all(b <= a + 1e-9 for a, b in zip(hist, hist[1:])), "an accepted step raised the energy"
    assert hist[-1] < hist[0] - 1.0
    assert hist[-1] > E_exact - 1e-6
    assert hist[-1] < E_exact + 0.2


def test_descent_reaches_the_ground_energy():
    """test_ad.jl:116-156 at 200 steps, from the three starts the device test uses."""
    H, starts, E_exact = descent_setup()
    for psi0 in starts:
        hist, _ = GR.descend(H, psi0, steps=200)
        print("descent: E0 %.4f -> %.6f, exact %.6f" % (hist[0], hist[-1], E_exact))
        check_descent(hist, E_exact)
