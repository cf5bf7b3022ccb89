"""GPU checks of als_eigsolve / als_gen_eigsolv (csrc/ttn_als_eig_kernels.h): the reference's cases (test/test_als.jl) through the device,
parity with the NumPy restatement (tests/als_eig_reference.py) on the dense local branch, closed forms (the shifted QTT Laplacian, the
pencil with the consistent mass matrix, the free-fermion Ising chain above the dense limit), the matrix-free branches against the dense
one, batch = single calls bitwise, rank growth, and the refusals."""
import math

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import als_eig_reference as AR
from tests import eig_reference as ER
from tests.helpers import to_oracle, to_product

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _spd(d, s):
    return O.tto_add(O.Delta(d), O.tto_scale(s, O.id_tto(d)))


def _mass(d):
    return O.toeplitz_to_qtto(4 / 6, 1 / 6, 1 / 6, d)


def _std(T, A, x0, **kw):
    E, x = T.als_eigsolve(to_product(A), to_product(x0), **kw)
    return E, to_oracle(x)


def _gen(T, A, S, x0, **kw):
    E, x = T.als_gen_eigsolv(to_product(A), to_product(S), to_product(x0), **kw)
    return E, to_oracle(x)


def _vec(x):
    return np.asarray(O.qtt_to_vector(x), dtype=float)


def _dir_diff(a, b):
    """Distance of two vectors up to a global sign (a sign fix by the largest entry is ambiguous where two entries tie in modulus)."""
    return min(np.max(np.abs(a - b)), np.max(np.abs(a + b)))


def test_reference_cases(T):
    """test/test_als.jl (als_eigsolve / als_gen_eigsolv) through the device."""
    rng = np.random.default_rng(21)
    d = 4
    x0 = O.rand_tt((2,) * d, [1, 2, 2, 2, 1], rng)
    A = _spd(d, 3.0)
    for E, x in (_std(T, A, x0, sweep_schedule=[2]), _gen(T, A, O.id_tto(d), x0, sweep_schedule=[2])):
        assert all(isinstance(v, float) for v in E) and len(E) == 2 * (d - 1)
        assert x.N == d and tuple(x.ttv_dims) == (2,) * d and x.ttv_ot == [0, 1, 1, 1]
        rq = O.dot(x, O.apply(A, x)) / O.dot(x, x)
        assert E[-1] > 0 and math.isclose(rq, E[-1], rel_tol=1e-10)
    E, _ = _std(T, _spd(d, 2.0), x0, sweep_schedule=[4])
    assert E[-1] <= E[0] + 1e-12
    x1 = O.rand_tt((2,) * d, [1] * 5, rng)
    for run in (lambda **k: _std(T, _spd(d, 2.0), x1, **k), lambda **k: _gen(T, _spd(d, 2.0), _mass(d), x1, **k)):
        E, x = run(sweep_schedule=[1, 2], rmax_schedule=[1, 2])
        assert x.ttv_rks == [1, 2, 2, 2, 1] and len(E) == 2 * (d - 1) and all(np.isfinite(E))
        E, x = run(sweep_schedule=[2, 4], rmax_schedule=[2, 4])
        assert max(x.ttv_rks) <= 4 and len(E) == 2 * (d - 1) * 3 and all(np.isfinite(E))
    E, _ = _std(T, _spd(d, 2.0), x0, sweep_schedule=[2], it_solver=True, itslv_thresh=1)
    assert all(np.isfinite(E))
    E, _ = _gen(T, _spd(d, 2.0), _mass(d), x0, sweep_schedule=[2], it_solver=True, itslv_thresh=1)
    assert all(np.isfinite(E))


def _ops(T, d):
    # ranks at which the local solutions have full rank (a rank-deficient V leaves the QR free in rounding-level directions)
    return [(_spd(d, 0.5), 2), (to_oracle(T.ising_tto(d, J=1.0, h=1.5)), 3), (to_oracle(T.xxz_tto(d, J=1.0, Delta=0.5, h=0.3)), 3)]


@pytest.mark.parametrize("d", [3, 5, 8])
def test_dense_parity_with_restatement(T, d):
    rng = np.random.default_rng(100 + d)
    for A, r in _ops(T, d):
        x0 = O.rand_tt((2,) * d, r, rng)
        E, x = _std(T, A, x0, sweep_schedule=[3])
        Er, xr = AR.als_eigsolve(A, x0, sweep_schedule=[3])
        assert len(E) == len(Er)
        assert np.max(np.abs(np.array(E) - Er) / np.maximum(1.0, np.abs(Er))) <= 1e-10
        assert _dir_diff(_vec(x), _vec(xr)) <= 1e-8
        M = _mass(d)
        E, x = _gen(T, A, M, x0, sweep_schedule=[3])
        Er, xr = AR.als_gen_eigsolv(A, M, x0, sweep_schedule=[3])
        assert np.max(np.abs(np.array(E) - Er) / np.maximum(1.0, np.abs(Er))) <= 1e-10
        v, vr = _vec(x), _vec(xr)
        assert _dir_diff(v, vr) <= 1e-8


@pytest.mark.parametrize("d", [4, 6])
def test_closed_forms(T, d):
    rng = np.random.default_rng(10 + d)
    th = math.pi / (2 ** d + 1)
    for s in (0.5, 2.0):
        x0 = O.rand_tt((2,) * d, 4, rng)
        E, _ = _std(T, _spd(d, s), x0, sweep_schedule=[4])
        assert abs(E[-1] - (2 - 2 * math.cos(th) + s)) <= 1e-10
        M = _mass(d)
        E, x = _gen(T, _spd(d, s), M, x0, sweep_schedule=[4])
        assert abs(E[-1] - 6 * (2 - 2 * math.cos(th) + s) / (4 + 2 * math.cos(th))) <= 1e-10
        v = _vec(x)
        assert abs(v @ O.qtto_to_matrix(M) @ v - 1.0) <= 1e-12


def test_matrix_free_against_dense(T):
    rng = np.random.default_rng(5)
    d = 6
    A = to_oracle(T.ising_tto(d, J=1.0, h=1.5))
    x0 = O.rand_tt((2,) * d, 4, rng)
    Ed, _ = _std(T, A, x0, sweep_schedule=[3])
    El, _ = _std(T, A, x0, sweep_schedule=[3], it_solver=True, itslv_thresh=1)
    assert T.solvers.eigsolve_stats(1)[0][0] > 0
    assert abs(El[-1] - Ed[-1]) <= 1e-8 * abs(Ed[-1])
    M = _mass(d)
    Ed, _ = _gen(T, A, M, x0, sweep_schedule=[3])
    El, x = _gen(T, A, M, x0, sweep_schedule=[3], it_solver=True)
    its, res = T.solvers.eigsolve_stats(1)
    assert its[0] > 0 and res[0] <= 1e-5
    assert abs(El[-1] - Ed[-1]) <= 1e-8 * abs(Ed[-1])
    v = _vec(x)
    assert abs(v @ O.qtto_to_matrix(M) @ v - 1.0) <= 1e-10


def test_above_the_dense_limit(T):
    """Rank 33 at n = 2: local problems of 2 * 32 * 33 = 2112 unknowns go to Lanczos / LOBPCG whatever the threshold."""
    d = 12
    rng = np.random.default_rng(33)
    A = to_oracle(T.ising_tto(d, J=1.0, h=1.5))
    e0 = ER.free_fermion_ground_energy(d, 1.0, 1.5)
    x0 = O.rand_tt((2,) * d, 33, rng)
    E, _ = _std(T, A, x0, sweep_schedule=[3])
    assert T.solvers.eigsolve_stats(1)[0][0] > 0
    assert abs(E[-1] - e0) <= 1e-8 * abs(e0)
    S = O.tto_scale(2.0, O.id_tto(d))
    E, _ = _gen(T, A, S, x0, sweep_schedule=[3])
    assert T.solvers.eigsolve_stats(1)[0][0] > 0
    assert abs(E[-1] - e0 / 2) <= 1e-8 * abs(e0)


def _batch_vs_single(T, gen, A, S, starts, cap, **kw):
    dA = T.DeviceTTO(to_product(A))
    dS = T.DeviceTTO(to_product(S)) if gen else None
    dims = tuple(starts[0].ttv_dims)
    x0 = T.DeviceTT(dims, cap, batch=len(starts))
    for b, s in enumerate(starts):
        x0.upload(b, to_product(s))
    x = T.DeviceTT(dims, cap, batch=len(starts))
    Eb = T.solvers.als_gen_eigsolv_(dA, dS, x0, x, **kw) if gen else T.solvers.als_eigsolve_(dA, x0, x, **kw)
    for b, s in enumerate(starts):
        y0 = T.DeviceTT.from_host(to_product(s), cap_rks=cap)
        y = T.DeviceTT(dims, cap)
        E1 = T.solvers.als_gen_eigsolv_(dA, dS, y0, y, **kw) if gen else T.solvers.als_eigsolve_(dA, y0, y, **kw)
        assert E1[0] == Eb[b]
        xb, x1 = to_oracle(x.download(b)), to_oracle(y.download(0))
        assert xb.ttv_rks == x1.ttv_rks
        assert all(np.array_equal(p, q) for p, q in zip(xb.ttv_vec, x1.ttv_vec))


def test_batch_equals_single_calls(T):
    rng = np.random.default_rng(9)
    d = 6
    A = to_oracle(T.ising_tto(d, J=1.0, h=1.5))
    starts = [O.rand_tt((2,) * d, 3, rng), O.rand_tt((2,) * d, 2, rng), O.rand_tt((2,) * d, [1, 2, 3, 2, 2, 2, 1], rng)]
    cap = [1, 2, 4, 4, 4, 2, 1]
    _batch_vs_single(T, False, A, None, starts, cap, sweep_schedule=[2, 4], rmax_schedule=[3, 4], noise_schedule=[0.0, 1e-2], seed=7)
    _batch_vs_single(T, False, A, None, starts, cap, sweep_schedule=[3], rmax_schedule=[3], it_solver=True, itslv_thresh=1)
    _batch_vs_single(T, True, A, _mass(d), starts, cap, sweep_schedule=[2, 4], rmax_schedule=[3, 4])
    _batch_vs_single(T, True, A, _mass(d), starts, cap, sweep_schedule=[3], rmax_schedule=[3], it_solver=True)


def test_noise_zero_is_exact_padding(T):
    d = 5
    rng = np.random.default_rng(12)
    th = math.pi / (2 ** d + 1)
    A = _spd(d, 1.0)
    x0 = O.rand_tt((2,) * d, 1, rng)
    E, x = _std(T, A, x0, sweep_schedule=[2, 6], rmax_schedule=[1, 3], noise_schedule=[0.0, 0.0])
    Er, xr = AR.als_eigsolve(A, x0, sweep_schedule=[2, 6], rmax_schedule=[1, 3])
    assert x.ttv_rks == xr.ttv_rks == [1, 2, 3, 3, 2, 1]
    assert len(E) == len(Er)
    assert np.max(np.abs(np.array(E[: 2 * (d - 1)]) - Er[: 2 * (d - 1)])) <= 1e-10       # the stage before the increase
    assert abs(E[-1] - (2 - 2 * math.cos(th) + 1.0)) <= 1e-10
    E, x = _std(T, A, x0, sweep_schedule=[2, 6], rmax_schedule=[1, 3], noise_schedule=[0.0, 1e-3], seed=3)
    assert x.ttv_rks == [1, 2, 3, 3, 2, 1] and abs(E[-1] - (2 - 2 * math.cos(th) + 1.0)) <= 1e-10


def test_refusals_and_statuses(T):
    d = 4
    rng = np.random.default_rng(13)
    A = to_product(_spd(d, 1.0))
    x0h = to_product(O.rand_tt((2,) * d, 2, rng))
    dA = T.DeviceTTO(A)
    x0 = T.DeviceTT.from_host(x0h)
    small = T.DeviceTT((2,) * d, [1, 2, 2, 2, 1])
    with pytest.raises(T.TTNError, match="capacity"):
        T.solvers.als_eigsolve_(dA, x0, small, sweep_schedule=[2, 3], rmax_schedule=[2, 4])
    with pytest.raises(T.TTNError, match="capacity"):
        T.solvers.als_gen_eigsolv_(dA, T.DeviceTTO(to_product(O.id_tto(d))), x0, small, sweep_schedule=[2, 3], rmax_schedule=[2, 4])
    neg = T.DeviceTTO(to_product(O.tto_scale(-1.0, O.id_tto(d))))
    for it in (False, True):
        x = T.DeviceTT((2,) * d, [1, 2, 2, 2, 1])
        with pytest.raises(T.TTNError, match="positive definite"):
            T.solvers.als_gen_eigsolv_(dA, neg, x0, x, sweep_schedule=[2], it_solver=it)
    other = T.DeviceTT.from_host(to_product(O.rand_tt((2,) * (d + 1), 2, rng)))
    with pytest.raises((T.TTNError, AssertionError), match="Incompatible"):
        T.solvers.als_eigsolve_(T.DeviceTTO(to_product(_spd(d + 1, 1.0))), x0, T.DeviceTT((2,) * d, [1, 2, 2, 2, 1]))
    with pytest.raises((T.TTNError, AssertionError), match="Incompatible"):
        T.solvers.als_eigsolve_(dA, other, T.DeviceTT((2,) * (d + 1), [1, 2, 2, 2, 2, 1]))
    with pytest.raises((T.TTNError, AssertionError), match="batch"):
        T.solvers.als_eigsolve_(dA, x0, T.DeviceTT((2,) * d, [1, 2, 2, 2, 1], batch=2))
    # the solver still works after the refusals
    E, _ = T.als_eigsolve(A, x0h, sweep_schedule=[3])
    assert abs(E[-1] - np.linalg.eigvalsh(O.qtto_to_matrix(_spd(d, 1.0)))[0]) <= 1e-10
