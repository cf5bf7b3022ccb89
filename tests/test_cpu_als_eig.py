"""CPU checks of the one-site eigensolvers: the NumPy restatement (tests/als_eig_reference.py) against exact answers, the history length
of mode 2, and the schedule refusals that come back before anything reaches a device."""
import math

import numpy as np
import pytest
import scipy.linalg as sla

from oracle import tt_oracle as O
from tests import als_eig_reference as AR
from tests.helpers import to_oracle, to_product


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    return ttn_amd


def _spd(d, s):
    return O.tto_add(O.Delta(d), O.tto_scale(s, O.id_tto(d)))


def _full_ranks(d):
    return O.r_and_d_to_rks([1] + [2 ** d] * (d - 1) + [1], (2,) * d, 2 ** d)


@pytest.mark.parametrize("d", [4, 5, 6])
def test_restatement_reaches_min_eig_at_full_ranks(T, d):
    rng = np.random.default_rng(d)
    x0 = O.rand_tt((2,) * d, _full_ranks(d), rng)
    for A in (_spd(d, 0.5), to_oracle(T.ising_tto(d, J=1.0, h=1.5))):
        Ad = O.qtto_to_matrix(A)
        w, v = np.linalg.eigh(Ad)
        E, x = AR.als_eigsolve(A, x0, sweep_schedule=[2])
        assert len(E) == 2 * (d - 1)
        assert abs(E[-1] - w[0]) <= 1e-10 * max(1.0, abs(w[0]))
        assert np.max(np.abs(AR.full_vector(x) - AR._fix_sign(v[:, 0]))) <= 1e-8
    M = O.toeplitz_to_qtto(4 / 6, 1 / 6, 1 / 6, d)
    A = _spd(d, 0.5)
    lam = float(sla.eigh(O.qtto_to_matrix(A), O.qtto_to_matrix(M), eigvals_only=True)[0])
    E, x = AR.als_gen_eigsolv(A, M, x0, sweep_schedule=[2])
    assert abs(E[-1] - lam) <= 1e-10 * max(1.0, abs(lam))
    xv = np.asarray(O.qtt_to_vector(x), dtype=float)
    assert abs(xv @ O.qtto_to_matrix(M) @ xv - 1.0) <= 1e-12


@pytest.mark.parametrize("d", [4, 6])
def test_closed_forms(d):
    """The closed forms the GPU tests check, reached by the restatement with the same ranks and sweeps."""
    rng = np.random.default_rng(10 + d)
    th = math.pi / (2 ** d + 1)
    for s in (0.5, 2.0):
        x0 = O.rand_tt((2,) * d, 4, rng)
        E, _ = AR.als_eigsolve(_spd(d, s), x0, sweep_schedule=[4])
        assert abs(E[-1] - (2 - 2 * math.cos(th) + s)) <= 1e-10
        E, x = AR.als_gen_eigsolv(_spd(d, s), O.toeplitz_to_qtto(4 / 6, 1 / 6, 1 / 6, d), x0, sweep_schedule=[4])
        assert abs(E[-1] - 6 * (2 - 2 * math.cos(th) + s) / (4 + 2 * math.cos(th))) <= 1e-10


def test_identity_metric_gives_the_standard_history(T):
    """S = I: the same history.  (The local solutions must have full rank at the chosen ranks: a rank-deficient V leaves the QR free in
    rounding-level directions, and the two runs walk apart from there.)"""
    rng = np.random.default_rng(3)
    d = 5
    A = to_oracle(T.ising_tto(d, J=1.0, h=1.5))
    x0 = O.rand_tt((2,) * d, 3, rng)
    E1, x1 = AR.als_eigsolve(A, x0, sweep_schedule=[3])
    E2, x2 = AR.als_gen_eigsolv(A, O.id_tto(d), x0, sweep_schedule=[3])
    assert len(E1) == len(E2) == 2 * (d - 1) * 2
    assert np.max(np.abs(np.array(E1) - np.array(E2))) <= 1e-10
    assert np.max(np.abs(AR.full_vector(x1) - AR.full_vector(x2))) <= 1e-8


def test_rank_growth_zero_padding():
    """A [1, 2] / [2, 4] schedule: the ranks follow r_and_d_to_rks(fill(rmax)) and the energy keeps improving."""
    rng = np.random.default_rng(4)
    d = 5
    A = _spd(d, 1.0)
    x0 = O.rand_tt((2,) * d, 2, rng)
    E, x = AR.als_eigsolve(A, x0, sweep_schedule=[2, 4], rmax_schedule=[2, 4])
    assert x.ttv_rks == [1, 2, 4, 4, 2, 1]
    assert len(E) == 2 * (d - 1) * 3
    assert E[-1] <= E[2 * (d - 1) - 1] + 1e-12
    E, x = AR.als_eigsolve(A, O.rand_tt((2,) * d, 1, rng), sweep_schedule=[1, 2], rmax_schedule=[1, 2])
    assert x.ttv_rks == [1, 2, 2, 2, 2, 1] and len(E) == 2 * (d - 1)


@pytest.mark.parametrize("d,ss", [(2, [2]), (4, [3]), (5, [1, 2]), (6, [2, 4, 7])])
def test_history_len_mode2(T, d, ss):
    assert T.solvers.eigsolve_history_len(2, d, ss) == 2 * (d - 1) * (ss[-1] - 1)


def test_refusals_before_the_device(T):
    d = 4
    A = T.Delta(d)
    S = T.id_tto(d)
    x0 = to_product(O.rand_tt((2,) * d, 2, np.random.default_rng(1)))
    for fn, args, extra in ((T.als_eigsolve, (A, x0), {"noise_schedule": None}), (T.als_gen_eigsolv, (A, S, x0), {})):
        with pytest.raises(T.TTNError, match="Sweep schedule error"):
            fn(*args, sweep_schedule=[2, 4], rmax_schedule=[4])
        with pytest.raises(T.TTNError):
            fn(*args, sweep_schedule=[2, 2], rmax_schedule=[2, 4])
        with pytest.raises(T.TTNError):
            fn(*args, sweep_schedule=[0], rmax_schedule=[4])
        with pytest.raises(T.TTNError, match="too low"):
            fn(*args, sweep_schedule=[2, 4], rmax_schedule=[2, 2])
    with pytest.raises(T.TTNError, match="Sweep schedule error"):
        T.als_eigsolve(A, x0, sweep_schedule=[2, 4], rmax_schedule=[2, 4], noise_schedule=[0.0])
    # d < 2
    x1 = to_product(O.rand_tt((4,), 1, np.random.default_rng(2)))
    A1 = to_product(O.id_tto(2))
    A1 = type(A1)(1, [np.eye(4).reshape(4, 4, 1, 1)], (4,), [1, 1], [0])
    for fn, args in ((T.als_eigsolve, (A1, x1)), (T.als_gen_eigsolv, (A1, A1, x1))):
        with pytest.raises(T.TTNError, match="two sites"):
            fn(*args)
    # start ranks beyond what orthogonalize keeps, and a core too flat for the QR moves
    big = O.rand_tt((2,) * d, [1, 3, 4, 2, 1], np.random.default_rng(3))
    flat = O.rand_tt((2,) * d, [1, 1, 4, 2, 1], np.random.default_rng(4))
    for fn, pre in ((T.als_eigsolve, (A,)), (T.als_gen_eigsolv, (A, S))):
        with pytest.raises(T.TTNError, match="orthogonalize"):
            fn(*pre, to_product(big))
        with pytest.raises(T.TTNError, match="flat"):
            fn(*pre, to_product(flat))
