"""Pins tests/resite_reference.py, the NumPy restatement of to_qtt / to_ttv that tests/test_gpu_resite.py compares the device against.
No GPU.  The identities are exact in exact arithmetic; 1e-12 relative leaves two orders above the 5e-14 measured for these shapes
(a handful of 24 x 20 SVDs and products in fp64)."""
import numpy as np
import pytest

from tests import resite_reference as R

DIMS, RKS, SPLITS = (8, 6, 4), (1, 5, 3, 1), [[2, 2, 2], [3, 2], [4]]


@pytest.fixture(scope="module")
def x():
    return R.random_train(DIMS, RKS, seed=11)


def _flat(sd):
    return [f for s in sd for f in s]


def test_to_qtt_is_the_c_order_split_of_every_axis(x):
    full = R.dense(x)
    q = R.to_qtt(x, SPLITS)
    assert q.ttv_dims == tuple(_flat(SPLITS))
    assert q.ttv_rks == [1, 2, 4, 5, 6, 3, 1]                    # min(rows, cols) of every unfolding
    err = np.max(np.abs(R.dense(q) - full.reshape(_flat(SPLITS))))
    assert err <= 1e-12 * np.max(np.abs(full)), err


def test_non_palindromic_factors_tell_coarse_from_fine():
    x = R.random_train((12, 6, 4), RKS, seed=12)
    sd = [[2, 3, 2], [3, 2], [4]]
    full = R.dense(x)
    got = R.dense(R.to_qtt(x, sd))
    assert np.max(np.abs(got - full.reshape(_flat(sd)))) <= 1e-12 * np.max(np.abs(full))
    # the little-endian reading of the same lists (first factor least significant) is a different tensor
    little = np.stack([full[:, j, k].reshape((2, 3, 2), order="F") for j in range(6) for k in range(4)], axis=-1).reshape(2, 3, 2, 3, 2, 4)
    assert np.max(np.abs(got - little)) > 1e-3


def test_round_trip_reproduces_the_tensor(x):
    back = R.to_ttv(R.to_qtt(x, SPLITS), [len(s) for s in SPLITS])
    assert back.ttv_dims == DIMS and back.ttv_rks == list(RKS)
    assert np.max(np.abs(R.dense(back) - R.dense(x))) <= 1e-12 * np.max(np.abs(R.dense(x)))


def test_to_ttv_merges_big_endian(x):
    y = R.to_ttv(x, [2, 1])
    assert y.ttv_dims == (48, 4) and y.ttv_rks == [1, 3, 1]
    assert np.max(np.abs(R.dense(y) - R.dense(x).reshape(48, 4))) <= 1e-12 * np.max(np.abs(R.dense(x)))


def test_threshold_finds_the_rank_of_a_sum_of_angles():
    # sin(x + y + z) on three 8-point sites has TT ranks (1, 2, 2, 1); every binary split keeps rank 2
    t = np.arange(8) / 8.0
    c0 = np.stack([np.sin(t), np.cos(t)], axis=1)[:, None, :]                                        # (8, 1, 2): [sin x, cos x]
    c1 = np.stack([np.stack([np.cos(t), -np.sin(t)], axis=1), np.stack([np.sin(t), np.cos(t)], axis=1)], axis=1)   # rotation by y
    c2 = np.stack([np.cos(t), np.sin(t)], axis=1)[:, :, None]                                        # (8, 2, 1)
    x = R.Train([c0, c1, c2])
    full = R.dense(x)
    assert np.max(np.abs(full - np.sin(t[:, None, None] + t[None, :, None] + t[None, None, :]))) <= 1e-14
    sd = [[2, 2, 2]] * 3
    q = R.to_qtt(x, sd, threshold=1e-10)
    assert q.ttv_rks == [1] + [2] * 8 + [1]
    assert np.max(np.abs(R.dense(q) - full.reshape((2,) * 9))) <= 1e-12
    assert R.to_qtt(x, sd).ttv_rks == [1, 2, 4, 2, 4, 4, 2, 4, 2, 1]


def test_edge_lists():
    x = R.random_train((4,), (1, 1), seed=13)
    q = R.to_qtt(x, [[1, 4]])
    assert q.ttv_dims == (1, 4) and q.ttv_rks == [1, 1, 1]
    assert np.max(np.abs(R.dense(q).reshape(4) - R.dense(x))) <= 1e-14
    assert np.array_equal(R.to_qtt(x, [[4]]).ttv_vec[0], x.ttv_vec[0])
