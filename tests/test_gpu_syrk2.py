"""wg_syrk2, the two-team Gram product of route F: the bits of two wg_syrk calls, at the sizes where the pairing can go wrong.

wg_syrk2 gives each of two independent products G_i = alpha_i A_i A_i^T (p_i <= 64) to one half of the workgroup's waves.  Each team
stages chunks of 48 k into its own half of the LDS region (the single form stages 96), the accumulators carry over the chunks, and both
teams run the chunk count of the longer product so that they meet at the same barriers.  So the sizes are: row counts with one to four
16-row tile rows, full and partly filled (1, 15, 16, 17, 63, 64: a team's waves then own 0 ... 3 live tiles, every copy of the loops
runs); depths below one k-step, around the half-chunk edge (47, 48, 49), around the old chunk edge (95, 96, 97) and 128 — paired so that
the two members differ in rows, in depth and in their number of chunks; operands stored transposed or not, mixed; and a member of 65
rows, which the wrapper must hand to two single calls.  Integer data in [-8, 8]: every sum is exact in fp64, so the paired result is
compared for equality with the two single calls (k_selftest_syrk2 with pair = 0, the same launch shape) AND with numpy.  G is
pre-filled with NaN, so an element the leaf does not write shows.  Every case is a single-workgroup launch; both builds."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = [1, 15, 16, 17, 63, 64]
Q = [1, 47, 48, 49, 95, 96, 97, 128]


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _operand(p, q, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(p, q)).astype(np.float64)


def _launch(T, A1, ta1, alpha1, A2, ta2, alpha2, pair):
    """G1, G2 of one k_selftest_syrk2 launch; A_i is p_i x q_i, handed over transposed in memory if ta_i"""
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    (p1, q1), (p2, q2) = A1.shape, A2.shape
    M1 = np.ascontiguousarray(A1.T if ta1 else A1)
    M2 = np.ascontiguousarray(A2.T if ta2 else A2)
    G1, G2 = np.full((p1, p1), np.nan), np.full((p2, p2), np.nan)
    T._lib.check(T._lib.lib().ttn_selftest_syrk2(p1, q1, ptr(M1), ptr(G1), alpha1, int(ta1), p2, q2, ptr(M2), ptr(G2), alpha2, int(ta2), int(pair)))
    return G1, G2


def _check_pair(T, p1, q1, ta1, p2, q2, ta2):
    A1, A2 = _operand(p1, q1, 1000 * p1 + q1), _operand(p2, q2, 500000 + 1000 * p2 + q2)
    G1, G2 = _launch(T, A1, ta1, 0.5, A2, ta2, -0.25, 1)
    S1, S2 = _launch(T, A1, ta1, 0.5, A2, ta2, -0.25, 0)
    what = f"({p1} x {q1}, ta {ta1}) with ({p2} x {q2}, ta {ta2})"
    assert np.array_equal(G1, S1) and np.array_equal(G2, S2), f"{what}: the paired call differs from two single calls"
    assert np.array_equal(G1, 0.5 * (A1 @ A1.T)), f"{what}: first member"
    assert np.array_equal(G2, -0.25 * (A2 @ A2.T)), f"{what}: second member"


@pytest.mark.parametrize("ta2", [0, 1])
@pytest.mark.parametrize("ta1", [0, 1])
@pytest.mark.parametrize("wg512", [0, 1])
def test_syrk2_equals_two_single_calls(T, monkeypatch, wg512, ta1, ta2):
    """every (p1, q1) of the grid as first member; the second member walks the grid at another pace, so the rows always differ and the
    depths and chunk counts mostly do (and agree in a few pairs)"""
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    n = 0
    for i, p1 in enumerate(P):
        for j, q1 in enumerate(Q):
            p2, q2 = P[(i + 1) % len(P)], Q[(3 * j + i + 5) % len(Q)]          # a bijection of the grid: every shape is second member once
            _check_pair(T, p1, q1, ta1, p2, q2, ta2)
            n += (p1 != p2) and (q1 != q2) and ((q1 + 47) // 48 != (q2 + 47) // 48)
    assert n >= 24          # (the walk above does make most pairs unequal in rows, depth and chunk count)


@pytest.mark.parametrize("wg512", [0, 1])
def test_syrk2_same_shape_members_and_the_bond_step_shape(T, monkeypatch, wg512):
    """both members alike (the same barriers for the same reason), and route F's own pair: 64 x 128, the left one stored transposed"""
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    for p, q in [(64, 128), (64, 48), (17, 97), (1, 1)]:
        _check_pair(T, p, q, 1, p, q, 0)


@pytest.mark.parametrize("wg512", [0, 1])
def test_syrk2_falls_back_for_a_tall_member(T, monkeypatch, wg512):
    """65 rows on either side (and on both): the wrapper runs two wg_syrk calls.  A depth of 700 is beyond the offset tables of a team
    in the 512-thread build (two single calls) and 15 chunks against one in the 1024-thread build."""
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    for (p1, q1), (p2, q2) in [((65, 97), (64, 48)), ((16, 49), (65, 128)), ((65, 50), (128, 96)), ((64, 700), (33, 48))]:
        for ta in (0, 1):
            _check_pair(T, p1, q1, ta, p2, q2, 1 - ta)
