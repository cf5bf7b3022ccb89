"""wg_gemm_ra2, the two-team register-A product of route F: the bits of two wg_gemm_ra calls, at the sizes where the pairing can go wrong.

wg_gemm_ra2 gives each of two independent products C_i = alpha_i A_i B_i (m_i, k_i <= 64, n_i >= 64) to one team of four waves of the
512-thread build: a wave keeps the A fragments of its 16-row tile in 16 registers, B streams through the team's half of the LDS region
in chunks of 32 columns, the wave multiplies both 16-column groups of a chunk, and both teams run the chunk count of the wider product.
So the sizes are: row counts with idle and partly filled waves (1, 16, 17, 64); depths below one k-step, with k-step remainders, in
and around the first group of eight k-steps and the second (1, 3, 4, 5, 31, 32, 33, 64); widths around the column groups and chunks
(64, 65, 96, 127, 128) — paired so that the members differ in rows, depth and number of chunks; and the shapes the wrapper must hand
to two single calls: k = 65, n = 63.  The operands are passed as route F passes them — the left product with A, B and C transposed,
the right one with A transposed — and the other way round.  Integer data in [-8, 8]: every sum is exact in fp64, so the paired
result is compared for equality with the two single calls (k_selftest_gemm_ra2 with pair = 0) AND with numpy.  C is pre-filled with
NaN, so an element the leaf does not write shows.  Single-workgroup launches, both builds (the 1024-thread build has no register-A
form: there the wrapper is two general products, checked on a part of the grid)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = [1, 16, 17, 64]
K = [1, 3, 4, 5, 31, 32, 33, 64]
N = [64, 65, 96, 127, 128]


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _launch(T, members, pair):
    """members: two (A (m x k), B (k x n), alpha, f); returns C1, C2 (m x n) of one k_selftest_gemm_ra2 launch"""
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    args, outs, keep = [], [], []
    for A, B, alpha, f in members:
        (m, k), n = A.shape, B.shape[1]
        As = np.ascontiguousarray(A.T if f & 1 else A)
        Bs = np.ascontiguousarray(B.T if f & 2 else B)
        Cs = np.full((n, m) if f & 4 else (m, n), np.nan)
        keep += [As, Bs]                    # alive until the call returns
        outs.append((Cs, f))
        args += [m, n, k, ptr(As), ptr(Bs), ptr(Cs), alpha, int(f)]
    T._lib.check(T._lib.lib().ttn_selftest_gemm_ra2(*args, int(pair)))
    return [np.ascontiguousarray(Cs.T) if f & 4 else Cs for Cs, f in outs]


def _check_pair(T, s1, f1, s2, f2):
    (m1, k1, n1), (m2, k2, n2) = s1, s2
    rng = np.random.default_rng(100000 * m1 + 1000 * k1 + n1 + 7 * m2 + 13 * k2)
    mk = lambda m, k, n: (rng.integers(-8, 9, size=(m, k)).astype(np.float64), rng.integers(-8, 9, size=(k, n)).astype(np.float64))
    (A1, B1), (A2, B2) = mk(m1, k1, n1), mk(m2, k2, n2)
    members = [(A1, B1, -1.5, f1), (A2, B2, 0.25, f2)]
    G1, G2 = _launch(T, members, 1)
    S1, S2 = _launch(T, members, 0)
    what = f"({m1} x {n1} x {k1}, f {f1}) with ({m2} x {n2} x {k2}, f {f2})"
    assert np.array_equal(G1, S1) and np.array_equal(G2, S2), f"{what}: the paired call differs from two single calls"
    assert np.array_equal(G1, -1.5 * (A1 @ B1)), f"{what}: first member"
    assert np.array_equal(G2, 0.25 * (A2 @ B2)), f"{what}: second member"


def _grid():
    """every shape of the grid as first member and, by a bijection, once as second member: rows and depth always differ, the width
    mostly does"""
    for i, m in enumerate(M):
        for j, k in enumerate(K):
            for l, n in enumerate(N):
                yield (m, k, n), (M[(i + 1) % len(M)], K[(3 * j + 3) % len(K)], N[(2 * l + 1) % len(N)])


@pytest.mark.parametrize("f1,f2", [(7, 1), (1, 7), (0, 2)])
def test_gemm_ra2_equals_two_single_calls_wg512(T, monkeypatch, f1, f2):
    monkeypatch.setenv("TTN_WG512_SELFTEST", "1")
    pairs = list(_grid())
    assert len({b for _, b in pairs}) == len(pairs) == len(M) * len(K) * len(N)
    assert sum(a[1] != b[1] and (a[2] + 31) // 32 != (b[2] + 31) // 32 for a, b in pairs) >= len(pairs) // 3      # unequal depth AND chunk count
    for s1, s2 in pairs:
        _check_pair(T, s1, f1, s2, f2)


def test_gemm_ra2_wrapper_in_the_1024_thread_build(T, monkeypatch):
    monkeypatch.setenv("TTN_WG512_SELFTEST", "0")
    for s1, s2 in list(_grid())[::7]:
        _check_pair(T, s1, 7, s2, 1)


@pytest.mark.parametrize("wg512", [0, 1])
def test_gemm_ra2_same_shape_members_and_the_bond_step_shape(T, monkeypatch, wg512):
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    for s in [(64, 64, 128), (64, 64, 64), (17, 33, 97), (1, 1, 64)]:
        _check_pair(T, s, 7, s, 1)


@pytest.mark.parametrize("wg512", [0, 1])
def test_gemm_ra2_falls_back(T, monkeypatch, wg512):
    """k = 65 or n = 63 (or 65 rows) on either side: the wrapper runs two wg_gemm_ra calls"""
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    for s1, s2 in [((64, 65, 128), (64, 64, 128)), ((16, 32, 96), (17, 65, 65)), ((64, 64, 63), (64, 64, 64)), ((33, 5, 127), (1, 4, 63)),
                   ((65, 64, 128), (64, 64, 128))]:
        _check_pair(T, s1, 7, s2, 1)
        _check_pair(T, s1, 1, s2, 7)
