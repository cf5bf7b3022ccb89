"""The SYRK and register-A leaves at the sizes where their batched fragment reads can go wrong, both builds, exact on integers.

wg_syrk_impl picks one copy of its loops per number of live tiles of a wave and reads its fragments through a ring of registers that
runs a whole number of rounds per staged chunk; wg_gemm_ra_impl runs its k-steps in straight-line groups of eight picked once per
call.  So the sizes are: SYRK row counts that give waves 0 ... MAXT live tiles in either form (p = 16 ... 64 and 80 ... 128: every copy
of the loops runs) times depths around the chunk edges (48 and 96), below one k-step and with k-step remainders; register-A depths
in and around every group of eight k-steps (up to 32, 64, 96, 128: each of the four groups runs) and with k-step remainders, row counts
with idle and partly filled waves, widths around the column chunks.  Integer data in [-8, 8]: the
products are exact in fp64, so the comparison with numpy is for equality; C is pre-filled with NaN, so an element the leaf does not
write, or an accumulator it should not have stored, shows.  Every case is one single-workgroup launch of k_selftest_gemm."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SYRK_P = [16, 48, 64, 80, 112, 128]          # 64: the two-tile copy of the <= 64-row form (rounds of three k-steps)
SYRK_Q = [1, 3, 4, 47, 48, 49, 95, 97, 100]
RA_M = [1, 16, 17, 48, 64]
RA_K = [4, 5, 31, 33, 60, 64, 95, 96, 97, 100, 127, 128]     # 65 ... 96: the group of 24 k-steps
RA_N = [64, 65, 95, 97, 130]


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _launch(T, m, n, k, A, B, alpha, flag):
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    Cc = np.full((m, n), np.nan)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    T._lib.check(T._lib.lib().ttn_selftest_gemm(m, n, k, p(A), p(B), p(Cc), alpha, 0.0, int(flag), 0))
    return Cc


@pytest.mark.parametrize("q", SYRK_Q)
@pytest.mark.parametrize("p", SYRK_P)
@pytest.mark.parametrize("ta", [0, 1])
@pytest.mark.parametrize("wg512", [0, 1])
def test_syrk_edges_exact(T, monkeypatch, wg512, ta, p, q):
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    rng = np.random.default_rng(1000 * p + 10 * q + ta)
    A = rng.integers(-8, 9, size=(p, q)).astype(np.float64)
    got = _launch(T, p, p, q, A.T if ta else A, np.zeros((q, p)), 0.5, 2 | ta)      # ta & 1: A stored q x p
    assert np.array_equal(got, 0.5 * (A @ A.T))


@pytest.mark.parametrize("n", RA_N)
@pytest.mark.parametrize("k", RA_K)
@pytest.mark.parametrize("m", RA_M)
@pytest.mark.parametrize("wg512", [0, 1])
def test_register_a_edges_exact(T, monkeypatch, wg512, m, k, n):
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    rng = np.random.default_rng(100000 * m + 1000 * k + n)
    A = rng.integers(-8, 9, size=(m, k)).astype(np.float64)
    B = rng.integers(-8, 9, size=(k, n)).astype(np.float64)
    got = _launch(T, m, n, k, A, B, -1.5, 4)
    assert np.array_equal(got, -1.5 * (A @ B))
