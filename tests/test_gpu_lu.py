"""Kernel unit tests of the dense local solve and of the matrix-free two-site operator, through the hooks ttn_selftest_lu_solve and
ttn_selftest_two_site_apply (include/ttn.h).

wg_lu_solve (csrc/ttn_als_kernels.h; what als / mals / dmrg_linsolve run in one workgroup) and the grid-form stages k_lu_panel /
k_lu_rows / k_lu_trail / k_lu_back_* (csrc/ttn_als_grid.h) are Gaussian elimination with partial pivoting in panels of 32 columns.
On random normal systems nearly every step exchanges rows, so a wrong interchange outside the panel, on the right-hand side or in the
global-memory panel path (more than 512 rows left) shows at once:
  * the pivot rows must EQUAL LAPACK's (scipy.linalg.lu_factor) — both take the first row of maximal modulus; that the choice is
    unambiguous is checked on the CPU first: an elimination in numpy.longdouble chooses the same rows, with a relative margin between
    pivot and runner-up far above what fp64 rounding can move (N 2^-53 times the growth, < 1e-11 here);
  * the normwise backward error eta = ||b - K x||_inf / (||K||_inf ||x||_inf + ||b||_inf), evaluated in longdouble, must satisfy
    eta_device <= 4 eta_LAPACK + N 2^-53: both sides run the same elimination on the same pivots and differ in summation order only.
Sizes: around the panel width (31, 32, 33, 64, 65), 513 (every panel but the first in LDS), 544 (two global-memory panels, then LDS
panels), 2048 (the limit of the one-workgroup form).  N <= 33 cannot exchange rows at a step >= 32; every larger case is asserted to.
wg_two_site_apply computes 1/2 (K + K^T) v; on small integers every product and sum is exact in fp64, so the result must equal the
NumPy expression bit for bit, and with non-symmetric G_z, H_z the K and K^T halves differ (asserted), so computing K v twice fails."""
import ctypes as C
import functools
import os
import warnings

import numpy as np
import pytest
import scipy.linalg as sla

from tests.helpers import GOLDEN
from tests.linsolve_reference import LU_NB, backward_error, lu_pivots_longdouble, lu_test_system, matrix_fingerprint

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 31, 32, 33, 64, 65, 100, 257, 512, 513, 544, 1000, 2048)
GRID_SIZES = (33, 100, 544, 1000)
MIN_MARGIN = 1.0e-8          # relative pivot margin demanded of the inputs: > 1e3 x (N 2^-53 x growth) at N = 2048


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _lu_solve(T, K, b, form):
    """(return code, x, pivot rows) of the device LU; K column-major."""
    N = len(b)
    K = np.asfortranarray(K, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros(N)
    piv = np.full(N, -7, dtype=np.int64)
    rc = T._lib.lib().ttn_selftest_lu_solve(N, _p(K), _p(b), _p(x), piv.ctypes.data_as(C.POINTER(C.c_int64)), int(form))
    if rc < 0:
        T._lib.check(rc)
    return rc, x, piv


@functools.lru_cache(maxsize=None)
def _reference(N):
    """The system of size N with LAPACK's pivots, solution and backward error (computed once, shared by the tests below)."""
    K, b = lu_test_system(N)
    lu, piv = sla.lu_factor(K, check_finite=False)
    x = sla.lu_solve((lu, piv), b, check_finite=False)
    for a in (K, b, piv, x):
        a.setflags(write=False)
    return K, b, piv.astype(np.int64), x, backward_error(K, x, b)


@functools.lru_cache(maxsize=None)
def _one_workgroup(T, N):
    K, b, _, _, _ = _reference(N)
    return _lu_solve(T, K, b, 0)


def _longdouble_pivots(N, K):
    if N == 2048:                       # 15 s of longdouble arithmetic: recorded (tests/golden/make_lu_golden.py) and tied to the matrix
        g = np.load(os.path.join(GOLDEN, "lu2048_pivots_longdouble.npz"))
        fp, want = matrix_fingerprint(K), g["fingerprint"]
        if np.array_equal(fp[:4], want[:4]) and np.allclose(fp[4:], want[4:], rtol=1e-12, atol=0.0):
            return g["piv"].astype(np.int64), float(g["margin"])
    return lu_pivots_longdouble(K)


@pytest.mark.parametrize("N", SIZES)
def test_lu_pivots_and_backward_error_vs_lapack(T, N):
    K, b, piv, x_ref, eta_ref = _reference(N)
    steps = np.arange(N)
    beyond = int(np.sum((piv != steps) & (steps >= LU_NB)))
    if N > LU_NB + 1:
        assert beyond > 0, "the input never exchanges rows outside the first panel: the test would prove nothing"
    piv_ld, margin = _longdouble_pivots(N, K)
    assert np.array_equal(piv_ld, piv), "LAPACK's pivot choice is not the exact one: ambiguous input"
    assert margin > MIN_MARGIN, margin
    rc, x, got = _one_workgroup(T, N)
    assert rc == 0
    assert np.array_equal(got, piv), np.flatnonzero(got != piv)[:8]
    eta = backward_error(K, x, b)
    print(f"lu form 0  N={N:5d}  exchanges at steps >= 32: {beyond:4d}  margin {margin:.1e}  eta_device {eta:.3e}  eta_lapack {eta_ref:.3e}  "
          f"ratio {eta / eta_ref:.3f}")
    assert eta <= 4.0 * eta_ref + N * 2.0 ** -53, (eta, eta_ref)


@pytest.mark.parametrize("N", GRID_SIZES)
def test_lu_grid_form_equals_one_workgroup_form(T, N):
    """The grid-form stages on the same systems: identical pivots, x to 1e-12 relative (the bar of
    test_als_grid_form_equals_one_workgroup_form), and the same backward-error bound against LAPACK."""
    K, b, piv, _, eta_ref = _reference(N)
    rc0, x0, piv0 = _one_workgroup(T, N)
    rc, x, got = _lu_solve(T, K, b, 1)
    assert rc == 0 and rc0 == 0
    assert np.array_equal(got, piv0) and np.array_equal(got, piv)
    rel = np.linalg.norm(x - x0) / np.linalg.norm(x0)
    eta = backward_error(K, x, b)
    print(f"lu form 1  N={N:5d}  |x_grid - x_wg| / |x_wg| {rel:.3e}  eta_device {eta:.3e}  eta_lapack {eta_ref:.3e}  ratio {eta / eta_ref:.3f}")
    assert rel <= 1e-12, rel
    assert eta <= 4.0 * eta_ref + N * 2.0 ** -53, (eta, eta_ref)


@pytest.mark.parametrize("N,form", [(40, 0), (40, 1), (600, 0), (600, 1)])
def test_lu_tie_takes_the_first_row_like_idamax(T, N, form):
    """Integer K whose first column holds its maximum modulus twice, with opposite signs: the pivot is the FIRST such row.  N = 40:
    the panel in LDS; N = 600: the global-memory panel."""
    rng = np.random.default_rng(7 + N)
    K = rng.integers(-3, 4, size=(N, N)).astype(np.float64)
    lo, hi = N // 3, (2 * N) // 3
    K[lo, 0], K[hi, 0] = -7.0, 7.0
    assert np.max(np.abs(K[:, 0])) == 7.0 and list(np.flatnonzero(np.abs(K[:, 0]) == 7.0)) == [lo, hi]
    b = rng.integers(-3, 4, size=N).astype(np.float64)
    _, piv = sla.lu_factor(K, check_finite=False)
    assert piv[0] == lo                                         # LAPACK's idamax
    rc, x, got = _lu_solve(T, K, b, form)
    assert rc == 0 and got[0] == lo, (rc, got[0], lo, hi)
    x_ref = sla.solve(K, b)
    assert backward_error(K, x, b) <= 4.0 * backward_error(K, x_ref, b) + N * 2.0 ** -53


@pytest.mark.parametrize("N,col,form", [(64, 40, 0), (64, 40, 1), (600, 5, 0), (600, 5, 1)])
def test_lu_reports_an_exactly_singular_system(T, N, col, form):
    """Column `col` exactly zero — it stays exactly zero through interchanges and updates, so the elimination meets a zero pivot
    column at step `col`: return code 1, the pivots of the steps before it as LAPACK's, none after it, nothing non-finite in x_out.
    N = 64, column 40: an LDS panel (the second); N = 600, column 5: a global-memory panel."""
    rng = np.random.default_rng(11 + N)
    K = rng.standard_normal((N, N))
    K[:, col] = 0.0
    b = rng.standard_normal(N)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # LAPACK reports U[col, col] == 0 as a warning and goes on
        _, piv = sla.lu_factor(K, check_finite=False)
    rc, x, got = _lu_solve(T, K, b, form)
    assert rc == 1
    assert np.all(np.isfinite(x))
    assert np.array_equal(got[:col], piv[:col])
    assert np.all(got[col:] == -1)


@pytest.mark.parametrize("na,nb,Rz", [(1, 1, 1), (2, 3, 1), (6, 4, 3), (17, 33, 5), (64, 64, 4), (130, 70, 2), (256, 256, 6)])
def test_two_site_apply_is_exact_on_integers(T, na, nb, Rz):
    """out = 1/2 (sum_z G_z V H_z^T + sum_z G_z^T V H_z) with G, H, v drawn from the integers in [-4, 4]: every partial sum stays below
    256 * 1536 * 4^3 < 2^53, so fp64 (MFMA included) is exact and the device must reproduce NumPy bit for bit."""
    rng = np.random.default_rng(900 + na + nb + Rz)
    Gz = rng.integers(-4, 5, size=(Rz, na, na)).astype(np.float64)
    Hz = rng.integers(-4, 5, size=(Rz, nb, nb)).astype(np.float64)
    V = rng.integers(-4, 5, size=(na, nb)).astype(np.float64)
    Kv = sum(Gz[z] @ V @ Hz[z].T for z in range(Rz))
    KTv = sum(Gz[z].T @ V @ Hz[z] for z in range(Rz))
    if na * nb > 1:                                             # (a 1 x 1 operator is its own transpose)
        assert any(not np.array_equal(Gz[z], Gz[z].T) for z in range(Rz)) or na == 1
        assert any(not np.array_equal(Hz[z], Hz[z].T) for z in range(Rz)) or nb == 1
        assert not np.array_equal(Kv, KTv), "the K v and K^T v halves coincide: the test could not tell them apart"
    want = 0.5 * (Kv + KTv)
    G = np.asfortranarray(np.transpose(Gz, (1, 2, 0)))          # (na, na, Rz) column-major
    H = np.asfortranarray(Hz)                                   # (Rz, nb, nb), z fastest
    v = np.asfortranarray(V)
    out = np.asfortranarray(np.full((na, nb), np.nan))
    T._lib.check(T._lib.lib().ttn_selftest_two_site_apply(na, nb, Rz, _p(G), _p(H), _p(v), _p(out)))
    assert np.array_equal(out, want), float(np.max(np.abs(out - want)))
