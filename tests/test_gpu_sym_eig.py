"""GPU unit tests of wg_sym_eig_smallest (csrc/ttn_eigsolve_kernels.h), the dense symmetric eigen routine of the two-site eigensolvers,
through ttn_selftest_sym_eig: the k smallest eigenpairs against numpy.linalg.eigh, with residuals and orthogonality, on random, diagonal
(split tridiagonal), zero and scaled identity, repeated and clustered, Wilkinson, identical-block, arrow (thick-restart shaped), weakly
coupled tridiagonal, graded and negative definite matrices, scaled by 1e+-100, for N up to TTN_DENSE_LOCAL_MAX = 2048 and k up to 11 (the
thick restart's TTN_LZ_KEEP + 1).  Tolerances (relative to ||A||_2): 1e-13 for N <= 256, 1e-12 above; vectors in a cluster are judged by
their invariant subspace (tests/sym_eig_reference.check_eigpairs)."""
import ctypes as C

import numpy as np
import pytest

from tests import sym_eig_reference as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _eig(T, A, k):
    """(lam[k], Y[N, k]) from the device."""
    N = A.shape[0]
    Acm = np.ascontiguousarray(np.asarray(A, dtype=np.float64).T)        # column-major
    lam = np.zeros(k)
    Y = np.zeros(N * k)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    T._lib.check(T._lib.lib().ttn_selftest_sym_eig(N, k, p(Acm), p(lam), p(Y)))
    return lam, Y.reshape(k, N).T


def _tol(N):
    return 1e-13 if N <= 256 else 1e-12


def _check(T, name, A, ks, w=None, U=None):
    N = A.shape[0]
    if w is None:
        w, U = np.linalg.eigh(A)
    for k in ks:
        if k > N:
            continue
        lam, Y = _eig(T, A, k)
        msg = SR.check_eigpairs(A, k, lam, Y, _tol(N), w, U)
        assert msg is None, "%s N=%d k=%d: %s" % (name, N, k, msg)


@pytest.mark.parametrize("N", [1, 2, 3, 4, 29, 30, 31, 64, 255, 256])
def test_families(T, N):
    rng = np.random.default_rng(1000 + N)
    for name, A in SR.families(N, rng):
        _check(T, name, A, (1, 2, 6, 11))


def test_families_1000(T):
    for name, A in SR.families(1000, np.random.default_rng(1999)):
        _check(T, name, A, (1, 2, 6, 11))


def test_families_2048(T):
    """The cheaper family subset (random, diagonal, zero, c I, multiplicity 2 and 3, one cluster) at k = 1 (the dense branch) and k = 11
    (the largest restart): every k and family here took 52 s, mostly host eigh of 2048."""
    for name, A in SR.families(2048, np.random.default_rng(2048), heavy=False):
        _check(T, name, A, (1, 11))


def test_repeated_smallest_diag(T):
    """diag(1, 1, 2, 3, 4, 5), k = 2: the tridiagonal splits, lambda = 1 comes twice and inverse iteration from the common start returns
    the same vector twice.  Before collapsed vectors were recomputed, the second one was 0/0 = NaN."""
    A = np.diag([1.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    lam, Y = _eig(T, A, 2)
    assert np.all(np.isfinite(Y)), Y
    assert SR.check_eigpairs(A, 2, lam, Y, 1e-13) is None
    assert np.max(np.abs(Y[2:, :])) <= 1e-30 and lam[0] == 1.0 and lam[1] == 1.0
    lam, Y = _eig(T, np.zeros((6, 6)), 2)
    assert np.all(np.isfinite(Y)) and np.max(np.abs(Y.T @ Y - np.eye(2))) <= 1e-13


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_wilkinson(T, sign):
    """+-W21+: -W21+ starts with its closest pair (gap below 1e-13)."""
    _check(T, "wilkinson", sign * SR.wilkinson_plus(10), (1, 2, 6, 11))


@pytest.mark.parametrize("c", [1e100, 1e-100])
def test_scale_equivariance(T, c):
    """Eigenvalues of c A are c times those of A (to the tolerance), the vectors span the same subspaces, and the scaled problem passes
    the same checks."""
    rng = np.random.default_rng(7)
    for name, A in SR.families(64, rng)[:1] + [("wilkinson", SR.wilkinson_plus(10)), ("neg", -SR.wilkinson_plus(10))]:
        N = A.shape[0]
        k = 6
        l1, Y1 = _eig(T, A, k)
        l2, Y2 = _eig(T, c * A, k)
        nrm = float(np.max(np.abs(np.linalg.eigvalsh(A))))
        assert np.max(np.abs(l2 / c - l1)) <= 1e-13 * nrm, name
        _check(T, name, c * A, (k,))
        assert np.all(np.isfinite(Y2)), name
        if name == "random":                                 # separated eigenvalues: the vectors agree up to sign
            assert np.max(np.abs(np.abs(np.sum(Y1 * Y2, axis=0)) - 1.0)) <= 1e-12, name


def test_bitwise_repeatable(T):
    rng = np.random.default_rng(3)
    fam = dict(SR.families(256, rng))
    for name, k in (("random", 11), ("mult3", 6), ("diag_112345", 2), ("cluster1e-14", 6), ("zero", 11)):
        l1, Y1 = _eig(T, fam[name], k)
        l2, Y2 = _eig(T, fam[name], k)
        assert np.array_equal(l1, l2) and np.array_equal(Y1, Y2), name


def test_refusals(T):
    A = np.zeros(16)
    lam = np.zeros(16)
    Y = np.zeros(16 * 16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = T._lib.lib()
    for N, k in ((0, 1), (2049, 1), (3, 4), (40, 17), (4, 0)):
        assert L.ttn_selftest_sym_eig(N, k, p(A), p(lam), p(Y)) == T._lib.TTN_ERR_ARG
