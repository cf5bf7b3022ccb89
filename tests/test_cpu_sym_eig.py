"""CPU checks of the NumPy restatement of wg_sym_eig_smallest (tests/sym_eig_reference.py) with the tolerances of the device test
(tests/test_gpu_sym_eig.py), the defect the restart of collapsed vectors fixes, and the self-test's argument refusals."""
import numpy as np
import pytest

from tests import sym_eig_reference as SR


@pytest.mark.parametrize("N", [1, 2, 3, 4, 6, 29, 31])
def test_restatement_families(N):
    rng = np.random.default_rng(900 + N)
    for name, A in SR.families(N, rng):
        w, U = np.linalg.eigh(A)
        for k in (1, 2, 6, 11):
            if k > N:
                continue
            lam, Y = SR.sym_eig_smallest(A, k)
            msg = SR.check_eigpairs(A, k, lam, Y, 1e-13, w, U)
            assert msg is None, "%s N=%d k=%d: %s" % (name, N, k, msg)


def test_restatement_wilkinson_and_scaling():
    W = SR.wilkinson_plus(10)
    for A in (W, -W, 1e100 * W, -1e-100 * W):
        lam, Y = SR.sym_eig_smallest(A, 6)
        assert SR.check_eigpairs(A, 6, lam, Y, 1e-13) is None


def test_repeated_eigenvalue_defect():
    """diag(1, 1, 2, 3, 4, 5), k = 2: the split tridiagonal gives lambda = 1 twice, inverse iteration from the common start the same
    vector twice, and without the restart Gram-Schmidt divides 0 by 0."""
    A = np.diag([1.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    lam, Y = SR.sym_eig_smallest(A, 2, restart=False)
    assert np.all(np.isnan(Y[:, 1]))
    lam, Y = SR.sym_eig_smallest(A, 2)
    assert SR.check_eigpairs(A, 2, lam, Y, 1e-13) is None
    assert np.max(np.abs(Y[2:, :])) <= 1e-30


def test_selftest_refusals():
    """ttn_selftest_sym_eig refuses its arguments before it needs a device."""
    import ctypes as C

    import ttn_amd as T
    L = T._lib.lib()
    A = np.zeros(4)
    lam = np.zeros(16)
    Y = np.zeros(16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for N, k in ((0, 1), (2049, 1), (2, 3), (20, 17), (4, 0)):
        assert L.ttn_selftest_sym_eig(N, k, p(A), p(lam), p(Y)) == T._lib.TTN_ERR_ARG
