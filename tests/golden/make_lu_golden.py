"""Regenerates lu2048_pivots_longdouble.npz: the pivot rows a numpy.longdouble Gaussian elimination with partial pivoting chooses on the
2048 x 2048 system of tests/test_gpu_lu.py, and the smallest relative margin between a pivot and its runner-up.  The elimination takes
about 15 s (longdouble has no BLAS), too long for a test; the test checks the fingerprint of the matrix stored here against the matrix
it draws and falls back to the elimination itself if they differ.  Run from the repository root: python tests/golden/make_lu_golden.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.linsolve_reference import lu_pivots_longdouble, lu_test_system, matrix_fingerprint  # noqa: E402

if __name__ == "__main__":
    N = 2048
    K, _ = lu_test_system(N)
    piv, margin = lu_pivots_longdouble(K)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lu2048_pivots_longdouble.npz")
    np.savez_compressed(out, piv=piv.astype(np.int16), margin=np.float64(margin), fingerprint=matrix_fingerprint(K))
    print(out, "margin %.3e" % margin)
