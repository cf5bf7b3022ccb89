"""NumPy restatement of the reference's dense bridge for operators, on top of the CPU oracle.

    tto_decomp(tensor; index)     src/tt_tools.jl:338-362: ttv_decomp of permutedims(tensor, [1, d+1, 2, d+2, ...]) reshaped to
                                  (n_1^2, ..., n_d^2), the cores reshaped to (n, n, r, r'); ttv_decomp's tol is exposed
    tto_to_tensor, qtto_to_matrix are the oracle's own (oracle/tt_oracle.py)

and the inputs the CPU and the GPU tests share.  Pinned to the reference's test/test_tt_tools.jl:327-368 by tests/test_cpu_dense_operator.py."""
import numpy as np

from oracle import tt_oracle as O


def interleave(tensor):
    """tensor[x_1..x_d, y_1..y_d] -> the array (n_1^2, ..., n_d^2) with merged index x_k + n_k y_k (0-based) that tto_decomp decomposes"""
    t = np.asarray(tensor, dtype=float)
    d = t.ndim // 2
    perm = [v for k in range(d) for v in (k, d + k)]
    return np.reshape(np.transpose(t, perm), [n * n for n in t.shape[:d]], order="F")


def tto_decomp(tensor, index=1, tol=1.0e-12):
    t = np.asarray(tensor, dtype=float)
    assert t.ndim % 2 == 0 and t.shape[: t.ndim // 2] == t.shape[t.ndim // 2:]
    d = t.ndim // 2
    dims = tuple(int(n) for n in t.shape[:d])
    ttv = O.ttv_decomp(interleave(t), index=index, tol=tol)
    vec = [np.reshape(c, (dims[k], dims[k], ttv.ttv_rks[k], ttv.ttv_rks[k + 1]), order="F") for k, c in enumerate(ttv.ttv_vec)]
    return O.TToperator(d, vec, dims, list(ttv.ttv_rks), list(ttv.ttv_ot))


def address_table(dims, xstrides, ystrides):
    """the address of every entry of the array of shape dims + dims"""
    idx = np.indices(tuple(dims) * 2)
    return sum(idx[k] * s for k, s in enumerate(list(xstrides) + list(ystrides)))


# ---- the reference's three test inputs (test_tt_tools.jl:327-368), with NumPy generators in place of Julia's randn ----------------------
def round_trip_operator():
    """dims (2, 2, 2), ranks [1, 2, 2, 1] (:330-335)"""
    rng = np.random.default_rng(10)
    vec = [rng.standard_normal((2, 2, 1, 2)), rng.standard_normal((2, 2, 2, 2)), rng.standard_normal((2, 2, 2, 1))]
    return O.TToperator(3, vec, (2, 2, 2), [1, 2, 2, 1], [0, 0, 0])


def matvec_case(dims, seed):
    """A non-symmetric N x N matrix and a vector (:347-357, :361-364): (A_mat, its tensor reshape(A_mat, dims..., dims...), v)"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims))
    A_mat = rng.standard_normal((n, n))
    v = rng.standard_normal(n)
    return A_mat, np.reshape(A_mat, tuple(dims) * 2, order="F"), v


REFERENCE_MATVEC_CASES = (((2, 2), 11), ((2, 3), 12))


def isapprox(a, b, rtol):
    """Julia's isapprox(a, b; rtol) for arrays: norm(a - b) <= rtol * max(norm(a), norm(b))"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.linalg.norm(a - b) <= rtol * max(np.linalg.norm(a), np.linalg.norm(b))


# ---- random operators of the GPU tests: (dims, rmax of O.rand_tto, seed, the ranks rand_tto gives) ----------------------------------------
# The seeds are those at which the dense array has a wide spectral gap around tol = 1e-10 max|dense| in every unfolding of the
# decomposition, for index 1 and index d (spectral_gap below; asserted where the inputs are used).
RANDOM_OPERATORS = (((5,), 1, 1, [1, 1]), ((2, 3, 2), 2, 1, [1, 2, 2, 1]), ((3, 2, 2, 3), 3, 5, [1, 3, 3, 3, 1]), ((65, 2), 3, 1, [1, 2, 1]))


def random_operator(dims, r, seed):
    return O.rand_tto(dims, r, np.random.default_rng(seed))


def spectral_gap(tensor, index, tol):
    """(smallest kept singular value, largest dropped one) over the unfoldings of tto_decomp(tensor, index, tol); (inf, 0) without any"""
    sp = decomp_spectra(tensor, index, tol)
    kept = min([s[s >= tol].min() for s in sp if (s >= tol).any()], default=np.inf)
    dropped = max([s[s < tol].max() for s in sp if (s < tol).any()], default=0.0)
    return kept, dropped


def decomp_spectra(tensor, index=1, tol=1.0e-12):
    """the singular values of every unfolding O.ttv_decomp cuts on the way to tto_decomp(tensor, index, tol), in its order"""
    import scipy.linalg as sla
    cur = interleave(tensor)
    dims = cur.shape
    d = len(dims)
    out, rl, rr = [], 1, 1
    for i in range(1, index):
        cur = np.reshape(cur, (rl * dims[i - 1], -1), order="F")
        u, sv, vt = sla.svd(cur, full_matrices=False, lapack_driver="gesdd")
        r = int(np.count_nonzero(sv >= tol))
        out.append(sv)
        cur, rl = sv[:r, None] * vt[:r, :], r
    for i in range(d, index, -1):
        cur = np.reshape(cur, (-1, dims[i - 1] * rr), order="F")
        u, sv, vt = sla.svd(cur, full_matrices=False, lapack_driver="gesdd")
        r = int(np.count_nonzero(sv >= tol))
        out.append(sv)
        cur, rr = u[:, :r] * sv[None, :r], r
    return out
