"""NumPy restatement of the reference's multi-dimensional QTT interface, on top of oracle.tt_oracle.

    function_to_qttv, qttv_to_array      src/qtt_tools.jl:805-839, :943-972
    Δ_DN, Δ_ND, Δ_NN                     src/tt_operators.jl:290-349
    qtt_laplacian                        src/tt_operators.jl:644-703
    entanglemententropy                  src/tt_tools.jl:554-587

The loops are the reference's, 1-based site / dimension numbers included, so that each function can be checked by eye against the
Julia source; tests/test_cpu_qttnd.py pins them to the known answers of the reference's test/test_qtt_multidim.jl.  A QTT vector or
operator is the oracle's TTvector / TToperator plus (n_dims, bits_per_dim, ordering) in a small record.
"""
import math
from collections import namedtuple

import numpy as np

from oracle import tt_oracle as O

QTTv = namedtuple("QTTv", "ttv n_dims bits_per_dim ordering")
QTTo = namedtuple("QTTo", "tto n_dims bits_per_dim ordering")


def _dim_level(site, n_dims, bits_per_dim, ordering):
    """(dim 1-based, level 0-based) of the 1-based site — src/qtt_tools.jl:822-828"""
    if ordering == "interleaved":
        dim = ((site - 1) % n_dims) + 1
        level = (site - 1) // n_dims
    else:
        dim = ((site - 1) // bits_per_dim) + 1
        level = (site - 1) % bits_per_dim
    return dim, level


def sample_tensor(f, n_dims, bits_per_dim, ordering="interleaved", a=0.0, b=1.0):
    """the tensor loop of function_to_qttv (:813-835); f receives the coordinate vector of ONE grid point"""
    assert ordering in ("interleaved", "serial")
    N = n_dims * bits_per_dim
    n_pts = 2 ** bits_per_dim
    h = (b - a) / (n_pts - 1)
    tensor = np.zeros((2,) * N)
    for idx in np.ndindex(*tensor.shape):
        grid_idx = [0] * n_dims
        for site in range(1, N + 1):
            bit_val = idx[site - 1]                      # bits[site] - 1
            dim, level = _dim_level(site, n_dims, bits_per_dim, ordering)
            grid_idx[dim - 1] += bit_val * 2 ** (bits_per_dim - 1 - level)
        coords = [a + grid_idx[d] * h for d in range(n_dims)]
        tensor[idx] = f(coords)
    return tensor


def sample_tensor_fast(fv, n_dims, bits_per_dim, ordering="interleaved", a=0.0, b=1.0):
    """sample_tensor with the loop over the entries vectorised (for grids too large for the literal loop); fv receives the
    coordinates of all points as an array (P, n_dims).  test_cpu_qttnd.py checks it against sample_tensor entry by entry."""
    N = n_dims * bits_per_dim
    h = (b - a) / (2 ** bits_per_dim - 1)
    e = np.arange(2 ** N, dtype=np.int64)               # Julia linear index - 1: site 1 fastest
    g = np.zeros((2 ** N, n_dims), dtype=np.int64)
    for site in range(1, N + 1):
        dim, level = _dim_level(site, n_dims, bits_per_dim, ordering)
        g[:, dim - 1] += ((e >> (site - 1)) & 1) * 2 ** (bits_per_dim - 1 - level)
    vals = np.asarray(fv(a + g * h), dtype=float)
    return np.reshape(vals, (2,) * N, order="F")


def function_to_qttv(f, n_dims, bits_per_dim, ordering="interleaved", a=0.0, b=1.0):
    tensor = sample_tensor(f, n_dims, bits_per_dim, ordering, a, b)
    return QTTv(O.ttv_decomp(tensor), n_dims, bits_per_dim, ordering)


def qttv_to_array(q):
    """:943-972"""
    N = q.ttv.N
    n_dims, bits_per_dim, ordering = q.n_dims, q.bits_per_dim, q.ordering
    n_pts = 2 ** bits_per_dim
    full_tensor = O.ttv_to_tensor(q.ttv)
    out = np.zeros((n_pts,) * n_dims, dtype=full_tensor.dtype)
    for idx in np.ndindex(*full_tensor.shape):
        grid_idx = [0] * n_dims
        for site in range(1, N + 1):
            bit_val = idx[site - 1]
            dim, level = _dim_level(site, n_dims, bits_per_dim, ordering)
            grid_idx[dim - 1] += bit_val * 2 ** (bits_per_dim - 1 - level)
        out[tuple(grid_idx)] = full_tensor[idx]
    return out


def grid_strides(n_dims, bits_per_dim, ordering):
    """where the loop of qttv_to_array sends the unit bit of each site, as an offset into the column-major output"""
    n_pts = 2 ** bits_per_dim
    out = []
    for site in range(1, n_dims * bits_per_dim + 1):
        dim, level = _dim_level(site, n_dims, bits_per_dim, ordering)
        out.append(2 ** (bits_per_dim - 1 - level) * n_pts ** (dim - 1))
    return out


# ---- boundary-condition Laplacians ---------------------------------------------------------------------------------------------------
_id = np.array([[1.0, 0.0], [0.0, 1.0]])
_J = np.array([[0.0, 1.0], [0.0, 0.0]])
_I1 = np.array([[1.0, 0.0], [0.0, 0.0]])
_I2 = np.array([[0.0, 0.0], [0.0, 1.0]])


def _delta_4(d, Ic):
    assert d >= 4, "Dimension must be at least 4"
    out = O.zeros_tto_ndr(2, d, 4)
    id, J = _id, _J
    for i in range(2):
        for j in range(2):
            out.tto_vec[0][i, j, 0, :] = [id[i, j], J[j, i], J[i, j], Ic[i, j]]
            for k in range(1, d - 1):
                out.tto_vec[k][i, j, :, :] = [[id[i, j], J[j, i], J[i, j], 0], [0, J[i, j], 0, 0], [0, 0, J[j, i], 0], [0, 0, 0, Ic[i, j]]]
            out.tto_vec[d - 1][i, j, :, 0] = [2 * id[i, j] - J[i, j] - J[j, i], -J[i, j], -J[j, i], -Ic[i, j]]
    return out


def Delta_DN(d):
    """:290-306"""
    return _delta_4(d, _I2)


def Delta_ND(d):
    """:311-327"""
    return _delta_4(d, _I1)


def Delta_NN(d):
    """:332-349"""
    assert d >= 4, "Dimension must be at least 4"
    out = O.zeros_tto((2,) * d, [4] + [5] * (d - 1) + [4])
    id, J, I1, I2 = _id, _J, _I1, _I2
    for i in range(2):
        for j in range(2):
            out.tto_vec[0][i, j, 0, :] = [id[i, j], J[j, i], J[i, j], I2[i, j], I1[i, j]]
            for k in range(1, d - 1):
                out.tto_vec[k][i, j, :, :] = [[id[i, j], J[j, i], J[i, j], 0, 0], [0, J[i, j], 0, 0, 0], [0, 0, J[j, i], 0, 0],
                                              [0, 0, 0, I2[i, j], 0], [0, 0, 0, 0, -I1[i, j]]]
            out.tto_vec[d - 1][i, j, :, 0] = [2 * id[i, j] - J[i, j] - J[j, i], -J[i, j], -J[j, i], -I2[i, j], -I1[i, j]]
    return out


def kron(A, B):
    """kron(A::TToperator, B::TToperator): the cores of B behind those of A (src/tt_operations.jl:427-435)"""
    return O.TToperator(A.N + B.N, [np.array(c) for c in A.tto_vec + B.tto_vec], tuple(A.tto_dims) + tuple(B.tto_dims),
                        list(A.tto_rks[:-1]) + list(B.tto_rks), list(A.tto_ot) + list(B.tto_ot))


def qtt_laplacian(n_dims, bits_per_dim, ordering="interleaved", a=0.0, b=1.0, bc="DN"):
    """:644-703"""
    assert ordering in ("interleaved", "serial"), "ordering must be :interleaved or :serial"
    assert n_dims >= 1, "n_dims must be at least 1"
    assert bc in ("DD", "DN", "ND", "NN"), "bc must be :DD, :DN, :ND, or :NN"
    assert not (bc == "NN" and n_dims > 1), "bc=:NN is only supported for n_dims=1"
    d = bits_per_dim
    h = (b - a) / (2 ** d - 1)
    scale = 1.0 / h ** 2
    if bc == "DD":
        lap_1d = O.Delta(d)
    elif bc == "DN":
        lap_1d = Delta_DN(d)
    elif bc == "ND":
        lap_1d = Delta_ND(d)
    else:
        lap_1d = Delta_NN(d)
    id_1d = O.id_tto(d)
    if n_dims == 1:
        return QTTo(O.tto_scale(scale, lap_1d), 1, d, ordering)

    def build_term(k):
        ops = [lap_1d if dim == k else id_1d for dim in range(1, n_dims + 1)]
        term = ops[0]
        for dim in range(2, n_dims + 1):
            term = kron(term, ops[dim - 1])
        return term

    result = O.tto_scale(scale, build_term(1))
    for k in range(2, n_dims + 1):
        result = O.tto_add(result, O.tto_scale(scale, build_term(k)))
    if ordering == "serial":
        return QTTo(result, n_dims, d, "serial")
    return QTTo(O.reorder_op(result, n_dims, d, True), n_dims, d, "interleaved")


def qtto_to_matrix(A):
    return O.qtto_to_matrix(A.tto if isinstance(A, QTTo) else A)


def grid_matrix(A):
    """The operator of a QTTo as a matrix on the grid vector vec(qttv_to_array(v)) (column-major: dimension 1 fastest), whatever the
    ordering: the bits of both indices go through the rule of qttv_to_array."""
    N = A.tto.N
    T = O.tto_to_tensor(A.tto)                          # (x1..xN, y1..yN)
    n = 2 ** N
    M = np.reshape(T, (n, n))                           # C order: site 1 most significant
    st = grid_strides(A.n_dims, A.bits_per_dim, A.ordering)
    e = np.arange(n)
    tgt = np.zeros(n, dtype=np.int64)
    for site in range(1, N + 1):
        tgt += ((e >> (N - site)) & 1) * st[site - 1]
    out = np.zeros_like(M)
    out[np.ix_(tgt, tgt)] = M
    return out


# ---- entanglement entropy --------------------------------------------------------------------------------------------------------
def schmidt_spectra(psi):
    """the singular values F.S of every bond of the loop :565-585"""
    N = psi.N
    canonical = O.orthogonalize(psi, i=1)
    cores = [np.transpose(np.array(core), (1, 0, 2)) for core in canonical.ttv_vec]
    spectra = []
    for k in range(1, N):
        A = cores[k - 1]
        r_left, n, r_right = A.shape
        U, S, Vt = np.linalg.svd(np.reshape(A, (r_left * n, r_right), order="F"), full_matrices=False)
        spectra.append(S)
        if k < N - 1:
            transfer = np.diag(S) @ Vt
            B = cores[k]
            cores[k] = np.reshape(transfer @ np.reshape(B, (B.shape[0], -1), order="F"), (len(S), B.shape[1], B.shape[2]), order="F")
    return spectra


def entanglemententropy(psi, base=math.e):
    """:554-587"""
    assert base > 0 and base != 1, "base must be positive and not equal to 1"
    N = psi.N
    entropy = np.zeros(max(N - 1, 0))
    if N <= 1:
        return entropy
    logscale = math.log(base)
    for k, S in enumerate(schmidt_spectra(psi), start=1):
        probabilities = np.abs(S) ** 2
        total = probabilities.sum()
        if total > 0:
            probabilities = probabilities / total
            entropy[k - 1] = -sum(p * math.log(p) if p > 0 else 0.0 for p in probabilities) / logscale
    return entropy
