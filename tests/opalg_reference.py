"""NumPy restatement of the reference's TT operator algebra, on the oracle's containers (oracle.tt_oracle.TToperator / TTvector).

Written from the definitions; cores are (n, n, r_l, r_r) / (n, r_l, r_r) arrays and every merged index is spelled out as a
column-major (Fortran-order) reshape, the layout a Julia ``reshape`` produces.
"""
import math

import numpy as np

from oracle import tt_oracle as O

EPS = 2.0 ** -53


def rand_tto(dims, rks, rng):
    """A random operator with the given (possibly ragged) ranks."""
    d = len(dims)
    vec = [np.asfortranarray(rng.standard_normal((dims[k], dims[k], rks[k], rks[k + 1]))) for k in range(d)]
    return O.TToperator(d, vec, tuple(dims), list(rks), [0] * d)


def rand_ttv(dims, rks, rng):
    d = len(dims)
    vec = [np.asfortranarray(rng.standard_normal((dims[k], rks[k], rks[k + 1]))) for k in range(d)]
    return O.TTvector(d, vec, tuple(dims), list(rks), [0] * d)


def _mul_core(Ak, Bk):
    n, _, R, Rr = Ak.shape
    _, _, r, rr = Bk.shape
    Y = np.einsum("izac,zjbd->ijabcd", Ak, Bk)                    # [i, j, α, β, α', β']
    return np.reshape(Y, (n, n, R * r, Rr * rr), order="F")          # α fastest in the left bond, α' in the right


def tto_mul(A, B):
    """*(A::TToperator, B::TToperator), src/tt_operations.jl:162-172: Y_k[i, j, (α, β), (α', β')] = Σ_z A_k[i, z, α, α'] B_k[z, j, β, β'],
    A's bond index fastest (the reshape at :168); ranks A.rks .* B.rks, ot zeros."""
    assert tuple(A.tto_dims) == tuple(B.tto_dims), "Incompatible dimensions"
    vec = [_mul_core(a, b) for a, b in zip(A.tto_vec, B.tto_vec)]
    return O.TToperator(A.N, vec, A.tto_dims, [a * b for a, b in zip(A.tto_rks, B.tto_rks)], [0] * A.N)


def tto_mul_bound(A, B):
    """Per core 2 n ε (|A_k| ⋆ |B_k|): the bound of an n-term dot product in any summation order, with or without FMA."""
    return [2 * a.shape[0] * EPS * _mul_core(np.abs(a), np.abs(b)) for a, b in zip(A.tto_vec, B.tto_vec)]


def tto_inner(A, B):
    """A ⨝ B, src/tt_operations.jl:198-216: physical and bond indices all Kronecker products, A major and B minor (the B index is
    the fastest of every merged pair); dims and ranks multiply, ot zeros."""
    assert A.N == B.N, "Inner core product requires operators with the same number of cores"
    vec = []
    for a, b in zip(A.tto_vec, B.tto_vec):
        na, _, al, ar = a.shape
        nb, _, bl, br = b.shape
        T8 = np.einsum("IJLR,ijlr->iIjJlLrR", a, b)                # B index first (fastest) in every pair
        vec.append(np.reshape(T8, (na * nb, na * nb, al * bl, ar * br), order="F"))
    return O.TToperator(A.N, vec, tuple(x * y for x, y in zip(A.tto_dims, B.tto_dims)), [x * y for x, y in zip(A.tto_rks, B.tto_rks)],
                        [0] * A.N)


def tto_add(x, y):
    """+(x::TToperator, y::TToperator), src/tt_operations.jl:71-95: first core [X Y], middle cores block diagonal, last core [X; Y];
    ranks add with both ends forced to 1, ot zeros (d >= 2)."""
    assert tuple(x.tto_dims) == tuple(y.tto_dims), "Incompatible dimensions"
    d = x.N
    assert d >= 2
    rks = [a + b for a, b in zip(x.tto_rks, y.tto_rks)]
    rks[0] = rks[d] = 1
    vec = [np.zeros((x.tto_dims[k], x.tto_dims[k], rks[k], rks[k + 1]), order="F") for k in range(d)]
    vec[0][:, :, :, : x.tto_rks[1]] = x.tto_vec[0]
    vec[0][:, :, :, x.tto_rks[1]:] = y.tto_vec[0]
    for k in range(1, d - 1):
        vec[k][:, :, : x.tto_rks[k], : x.tto_rks[k + 1]] = x.tto_vec[k]
        vec[k][:, :, x.tto_rks[k]:, x.tto_rks[k + 1]:] = y.tto_vec[k]
    vec[d - 1][:, :, : x.tto_rks[d - 1], :] = x.tto_vec[d - 1]
    vec[d - 1][:, :, x.tto_rks[d - 1]:, :] = y.tto_vec[d - 1]
    return O.TToperator(d, vec, x.tto_dims, rks, [0] * d)


def tto_scale(a, A):
    """*(a::Number, A::TToperator), src/tt_operations.jl:271-281: a == 0 gives zeros_tto(dims, rks); otherwise the first core with
    ot == 0 (core 1 if there is none) is multiplied, ot kept."""
    a = float(a)
    if a == 0.0:
        return O.zeros_tto(A.tto_dims, A.tto_rks)
    i = next((k for k, o in enumerate(A.tto_ot) if o == 0), 0)
    vec = [np.array(c, order="F") for c in A.tto_vec]
    vec[i] = a * vec[i]
    return O.TToperator(A.N, vec, A.tto_dims, list(A.tto_rks), list(A.tto_ot))


def tto_sub(A, B):
    """-(A::TToperator, B::TToperator) = (-1.0 * B) + A, src/tt_operations.jl:289-291."""
    return tto_add(tto_scale(-1.0, B), A)


def concatenate(a, b):
    """concatenate, src/tt_tools.jl:708-735, and kron, src/tt_operations.jl:427-448: cores, dims and ot appended, ranks
    a.rks[1:end-1] followed by b.rks; concatenate refuses different ranks at the joint."""
    if isinstance(a, O.TToperator):
        if a.tto_rks[-1] != b.tto_rks[0]:
            raise ValueError("The final rank of the first TToperator must equal the initial rank of the second TToperator.")
        return O.TToperator(a.N + b.N, list(a.tto_vec) + list(b.tto_vec), tuple(a.tto_dims) + tuple(b.tto_dims),
                            list(a.tto_rks[:-1]) + list(b.tto_rks), list(a.tto_ot) + list(b.tto_ot))
    if a.ttv_rks[-1] != b.ttv_rks[0]:
        raise ValueError("The final rank of the first TTvector must equal the initial rank of the second TTvector.")
    return O.TTvector(a.N + b.N, list(a.ttv_vec) + list(b.ttv_vec), tuple(a.ttv_dims) + tuple(b.ttv_dims),
                      list(a.ttv_rks[:-1]) + list(b.ttv_rks), list(a.ttv_ot) + list(b.ttv_ot))


kron = concatenate


def outer_product(x, y):
    """outer_product(x, y), src/tt_operations.jl:297-304 (real): Y_k[i, j, (α, β), (α', β')] = x_k[i, α, α'] y_k[j, β, β'], x's bond
    index fastest; ranks multiply, ot zeros."""
    vec = []
    for a, b in zip(x.ttv_vec, y.ttv_vec):
        n, al, ar = a.shape
        _, bl, br = b.shape
        vec.append(np.reshape(np.einsum("iac,jbd->ijabcd", a, b), (n, n, al * bl, ar * br), order="F"))
    return O.TToperator(x.N, vec, x.ttv_dims, [p * q for p, q in zip(x.ttv_rks, y.ttv_rks)], [0] * x.N)


def ttv_to_diag_tto(x):
    """ttv_to_diag_tto(x), src/tt_operations.jl:310-338: D_k[j, j, s1, s2] = x_k[j, s1, s2], zero elsewhere; ranks kept, ot zeros."""
    vec = []
    for c in x.ttv_vec:
        n = c.shape[0]
        D = np.zeros((n, n) + c.shape[1:], order="F")
        for j in range(n):
            D[j, j] = c[j]
        vec.append(D)
    return O.TToperator(x.N, vec, x.ttv_dims, list(x.ttv_rks), [0] * x.N)


def tto_to_ttv(A):
    """tto_to_ttv(A), src/tt_tools.jl:296-304: every core reshaped to (n², r_l, r_r); dims squared, ranks and ot kept."""
    vec = [np.reshape(np.asfortranarray(c), (c.shape[0] ** 2,) + c.shape[2:], order="F") for c in A.tto_vec]
    return O.TTvector(A.N, vec, tuple(n * n for n in A.tto_dims), list(A.tto_rks), list(A.tto_ot))


def ttv_to_tto(x):
    """ttv_to_tto(x), src/tt_tools.jl:323-333: the inverse reshape; dimensions that are not perfect squares are refused."""
    dims = tuple(math.isqrt(n) for n in x.ttv_dims)
    assert tuple(n * n for n in dims) == tuple(x.ttv_dims), "DimensionMismatch"
    vec = [np.reshape(np.asfortranarray(c), (dims[k], dims[k]) + c.shape[1:], order="F") for k, c in enumerate(x.ttv_vec)]
    return O.TToperator(x.N, vec, dims, list(x.ttv_rks), list(x.ttv_ot))


def tto_compress(A, max_bond=2 ** 62, truncerr=0.0, sweeps=1):
    """ttv_to_tto(tt_compress!(tto_to_ttv(A), max_bond; truncerr, sweeps)) with the oracle's tt_compress! (src/tt_tools.jl:772-789)."""
    return ttv_to_tto(O.tt_compress_(tto_to_ttv(A), max_bond, truncerr=truncerr, sweeps=sweeps))


def tto_matrix(A):
    """The dense prod(dims) x prod(dims) matrix of an operator, row index (i_1, ..., i_d) with i_1 fastest (the reference's
    reshape(tto_to_tensor(A), n, n)), by contracting the cores directly."""
    M = np.ones((1, 1, 1))                                           # [row, col, bond]
    for c in A.tto_vec:
        n = c.shape[0]
        M = np.einsum("pqa,ijab->piqjb", M, c)
        M = np.reshape(M, (M.shape[0] * n, M.shape[2] * n, c.shape[3]), order="F")
    return M[:, :, 0]


def ttv_vector(x):
    """The dense vector of a train, i_1 fastest."""
    v = np.ones((1, 1))
    for c in x.ttv_vec:
        v = np.reshape(np.einsum("pa,iab->pib", v, c), (v.shape[0] * c.shape[0], c.shape[2]), order="F")
    return v[:, 0]


def ornstein2d_coupled(d, ops, theta=1.0, k=0.6, mu=(2.0, -2.0), D=0.5, a=-6.0, b=6.0):
    """The generator of examples/Ornstein2D_coupled.jl:22-29 on 2 d sites.  `ops` supplies the algebra so that one statement of the
    formula serves the restatement and the device: it has shift, id, nabla, delta, diag_poly(coef), and add / sub / scale / mul / kron."""
    h = (b - a) / (2 ** d - 1)
    idd = ops.id(d)
    dx = ops.scale(1 / (2 * h), ops.sub(ops.shift(d), ops.sub(idd, ops.nabla(d))))
    dxx = ops.scale(-(1 / h ** 2), ops.delta(d))
    Mx = ops.diag_poly([-mu[0], 1.0], d, a, b)
    My = ops.diag_poly([-mu[1], 1.0], d, a, b)
    drift = ops.scale(theta, ops.add(ops.kron(ops.mul(dx, Mx), idd), ops.kron(idd, ops.mul(dx, My))))
    coupling = ops.scale(k, ops.add(ops.kron(dx, My), ops.kron(Mx, dx)))
    diffusion = ops.scale(D, ops.add(ops.kron(dxx, idd), ops.kron(idd, dxx)))
    return ops.add(ops.sub(drift, coupling), diffusion)


class HostOps:
    """The algebra of ornstein2d_coupled on this module's functions and the oracle's constructors."""
    shift, delta = staticmethod(O.shift), staticmethod(O.Delta)
    add, sub, mul, kron = staticmethod(tto_add), staticmethod(tto_sub), staticmethod(tto_mul), staticmethod(kron)

    @staticmethod
    def id(d):
        return O.id_tto(d)

    @staticmethod
    def nabla(d):
        return O.toeplitz_to_qtto(1, 0, -1, d)

    @staticmethod
    def scale(a, A):
        return tto_scale(a, A)

    @staticmethod
    def diag_poly(coef, d, a, b):
        return ttv_to_diag_tto(O.qtt_polynom(coef, d, a, b))
