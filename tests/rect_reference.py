"""NumPy restatement of the reference's rectangular operator apply and grid-transfer operators, on the oracle's containers
(oracle.tt_oracle.TToperator / TTvector).

    *(A::TToperator{T,M}, v::TTvector{T,N}), M == N + 1     src/tt_operations.jl:116-148
    qtto_prolongation                                        src/tt_operators.jl:418-436
    qtto_constant_prolongation, qtto_linear_prolongation     src/tt_operators.jl:441-504
    qtt_basis_vector, function_to_tensor / function_to_qtt   src/qtt_tools.jl:190-199, :15-48
    the dense matrices of the reference's testsets           test/test_tt_operators.jl:404-523

Written from the definitions.  A rectangular operator core has shape (n_out, n_in, R_l, R_r); exactly one site has n_in == 1 (the
"singleton" site, which consumes no input site).  Merged bond indices are spelled out as column-major (Fortran-order) reshapes with
the operator's index fastest, the layout the reference's ``reshape`` produces.
"""
import numpy as np

from oracle import tt_oracle as O

EPS = 2.0 ** -53


# ---- the apply ---------------------------------------------------------------------------------------------------------------------
def singleton_sites(A):
    """1-based sites whose input index has one value (:118)."""
    return [k + 1 for k, c in enumerate(A.tto_vec) if c.shape[1] == 1]


def consumed(boundary, s):
    """c(b) = b - [b >= s]: input sites left of boundary b (0-based) when the singleton is site s (1-based) (:128)."""
    return boundary - (1 if boundary >= s else 0)


def out_ranks(A_rks, s, v_rks):
    """y.rks[b] = A.rks[b] * v.rks[c(b)] (:127-130)."""
    return [int(A_rks[b]) * int(v_rks[consumed(b, s)]) for b in range(len(A_rks))]


def _regular_core(Ak, Xk):
    n_out, _, Rl, Rr = Ak.shape
    _, rl, rr = Xk.shape
    Y = np.einsum("ijab,jcd->iacbd", Ak, Xk)                              # [i, a', v', a, v]
    return np.reshape(Y, (n_out, Rl * rl, Rr * rr), order="F")              # a' fastest in the left bond, a in the right


def _singleton_core(Ak, nu):
    n_out, _, Rl, Rr = Ak.shape
    Y = np.zeros((n_out, Rl, nu, Rr, nu), order="F")
    for v in range(nu):
        Y[:, :, v, :, v] = Ak[:, 0, :, :]
    return np.reshape(Y, (n_out, Rl * nu, Rr * nu), order="F")


def apply_rect(A, v):
    """A * v for A with one more site than v (:116-148), with the reference's four assertions."""
    M, N = A.N, v.N
    assert M == N + 1, "Rectangular TToperator must have one additional output site"
    sing = singleton_sites(A)
    assert len(sing) == 1, "Rectangular TToperator must have exactly one singleton input site"
    s = sing[0]
    input_dims = tuple(A.tto_vec[k if k + 1 < s else k + 1].shape[1] for k in range(N))
    assert input_dims == tuple(v.ttv_dims), "Incompatible input dimensions"
    assert v.ttv_rks[-1] == 1, "Input TTvector must have a closed right boundary rank"
    out_dims = tuple(c.shape[0] for c in A.tto_vec)
    rks = out_ranks(A.tto_rks, s, v.ttv_rks)
    vec = []
    for k in range(1, M + 1):
        Ak = np.asarray(A.tto_vec[k - 1])
        if k == s:
            vec.append(_singleton_core(Ak, int(v.ttv_rks[k - 1])))
        else:
            vec.append(_regular_core(Ak, np.asarray(v.ttv_vec[(k if k < s else k - 1) - 1])))
    return O.TTvector(M, vec, out_dims, rks, [0] * M)


def apply_rect_bound(A, v):
    """Per core 2 n_in eps (|A_k| * |X_k|): the bound of an n_in-term dot product in any summation order, with or without FMA.  Zero
    at the singleton site, which only copies."""
    s = singleton_sites(A)[0]
    out = []
    for k in range(1, A.N + 1):
        Ak = np.abs(np.asarray(A.tto_vec[k - 1]))
        if k == s:
            out.append(np.zeros((Ak.shape[0], Ak.shape[2] * v.ttv_rks[k - 1], Ak.shape[3] * v.ttv_rks[k - 1])))
        else:
            out.append(2 * Ak.shape[1] * EPS * _regular_core(Ak, np.abs(np.asarray(v.ttv_vec[(k if k < s else k - 1) - 1]))))
    return out


def rect_to_matrix(A):
    """Dense matrix of an operator with general (n_out, n_in) cores: rows and columns big-endian over the sites (site 1 the most
    significant digit), a singleton input index contributing a factor 1 to the column count."""
    cur = np.asarray(A.tto_vec[0])[:, :, 0, :]                             # (rows, cols, R)
    for k in range(1, A.N):
        G = np.asarray(A.tto_vec[k])
        cur = np.einsum("pqa,ijab->piqjb", cur, G)
        cur = np.reshape(cur, (cur.shape[0] * cur.shape[1], cur.shape[2] * cur.shape[3], cur.shape[4]))
    return cur[:, :, 0]


def rand_rect_tto(out_dims, in_dims, rks, rng):
    """A random operator with cores (out_dims[k], in_dims[k], rks[k], rks[k+1]); tto_dims are the output dimensions."""
    M = len(out_dims)
    vec = [np.asfortranarray(rng.standard_normal((out_dims[k], in_dims[k], rks[k], rks[k + 1]))) for k in range(M)]
    return O.TToperator(M, vec, tuple(out_dims), list(rks), [0] * M)


# ---- the three constructors --------------------------------------------------------------------------------------------------------
def qtto_prolongation(d):
    """:418-436: a square operator of ranks 2."""
    assert d >= 2, "Dimension must be at least 2"
    rks = [1] + [2] * (d - 1) + [1]
    vec = [np.zeros((2, 2, rks[k], rks[k + 1]), order="F") for k in range(d)]
    Id = np.eye(2)
    J = np.array([[0.0, 1.0], [0.0, 0.0]])
    for i in range(2):
        for j in range(2):
            vec[0][i, j, 0, :] = [0.5 * Id[i, j], 0.5 * J[j, i]]
            for k in range(1, d - 1):
                vec[k][i, j, :, :] = [[Id[i, j], J[j, i]], [0.0, J[i, j]]]
    vec[d - 1][0, 0, 0, 0] = 1.0
    vec[d - 1][1, 0, 0, 0] = 2.0
    vec[d - 1][0, 1, 0, 0] = 1.0
    vec[d - 1][1, 1, 0, 0] = 0.0
    return O.TToperator(d, vec, (2,) * d, rks, [0] * d)


def qtto_constant_prolongation(d):
    """:441-458: the cores of id_tto(d), then ones(2, 1, 1, 1)."""
    assert d >= 1, "Dimension must be at least 1"
    vec = [np.array(c, order="F") for c in O.id_tto(d).tto_vec] + [np.ones((2, 1, 1, 1), order="F")]
    return O.TToperator(d + 1, vec, (2,) * (d + 1), [1] * (d + 2), [0] * (d + 1))


def average_branch(d):
    """0.5 * (id_tto(d) + shift(d)) (:472; the scalar lands on the first core, src/tt_operations.jl:271-281), d == 1 as at :467-470."""
    if d == 1:
        core = np.zeros((2, 2, 1, 1), order="F")
        core[:, :, 0, 0] = 0.5 * np.array([[1.0, 1.0], [0.0, 1.0]])
        return O.TToperator(1, [core], (2,), [1, 1], [0])
    return O.tto_scale(0.5, O.tto_add(O.id_tto(d), O.shift(d)))


def qtto_linear_prolongation(d):
    """:463-504: the block-diagonal join of id_tto(d) and the average branch; the last core (2, 1, r, 1) selects the identity branch
    for output bit 0 and the average branch for output bit 1."""
    assert d >= 1, "Dimension must be at least 1"
    I, Av = O.id_tto(d), average_branch(d)
    rks = [1] + [I.tto_rks[k] + Av.tto_rks[k] for k in range(1, d + 1)] + [1]
    vec = []
    for k in range(d):
        l0, r0 = I.tto_rks[k], I.tto_rks[k + 1]
        core = np.zeros((2, 2, rks[k], rks[k + 1]), order="F")
        if k == 0:
            core[:, :, 0:1, :r0] = I.tto_vec[0]
            core[:, :, 0:1, r0:] = Av.tto_vec[0]
        else:
            core[:, :, :l0, :r0] = I.tto_vec[k]
            core[:, :, l0:, r0:] = Av.tto_vec[k]
        vec.append(core)
    l0 = I.tto_rks[d]
    last = np.zeros((2, 1, rks[d], 1), order="F")
    last[0, 0, :l0, 0] = 1.0
    last[1, 0, l0:, 0] = 1.0
    vec.append(last)
    return O.TToperator(d + 1, vec, (2,) * (d + 1), rks, [0] * (d + 1))


# ---- the helpers the reference's testsets are written with ---------------------------------------------------------------------------
def qtt_basis_vector(d, pos, val=1.0):
    """:190-199: the pos-th (1-based) unit vector of 2^d entries as a rank-1 QTT, site 1 the most significant bit; val on the first core."""
    vec = []
    for k in range(d):
        bit = ((pos - 1) >> (d - 1 - k)) & 1
        core = np.zeros((2, 1, 1), order="F")
        core[bit, 0, 0] = val if k == 0 else 1.0
        vec.append(core)
    return O.TTvector(d, vec, (2,) * d, [1] * (d + 1), [0] * d)


def index_to_point(bits, d):
    """:15-18: sum_i 2.0^(d - i) t_i / (2^d - 1), summed left to right; the interval length L is accepted and never used."""
    acc = None
    for i in range(1, d + 1):
        term = 2.0 ** (d - i) * bits[i - 1] / (2 ** d - 1)
        acc = term if acc is None else acc + term
    return acc


def function_to_tensor(f, d, a=0.0, b=1.0):
    """:25-31: out[t_1, ..., t_d] = f(index_to_point(t)); a and b do not move the points."""
    out = np.zeros((2,) * d, order="F")
    for t in np.ndindex(*(2,) * d):
        out[t] = f(index_to_point(t, d))
    return out


def function_to_qtt(f, d, a=0.0, b=1.0):
    """:45-48."""
    return O.ttv_decomp(function_to_tensor(f, d, a, b))


# ---- dense matrices of the reference's testsets ----------------------------------------------------------------------------------------
def prolongation_matrix(d):
    """test/test_tt_operators.jl:408-429."""
    assert d >= 2
    n = 2 ** (d - 1)
    P = np.zeros((2 * n, n))
    P[0, 0] = 0.5
    for k in range(1, n + 1):
        P[2 * k - 1, k - 1] = 1.0
    for k in range(1, n):
        P[2 * k, k - 1] += 0.5
        P[2 * k, k] += 0.5
    return P


def constant_prolongation_matrix(d):
    """:437-445."""
    n = 2 ** d
    P = np.zeros((2 * n, n))
    for al in range(n):
        P[2 * al, al] = 1.0
        P[2 * al + 1, al] = 1.0
    return P


def linear_prolongation_matrix(d):
    """:478-489."""
    n = 2 ** d
    P = np.zeros((2 * n, n))
    for al in range(n):
        P[2 * al, al] = 1.0
        P[2 * al + 1, al] += 0.5
        if al + 1 < n:
            P[2 * al + 1, al + 1] += 0.5
    return P
