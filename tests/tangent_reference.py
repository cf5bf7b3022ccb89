"""NumPy restatement of the fixed-rank TT manifold on oracle trains: the two gauges of a point, the orthogonal projection of a train onto
the tangent space, the train alpha x + beta xi at twice the ranks, the retraction (orthogonalize, then the reference's bond step with a
cap per bond), the two drivers, a DENSE projector built from the Jacobian of the train map, componentwise rounding bounds of the
projection, and the reference's Manopt extension (ext/TensorTrainNumericsManoptExt) with its methods under their names.  Plain einsum; it
shares no code with the product.

Cores are [z, al, a].  U = orthogonalize(x, d) (U_1 .. U_{d-1} left-orthogonal, U_d the centre), V = orthogonalize(x, 1) (V_2 .. V_d
right-orthogonal); a tangent is a list of cores dC_k with x's ranks that stands for sum_k U_1 .. U_{k-1} dC_k V_{k+1} .. V_d."""
import numpy as np

from oracle import tt_oracle as O

EPS = np.finfo(np.float64).eps


def gauges(x):
    return O.orthogonalize(x, x.N), O.orthogonalize(x, 1)


def chains(U, V, z):
    """L[k] (k = 0..d) with bra U, G[k] (k = 0..d) with bra V, 0-based: L[0] = G[d] = [1]; each r_k x rz_k."""
    d = U.N
    L, G = [None] * (d + 1), [None] * (d + 1)
    L[0] = np.zeros((U.ttv_rks[0], z.ttv_rks[0]))
    L[0][0, 0] = 1.0
    for k in range(d):
        L[k + 1] = np.einsum("zxa,zyb,xy->ab", U.ttv_vec[k], z.ttv_vec[k], L[k], optimize=True)
    G[d] = np.zeros((V.ttv_rks[d], z.ttv_rks[d]))
    G[d][0, 0] = 1.0
    for k in range(d - 1, -1, -1):
        G[k] = np.einsum("zxa,zyb,ab->xy", V.ttv_vec[k], z.ttv_vec[k], G[k + 1], optimize=True)
    return L, G


def project(U, V, z):
    """(cores dC_k of P_x z, <x, z>)."""
    d = U.N
    L, G = chains(U, V, z)
    out = []
    for k in range(d):
        M = np.einsum("xy,zyb->zxb", L[k], z.ttv_vec[k], optimize=True)
        if k < d - 1:
            M = M - np.einsum("zxa,ab->zxb", U.ttv_vec[k], L[k + 1], optimize=True)
        out.append(np.einsum("zxb,ab->zxa", M, G[k + 1], optimize=True))
    return out, float(L[d][0, 0])


def _abs_tt(x):
    return O.TTvector(x.N, [np.abs(c) for c in x.ttv_vec], x.ttv_dims, list(x.ttv_rks), list(x.ttv_ot))


def project_bound(U, V, z):
    """Componentwise rounding bounds of ``project``, in the style of grad_reference.dot_pullback_bound: a nested sum of products evaluated
    in any order (FMA or not) satisfies |fl - exact| <= p eps S_abs, with S_abs the same formula on the absolute values — the two terms of
    the middle factor ADDED, |L_k| |Z_k| + |U_k| |L_{k+1}| — and p the number of terms along the longest chain of sums: the chains of dot,
    sum_k (n_k r_{k-1} rz_{k-1} + r_k rz_k), plus the inner sum of the gauge term (max_k r_k terms) and its subtraction (1).  Device and
    restatement both round: the returned bounds are 2 p eps S_abs.  Returns (value bound, core bounds)."""
    d = U.N
    p = sum(U.ttv_dims[k] * U.ttv_rks[k] * z.ttv_rks[k] + U.ttv_rks[k + 1] * z.ttv_rks[k + 1] for k in range(d)) + max(U.ttv_rks) + 1
    aU, aV, az = _abs_tt(U), _abs_tt(V), _abs_tt(z)
    L, G = chains(aU, aV, az)
    f = 2.0 * p * EPS
    out = []
    for k in range(d):
        M = np.einsum("xy,zyb->zxb", L[k], az.ttv_vec[k], optimize=True)
        if k < d - 1:
            M = M + np.einsum("zxa,ab->zxb", aU.ttv_vec[k], L[k + 1], optimize=True)
        out.append(f * np.einsum("zxb,ab->zxa", M, G[k + 1], optimize=True))
    return f * float(L[d][0, 0]), out


def to_tt(U, V, cores, alpha=1.0, beta=1.0):
    """The train alpha x + beta xi at ranks 2 r: W_1 = [dC_1, U_1], W_k = [[V_k, 0], [dC_k, U_k]], W_d = [beta V_d ; beta dC_d + alpha U_d]."""
    d = U.N
    r = list(U.ttv_rks)
    if d == 1:
        return O.TTvector(1, [alpha * U.ttv_vec[0] + beta * cores[0]], U.ttv_dims, [1, 1], [0])
    rk = [1] + [2 * v for v in r[1:d]] + [1]
    out = []
    for k in range(d):
        n, rl, rr = U.ttv_dims[k], r[k], r[k + 1]
        W = np.zeros((n, rk[k], rk[k + 1]))
        if k == 0:
            W[:, :, :rr] = cores[0]
            W[:, :, rr:] = U.ttv_vec[0]
        elif k == d - 1:
            W[:, :rl, :] = beta * V.ttv_vec[k]
            W[:, rl:, :] = beta * cores[k] + alpha * U.ttv_vec[k]
        else:
            W[:, :rl, :rr] = V.ttv_vec[k]
            W[:, rl:, :rr] = cores[k]
            W[:, rl:, rr:] = U.ttv_vec[k]
        out.append(W)
    return O.TTvector(d, out, U.ttv_dims, rk, [0] * d)


def tangent_dense(U, V, cores):
    return O.ttv_to_tensor(to_tt(U, V, cores, 0.0, 1.0))


def tangent_inner(a, b):
    return float(sum(np.vdot(p, q) for p, q in zip(a, b)))


def retract(U, V, cores, t=1.0, alpha=1.0):
    """alpha x + t xi back at x's ranks: orthogonalize(y, d), then the bond step with the cap r_k for k = d - 1 .. 1."""
    d = U.N
    y = O.orthogonalize(to_tt(U, V, cores, alpha, t), d)
    for k in range(d - 1, 0, -1):
        O.tt_bond_truncate_(y, k, max_bond=U.ttv_rks[k], truncerr=0.0)
    return y


def distance_rel(x, target):
    """||x - target|| / ||target|| through dot, as the device driver computes it."""
    tt = O.dot(target, target)
    return float(np.sqrt(max(O.dot(x, x) - 2.0 * O.dot(x, target) + tt, 0.0)) / np.sqrt(tt))


def fit_fixed_rank(target, x0, iters):
    """x <- retract(P_x target) (alpha = 0), `iters` times.  Returns (x, errors after every iteration)."""
    x, errs = x0, []
    for _ in range(iters):
        U, V = gauges(x)
        xi, _ = project(U, V, target)
        x = retract(U, V, xi, 1.0, 0.0)
        errs.append(distance_rel(x, target))
    return x, errs


def rayleigh(A, x):
    return O.dot(x, O.apply(A, x)) / O.dot(x, x)


ARMIJO_C = 1.0e-4
MAX_HALVINGS = 40


def rayleigh_descent(A, x0, iters, step, backtrack=True):
    """Riemannian steepest descent of <x, A x> / <x, x>: z = A x, xi = P_x z, rho = <x, z> / <x, x>, grad = 2 (xi - rho x) / <x, x>,
    x - t grad = (1 + 2 t rho / <x, x>) x - (2 t / <x, x>) xi in one to_tt, retracted and normalised.  With ``backtrack`` t is halved until
    E(new) <= E - c t ||grad||^2, ||grad||^2 = 4 (<xi, xi> - rho^2 <x, x>) / <x, x>^2 (at most MAX_HALVINGS times, else the point stays);
    the energies are then the accepted ones.  Returns (x, energies: start, then every iteration)."""
    x = x0
    t = float(step)
    energies = [rayleigh(A, x)] if backtrack else []
    for _ in range(iters):
        U, V = gauges(x)
        z = O.apply(A, x)
        xi, xz = project(U, V, z)
        nn = O.dot(x, x)
        rho = xz / nn
        if not backtrack:
            energies.append(rho)
            y = retract(U, V, xi, -2.0 * t / nn, 1.0 + 2.0 * t * rho / nn)
            x = O.scale(1.0 / O.norm(y), y)
            continue
        E = energies[-1]
        g2 = 4.0 * (tangent_inner(xi, xi) - rho * rho * nn) / (nn * nn)
        accepted = False
        for _h in range(MAX_HALVINGS):
            y = retract(U, V, xi, -2.0 * t / nn, 1.0 + 2.0 * t * rho / nn)
            Etry = rayleigh(A, y)
            if Etry <= E - ARMIJO_C * t * g2:
                accepted = True
                break
            t /= 2
        if accepted:
            x = O.scale(1.0 / O.norm(y), y)
            energies.append(Etry)
        else:
            energies.append(E)
    if not backtrack:
        energies.append(rayleigh(A, x))
    return x, energies


# ---- the dense projector ---------------------------------------------------------------------------------------------------------------
def dense_projector(x):
    """The orthogonal projector onto the tangent space at x as a dense matrix, from the Jacobian of the train map cores -> tensor (one
    column per core entry; the map is linear in each core): P = Q Q^T with Q an orthonormal basis of the Jacobian's range."""
    cols = []
    for k in range(x.N):
        for e in range(x.ttv_vec[k].size):
            cores = [c.copy() for c in x.ttv_vec]
            unit = np.zeros(cores[k].size)
            unit[e] = 1.0
            cores[k] = unit.reshape(cores[k].shape)
            cols.append(O.ttv_to_tensor(O.TTvector(x.N, cores, x.ttv_dims, list(x.ttv_rks), [0] * x.N)).reshape(-1))
    J = np.array(cols).T
    Q, s, _ = np.linalg.svd(J, full_matrices=False)
    rank = int(np.sum(s > 1e-10 * s[0]))
    Q = Q[:, :rank]
    return Q @ Q.T


def manifold_dimension(dims, rks):
    """sum_k n_k r_{k-1} r_k - sum of the interior r_k^2: the dimension of the fixed-rank manifold."""
    return sum(dims[k] * rks[k] * rks[k + 1] for k in range(len(dims))) - sum(r * r for r in rks[1:-1])


# ---- the reference's Manopt extension ----------------------------------------------------------------------------------------------------
class TTManifold:
    """ext/TensorTrainNumericsManoptExt on oracle trains: TTVectorSpace and its methods."""

    def __init__(self, x):
        self.dims = tuple(x.ttv_dims)
        self.ranks = list(x.ttv_rks)                     # a copy, not an alias (test_manopt.jl:10)

    def representation_size(self):
        return self.dims

    def zero_vector(self, p):
        return O.zeros_tt(p.ttv_dims, p.ttv_rks)

    def copy(self, p):
        return O.copy_tt(p)

    def inner(self, p, X, Y):
        return float(np.real(O.dot(X, Y)))

    def norm(self, p, X):
        return float(np.sqrt(max(self.inner(p, X, X), 0.0)))

    def distance(self, p, q):
        return self.norm(p, O.sub(p, q))

    def retract_project(self, p, X, t=1.0):
        return O.orthogonalize(O.add(p, O.scale(t, X)))


def ttvector_manifold(x):
    return TTManifold(x)
