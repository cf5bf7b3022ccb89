"""NumPy restatement of the reference's ChainRulesCore extension (ext/TensorTrainNumericsChainRulesCoreExt.jl) on oracle trains: the
environments of a pair of trains (:8-34), the pullback of dot(A, B) (:36-65), the pullback of H * psi (:67-88), the Rayleigh quotient and
its gradient composed from them (test/test_ad.jl:104-113) and the fixed-rank gradient descent of test_ad.jl:116-156.  Plain einsum; it
shares no code with the product."""
import numpy as np

from oracle import tt_oracle as O

EPS = np.finfo(np.float64).eps


def environments(A, B):
    """L[k] (k = 0..N) and G[k] (k = 0..N), 0-based: L[0] = G[N] = [1]; each r^A_k x r^B_k."""
    N = A.N
    L = [None] * (N + 1)
    G = [None] * (N + 1)
    L[0] = np.zeros((A.ttv_rks[0], B.ttv_rks[0]))
    L[0][0, 0] = 1.0
    for k in range(N):
        L[k + 1] = np.einsum("zxa,zyb,xy->ab", A.ttv_vec[k], B.ttv_vec[k], L[k], optimize=True)
    G[N] = np.zeros((A.ttv_rks[N], B.ttv_rks[N]))
    G[N][0, 0] = 1.0
    for k in range(N - 1, -1, -1):
        G[k] = np.einsum("zxa,zyb,ab->xy", A.ttv_vec[k], B.ttv_vec[k], G[k + 1], optimize=True)
    return L, G


def dot_pullback(A, B, delta=1.0):
    """(dot(A, B), Abar cores, Bbar cores) for the cotangent delta."""
    L, G = environments(A, B)
    abar = [delta * np.einsum("xy,zyb,ab->zxa", L[k], B.ttv_vec[k], G[k + 1], optimize=True) for k in range(A.N)]
    bbar = [delta * np.einsum("xy,zxa,ab->zyb", L[k], A.ttv_vec[k], G[k + 1], optimize=True) for k in range(A.N)]
    return float(L[A.N][0, 0]), abar, bbar


def apply_pullback(H, ybar_cores, x_rks):
    """psibar cores of Y = H * psi for the cotangent cores ybar (ranks H.tto_rks .* x_rks, operator index fastest)."""
    out = []
    for k in range(H.N):
        Hk = H.tto_vec[k]
        n, _, Rl, Rr = Hk.shape
        rl, rr = x_rks[k], x_rks[k + 1]
        Yr = np.reshape(ybar_cores[k], (n, Rl, rl, Rr, rr), order="F")            # [i, al, vl, ar, vr]
        out.append(np.einsum("ijab,iavbw->jvw", Hk, Yr))
    return out


def _abs_tt(x):
    return O.TTvector(x.N, [np.abs(c) for c in x.ttv_vec], x.ttv_dims, list(x.ttv_rks), list(x.ttv_ot))


def _abs_tto(H):
    return O.TToperator(H.N, [np.abs(c) for c in H.tto_vec], H.tto_dims, list(H.tto_rks), list(H.tto_ot))


def dot_pullback_bound(A, B, delta=1.0):
    """Componentwise rounding bounds of the dot pullback: a nested sum of products evaluated in any order (FMA or not) satisfies
    |fl - exact| <= p eps S_abs, S_abs = the same formula on the absolute values, p = the number of terms along the longest chain,
    p = sum_k (n_k r^A_{k-1} r^B_{k-1} + r^A_k r^B_k).  Device and restatement both round: the returned bounds are 2 p eps S_abs.
    Returns (value bound, Abar bounds, Bbar bounds)."""
    p = sum(A.ttv_dims[k] * A.ttv_rks[k] * B.ttv_rks[k] + A.ttv_rks[k + 1] * B.ttv_rks[k + 1] for k in range(A.N))
    v, ab, bb = dot_pullback(_abs_tt(A), _abs_tt(B), abs(delta))
    f = 2.0 * p * EPS
    return f * v, [f * c for c in ab], [f * c for c in bb]


def apply_pullback_bound(H, ybar_cores, x_rks):
    """2 p eps |H| |Ybar| per core, p = n_k R_{k-1} R_k + 1."""
    S = apply_pullback(_abs_tto(H), [np.abs(c) for c in ybar_cores], x_rks)
    return [2.0 * (H.tto_dims[k] * H.tto_rks[k] * H.tto_rks[k + 1] + 1) * EPS * S[k] for k in range(H.N)]


def rayleigh(H, psi):
    return O.dot(psi, O.apply(H, psi)) / O.dot(psi, psi)


def rayleigh_value_and_grad(H, psi):
    """E = <psi, H psi> / <psi, psi> and dE / d(cores of psi), composed from the two rules as AD composes them."""
    Y = O.apply(H, psi)
    nn = O.dot(psi, psi)
    num, g1, ybar = dot_pullback(psi, Y, 1.0 / nn)
    E = num / nn
    g2 = apply_pullback(H, ybar, psi.ttv_rks)
    _, g3, g4 = dot_pullback(psi, psi, -E / nn)
    return E, [a + b + c + e for a, b, c, e in zip(g1, g2, g3, g4)]


def ladot(x, y):
    return float(sum(np.vdot(a, b) for a, b in zip(x, y)))


def with_cores(x, cores):
    return O.TTvector(x.N, [np.array(c) for c in cores], x.ttv_dims, list(x.ttv_rks), [0] * x.N)


def shifted(x, direction, t):
    return with_cores(x, [c + t * dch for c, dch in zip(x.ttv_vec, direction)])


def descend(H, psi0, steps=200, alpha=0.05):
    """The backtracking gradient descent of test_ad.jl:134-151 on the cores at fixed ranks: try theta - alpha g, halve alpha while the
    energy rises (and alpha > 1e-12), accept, let alpha grow by 1.5.  Returns (energies: start, then every accepted step; final train)."""
    psi = psi0
    E = rayleigh(H, psi)
    hist = [E]
    for _ in range(steps):
        _, g = rayleigh_value_and_grad(H, psi)
        cand = shifted(psi, g, -alpha)
        Etry = rayleigh(H, cand)
        while Etry > E and alpha > 1.0e-12:
            alpha /= 2
            cand = shifted(psi, g, -alpha)
            Etry = rayleigh(H, cand)
        psi, E = cand, Etry
        hist.append(E)
        alpha *= 1.5
    return hist, psi
