"""NumPy restatement of the pullback of s = <x, A y> on the three-layer environments, written from the formulas (plain einsum, one
contraction at a time in the stated order; it shares no code with the product):

    L_1 = [1],      L_{k+1}[a, r, b]  = sum L_k[al, rl, bl] x_k[i, al, a] A_k[i, j, rl, r] y_k[j, bl, b]
    G_{N+1} = [1],  G_k[al, rl, bl]   = sum G_{k+1}[a, r, b] x_k[i, al, a] A_k[i, j, rl, r] y_k[j, bl, b]
    xbar_k[i, al, a] = delta sum L_k[al, rl, bl] A_k[i, j, rl, r] y_k[j, bl, b] G_{k+1}[a, r, b]
    ybar_k[j, bl, b] = delta sum L_k[al, rl, bl] x_k[i, al, a] A_k[i, j, rl, r] G_{k+1}[a, r, b]

and the Rayleigh gradient built on it.  Cores: x_k (n, r_l, r_r), A_k (n, n, R_l, R_r) with the first physical index the output index.

Rounding bounds (``sandwich_pullback_bound``), derived as tests/grad_reference.py derives ``dot_pullback_bound``: a nested sum of products
evaluated in any order, FMA or not, satisfies |fl - exact| <= p eps S_abs, S_abs the same formula on absolute values, p the number of terms
along the longest chain.  The chain of one entry, every contraction a sum in any order:

    one step of the L chain at site m      l_m = ry_m + n_m R_m + n_m rx_m              (over bl; over (j, rl); over (i, al))
    one step of the G chain at site m      g_m = ry_{m+1} + n_m R_{m+1} + n_m rx_{m+1}  (over b;  over (j, r);  over (i, a))
    the gradient's own three contractions  xbar_k: ry_k + n_k R_k + R_{k+1} ry_{k+1}    (over bl; over (j, rl); over (r, b))
                                           ybar_k: rx_k + n_k R_k + R_{k+1} rx_{k+1}    (over al; over (i, rl); over (r, a))
    the product with delta                 1

    p(xbar_k) = sum_{m < k} l_m + sum_{m > k} g_m + ry_k + n_k R_k + R_{k+1} ry_{k+1} + 1,      p(ybar_k) likewise,      p(s) = sum_m l_m

(0-based ranks rx_m: the left rank of site m).  Device and restatement both round: the returned bounds are 2 p eps S_abs per entry."""
import numpy as np

from oracle import tt_oracle as O
from tests import grad_reference as GR

EPS = GR.EPS


def _f(c):
    return np.asarray(c, dtype=np.float64)


def environments(x, A, y):
    """L[k], G[k] for k = 0 .. N (0-based: L[0] = G[N] = [1]), each (rx_k, R_k, ry_k)."""
    N = x.N
    L, G = [None] * (N + 1), [None] * (N + 1)
    L[0] = np.zeros((x.ttv_rks[0], A.tto_rks[0], y.ttv_rks[0]))
    L[0][0, 0, 0] = 1.0
    for k in range(N):
        U = np.einsum("agb,jbB->agjB", L[k], _f(y.ttv_vec[k]))
        V = np.einsum("agjB,ijgG->aiGB", U, _f(A.tto_vec[k]))
        L[k + 1] = np.einsum("aiGB,iaA->AGB", V, _f(x.ttv_vec[k]))
    G[N] = np.zeros((x.ttv_rks[N], A.tto_rks[N], y.ttv_rks[N]))
    G[N][0, 0, 0] = 1.0
    for k in range(N - 1, -1, -1):
        U = np.einsum("AGB,jbB->AGjb", G[k + 1], _f(y.ttv_vec[k]))
        V = np.einsum("AGjb,ijgG->Aigb", U, _f(A.tto_vec[k]))
        G[k] = np.einsum("Aigb,iaA->agb", V, _f(x.ttv_vec[k]))
    return L, G


def sandwich_pullback(x, A, y, delta=1.0):
    """(<x, A y>, xbar cores, ybar cores) for the cotangent delta; the contraction order of the issue: L with the other train's core, the
    operator core, then G."""
    L, G = environments(x, A, y)
    xbar, ybar = [], []
    for k in range(x.N):
        Ak = _f(A.tto_vec[k])
        T1 = np.einsum("agb,jbB->agjB", L[k], _f(y.ttv_vec[k]))
        T2 = np.einsum("agjB,ijgG->aiGB", T1, Ak)
        xbar.append(delta * np.einsum("aiGB,AGB->iaA", T2, G[k + 1]))
        T1 = np.einsum("agb,iaA->gbiA", L[k], _f(x.ttv_vec[k]))
        T2 = np.einsum("gbiA,ijgG->bjGA", T1, Ak)
        ybar.append(delta * np.einsum("bjGA,AGB->jbB", T2, G[k + 1]))
    return float(L[x.N][0, 0, 0]), xbar, ybar


def chain_terms(x, A, y):
    """(p(s), [p(xbar_k)], [p(ybar_k)]): the number of terms along the longest chain (module docstring)."""
    N, n, rx, R, ry = x.N, x.ttv_dims, x.ttv_rks, A.tto_rks, y.ttv_rks
    l = [ry[m] + n[m] * R[m] + n[m] * rx[m] for m in range(N)]
    g = [ry[m + 1] + n[m] * R[m + 1] + n[m] * rx[m + 1] for m in range(N)]
    px = [sum(l[:k]) + sum(g[k + 1:]) + ry[k] + n[k] * R[k] + R[k + 1] * ry[k + 1] + 1 for k in range(N)]
    py = [sum(l[:k]) + sum(g[k + 1:]) + rx[k] + n[k] * R[k] + R[k + 1] * rx[k + 1] + 1 for k in range(N)]
    return sum(l), px, py


def _abs_tt(x):
    return O.TTvector(x.N, [np.abs(c) for c in x.ttv_vec], x.ttv_dims, list(x.ttv_rks), list(x.ttv_ot))


def _abs_tto(H):
    return O.TToperator(H.N, [np.abs(c) for c in H.tto_vec], H.tto_dims, list(H.tto_rks), list(H.tto_ot))


def sandwich_pullback_bound(x, A, y, delta=1.0):
    """(value bound, xbar bounds, ybar bounds): 2 p eps S_abs per entry, p from ``chain_terms``."""
    ps, px, py = chain_terms(x, A, y)
    v, xb, yb = sandwich_pullback(_abs_tt(x), _abs_tto(A), _abs_tt(y), abs(delta))
    return 2.0 * ps * EPS * v, [2.0 * p * EPS * c for p, c in zip(px, xb)], [2.0 * p * EPS * c for p, c in zip(py, yb)]


def expect_value_and_grad(H, psi):
    s, xb, yb = sandwich_pullback(psi, H, psi, 1.0)
    return s, [a + b for a, b in zip(xb, yb)]


def rayleigh_value_and_grad(H, psi):
    """E = <psi, H psi> / <psi, psi> and dE / d(cores of psi) from the three-layer pullback at 1 / <psi, psi> and the pullback of
    dot(psi, psi) at -E / <psi, psi>: no H psi anywhere."""
    nn = O.dot(psi, psi)
    num, xb, yb = sandwich_pullback(psi, H, psi, 1.0 / nn)
    E = num / nn
    _, g3, g4 = GR.dot_pullback(psi, psi, -E / nn)
    return E, [a + b + c + e for a, b, c, e in zip(xb, yb, g3, g4)]


def _rayleigh_bound(H, psi, sand_factor_x, sand_factor_y, num_factor):
    """Per-core bound of the Rayleigh gradient g = (xbar + ybar) / nn - (E / nn) (abar + bbar) between two evaluations that both round:
    sand_factor_* are the per-core factors (in units of eps) that multiply S_abs of xbar / ybar for the two evaluations together,
    num_factor the same for the numerator <psi, H psi>.  Besides the pullbacks' own bounds the two cotangents differ between the
    evaluations, by the value bounds of nn and of the numerator and a few roundings, and the three sums of four terms round three times
    on each side."""
    nn = O.dot(psi, psi)
    num = O.dot(psi, O.apply(H, psi))
    E = num / nn
    an, aH = _abs_tt(psi), _abs_tto(H)
    _, sx, sy = sandwich_pullback(an, aH, an, 1.0 / nn)                     # S_abs of the two sandwich tangents at 1 / nn
    vnum = sandwich_pullback(an, aH, an, 1.0)[0]
    bnn, ba, bb = GR.dot_pullback_bound(psi, psi, -E / nn)
    _, sa, sb = GR.dot_pullback(an, an, abs(E) / nn)                        # S_abs of the two dot tangents at |E| / nn
    rel_nn = bnn / nn                                                      # the two <psi, psi> (the value bound is not scaled by delta)
    dnum = num_factor * EPS * vnum                                         # the two numerators
    d1 = rel_nn + 4 * EPS                                                  # relative difference of the two 1 / nn
    dE = (dnum + abs(num) * rel_nn) / nn + 4 * EPS * abs(E)
    d2 = dE / abs(E) + rel_nn + 4 * EPS if E != 0 else 0.0                 # relative difference of the two E / nn (E = 0: S_abs of sa, sb is 0 too)
    out = []
    for k in range(psi.N):
        own = sand_factor_x[k] * EPS * sx[k] + sand_factor_y[k] * EPS * sy[k] + ba[k] + bb[k]
        coef = d1 * (sx[k] + sy[k]) + d2 * (sa[k] + sb[k])
        sums = 2 * 3 * EPS * (sx[k] + sy[k] + sa[k] + sb[k])
        out.append(own + coef + sums)
    return out


def rayleigh_fused_bound(H, psi):
    """Per-core bound between the device's fused Rayleigh gradient and ``rayleigh_value_and_grad`` above (both three-layer, both round)."""
    ps, px, py = chain_terms(psi, H, psi)
    return _rayleigh_bound(H, psi, [2 * p for p in px], [2 * p for p in py], 2 * ps)


def rayleigh_composed_bound(H, psi):
    """Per-core bound between the three-layer form (one side) and the composition dot_pullback(psi, H psi) + apply_pullback (the other):
    the composition is another nesting of the same sum of products, so the same S_abs applies with its own chain length — per site the
    two-layer step on ranks (r, R r), n r (R r) + r' (R' r') terms as ``GR.dot_pullback_bound`` counts them, the n terms of a core of
    H psi, and the n R R' + 1 terms of ``GR.apply_pullback_bound``."""
    ps, px, py = chain_terms(psi, H, psi)
    n, r, R = psi.ttv_dims, psi.ttv_rks, H.tto_rks
    pc = sum(n[k] * r[k] * r[k] * R[k] + r[k + 1] * r[k + 1] * R[k + 1] + n[k] for k in range(psi.N)) + max(n[k] * R[k] * R[k + 1] + 1 for k in range(psi.N))
    return _rayleigh_bound(H, psi, [p + pc for p in px], [p + pc for p in py], ps + pc)
