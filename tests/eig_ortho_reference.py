"""CPU restatement of the penalised two-site eigensolvers (csrc/ttn_eig_ortho_kernels.h) for the tests, on top of eig_reference.py: the
walk, rank rules and core moves of ER.two_site_eigsolve with the local problem

    K_eff = 1/2 (K + K^T) + sum_j w_j p_j p_j^T,

p_j the projection of phi_j / ||phi_j|| onto the two-site basis of the window.  Per phi_j two chains of overlap environments are walked
INCREMENTALLY, as the kernel walks them: all right chains R_j[k] (r_k x p_k, the cores k .. d-1 of x and phi_j contracted) are built
once after orthogonalize(x0); a right move of window i advances the left chain to L_j[i+1] from the new core i, a left move the right
chain to R_j[i+1] from the new core i+1.  Nothing is rebuilt per window.  Local problems: numpy.linalg.eigh of the penalised dense
matrix, or scipy's eigsh on the penalised operator applied matrix-free.  With no phi the local solver is ER.local_eig itself and the
function returns ER.two_site_eigsolve's result bit for bit.  Also free_fermion_levels, the lowest levels of the open Ising chain."""
import math

import numpy as np
import scipy.linalg as sla
from scipy.sparse.linalg import LinearOperator, eigsh

from oracle import tt_oracle as O
from tests import eig_reference as ER


def _advance_left(L, xk, pk):
    # L[k+1][be, be'] = sum x_k[s, al, be] L[k][al, al'] phi_k[s, al', be']
    return np.einsum("sab,ac,scd->bd", xk, L, pk, optimize=True)


def _advance_right(R, xk, pk):
    # R[k][be, be'] = sum x_k[t, be, ga] R[k+1][ga, ga'] phi_k[t, be', ga']
    return np.einsum("sab,bd,scd->ac", xk, R, pk, optimize=True)


def local_eig_penalised(Gi, Hi, V0, ps, ws, iterative, linsolv_tol, linsolv_maxiter, info=None):
    """(lambda, V) of the smallest eigenpair of K_eff; ps: the projected vectors (N,), ws their weights.  info["min_gap"] keeps the
    smallest distance between the two lowest eigenvalues of a dense K_eff (N >= 2): below it the vector is not determined."""
    kd = (Gi.shape[0], Gi.shape[1], Hi.shape[1], Hi.shape[2])
    N = int(np.prod(kd))
    K = np.reshape(np.einsum("abefz,zcdgh->abcdefgh", Gi, Hi, optimize=True), (N, N), order="F")
    Ks = 0.5 * (K + K.T)
    if iterative and N > 2:
        def mv(v):
            v = np.reshape(v, N)
            out = Ks @ v
            for w, p in zip(ws, ps):
                out = out + w * p * float(p @ v)
            return out
        v0 = np.reshape(V0, N, order="F")
        if not np.any(v0):
            v0 = np.ones(N)
        lam, v = eigsh(LinearOperator((N, N), matvec=mv, dtype=np.float64), k=1, which="SA", v0=v0, tol=linsolv_tol,
                       maxiter=max(linsolv_maxiter, 1) * N)
        lam, vec = float(lam[0]), v[:, 0] / np.linalg.norm(v[:, 0])
    else:
        for w, p in zip(ws, ps):
            Ks = Ks + w * np.outer(p, p)
        lam, v = np.linalg.eigh(Ks)
        if info is not None and N >= 2:
            info["min_gap"] = min(info.get("min_gap", math.inf), float(lam[1] - lam[0]))
        lam, vec = float(lam[0]), v[:, 0]
    return lam, np.reshape(ER._fix_sign(vec), kd, order="F")


def two_site_eigsolve_ortho(mode, A, tt_start, phis, weights, tol=1.0e-12, sweep_schedule=(2,), rmax_schedule=None, it_solver=False,
                            linsolv_maxiter=200, linsolv_tol=None, itslv_thresh=256, info=None):
    """mode 1: dmrg_eigsolve (N = 2), mode 0: mals_eigsolve, penalised against the trains `phis` (any norm) with `weights` (a scalar or one
    per train).  Returns (E, x, r_hist, overlaps): E the local eigenvalues of K_eff, overlaps[j] = <phi_j, x> / ||phi_j|| read from the
    chains at the end of the walk."""
    phis = list(phis)
    m = len(phis)
    ws = [float(w) for w in np.broadcast_to(np.asarray(weights, dtype=np.float64), (m,))] if m else []
    d = A.N
    dims = tuple(tt_start.ttv_dims)
    if rmax_schedule is None:
        rmax_schedule = (math.isqrt(int(np.prod(dims))),) if mode == 1 else (int(round(math.sqrt(int(np.prod(dims))))),)
    assert len(rmax_schedule) == len(sweep_schedule), "Sweep schedule error"
    if linsolv_tol is None:
        linsolv_tol = max(math.sqrt(tol), 1.0e-8)
    thresh = itslv_thresh if mode == 1 else 256
    plan, rmax_final = O.dmrg_sweep_plan(list(sweep_schedule), list(rmax_schedule))
    x = O.orthogonalize(tt_start)
    Av = A.tto_vec
    G = [None] * d
    H = [None] * (d - 1)
    G[0] = np.reshape(Av[0][:, :, 0, :], (dims[0], 1, dims[0], 1, -1))
    H[d - 2] = np.reshape(np.transpose(Av[d - 1], (2, 0, 1, 3)), (-1, dims[d - 1], 1, dims[d - 1], 1))
    for i in range(d - 2, 0, -1):
        H[i - 1] = ER._mals_update_H(x.ttv_vec[i + 1], H[i], Av[i])
    inv_norm = [1.0 / math.sqrt(float(O.dot(p, p))) for p in phis]
    Lc = [[None] * (d + 1) for _ in range(m)]
    Rc = [[None] * (d + 1) for _ in range(m)]
    for j, p in enumerate(phis):
        Lc[j][0] = np.ones((1, 1))
        Rc[j][d] = np.ones((1, 1))
        for k in range(d - 1, 1, -1):
            Rc[j][k] = _advance_right(Rc[j][k + 1], x.ttv_vec[k], p.ttv_vec[k])
    E, r_hist = [], []

    def solve(i):
        Gi = G[i][:, : x.ttv_rks[i], :, : x.ttv_rks[i], :]
        Hi = H[i][:, :, : x.ttv_rks[i + 2], :, : x.ttv_rks[i + 2]]
        V0 = np.einsum("abz,czd->abcd", x.ttv_vec[i], x.ttv_vec[i + 1])
        N = dims[i] * x.ttv_rks[i] * dims[i + 1] * x.ttv_rks[i + 2]
        iterative = it_solver or N > thresh
        if not m:
            return ER.local_eig(Gi, Hi, V0, iterative, linsolv_tol, linsolv_maxiter)
        ps = [np.reshape(np.einsum("ae,seb,tbg,cg->satc", Lc[j][i], p.ttv_vec[i], p.ttv_vec[i + 1], Rc[j][i + 2], optimize=True), N, order="F")
              * inv_norm[j] for j, p in enumerate(phis)]
        return local_eig_penalised(Gi, Hi, V0, ps, ws, iterative, linsolv_tol, linsolv_maxiter, info)

    def move(V, i, right, rmax):
        n1, rl, n2, rr = V.shape
        u, s, vt = sla.svd(np.reshape(V, (n1 * rl, n2 * rr), order="F"), full_matrices=False, lapack_driver="gesdd")
        k = O.cut_off_index(s, tol) if mode == 1 else len(O.sv_trunc(s, tol))
        r = min(k, rmax)
        x.ttv_rks[i + 1] = r
        if right:
            x.ttv_vec[i] = np.reshape(u[:, :r], (n1, rl, r), order="F")
            x.ttv_vec[i + 1] = np.transpose(np.reshape(s[:r, None] * vt[:r, :], (r, n2, rr), order="F"), (1, 0, 2)).copy()
        else:
            x.ttv_vec[i + 1] = np.transpose(np.reshape(vt[:r, :], (r, n2, rr), order="F"), (1, 0, 2)).copy()
            x.ttv_vec[i] = np.reshape(u[:, :r] * s[None, :r], (n1, rl, r), order="F")
        for j, p in enumerate(phis):                                   # the chains follow the move
            if right:
                Lc[j][i + 1] = _advance_left(Lc[j][i], x.ttv_vec[i], p.ttv_vec[i])
            else:
                Rc[j][i + 1] = _advance_right(Rc[j][i + 2], x.ttv_vec[i + 1], p.ttv_vec[i + 1])

    def step(i, right, rmax):
        lam, V = solve(i)
        E.append(lam)
        move(V, i, right, rmax)
        r_hist.append(max(x.ttv_rks))
        if right:
            G[i + 1] = O._als_update_G(x.ttv_vec[i], Av[i + 1], G[i])
        elif i > 0:
            H[i - 1] = ER._mals_update_H(x.ttv_vec[i + 1], H[i], Av[i])

    last = d - 2 if mode == 1 else d - 1
    for rmax in plan:
        for i in range(last):
            step(i, True, rmax)
        for i in range(last if mode == 1 else last - 1, 0 if mode == 1 else -1, -1):
            step(i, False, rmax)
    if mode == 1:
        lam, V = solve(0)
        E.append(lam)
        r_hist.append(max(x.ttv_rks))
        move(V, 0, False, rmax_final)
    x.ttv_ot = [0] + [(-1 if mode == 1 else 1)] * (d - 1)
    # both walks end with a left move of window 0: R[1] is current, one more step gives the 1 x 1 overlap
    overlaps = [float(_advance_right(Rc[j][1], x.ttv_vec[0], p.ttv_vec[0])[0, 0]) * inv_norm[j] for j, p in enumerate(phis)]
    return E, x, r_hist, overlaps


def rayleigh(A, x):
    return float(O.dot(x, O.apply(A, x))) / float(O.dot(x, x))


def lowest_states(mode, A, starts, k, weight, **kw):
    """Levels 0 .. k-1 one after the other, level j against the results of 0 .. j-1.  Returns (energies, states)."""
    xs = []
    for j in range(k):
        xs.append(two_site_eigsolve_ortho(mode, A, starts[j], xs, weight, **kw)[1])
    return [rayleigh(A, x) for x in xs], xs


def level_cases():
    """(name, operator, seed base, solver keywords) of the level tests, CPU and GPU: weight 10, rank-2 random starts from
    level_starts(A, seed base + mode)."""
    import ttn_amd as T
    from tests.helpers import to_oracle
    lap = O.tto_add(O.Delta(8), O.tto_scale(0.5, O.id_tto(8)))
    return [("ising", to_oracle(T.ising_tto(8, J=1.0, h=1.5)), 3, dict(tol=1e-10, sweep_schedule=[4], rmax_schedule=[16])),
            ("lap", lap, 5, dict(tol=1e-10, sweep_schedule=[4], rmax_schedule=[16])),
            ("xxx", to_oracle(T.xxx_tto(6)), 7, dict(tol=1e-10, sweep_schedule=[4], rmax_schedule=[8]))]


def level_starts(A, seed, k=4):
    rng = np.random.default_rng(seed)
    return [O.rand_tt(tuple(A.tto_dims), 2, rng) for _ in range(k)]


def free_fermion_levels(d, J=1.0, h=1.0):
    """(E0, E1, E2) of the open transverse-field Ising chain J sum Z_k Z_{k+1} + h sum X_k: E0 = -1/2 sum eps, E1 = E0 + eps_min,
    E2 = E0 + eps_2, eps the singular values ER.free_fermion_ground_energy uses (the single-particle energies), ascending."""
    M = np.diag(np.full(d, 2.0 * h)) + np.diag(np.full(d - 1, 2.0 * J), 1)
    eps = np.sort(np.linalg.svd(M, compute_uv=False))
    E0 = -0.5 * float(np.sum(eps))
    return E0, E0 + float(eps[0]), E0 + float(eps[1])
