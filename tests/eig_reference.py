"""CPU restatement of the two-site eigensolvers for the tests: dmrg_eigsolve with N = 2 (src/solvers/dmrg.jl:501-578, local problem
K_eigmin :235-259) and mals_eigsolve (src/solvers/mals.jl:335-425, local problem K_eigmin_mals :171-217), in NumPy.

Both run on the MALS-form environments G_i (n_i, r_i, n_i, r_i, R_{i+1}) / H_i (R_{i+1}, n_{i+1}, r_{i+2}, n_{i+1}, r_{i+2}) — the local
operator K = sum_z G_z (x) H_z equals the reference's three-tensor DMRG sandwich G (x) Amid (x) H up to the order of the unknown's
indices — and differ in the walk (DMRG: windows 0..d-3 forward, d-2..1 backward, then the closing solve at window 0; MALS: 0..d-2
forward, d-2..0 backward), the rank rule (cut_off_index / sv_trunc) and where the closing history entry is taken (dmrg.jl:539-540).
Local problems: numpy.linalg.eigh on the upper triangle (the reference's eigen(Hermitian(K), 1:1)), or scipy's eigsh on 1/2 (K + K^T)
applied matrix-free for the iterative branch.  Every local eigenvector is signed so that its first entry of largest modulus is
positive, as the device does.  Shared pieces come from the oracle: orthogonalize, _als_update_G, sv_trunc, cut_off_index,
dmrg_sweep_plan."""
import math

import numpy as np
import scipy.linalg as sla
from scipy.sparse.linalg import LinearOperator, eigsh

from oracle import tt_oracle as O


def _mals_update_H(x_next, Hi, A):
    # Him[a, i, al, l, be] = conj(x)[j, al, x] * (Hi[z, j, x, k, y] * x[k, be, y]) * A[i, l, a, z]    (mals.jl:10-13)
    return np.einsum("jax,zjxky,kby,ilwz->wialb", x_next, Hi, x_next, A, optimize=True)


def _fix_sign(v):
    k = int(np.argmax(np.abs(v)))
    return -v if v[k] < 0 else v


def local_eig(Gi, Hi, V0, iterative, linsolv_tol, linsolv_maxiter):
    """(lambda, V) of the smallest eigenpair of the two-site problem; V (n1, r_i, n2, r_{i+2}) column-major like the device."""
    kd = (Gi.shape[0], Gi.shape[1], Hi.shape[1], Hi.shape[2])
    N = int(np.prod(kd))
    K = np.reshape(np.einsum("abefz,zcdgh->abcdefgh", Gi, Hi, optimize=True), (N, N), order="F")
    if iterative and N > 2:
        Ks = 0.5 * (K + K.T)
        op = LinearOperator((N, N), matvec=lambda v: Ks @ v, dtype=np.float64)
        v0 = np.reshape(V0, N, order="F")
        if not np.any(v0):
            v0 = np.ones(N)
        w, v = eigsh(op, k=1, which="SA", v0=v0, tol=linsolv_tol, maxiter=max(linsolv_maxiter, 1) * N)
        lam, vec = float(w[0]), v[:, 0] / np.linalg.norm(v[:, 0])
    else:
        w, v = np.linalg.eigh(K, UPLO="U")
        lam, vec = float(w[0]), v[:, 0]
    return lam, np.reshape(_fix_sign(vec), kd, order="F")


def two_site_eigsolve(mode, A, tt_start, tol=1.0e-12, sweep_schedule=(2,), rmax_schedule=None, it_solver=False, linsolv_maxiter=200,
                      linsolv_tol=None, itslv_thresh=256):
    """mode 1: dmrg_eigsolve (N = 2); mode 0: mals_eigsolve.  Returns (E, x, r_hist)."""
    d = A.N
    dims = tuple(tt_start.ttv_dims)
    if rmax_schedule is None:
        rmax_schedule = (math.isqrt(int(np.prod(dims))),) if mode == 1 else (int(round(math.sqrt(int(np.prod(dims))))),)
    assert len(rmax_schedule) == len(sweep_schedule), "Sweep schedule error"
    if linsolv_tol is None:
        linsolv_tol = max(math.sqrt(tol), 1.0e-8)
    thresh = itslv_thresh if mode == 1 else 256          # mals.jl:383-390, :403-410 do not forward itslv_thresh
    plan, rmax_final = O.dmrg_sweep_plan(list(sweep_schedule), list(rmax_schedule))
    x = O.orthogonalize(tt_start)
    Av = A.tto_vec
    G = [None] * d
    H = [None] * (d - 1)
    G[0] = np.reshape(Av[0][:, :, 0, :], (dims[0], 1, dims[0], 1, -1))
    H[d - 2] = np.reshape(np.transpose(Av[d - 1], (2, 0, 1, 3)), (-1, dims[d - 1], 1, dims[d - 1], 1))
    for i in range(d - 2, 0, -1):
        H[i - 1] = _mals_update_H(x.ttv_vec[i + 1], H[i], Av[i])
    E, r_hist = [], []

    def solve(i):
        Gi = G[i][:, : x.ttv_rks[i], :, : x.ttv_rks[i], :]
        Hi = H[i][:, :, : x.ttv_rks[i + 2], :, : x.ttv_rks[i + 2]]
        V0 = np.einsum("abz,czd->abcd", x.ttv_vec[i], x.ttv_vec[i + 1])
        N = dims[i] * x.ttv_rks[i] * dims[i + 1] * x.ttv_rks[i + 2]
        return local_eig(Gi, Hi, V0, it_solver or N > thresh, linsolv_tol, linsolv_maxiter)

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

    def step(i, right, rmax):
        lam, V = solve(i)
        E.append(lam)
        move(V, i, right, rmax)
        r_hist.append(max(x.ttv_rks))
        if right:
            G[i + 1] = O._als_update_G(x.ttv_vec[i], Av[i + 1], G[i])
        elif i > 0:
            H[i - 1] = _mals_update_H(x.ttv_vec[i + 1], H[i], Av[i])

    last = d - 2 if mode == 1 else d - 1                  # windows of a forward half sweep
    for rmax in plan:
        for i in range(last):
            step(i, True, rmax)
        for i in range(last if mode == 1 else last - 1, 0 if mode == 1 else -1, -1):
            step(i, False, rmax)
    if mode == 1:                                          # the closing solve at window 0 (dmrg.jl:530-550)
        lam, V = solve(0)
        E.append(lam)
        r_hist.append(max(x.ttv_rks))
        move(V, 0, False, rmax_final)
    x.ttv_ot = [0] + [(-1 if mode == 1 else 1)] * (d - 1)
    return E, x, r_hist


def dmrg_eigsolve(A, tt_start, **kw):
    return two_site_eigsolve(1, A, tt_start, **kw)


def mals_eigsolve(A, tt_start, **kw):
    return two_site_eigsolve(0, A, tt_start, **kw)


def free_fermion_ground_energy(d, J=1.0, h=1.0):
    """Ground energy of the open transverse-field Ising chain J sum Z_k Z_{k+1} + h sum X_k: -1/2 sum of the singular values of the d x d
    upper-bidiagonal matrix with diagonal 2h and superdiagonal 2J."""
    M = np.diag(np.full(d, 2.0 * h)) + np.diag(np.full(d - 1, 2.0 * J), 1)
    return -0.5 * float(np.sum(np.linalg.svd(M, compute_uv=False)))
