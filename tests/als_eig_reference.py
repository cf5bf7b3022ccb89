"""CPU restatement of the one-site eigensolvers for the tests: als_eigsolve (src/solvers/als.jl:251-326, local problem K_eigmin :72-91)
and als_gen_eigsolv (src/solvers/als.jl:344-426, local problem K_eiggenmin :93-105), in NumPy.

Environments G_i (n_i, r_{i-1}, n_i, r_{i-1}, R_i) and H_i (R_i, r_i, r_i) come from the oracle (_als_update_G / _als_update_H), the QR
core moves are those of its als_linsolve.  Local problems are solved densely: numpy.linalg.eigh on K_s = 1/2 (K + K^T) for the standard
problem, scipy.linalg.eigh(K_s, S_s) for the generalized one (the vector S-normalised).  Every local eigenvector is signed so that its
first entry of largest modulus is positive, as the device does.  Between stages: increase_ranks with exact zero-padding (noise = 0),
orthogonalize, and both environments rebuilt from the new train — also for als_gen_eigsolv, where the reference zero-pads its stale right
environments (deviation 1 of the device); its history is the full 2 (d - 1) (sweep_schedule[end] - 1) entries (deviation 2)."""
import numpy as np
import scipy.linalg as sla

from oracle import tt_oracle as O


def _fix_sign(v):
    k = int(np.argmax(np.abs(v)))
    return -v if v[k] < 0 else v


def _local_matrix(Gi, Hi):
    n, rl, rr = Gi.shape[0], Gi.shape[1], Hi.shape[1]
    N = n * rl * rr
    K = np.reshape(np.einsum("abdez,zcf->abcdef", Gi, Hi, optimize=True), (N, N), order="F")
    return 0.5 * (K + K.T)


def increase_ranks(x, rmax):
    """increase_ranks(x, rmax; noise = 0) (src/tt_tools.jl:474-489): zero-padding to r_and_d_to_rks(fill(rmax), dims; rmax)."""
    d = x.N
    rn = O.r_and_d_to_rks([1] + [rmax] * (d - 1) + [1], x.ttv_dims, rmax)
    cores = []
    for i in range(d):
        c = np.zeros((x.ttv_dims[i], rn[i], rn[i + 1]))
        c[:, : x.ttv_rks[i], : x.ttv_rks[i + 1]] = x.ttv_vec[i]
        cores.append(c)
    return O.TTvector(d, cores, tuple(x.ttv_dims), rn, [0] * d)


def _sweeps(A, S, tt_start, sweep_schedule, rmax_schedule):
    d = A.N
    ss = list(sweep_schedule)
    if rmax_schedule is None:
        rmax_schedule = [max(tt_start.ttv_rks)]
    assert len(rmax_schedule) == len(ss), "Sweep schedule error"
    ops = [A] if S is None else [A, S]
    x = O.orthogonalize(tt_start)
    dims = tuple(tt_start.ttv_dims)

    def init_env():
        G, H = [], []
        for Op in ops:
            g = [None] * d
            g[0] = np.reshape(Op.tto_vec[0][:, :, 0, :], (dims[0], 1, dims[0], 1, -1))
            h = [None] * d
            h[d - 1] = np.ones((1, 1, 1))
            for i in range(d - 1, 0, -1):
                h[i - 1] = O._als_update_H(x.ttv_vec[i], Op.tto_vec[i], h[i])
            G.append(g)
            H.append(h)
        return G, H

    def local(i, G, H):
        Ks = _local_matrix(G[0][i], H[0][i])
        if S is None:
            w, v = np.linalg.eigh(Ks)
            lam, vec = float(w[0]), v[:, 0]
        else:
            Ss = _local_matrix(G[1][i], H[1][i])
            w, v = sla.eigh(Ks, Ss)
            lam, vec = float(w[0]), v[:, 0]
        return lam, np.reshape(_fix_sign(vec), (dims[i], x.ttv_rks[i], x.ttv_rks[i + 1]), order="F")

    E = []
    G, H = init_env()
    nsweeps, stage = 0, 0
    while True:
        nsweeps += 1
        if nsweeps == ss[stage]:
            stage += 1
            if stage >= len(ss):
                return E, x
            x = O.orthogonalize(increase_ranks(x, rmax_schedule[stage]))
            G, H = init_env()
        for i in range(d - 1):                                               # als.jl:302-309
            lam, V = local(i, G, H)
            E.append(lam)
            n, rim, ri = dims[i], x.ttv_rks[i], x.ttv_rks[i + 1]
            Q, R = np.linalg.qr(np.reshape(V, (n * rim, ri), order="F"))
            x.ttv_vec[i] = np.reshape(Q[:, :ri], (n, rim, ri), order="F")
            x.ttv_vec[i + 1] = np.einsum("bz,azc->abc", R[:ri, :], x.ttv_vec[i + 1])
            for k, Op in enumerate(ops):
                G[k][i + 1] = O._als_update_G(x.ttv_vec[i], Op.tto_vec[i + 1], G[k][i])
        for i in range(d - 1, 0, -1):                                        # als.jl:312-318
            lam, V = local(i, G, H)
            E.append(lam)
            n, rim, ri = dims[i], x.ttv_rks[i], x.ttv_rks[i + 1]
            Q, R = np.linalg.qr(np.reshape(np.transpose(V, (0, 2, 1)), (n * ri, rim), order="F"))
            x.ttv_vec[i] = np.transpose(np.reshape(Q[:, :rim], (n, ri, rim), order="F"), (0, 2, 1)).copy()
            x.ttv_vec[i - 1] = np.einsum("abz,cz->abc", x.ttv_vec[i - 1], R[:rim, :])
            for k, Op in enumerate(ops):
                H[k][i - 1] = O._als_update_H(x.ttv_vec[i], Op.tto_vec[i], H[k][i])
        x.ttv_ot = [0] + [1] * (d - 1)


def als_eigsolve(A, tt_start, sweep_schedule=(2,), rmax_schedule=None):
    """(E, x) of als_eigsolve with noise = 0 and dense local solves."""
    return _sweeps(A, None, tt_start, sweep_schedule, rmax_schedule)


def als_gen_eigsolv(A, S, tt_start, sweep_schedule=(2,), rmax_schedule=None):
    """(E, x) of als_gen_eigsolv with dense local solves, environments rebuilt after a rank increase, the full history."""
    return _sweeps(A, S, tt_start, sweep_schedule, rmax_schedule)


def full_vector(x):
    """The train as a vector (in the order of qtto_to_matrix), signed like a local eigenvector."""
    return _fix_sign(np.asarray(O.qtt_to_vector(x), dtype=float))
