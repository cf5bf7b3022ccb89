"""NumPy / SciPy restatement of TT-cross (src/tt_cross_interpolation.jl: MaxVol and DMRG cross, maxvol, the index helpers), the
yardstick of tests/test_cpu_cross.py and tests/test_gpu_cross.py.

Arrays are in the reference's index order: cores (n, r_left, r_right), index matrices (rows x cols, 1-based int64), reshapes in
column-major order.  Initial maxvol rows come from scipy.linalg.lu_factor (getrf), the QR from numpy.linalg.qr, the SVD from LAPACK
(numpy.linalg.svd) with the reference's relative-tail rank rule.  The random draws use the product's own helper (draw_indices), so
both sides see the same index sets.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.linalg as sl

import ttn_amd

X = ttn_amd.cross
draw_indices = X.draw_indices
_cap_ranks_ = X._cap_ranks_
_gauss_legendre = X._gauss_legendre


def maxvol(A, tol=1.05, maxiter=100):
    """(piv 1-based in column order, C = A / A[piv,:], swaps): LU rows, then swaps at the largest |C_ij| (first in column-major
    order) while it exceeds tol, C updated by Sherman-Morrison; the returned C solved again from scratch."""
    A = np.asarray(A)
    A = A.astype(np.complex128 if np.iscomplexobj(A) else np.float64)
    m, r = A.shape
    lu, ipiv = sl.lu_factor(A, check_finite=False)
    perm = np.arange(m)
    for j in range(r):
        perm[j], perm[ipiv[j]] = perm[ipiv[j]], perm[j]
    L1 = np.tril(lu[:r], -1) + np.eye(r)
    Cp = np.empty_like(A)
    Cp[:r] = np.eye(r)
    if m > r:
        Cp[r:] = sl.solve_triangular(L1, lu[r:].T, trans="T", lower=True, unit_diagonal=True).T
    C = np.empty_like(A)
    C[perm] = Cp
    piv = perm[:r].copy()
    swaps = 0
    while swaps < maxiter:
        a = np.abs(C)
        lin = int(np.argmax(a.reshape(-1, order="F")))
        i, j = lin % m, lin // m
        if not a[i, j] > tol:
            break
        fcol = C[:, j] * (1.0 / C[i, j])
        row = C[i].copy()
        row[j] -= 1.0
        C = C - np.outer(fcol, row)
        piv[j] = i
        swaps += 1
    B = A[piv]
    Cf = sl.lu_solve(sl.lu_factor(B, check_finite=False), A.T, trans=1, check_finite=False).T
    return piv + 1, Cf, swaps


def _svd_rank(s, max_bond, truncerr):
    r = len(s)
    if truncerr > 0:
        nrm = float(np.linalg.norm(s))
        cum = 0.0
        for i in range(r, 0, -1):
            cum += float(s[i - 1]) ** 2
            if math.sqrt(cum) > truncerr * nrm:
                r = i
                break
    return min(r, int(max_bond))


def _qr(A):
    return np.linalg.qr(A, mode="reduced")[0]


def _evaluate_on_domain(f, domain, indices):
    indices = np.asarray(indices, dtype=np.int64)
    coords = np.stack([np.asarray(domain[d])[indices[:, d] - 1] for d in range(len(domain))], axis=1)
    return np.asarray(f(coords)).reshape(-1)


def _evaluate_tt(cores, indices, N):
    indices = np.asarray(indices, dtype=np.int64)
    state = np.ones((indices.shape[0], 1), dtype=np.result_type(*cores))
    for d in range(N):
        slices = cores[d][indices[:, d] - 1]                      # (P, r_left, r_right)
        state = np.einsum("pa,pab->pb", state, slices)
    return state.reshape(-1)


def _contract_with_weights(cores, weights):
    result = np.ones(1, dtype=np.result_type(*cores, *weights))
    for k, c in enumerate(cores):
        contracted = sum(weights[k][i] * c[i] for i in range(c.shape[0]))
        result = np.conj(result) @ contracted
    return result[0]


def _build_fiber_indices(lsets, rsets, j, Is, Rs, N):
    """(1-based j, lists indexed 1..N)"""
    out = np.empty((Rs[j] * Is[j] * Rs[j + 1], N), dtype=np.int64)
    idx = 0
    for rr in range(Rs[j + 1]):
        for rl in range(Rs[j]):
            for i in range(Is[j]):
                if j > 1:
                    out[idx, : j - 1] = lsets[j][rl]
                out[idx, j - 1] = i + 1
                if j < N:
                    out[idx, j:] = rsets[j][rr]
                idx += 1
    return out


def _superblock_indices(I_l, I_g, k, Is, N):
    r_l, r_g = I_l[k].shape[0], I_g[k + 1].shape[0]
    s1, s2 = Is[k], Is[k + 1]
    out = np.empty((r_l * s1 * s2 * r_g, N), dtype=np.int64)
    idx = 0
    for rg in range(r_g):
        for i2 in range(s2):
            for i1 in range(s1):
                for rl in range(r_l):
                    if k > 1:
                        out[idx, : k - 1] = I_l[k][rl]
                    out[idx, k - 1] = i1 + 1
                    out[idx, k] = i2 + 1
                    if k + 1 < N:
                        out[idx, k + 1:] = I_g[k + 1][rg]
                    idx += 1
    return out


def _sample_superblock(f, domain, I_l, I_g, k, Is, N):
    r_l, r_g = I_l[k].shape[0], I_g[k + 1].shape[0]
    v = _evaluate_on_domain(f, domain, _superblock_indices(I_l, I_g, k, Is, N))
    return v.reshape((r_l, Is[k], Is[k + 1], r_g), order="F")


def _combine_indices_left(I_l_k, s):
    r_l, nc = I_l_k.shape
    out = np.zeros((r_l * s, nc + 1), dtype=np.int64)
    idx = 0
    for i in range(s):
        for r in range(r_l):
            out[idx, :nc] = I_l_k[r]
            out[idx, nc] = i + 1
            idx += 1
    return out


def _combine_indices_right(s, I_g_k):
    r_g, nc = I_g_k.shape
    out = np.zeros((s * r_g, nc + 1), dtype=np.int64)
    idx = 0
    for r in range(r_g):
        for i in range(s):
            out[idx, 0] = i + 1
            out[idx, 1:] = I_g_k[r]
            idx += 1
    return out


def _domain(domain):
    if all(isinstance(d, (int, np.integer)) for d in domain):
        return [np.arange(1.0, d + 1.0) for d in domain]
    cplx = any(np.iscomplexobj(d) for d in domain)
    return [np.asarray(d, dtype=np.complex128 if cplx else np.float64) for d in domain]


def _ranks(ranks, N, Is, rmax):
    Rs = [None, 1] + ([int(ranks)] * (N - 1) if isinstance(ranks, (int, np.integer)) else list(ranks)) + [1]
    return _cap_ranks_(Rs, Is, rmax)


def _vt(f, domain):
    v = _evaluate_on_domain(f, domain, np.ones((1, len(domain)), dtype=np.int64))
    return np.complex128 if np.iscomplexobj(v) else np.float64


def cross_maxvol(f, domain, tol=1e-10, maxiter=50, rmax=500, kickrank=5, ptol=1.05, pmaxiter=100, ranks=2, val_size=1000, seed=0):
    """tt_cross(f, domain, MaxVol(...)): (cores, ranks of the cores, trace {eps, lsets, rsets, sweeps})"""
    domain = _domain(domain)
    N = len(domain)
    Is = [None] + [len(d) for d in domain]
    Tv = _vt(f, domain)
    Rs = _ranks(ranks, N, Is, rmax)
    cores = [None] * (N + 1)
    lsets, rsets = [None] * (N + 1), [None] * (N + 1)
    max_R = max(Rs[1:])
    randint = draw_indices(seed, X.DRAW_MAXVOL_RSETS, 0, 0, max_R, Is[1:])
    for n in range(1, N):
        rsets[n] = randint[: Rs[n + 1], n:]
    Xs_val = draw_indices(seed, X.DRAW_VALIDATION, 0, 0, val_size, Is[1:])
    ys_val = _evaluate_on_domain(f, domain, Xs_val).astype(Tv)
    norm_ys = max(np.linalg.norm(ys_val), tol)
    hist = []
    for it in range(1, maxiter + 1):
        for j in range(1, N):
            V = _evaluate_on_domain(f, domain, _build_fiber_indices(lsets, rsets, j, Is, Rs, N)).astype(Tv)
            V = V.reshape((Rs[j] * Is[j], Rs[j + 1]), order="F")
            Q = _qr(V)
            piv, G, _ = maxvol(Q, ptol, pmaxiter)
            r = len(piv)
            cores[j] = G.reshape((Is[j], Rs[j], r), order="F")
            li, lr = (piv - 1) % Is[j] + 1, (piv - 1) // Is[j]
            lsets[j + 1] = li.reshape(-1, 1) if j == 1 else np.hstack([lsets[j][lr], li.reshape(-1, 1)])
            Rs[j + 1] = r
        for j in range(N, 1, -1):
            V = _evaluate_on_domain(f, domain, _build_fiber_indices(lsets, rsets, j, Is, Rs, N)).astype(Tv)
            V3 = V.reshape((Is[j], Rs[j], Rs[j + 1]), order="F")
            Vr = np.transpose(V3, (1, 0, 2)).reshape((Rs[j], Is[j] * Rs[j + 1]), order="F")
            Q = _qr(Vr.T)
            piv, G, _ = maxvol(Q, ptol, pmaxiter)
            r = len(piv)
            cores[j] = np.transpose(G.reshape((Is[j], Rs[j + 1], r), order="F"), (0, 2, 1))
            li, lr = (piv - 1) % Is[j] + 1, (piv - 1) // Is[j]
            rsets[j - 1] = li.reshape(-1, 1) if j == N else np.hstack([li.reshape(-1, 1), rsets[j][lr]])
            Rs[j] = r
        V = _evaluate_on_domain(f, domain, _build_fiber_indices(lsets, rsets, 1, Is, Rs, N)).astype(Tv)
        cores[1] = V.reshape((Is[1], Rs[1], Rs[2]), order="F")
        eps = np.linalg.norm(ys_val - _evaluate_tt(cores[1:], Xs_val, N)) / norm_ys
        hist.append(eps)
        if eps < tol:
            break
        if kickrank is not None:
            newRs = list(Rs)
            for n in range(2, N + 1):
                newRs[n] = min(newRs[n] + kickrank, rmax)
            _cap_ranks_(newRs, Is, rmax)
            for n in range(1, N):
                if newRs[n + 1] > Rs[n + 1]:
                    extra = draw_indices(seed, X.DRAW_KICK, it, n, newRs[n + 1] - Rs[n + 1], Is[n + 1:])
                    rsets[n] = np.vstack([rsets[n][: Rs[n + 1]], extra])
            Rs = newRs
    out = cores[1:]
    return out, [1] + [c.shape[2] for c in out], dict(eps=hist, sweeps=len(hist), lsets=lsets, rsets=rsets)


def cross_dmrg(f, domain, tol=1e-10, maxiter=50, rmax=500, ptol=1.05, pmaxiter=100, ranks=2, val_size=1000, seed=0):
    """tt_cross(f, domain, DMRG(...)): (cores, ranks, trace {eps, I_l, I_g, sweeps})"""
    domain = _domain(domain)
    N = len(domain)
    Is = [None] + [len(d) for d in domain]
    Tv = _vt(f, domain)
    if N == 1:
        v = _evaluate_on_domain(f, domain, np.arange(1, Is[1] + 1).reshape(-1, 1)).astype(Tv)
        return [v.reshape((Is[1], 1, 1), order="F")], [1, 1], dict(eps=[], sweeps=0)
    Rs = _ranks(ranks, N, Is, rmax)
    I_l, I_g = [None] * (N + 1), [None] * (N + 1)
    I_l[1], I_g[N] = np.ones((1, 0), dtype=np.int64), np.ones((1, 0), dtype=np.int64)
    for k in range(2, N + 1):
        I_l[k] = draw_indices(seed, X.DRAW_DMRG_LEFT, k, 0, Rs[k], Is[1:k])
    for k in range(1, N):
        I_g[k] = draw_indices(seed, X.DRAW_DMRG_RIGHT, k, 0, Rs[k + 1], Is[k + 1:])
    cores = [None] * (N + 1)
    Xs_val = draw_indices(seed, X.DRAW_VALIDATION, 0, 0, val_size, Is[1:])
    ys_val = _evaluate_on_domain(f, domain, Xs_val).astype(Tv)
    norm_ys = max(np.linalg.norm(ys_val), tol)
    hist = []

    def svdtrunc(k):
        sb = _sample_superblock(f, domain, I_l, I_g, k, Is, N).astype(Tv)
        r_l, s1, s2, r_g = sb.shape
        U, s, Vt = np.linalg.svd(sb.reshape((r_l * s1, s2 * r_g), order="F"), full_matrices=False)
        r = _svd_rank(s, rmax, tol)
        return r_l, s1, s2, r_g, U[:, :r], s[:r], Vt[:r], r

    done = False
    for it in range(1, maxiter + 1):
        for k in range(1, N):
            r_l, s1, s2, r_g, U, s, Vt, r = svdtrunc(k)
            if k < N - 1:
                Q = _qr(U)
                I_idx, G, _ = maxvol(Q, ptol, pmaxiter)
                I_l[k + 1] = _combine_indices_left(I_l[k], s1)[I_idx - 1]
                Rs[k + 1] = len(I_idx)
                cores[k] = np.transpose(G.reshape((r_l, s1, Rs[k + 1]), order="F"), (1, 0, 2))
            else:
                cores[k] = np.transpose(U.reshape((r_l, s1, r), order="F"), (1, 0, 2))
                cores[k + 1] = np.transpose((s[:, None] * Vt).reshape((r, s2, r_g), order="F"), (1, 0, 2))
                Rs[k + 1] = r
        eps = np.linalg.norm(ys_val - _evaluate_tt(cores[1:], Xs_val, N)) / norm_ys
        hist.append(eps)
        if eps < tol:
            break
        for k in range(N - 1, 0, -1):
            r_l, s1, s2, r_g, U, s, Vt, r = svdtrunc(k)
            if k > 1:
                Q = _qr(Vt.conj().T)
                I_idx, G, _ = maxvol(Q, ptol, pmaxiter)
                I_g[k] = _combine_indices_right(s2, I_g[k + 1])[I_idx - 1]
                Rs[k + 1] = len(I_idx)
                cores[k + 1] = np.transpose(G.conj().T.reshape((Rs[k + 1], s2, r_g), order="F"), (1, 0, 2))
            else:
                cores[k] = np.transpose((U * s[None, :]).reshape((r_l, s1, r), order="F"), (1, 0, 2))
                cores[k + 1] = np.transpose(Vt.reshape((r, s2, r_g), order="F"), (1, 0, 2))
                Rs[k + 1] = r
        eps = np.linalg.norm(ys_val - _evaluate_tt(cores[1:], Xs_val, N)) / norm_ys
        hist.append(eps)
        if eps < tol:
            break
    out = cores[1:]
    return out, [1] + [c.shape[2] for c in out], dict(eps=hist, sweeps=len(hist), I_l=I_l, I_g=I_g)


def full_tensor(cores):
    """the dense tensor T[i_1, ..., i_N] of a train (small cases only)"""
    T = np.ones((1,), dtype=np.result_type(*cores))
    for c in cores:
        T = np.tensordot(T, c, axes=([T.ndim - 1], [1]))             # (..., a) x (n, a, b) -> (..., n, b)
    return T[..., 0]
