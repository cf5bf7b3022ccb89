"""NumPy restatement of the reference's time steppers (src/solvers/euler.jl:76-222) with tt_solver in {als, mals, dmrg} and the
return_error branches, and of increase_ranks at noise = 0 (src/tt_tools.jl:443-490), composed from oracle.tt_oracle's functions.
Not a test: the CPU and GPU stepper tests import it.

Statement for statement with the reference; `-` is `(-1 * B) + A` for vectors and operators alike (tt_operations.jl:289-291)."""
import math

import numpy as np

from oracle import tt_oracle as O

EPS = float(np.finfo(np.float64).eps)


def tto_sub(A, B):
    return O.tto_add(O.tto_scale(-1.0, B), A)


def heat_operator(d):
    """A = -h^2 * toeplitz_to_qtto(-2, 1, 1, d), h = 1 / d^2 — test/test_euler.jl:6-8."""
    h = 1.0 / d ** 2
    return O.tto_scale(-h ** 2, O.toeplitz_to_qtto(-2.0, 1.0, 1.0, d))


def dense(A):
    return O.qtto_to_matrix(A)


def _linsolve(tt_solver, M, b, guess, kw):
    if tt_solver == "als":
        return O.als_linsolve(M, b, guess, sweep_count=kw.get("sweep_count", 2))
    if tt_solver == "mals":
        return O.mals_linsolve(M, b, guess, **{k: v for k, v in kw.items() if k in ("tol", "rmax")})
    if tt_solver == "dmrg":
        return O.dmrg_linsolve(M, b, guess, **kw)
    raise ValueError(f"Unknown TT solver: {tt_solver}")


def _round(x, max_bond):
    return O.tt_compress_(x, max_bond) if max_bond > 0 else O.orthogonalize(x)


def implicit_euler_method(A, u0, guess, steps, normalize=True, return_error=False, tt_solver="mals", max_bond=0, **kw):
    """euler.jl:99-143"""
    solution = u_prev = u0
    I = O.id_tto(A.N)
    for h in steps:
        M = tto_sub(I, O.tto_scale(h, A))
        nxt = _linsolve(tt_solver, M, solution, guess, kw)
        if normalize:
            nxt = O.div(nxt, O.norm(nxt))
        u_prev = solution
        solution = _round(nxt, max_bond)
        guess = solution
    if return_error:
        M = tto_sub(I, O.tto_scale(steps[-1], A))
        residual = O.sub(O.apply(M, solution), u_prev)
        return solution, O.norm(residual) / O.norm(solution)
    return solution


def crank_nicholson_method(A, u0, guess, steps, normalize=True, return_error=False, tt_solver="mals", max_bond=0, **kw):
    """euler.jl:145-191"""
    solution = u_prev = u0
    I = O.id_tto(A.N)
    for h in steps:
        LHS = tto_sub(I, O.tto_scale(h / 2, A))
        RHS = O.apply(O.tto_add(I, O.tto_scale(h / 2, A)), solution)
        nxt = _linsolve(tt_solver, LHS, RHS, guess, kw)
        if normalize:
            nxt = O.div(nxt, O.norm(nxt))
        u_prev = solution
        solution = _round(nxt, max_bond)
        guess = solution
    if return_error:
        h = steps[-1]
        LHS = tto_sub(I, O.tto_scale(h / 2, A))
        RHS = O.apply(O.tto_add(I, O.tto_scale(h / 2, A)), u_prev)
        residual = O.sub(O.apply(LHS, solution), RHS)
        return solution, O.norm(residual) / O.norm(solution)
    return solution


def euler_method(A, u0, steps, normalize=True, return_error=False):
    """euler.jl:76-97"""
    solution = O.euler_method(A, u0, steps, normalize=normalize)
    if return_error:
        h = steps[-1]
        IhA = O.tto_add(O.id_tto(A.N), O.tto_scale(h, A))
        residual = O.sub(solution, O.apply(IhA, solution))
        return solution, O.norm(residual) / O.norm(solution)
    return solution


def rk4_method(A, u0, steps, max_bond, normalize=True, return_error=False):
    """euler.jl:193-222"""
    u = O.rk4_method(A, u0, steps, max_bond, normalize=normalize)
    if return_error:
        h = steps[-1]
        k1 = O.apply(A, u)
        k2 = O.apply(A, O.tt_compress_(O.add(u, O.scale(h / 2, k1)), max_bond))
        k3 = O.apply(A, O.tt_compress_(O.add(u, O.scale(h / 2, k2)), max_bond))
        k4 = O.apply(A, O.tt_compress_(O.add(u, O.scale(h, k3)), max_bond))
        incr = O.scale(h / 6, O.tt_compress_(O.add(O.add(O.add(k1, O.scale(2, k2)), O.scale(2, k3)), k4), max_bond))
        residual = O.tt_compress_(O.sub(O.sub(u, O.sub(u, incr)), incr), max_bond)
        return u, O.norm(residual) / max(O.norm(u), EPS)
    return u


def increase_ranks(x, max_bond, rks=None):
    """increase_ranks(x, max_bond; rks, noise = 0) — tt_tools.jl:480-490: exact zero-padding, ttv_ot zeros."""
    assert max_bond > max(x.ttv_rks), "New bond dimension too low"
    d = x.N
    new = O.r_and_d_to_rks(list(rks) if rks is not None else [1] + [max_bond] * (d - 1) + [1], x.ttv_dims, rmax=max_bond)
    cores = []
    for k, c in enumerate(x.ttv_vec):
        p = np.zeros((c.shape[0], new[k], new[k + 1]))
        p[:, : c.shape[1], : c.shape[2]] = c
        cores.append(p)
    return O.TTvector(d, cores, tuple(x.ttv_dims), list(new), [0] * d)


def dense_sequential(x):
    """The dense tensor of a train by one multiply-add per rank index, in index order: appending zero rows / columns to the cores adds
    exact zeros to every sum, so the result of a zero-padded train is the same in every bit (a BLAS contraction may regroup the sums)."""
    v = np.array(x.ttv_vec[0][:, 0, :])                                # (n_1, r_1)
    for k in range(1, x.N):
        c = x.ttv_vec[k]
        acc = np.zeros(v.shape[:-1] + (c.shape[0], c.shape[2]))
        for a in range(c.shape[1]):
            acc = acc + v[..., a, None, None] * c[:, a, :]
        v = acc
    return v[..., 0]


def dense_implicit_euler(A, u, steps):
    Ad, v = dense(A), O.qtt_to_vector(u)
    for h in steps:
        v = np.linalg.solve(np.eye(len(v)) - h * Ad, v)
    return v


def dense_crank_nicholson(A, u, steps):
    Ad, v = dense(A), O.qtt_to_vector(u)
    I = np.eye(len(v))
    for h in steps:
        v = np.linalg.solve(I - 0.5 * h * Ad, (I + 0.5 * h * Ad) @ v)
    return v


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def apply_axpby(alpha, x, beta, A, y):
    """The composition ttn_apply_axpby must equal bit for bit, on one train: apply, scalar * (beta), scalar * (alpha), +."""
    t = O.apply(A, y)
    return O.add(O.scale(1.0 if alpha is None else alpha, x), O.scale(1.0 if beta is None else beta, t))
