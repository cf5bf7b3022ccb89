"""Device-resident caller chains built from the hot-path ops (first step).

Mirrors of the explicit time steppers of the reference that are literally chains of
``A*u``, ``+``, scalar ``*``, ``tt_compress!`` / ``orthogonalize`` and ``dot``:

    euler_method(A, u0, steps; normalize)          src/solvers/euler.jl:76-97
    rk4_method(A, u0, steps, max_bond; normalize)   src/solvers/euler.jl:193-209

    krylov_linsolve(A, b, guess; max_bond, krylov_solver, ...)       src/solvers/euler.jl:34-74
    implicit_euler_method / crank_nicholson_method (tt_solver = "krylov")   src/solvers/euler.jl:98-190

They run on ``DeviceTT`` batches (every train of the batch is an independent initial condition / linear system),
never leave HBM between ops, and return a new ``DeviceTT``.  The implicit steppers take ``tt_solver`` in
{"krylov", "als", "mals", "dmrg"}; everything a step does around its linear solve is ``alpha x + beta (A y)``, one launch of
``device.apply_axpby`` (csrc/ttn_step_kernels.h).  ``return_error=True`` returns ``(solution, rel_error)`` with the reference's
residual formulas, ``rel_error`` a float64 array of length ``batch``.  Handed ``TTvector`` s instead of handles, the four steppers
upload, run with batch 1, download, and return a ``TTvector`` (and a float).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Sequence

from . import _lib
from . import device as D
from .device import DeviceTT, DeviceTTO


def _ranks_of(x: DeviceTT) -> List[int]:
    """Per-bond maximum of the current ranks over the batch (host sync)."""
    return x.max_ranks()


def _apply(A: DeviceTTO, x: DeviceTT, xr: Sequence[int]):
    yr = [a * c for a, c in zip(A.rks, xr)]
    y = DeviceTT(x.dims, yr, x.batch)
    D.apply(A, x, y)
    return y, yr


def _axpy(x: DeviceTT, xr, a: float, y: DeviceTT, yr):
    """x + a*y as the reference evaluates it: scalar * first, then +."""
    ay = DeviceTT(y.dims, yr, y.batch)
    D.scale(a, y, ay)
    zr = [p + q for p, q in zip(xr, yr)]
    zr[0] = zr[-1] = 1
    z = DeviceTT(x.dims, zr, x.batch)
    D.add(x, ay, z)
    ay.free()
    return z, zr


def _compress(x: DeviceTT, xr, max_bond: int):
    """tt_compress!(x, max_bond) into a handle whose capacity also covers rank growth; returns (handle, rank bound)."""
    need, fin = D.compress_rank_bound(x.dims, xr, max_bond)
    if any(n > c for n, c in zip(need, x.cap)):
        big = DeviceTT(x.dims, need, x.batch)
        _lib.check(_lib.lib().ttn_tt_copy(big.h, x.h))
        x.free()
        x = big
    D.tt_compress_(x, max_bond)     # asynchronous: a failure code stays on the handle (or moves to the library word when the handle
    return x, fin                   # is freed) until the chain's one check per time step / iteration (D.status_all)


def _normalize(u: DeviceTT) -> None:
    nrm2 = D.dot(u, u)                                    # (1 / sqrt(dot(u, u))) * u   (euler.jl:83-85, :205-207)
    D.scale_batch([1.0 / math.sqrt(v) for v in nrm2], u, u)


def _axpby(alpha, x: DeviceTT, xr, beta, A: DeviceTTO, y: DeviceTT, yr):
    """alpha x + beta (A y) in one launch (device.apply_axpby): bit for bit _apply -> scale -> scale -> add."""
    zr = [p + a * q for p, a, q in zip(xr, A.rks, yr)]
    zr[0] = zr[-1] = 1
    z = DeviceTT(x.dims, zr, x.batch)
    D.apply_axpby(alpha, x, beta, A, y, z)
    return z, zr


def _is_host(u) -> bool:
    return hasattr(u, "ttv_vec")


def _dev_op(A) -> DeviceTTO:
    return A if isinstance(A, DeviceTTO) else DeviceTTO(A)


def _single_op(A, who: str) -> None:
    """The linear solvers and the implicit steppers take one operator (the library's single_op refuses the rest of the list itself)."""
    if isinstance(A, DeviceTTO) and A.batch > 1:
        raise _lib.TTNError(f"{who}: an operator batch is not supported here (DeviceTTO.select(b) gives one operator of it)")


def _host_level(run, A, *trains):
    """A stepper called with TTvectors: upload, run with batch 1, download; (TTvector, float) when the run returns an error too."""
    if not all(_is_host(t) for t in trains):
        raise TypeError("the trains of one call must be all TTvectors or all DeviceTT handles")
    dA = _dev_op(A)
    hs = [DeviceTT.from_host(t.ttvector() if hasattr(t, "ttvector") else t) for t in trains]
    out = run(dA, *hs)
    sol, err = out if isinstance(out, tuple) else (out, None)
    res = sol.download(0)
    for h in hs + [sol]:
        h.free()
    return res if err is None else (res, float(err[0]))


def _rk4_increment(A: DeviceTTO, u: DeviceTT, ur, h: float, max_bond: int):
    """(h/6) * tt_compress!(k1 + 2k2 + 2k3 + k4, max_bond) of one step (euler.jl:199-203, :212-216) before the scalar: (handle, ranks)."""
    k1, k1r = _apply(A, u, ur)
    t, tr = _axpy(u, ur, h / 2, k1, k1r)
    t, tr = _compress(t, tr, max_bond)
    k2, k2r = _apply(A, t, tr); t.free()
    t, tr = _axpy(u, ur, h / 2, k2, k2r)
    t, tr = _compress(t, tr, max_bond)
    k3, k3r = _apply(A, t, tr); t.free()
    t, tr = _axpy(u, ur, h, k3, k3r)
    t, tr = _compress(t, tr, max_bond)
    k4, k4r = _apply(A, t, tr); t.free()
    # k1 + 2k2 + 2k3 + k4, left to right like the reference
    s, sr = _axpy(k1, k1r, 2.0, k2, k2r)
    s2, s2r = _axpy(s, sr, 2.0, k3, k3r); s.free()
    s3, s3r = _axpy(s2, s2r, 1.0, k4, k4r); s2.free()
    for k in (k1, k2, k3, k4):
        k.free()
    return _compress(s3, s3r, max_bond)


def rk4_method(A, u0, steps: Sequence[float], max_bond: int, normalize: bool = True, return_error: bool = False):
    """src/solvers/euler.jl:193-222 on a device-resident batch (A: TToperator or DeviceTTO).  return_error: (u, rel_error) with
    rel_error = norm(tt_compress!(u - (u - incr) - incr, max_bond)) / max(norm(u), eps) for one more increment of size steps[-1]."""
    if _is_host(u0):
        return _host_level(lambda dA, du: rk4_method(dA, du, steps, max_bond, normalize, return_error), A, u0)
    A = _dev_op(A)
    u, ur = u0, _ranks_of(u0)
    own = False
    for h in steps:
        s3, s3r = _rk4_increment(A, u, ur, h, max_bond)
        un, unr = _axpy(u, ur, h / 6, s3, s3r); s3.free()    # u + (h/6) * tt_compress!(...)
        un, unr = _compress(un, unr, max_bond)
        if normalize:
            _normalize(un)
        if own:
            u.free()
        u, ur, own = un, unr, True
        D.status_all()          # one check per time step: a non-converged SVD inside the step must not be committed silently
    if not return_error:
        return u
    h = steps[-1]
    s3, s3r = _rk4_increment(A, u, ur, h, max_bond)
    incr = DeviceTT(s3.dims, s3r, s3.batch)
    D.scale(h / 6, s3, incr); s3.free()
    uv, iv = _Vec(u, ur, own=False), _Vec(incr, s3r)
    t1 = _lin(1.0, uv, -1.0, iv)                              # u - incr          = (-1 * incr) + u
    t2 = _lin(1.0, uv, -1.0, t1); t1.free()                   # u - (u - incr)
    t3 = _lin(1.0, t2, -1.0, iv); t2.free(); iv.free()        # ... - incr
    res, _ = _compress(t3.h, t3.rks, max_bond)
    rel = D.norm(res) / np.maximum(D.norm(u), np.finfo(np.float64).eps)
    res.free()
    D.status_all()
    return u, rel


def euler_method(A, u0, steps: Sequence[float], normalize: bool = True, return_error: bool = False):
    """src/solvers/euler.jl:76-97: solution = orthogonalize(solution + h * (A * solution)), optional normalisation (A: TToperator or
    DeviceTTO).  return_error: (solution, rel_error), rel_error = norm(solution - (I + h A) solution) / norm(solution), h = steps[-1]."""
    if _is_host(u0):
        return _host_level(lambda dA, du: euler_method(dA, du, steps, normalize, return_error), A, u0)
    A = _dev_op(A)
    u, ur = u0, _ranks_of(u0)
    own = False
    for h in steps:
        t, tr = _axpby(None, u, ur, h, A, u, ur)              # solution + h * (A * solution): one launch
        un = DeviceTT(t.dims, tr, t.batch)
        D.orthogonalize(t, 1, un); t.free()
        unr = _ranks_of(un)
        if normalize:
            _normalize(un)
        if own:
            u.free()
        u, ur, own = un, unr, True
    if not return_error:
        return u
    w, wr = _axpby(None, u, ur, steps[-1], A, u, ur)          # (I + h A) * solution
    res = _lin(1.0, _Vec(u, ur, own=False), -1.0, _Vec(w, wr, own=False)); w.free()      # solution - (...)
    rel = D.norm(res.h) / D.norm(u)
    res.free()
    D.status_all()
    return u, rel


# ----------------------------------------------------------------------------------------------------------------------
# Krylov linear solves on handles: krylov_linsolve (src/solvers/euler.jl:34-74) and the implicit steppers
# that call it (implicit_euler_method :98-140, crank_nicholson_method :142-190) with tt_solver = "krylov".
#
# The reference hands `op`, `b`, `guess` to KrylovKit.linsolve (BiCGStab / GMRES / CG) — a third-party package that is not
# part of the reference tree (Project.toml compat 0.6.1, 0.9, 0.10), so its exact iteration (restart policy, breakdown
# handling) cannot be restated: what is mirrored here is the reference's OWN part — the operator
#     op = max_bond > 0 ? x -> tt_compress!(A*x, max_bond) : x -> A*x                              (euler.jl:55)
# the tolerance tol = max(atol, rtol*norm(b)) (:57), the solver selection (:56, :9-32) and the vector algebra of the
# VectorInterface extension (add = _round(beta*y + alpha*x) with _round = tt_compress!(., max_bond) during a bounded
# solve, orthogonalize otherwise; ext/...VectorInterfaceExt.jl:11-51) — around the textbook forms of the three Krylov
# methods.  Parity is therefore pinned where the reference's tests pin it: the solution against a dense solve
# (test/test_euler.jl:105-240: 1e-8 / 1e-7) and the rank bound; iterates are "parity unpinned".
# Every train of the batch is an independent system (same A, own right-hand side): scalars are per-train vectors.
# ----------------------------------------------------------------------------------------------------------------------
import numpy as np

from .tt import TToperator, TTvector


def _tto_scale(a: float, A: TToperator) -> TToperator:
    """a * A for operators: scales the first core (src/tt_operations.jl:268-281)."""
    cores = [np.array(c, order="F") for c in A.tto_vec]
    cores[0] = a * cores[0]
    return TToperator(A.N, cores, A.tto_dims, list(A.tto_rks), list(A.tto_ot))


def _tto_add(A: TToperator, B: TToperator) -> TToperator:
    """A + B for operators: block concatenation of the cores (src/tt_operations.jl:71-96)."""
    assert A.tto_dims == B.tto_dims, "Incompatible dimensions"
    d = A.N
    cores, rks = [], [1]
    for k in range(d):
        a, b = A.tto_vec[k], B.tto_vec[k]
        n = a.shape[0]
        ral, rar, rbl, rbr = a.shape[2], a.shape[3], b.shape[2], b.shape[3]
        rl = 1 if k == 0 else ral + rbl
        rr = 1 if k == d - 1 else rar + rbr
        c = np.zeros((n, n, rl, rr), order="F")
        if d == 1:
            c[:] = a + b
        elif k == 0:
            c[:, :, 0, :rar] = a[:, :, 0, :]; c[:, :, 0, rar:] = b[:, :, 0, :]
        elif k == d - 1:
            c[:, :, :ral, 0] = a[:, :, :, 0]; c[:, :, ral:, 0] = b[:, :, :, 0]
        else:
            c[:, :, :ral, :rar] = a; c[:, :, ral:, rar:] = b
        cores.append(c)
        rks.append(rr)
    return TToperator(d, cores, A.tto_dims, rks, [0] * d)


class _Vec:
    """A DeviceTT batch together with the host-side rank bound the capacity arithmetic needs."""

    def __init__(self, h: DeviceTT, rks, own: bool = True):
        self.h, self.rks, self.own = h, list(rks), own

    def free(self):
        if self.own and self.h is not None:
            self.h.free()
            self.h = None


def _lin(a, x: _Vec, b, y: _Vec) -> _Vec:
    """a .* x + b .* y with per-train scalars (b*y + a*x as the extension writes it: scalar * first, then +)."""
    B = x.h.batch
    ax, by = DeviceTT(x.h.dims, x.rks, B), DeviceTT(y.h.dims, y.rks, B)
    D.scale_batch(np.broadcast_to(np.asarray(a, dtype=float), (B,)).copy(), x.h, ax)
    D.scale_batch(np.broadcast_to(np.asarray(b, dtype=float), (B,)).copy(), y.h, by)
    zr = [p + q for p, q in zip(x.rks, y.rks)]
    zr[0] = zr[-1] = 1
    z = DeviceTT(x.h.dims, zr, B)
    D.add(by, ax, z)
    ax.free(); by.free()
    return _Vec(z, zr)


def _copy(v: _Vec) -> _Vec:
    from . import _lib
    c = DeviceTT(v.h.dims, v.rks, v.h.batch)
    _lib.check(_lib.lib().ttn_tt_copy(c.h, v.h.h))
    return _Vec(c, v.rks)


def _scale(v: _Vec, coef) -> _Vec:
    """coef .* v (per-train scalars) into a fresh handle; same ranks, so nothing to round."""
    c = DeviceTT(v.h.dims, v.rks, v.h.batch)
    D.scale_batch(np.broadcast_to(np.asarray(coef, dtype=float), (v.h.batch,)).copy(), v.h, c)
    return _Vec(c, v.rks)


def _round(v: _Vec, round_rank: int) -> _Vec:
    """VectorInterface ext `_round`: tt_compress!(r, rk) during a bounded Krylov solve, orthogonalize(r) otherwise."""
    if round_rank > 0:
        h, fin = _compress(v.h, v.rks, round_rank)
        return _Vec(h, fin)
    o = DeviceTT(v.h.dims, v.rks, v.h.batch)
    D.orthogonalize(v.h, 1, o)
    v.free()
    return _Vec(o, _ranks_of(o))


def _vi_add(y: _Vec, x: _Vec, alpha, beta, round_rank: int) -> _Vec:
    """VectorInterface.add(y, x, alpha, beta) = _round(beta*y + alpha*x)."""
    return _round(_lin(alpha, x, beta, y), round_rank)


def _make_op(A: DeviceTTO, max_bond: int):
    def op(x: _Vec) -> _Vec:
        y, yr = _apply(A, x.h, x.rks)
        if max_bond > 0:
            y, yr = _compress(y, yr, max_bond)
        return _Vec(y, yr)
    return op


def _safe_div(num, den):
    num, den = np.asarray(num, dtype=float), np.asarray(den, dtype=float)
    return np.where(den != 0.0, num / np.where(den != 0.0, den, 1.0), 0.0)


def _bicgstab(op, b: _Vec, x: _Vec, tol, maxiter: int, rr: int) -> _Vec:
    """van der Vorst's BiCGStab, per-train scalars; trains that have converged keep iterating with zero updates."""
    Ax = op(x)
    r = _vi_add(b, Ax, -1.0, 1.0, rr); Ax.free()
    rhat = _Vec(r.h, r.rks, own=False)
    rhat_keep = r                                             # r is replaced below; keep the shadow residual alive
    r = _copy(rhat)
    B = b.h.batch
    rho = alpha = omega = np.ones(B)
    v = p = None
    for it in range(maxiter):
        if np.all(D.norm(r.h) <= tol):
            break
        rho_new = D.dot(rhat.h, r.h)
        if p is None:
            p = _copy(r)
        else:
            beta = _safe_div(rho_new, rho) * _safe_div(alpha, omega)
            t = _vi_add(p, v, -omega, 1.0, rr)                # p - omega v
            pn = _vi_add(r, t, beta, 1.0, rr); t.free(); p.free(); p = pn
        if v is not None:
            v.free()
        v = op(p)
        alpha = _safe_div(rho_new, D.dot(rhat.h, v.h))
        s = _vi_add(r, v, -alpha, 1.0, rr)
        t = op(s)
        tt_ = D.dot(t.h, t.h)
        omega = _safe_div(D.dot(t.h, s.h), tt_)
        xa = _vi_add(x, p, alpha, 1.0, rr); x.free()
        x = _vi_add(xa, s, omega, 1.0, rr); xa.free()
        rn = _vi_add(s, t, -omega, 1.0, rr); s.free(); t.free(); r.free(); r = rn
        rho = rho_new
        D.status_all()                                        # one status check per Krylov iteration
    for w in (r, p, v, rhat_keep):
        if w is not None:
            w.free()
    return x


def _cg(op, b: _Vec, x: _Vec, tol, maxiter: int, rr: int) -> _Vec:
    Ax = op(x)
    r = _vi_add(b, Ax, -1.0, 1.0, rr); Ax.free()
    p = _copy(r)
    rs = D.dot(r.h, r.h)
    for it in range(maxiter):
        if np.all(np.sqrt(np.maximum(rs, 0.0)) <= tol):
            break
        Ap = op(p)
        alpha = _safe_div(rs, D.dot(p.h, Ap.h))
        xn = _vi_add(x, p, alpha, 1.0, rr); x.free(); x = xn
        rn = _vi_add(r, Ap, -alpha, 1.0, rr); r.free(); Ap.free(); r = rn
        rs_new = D.dot(r.h, r.h)
        pn = _vi_add(r, p, _safe_div(rs_new, rs), 1.0, rr); p.free(); p = pn
        rs = rs_new
        D.status_all()                                        # one status check per Krylov iteration
    r.free(); p.free()
    return x


def _gmres(op, b: _Vec, x: _Vec, tol, krylovdim: int, maxiter: int, rr: int) -> _Vec:
    """Restarted GMRES(krylovdim), modified Gram-Schmidt, the small least-squares problems per train on the host."""
    B = b.h.batch
    for outer in range(maxiter):
        Ax = op(x)
        r = _vi_add(b, Ax, -1.0, 1.0, rr); Ax.free()
        beta = D.norm(r.h)
        if np.all(beta <= tol):
            r.free()
            break
        V = [_scale(r, _safe_div(1.0, beta))]; r.free()
        H = np.zeros((B, krylovdim + 1, krylovdim))
        m = 0
        for j in range(krylovdim):
            w = op(V[j])
            for i in range(j + 1):
                hij = D.dot(V[i].h, w.h)
                H[:, i, j] = hij
                wn = _vi_add(w, V[i], -hij, 1.0, rr); w.free(); w = wn
            hn = D.norm(w.h)
            H[:, j + 1, j] = hn
            m = j + 1
            if np.all(hn <= 1e-300) or j + 1 == krylovdim:
                w.free()
                break
            V.append(_scale(w, _safe_div(1.0, hn))); w.free()
        ycoef = np.zeros((B, m))
        for t in range(B):
            e1 = np.zeros(m + 1); e1[0] = beta[t]
            ycoef[t] = np.linalg.lstsq(H[t, : m + 1, :m], e1, rcond=None)[0]
        for j in range(m):
            xn = _vi_add(x, V[j], ycoef[:, j], 1.0, rr); x.free(); x = xn
        for v in V:
            v.free()
        D.status_all()                                        # one status check per restart cycle
    return x


def krylov_linsolve(A, b: DeviceTT, guess: DeviceTT, max_bond: int = 0, krylov_solver: str = "auto", krylovdim: int = 8,
                    maxiter: int = 20, rtol: float = 1.0e-8, atol: float = 1.0e-12, tol=None, issymmetric: bool = False,
                    ishermitian=None, isposdef: bool = False) -> DeviceTT:
    """src/solvers/euler.jl:34-74 on device-resident batches (A: TToperator or DeviceTTO; every train its own system)."""
    ishermitian = issymmetric if ishermitian is None else ishermitian
    _single_op(A, "krylov_linsolve")
    dA = A if isinstance(A, DeviceTTO) else DeviceTTO(A)
    solver = "cg" if (krylov_solver == "auto" and isposdef and (issymmetric or ishermitian)) else krylov_solver   # :56
    if solver == "auto":
        solver = "bicgstab" if max_bond > 0 else "gmres"                                                             # :17
    if solver not in ("bicgstab", "gmres", "cg"):
        raise ValueError(f"Unknown Krylov solver: {krylov_solver}. Use :auto, :bicgstab, :cg, or :gmres.")           # :31
    bv = _Vec(b, _ranks_of(b), own=False)
    tol_value = np.maximum(atol, rtol * D.norm(b)) if tol is None else np.full(b.batch, float(tol))                   # :57
    x0 = _Vec(guess, _ranks_of(guess), own=False)
    x = _copy(x0)                                             # a working copy the iteration may free
    op = _make_op(dA, max_bond)
    if solver == "bicgstab":
        x = _bicgstab(op, bv, x, tol_value, maxiter, max_bond)
    elif solver == "cg":
        x = _cg(op, bv, x, tol_value, krylovdim * maxiter, max_bond)                                                 # :28
    else:
        x = _gmres(op, bv, x, tol_value, krylovdim, maxiter, max_bond)
    D.status_all()
    return x.h


# ----------------------------------------------------------------------------------------------------------------------
# The implicit steppers (src/solvers/euler.jl:99-191) on the Krylov, ALS, MALS and DMRG solvers.  Keywords are forwarded to the chosen
# solver exactly as the reference forwards `kwargs...`; they are checked against that solver's own list before anything reaches the
# device, so a misspelt one is a TypeError naming it.
# ----------------------------------------------------------------------------------------------------------------------
_TT_SOLVERS = ("krylov", "als", "mals", "dmrg")
_SOLVER_KW = {
    "krylov": ("krylov_solver", "krylovdim", "maxiter", "rtol", "atol", "tol", "issymmetric", "ishermitian", "isposdef"),     # euler.jl:34-46
    "als": ("sweep_count", "it_solver", "r_itsolver"),                                                                           # als.jl:161
    "mals": ("tol", "rmax"),                                                                                                     # mals.jl:239-244
    "dmrg": ("N", "tol", "sweep_schedule", "rmax_schedule", "it_solver", "linsolv_maxiter", "linsolv_tol", "itslv_thresh"),     # dmrg.jl:388-396
}


def _check_solver(who: str, tt_solver: str, kw: dict) -> None:
    if tt_solver not in _TT_SOLVERS:
        raise ValueError(f"Unknown TT solver: {tt_solver}")                                                                      # euler.jl:122
    for name in kw:
        if name not in _SOLVER_KW[tt_solver]:
            raise TypeError(f"{who}() got an unexpected keyword argument {name!r} for tt_solver={tt_solver!r}")
    if tt_solver == "dmrg" and kw.get("N", 2) != 2:
        raise _lib.TTNError("dmrg_linsolve: only the two-site scheme N = 2 is offered (single-site: als_linsolve)")


def _solve(tt_solver: str, lhs: DeviceTTO, rhs: DeviceTT, guess: DeviceTT, max_bond: int, kw: dict) -> DeviceTT:
    """One linear solve of a step into a fresh handle."""
    dims, B = guess.dims, guess.batch
    if tt_solver == "krylov":
        return krylov_linsolve(lhs, rhs, guess, max_bond=max_bond, **kw)
    gr = guess.max_ranks()
    if tt_solver == "als":                                     # it_solver / r_itsolver: accepted and ignored, as in als.jl:161
        return als_linsolve_(lhs, rhs, guess, DeviceTT(dims, gr, B), kw.get("sweep_count", 2))
    if tt_solver == "mals":
        rmax = kw.get("rmax")
        if rmax is None:
            rmax = int(round(math.sqrt(math.prod(dims))))                                                                        # mals.jl:244
        x = DeviceTT(dims, mals_capacity(dims, gr, rmax), B)
        return mals_linsolve_(lhs, rhs, guess, x, kw.get("tol", 1.0e-12), rmax)
    k = {n: v for n, v in kw.items() if n != "N"}
    rs = k.get("rmax_schedule")
    if rs is None:
        rs = k["rmax_schedule"] = (math.isqrt(math.prod(dims)),)                                                                 # dmrg.jl:391
    rtop = max(int(v) for v in rs)
    cap = dmrg_capacity(dims, gr, rtop)                        # the capacity the host dmrg_linsolve chooses
    if not k.get("it_solver", False) and max(dims[i] * cap[i] * dims[i + 1] * cap[i + 2] for i in range(len(cap) - 2)) <= 2048:
        cap = mals_capacity(dims, gr, rtop)
    return dmrg_linsolve_(lhs, rhs, guess, DeviceTT(dims, cap, B), **k)


def _implicit_stepper(who, A, u0, guess, steps, normalize, return_error, tt_solver, max_bond, crank, kw):
    _check_solver(who, tt_solver, kw)
    _single_op(A, who)
    if _is_host(u0) or _is_host(guess):
        return _host_level(lambda dA, du, dg: _implicit_stepper(who, dA, du, dg, steps, normalize, return_error, tt_solver, max_bond, crank, kw),
                           A, u0, guess)
    from .constructors import id_tto
    half = 0.5 if crank else 1.0
    lhs_of, rhs_of = {}, {}                                    # step size -> operator, built once per distinct h
    if tt_solver == "krylov":                                  # (this path keeps its host-built operators: block order [I, -cA])
        hostA = A.download() if isinstance(A, DeviceTTO) else A
        I = id_tto(hostA.N)
        dA = _dev_op(A) if (crank and return_error) else None

        def lhs(h):
            if h not in lhs_of:
                lhs_of[h] = DeviceTTO(_tto_add(I, _tto_scale(-h * half, hostA)))                     # I - h A (:115), I - (h/2) A (:161)
            return lhs_of[h]

        def rhs_op(h):
            if h not in rhs_of:
                rhs_of[h] = DeviceTTO(_tto_add(I, _tto_scale(h / 2, hostA)))                         # I + (h/2) A   (:162)
            return rhs_of[h]
    else:
        dA = _dev_op(A)
        dI = DeviceTTO(id_tto(dA.N))

        def lhs(h):
            if h not in lhs_of:
                cA = dA.scale(h * half)
                lhs_of[h] = dI.sub(cA)                          # tto_sub(I, tto_scale(c, A)) = (-1 * (c A)) + I, on the device
                cA.free()
            return lhs_of[h]
    sol, sol_own = u0, False
    prev, prev_own = u0, False
    for h in steps:
        M = lhs(h)
        if crank and tt_solver == "krylov":
            rhs, _ = _apply(rhs_op(h), sol, _ranks_of(sol))                                          # (I + (h/2) A) * solution
        elif crank:
            sr = _ranks_of(sol)
            rhs, _ = _axpby(None, sol, sr, h / 2, dA, sol, sr)                                       # solution + (h/2) (A solution), one launch
        else:
            rhs = sol
        nxt = _solve(tt_solver, M, rhs, guess, max_bond, kw)
        if crank:
            rhs.free()
        if normalize:
            D.scale_batch(1.0 / D.norm(nxt), nxt, nxt)                                 # next / norm(next)
        v = _round(_Vec(nxt, _ranks_of(nxt)), max_bond)                               # tt_compress!(next, max_bond) : orthogonalize(next)
        D.status_all()
        if prev_own and prev is not sol:
            prev.free()
        prev, prev_own = sol, sol_own                                                  # u_prev = solution
        sol, sol_own, guess = v.h, True, v.h
    rel = None
    if return_error:
        h = steps[-1]
        M = lhs(h)
        sr, pr = _ranks_of(sol), _ranks_of(prev)
        if crank:                                                                      # LHS * solution - (I + (h/2) A) * u_prev   (:182-186)
            w, wr = _axpby(None, prev, pr, h / 2, dA, prev, pr)
            res, _ = _axpby(-1.0, w, wr, None, M, sol, sr); w.free()
        else:                                                                          # M * solution - u_prev                    (:135-138)
            res, _ = _axpby(-1.0, prev, pr, None, M, sol, sr)
        rel = D.norm(res) / D.norm(sol)
        res.free()
        D.status_all()
    if prev_own and prev is not sol:
        prev.free()
    for M in list(lhs_of.values()) + list(rhs_of.values()):
        M.free()
    return sol if rel is None else (sol, rel)


def implicit_euler_method(A, u0, guess, steps, normalize: bool = True, tt_solver: str = "krylov", max_bond: int = 0,
                          return_error: bool = False, **kw):
    """src/solvers/euler.jl:99-143 on a device-resident batch: per step M = I - h A, next = <tt_solver>_linsolve(M, solution, guess; kw...),
    optional next / norm(next), solution = tt_compress!(next, max_bond) or orthogonalize(next), guess = solution.  A: TToperator or
    DeviceTTO.  tt_solver: "krylov" (the default HERE; the reference defaults to "mals"), "als", "mals" or "dmrg"; the keywords go to
    the chosen solver and an unknown one is a TypeError.  return_error: (solution, rel_error), rel_error = norm(M solution - u_prev) /
    norm(solution) per train.  TTvector arguments: upload, batch 1, download."""
    return _implicit_stepper("implicit_euler_method", A, u0, guess, steps, normalize, return_error, tt_solver, max_bond, False, kw)


def crank_nicholson_method(A, u0, guess, steps, normalize: bool = True, tt_solver: str = "krylov", max_bond: int = 0,
                           return_error: bool = False, **kw):
    """src/solvers/euler.jl:145-191: per step LHS = I - (h/2) A, RHS = (I + (h/2) A) solution — formed as solution + (h/2) (A solution)
    by one launch of apply_axpby: the same tensor, another internal rank order than the reference's intermediate, which no caller sees —
    then as implicit_euler_method.  tt_solver defaults to "krylov" HERE (the reference: "mals").  return_error: rel_error =
    norm(LHS solution - RHS(u_prev)) / norm(solution) per train."""
    return _implicit_stepper("crank_nicholson_method", A, u0, guess, steps, normalize, return_error, tt_solver, max_bond, True, kw)


# ---------------------------------------------------------------------------------------------------------------------
# als_linsolve (src/solvers/als.jl:161-222) — csrc/ttn_als_kernels.h
# ---------------------------------------------------------------------------------------------------------------------
def als_linsolve_(A: DeviceTTO, b: DeviceTT, x0: DeviceTT, x: DeviceTT, sweep_count: int = 2) -> DeviceTT:
    """x_b = als_linsolve(A, b_b, x0_b; sweep_count) for every train of the batch; x keeps x0's ranks."""
    assert sweep_count >= 1, "sweep_count must be >= 1"
    _lib.check(_lib.lib().ttn_als_linsolve(A.h, b.h, x0.h, x.h, int(sweep_count)))
    return x


def als_linsolve(A: TToperator, b: TTvector, tt_start: TTvector, sweep_count: int = 2) -> TTvector:
    """Host-level form for one right-hand side (upload, solve on the device, download)."""
    dA = DeviceTTO(A)
    db, dx0 = DeviceTT.from_host(b), DeviceTT.from_host(tt_start)
    dx = DeviceTT(tt_start.ttv_dims, tt_start.ttv_rks)
    als_linsolve_(dA, db, dx0, dx, sweep_count)
    D.compress_status(dx)
    return dx.download(0)


# ---------------------------------------------------------------------------------------------------------------------
# mals_linsolve (src/solvers/mals.jl:240-312) — csrc/ttn_als_kernels.h (k_mals_linsolve)
# ---------------------------------------------------------------------------------------------------------------------
def mals_linsolve_(A: DeviceTTO, b: DeviceTT, x0: DeviceTT, x: DeviceTT, tol: float = 1.0e-12, rmax: int = 2 ** 30) -> DeviceTT:
    """x_b = mals_linsolve(A, b_b, x0_b; tol, rmax) for every train of the batch; x's capacity bounds the adapted ranks."""
    _lib.check(_lib.lib().ttn_mals_linsolve(A.h, b.h, x0.h, x.h, float(tol), int(min(rmax, 2 ** 30))))
    return x


def mals_capacity(dims, start_rks, rmax: int, limit: int = 2048):
    """Rank capacity for the result handle: min(rmax, prod(dims[:k]), prod(dims[k:])) like the reference's buffers
    (mals.jl:258, :23), at least the start ranks, lowered uniformly until every two-site system fits the device limit."""
    d = len(dims)
    full = [1] + [min(int(rmax), int(math.prod(dims[:k])), int(math.prod(dims[k:]))) for k in range(1, d)] + [1]
    cut = max(full)
    while True:
        cap = [max(min(f, cut), int(s)) for f, s in zip(full, start_rks)]
        worst = max(dims[i] * cap[i] * dims[i + 1] * cap[i + 2] for i in range(d - 1)) if d > 1 else 1
        if worst <= limit or cut <= 1:
            return cap
        cut -= 1


def mals_linsolve(A: TToperator, b: TTvector, tt_start: TTvector, tol: float = 1.0e-12, rmax: int | None = None) -> TTvector:
    """Host-level form for one right-hand side.  rmax defaults to round(sqrt(prod(dims))) like the reference (mals.jl:244)."""
    if rmax is None:
        rmax = int(round(math.sqrt(math.prod(tt_start.ttv_dims))))
    dA = DeviceTTO(A)
    db, dx0 = DeviceTT.from_host(b), DeviceTT.from_host(tt_start)
    dx = DeviceTT(tt_start.ttv_dims, mals_capacity(tt_start.ttv_dims, tt_start.ttv_rks, rmax))
    mals_linsolve_(dA, db, dx0, dx, tol, rmax)
    D.compress_status(dx)
    dx.max_ranks()
    return dx.download(0)


# ---------------------------------------------------------------------------------------------------------------------
# dmrg_linsolve, N = 2 (src/solvers/dmrg.jl:388-472) — the same persistent two-site kernel in its DMRG mode
# ---------------------------------------------------------------------------------------------------------------------
def dmrg_linsolve_(A: DeviceTTO, b: DeviceTT, x0: DeviceTT, x: DeviceTT, tol: float = 1.0e-12, sweep_schedule: Sequence[int] = (2,),
                   rmax_schedule: Sequence[int] | None = None, it_solver: bool = False, linsolv_maxiter: int = 200,
                   linsolv_tol: float | None = None, itslv_thresh: int = 2048) -> DeviceTT:
    """x_b = dmrg_linsolve(A, b_b, x0_b; N = 2, tol, sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter, linsolv_tol,
    itslv_thresh) for every train of the batch; x's capacity bounds the adapted ranks.  Local systems: dense LU (the reference's
    it_solver = false branch, dmrg.jl:173-175) unless `it_solver` or the system has more than `itslv_thresh` unknowns — then
    matrix-free conjugate gradients (dmrg.jl:99-171).  The defaults here (it_solver False, itslv_thresh 2048) solve to rounding
    wherever the dense path reaches; the reference's own defaults are it_solver = True, itslv_thresh = 256."""
    if rmax_schedule is None:
        rmax_schedule = (math.isqrt(math.prod(x0.dims)),)                   # dmrg.jl:391
    if linsolv_tol is None:
        linsolv_tol = max(math.sqrt(tol), 1.0e-8)                           # dmrg.jl:394
    ss = [int(v) for v in sweep_schedule]
    rs = [int(min(v, 2 ** 30)) for v in rmax_schedule]
    if len(rs) < len(ss):
        raise _lib.TTNError("dmrg_linsolve: rmax_schedule is shorter than sweep_schedule")      # BoundsError in the reference
    n = len(ss)
    arr = (C.c_int64 * max(n, 1))
    _lib.check(_lib.lib().ttn_dmrg_linsolve_it(A.h, b.h, x0.h, x.h, float(tol), n, arr(*ss) if n else None, arr(*rs[:n]) if n else None,
                                               1 if it_solver else 0, int(linsolv_maxiter), float(linsolv_tol), int(itslv_thresh)))
    return x


def dmrg_cg_iterations(batch: int):
    """Total conjugate-gradient iterations per train of the last two-site solve (0 when every local system was solved densely)."""
    out = (C.c_int64 * batch)()
    _lib.check(_lib.lib().ttn_dmrg_cg_iterations(batch, out))
    return [int(v) for v in out]


def dmrg_capacity(dims, start_rks, rmax: int, dense_only: bool = False):
    """Rank capacity of the result handle of dmrg_linsolve: the reference's buffer bounds min(rmax, prod(dims[:k]), prod(dims[k:]))
    (dmrg.jl:411), at least the start ranks, clamped to what the SVD core moves take (n_i * rank <= 256: ranks saturate there
    instead of growing to rmax; only START ranks beyond it are refused).  dense_only: lowered until every two-site system fits
    the dense solver (2048 unknowns) like mals_capacity."""
    if dense_only:
        return mals_capacity(dims, start_rks, rmax)
    d = len(dims)
    cap = [1]
    for k in range(1, d):
        lim = 256 // max(int(dims[k - 1]), int(dims[k]))        # the device bound: n * rank <= 256 on both cores that share bond k
        if int(start_rks[k]) > lim:
            raise _lib.TTNError("dmrg_linsolve: a start rank with n_k * rank above 256 is not supported (ranks up to 128 for n = 2)")
        # the reference's buffer bound, CLAMPED to the device bound (so the default rmax_schedule = isqrt(prod(dims)) — 4096 for the
        # 24-site C5 problem — works: the ranks then saturate at 128 for n = 2, which is the documented rank limit of this backend)
        cap.append(max(min(int(rmax), int(math.prod(dims[:k])), int(math.prod(dims[k:])), lim), int(start_rks[k])))
    return cap + [1]


def dmrg_linsolve(A: TToperator, b: TTvector, tt_start: TTvector, tol: float = 1.0e-12, sweep_schedule: Sequence[int] = (2,),
                  rmax_schedule: Sequence[int] | None = None, N: int = 2, it_solver: bool = False, linsolv_maxiter: int = 200,
                  linsolv_tol: float | None = None, itslv_thresh: int = 2048) -> TTvector:
    """Host-level form for one right-hand side (same keywords as src/solvers/dmrg.jl:388-396; see dmrg_linsolve_ for the two
    defaults that differ)."""
    if N != 2:
        raise _lib.TTNError("dmrg_linsolve: only the two-site scheme N = 2 is offered (single-site: als_linsolve)")
    if rmax_schedule is None:
        rmax_schedule = (math.isqrt(math.prod(tt_start.ttv_dims)),)
    dA = DeviceTTO(A)
    db, dx0 = DeviceTT.from_host(b), DeviceTT.from_host(tt_start)
    rtop = max(int(v) for v in rmax_schedule)
    cap = dmrg_capacity(tt_start.ttv_dims, tt_start.ttv_rks, rtop)
    if not it_solver and max(tt_start.ttv_dims[i] * cap[i] * tt_start.ttv_dims[i + 1] * cap[i + 2] for i in range(len(cap) - 2)) <= 2048:
        cap = mals_capacity(tt_start.ttv_dims, tt_start.ttv_rks, rtop)
    dx = DeviceTT(tt_start.ttv_dims, cap)
    dmrg_linsolve_(dA, db, dx0, dx, tol, sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh)
    D.compress_status(dx)
    dx.max_ranks()
    return dx.download(0)


# ---------------------------------------------------------------------------------------------------------------------
# dmrg_eigsolve, N = 2 (src/solvers/dmrg.jl:501-578) and mals_eigsolve (src/solvers/mals.jl:335-425) — csrc/ttn_eigsolve_kernels.h
# ---------------------------------------------------------------------------------------------------------------------
def _eig_schedules(who, sweep_schedule, rmax_schedule):
    ss = [int(v) for v in sweep_schedule]
    rs = [int(min(v, 2 ** 30)) for v in rmax_schedule]
    if len(rs) != len(ss):
        raise _lib.TTNError(f"{who}: Sweep schedule error (rmax_schedule and sweep_schedule differ in length)")     # dmrg.jl:513, mals.jl:346
    if not ss or any(v < 1 for v in ss) or any(b <= a for a, b in zip(ss, ss[1:])) or any(v < 1 for v in rs):
        raise _lib.TTNError(f"{who}: sweep_schedule must be positive and strictly increasing, rmax_schedule positive")
    if ss[-1] - 1 > 32:
        raise _lib.TTNError(f"{who}: more than 32 sweeps in one call")
    return ss, rs


def eigsolve_history_len(mode: int, d: int, sweep_schedule: Sequence[int]) -> int:
    """Length of the E / r_hist history of one train: 2 (d - 2) nsweeps + 1 (DMRG, mode 1), 2 (d - 1) nsweeps (MALS, mode 0)."""
    ss = [int(v) for v in sweep_schedule]
    arr = (C.c_int64 * max(len(ss), 1))(*ss)
    out = C.c_int64()
    _lib.check(_lib.lib().ttn_eigsolve_history_len(int(mode), int(d), len(ss), arr, C.byref(out)))
    return int(out.value)


EIG_ORTHO_MAX = 8          # TTN_EIG_ORTHO_MAX of include/ttn_eig_ortho.h


def _ortho_list(who, ortho_to, kind):
    """ortho_to as a list: one train or a sequence of them, all of type `kind`."""
    states = [ortho_to] if isinstance(ortho_to, kind) else list(ortho_to)
    if any(not isinstance(p, kind) for p in states):
        raise TypeError(f"{who}: ortho_to must be a {kind.__name__} or a sequence of them")
    if len(states) > EIG_ORTHO_MAX:
        raise _lib.TTNError(f"{who}: at most {EIG_ORTHO_MAX} states in ortho_to")
    return states


def _ortho_weights(who, weight, batch: int, m: int) -> np.ndarray:
    """The (batch, m) weight table of a penalised solve from a scalar, one value per state, or a (batch, m) array.  Needs no device."""
    if m == 0:                      # an empty ortho_to: the plain solve through the penalised entry point
        return np.zeros((batch, 1))
    if weight is None:
        raise _lib.TTNError(f"{who}: ortho_to needs weight (the penalty must exceed the gap to the wanted level)")
    try:
        w = np.asarray(weight, dtype=np.float64)
    except (TypeError, ValueError):
        raise _lib.TTNError(f"{who}: weight must be a number, one number per state, or a (batch, states) array") from None
    if w.ndim == 0 or w.shape == (m,) or w.shape == (batch, m):
        w = np.ascontiguousarray(np.broadcast_to(w, (batch, m)))
    else:
        raise _lib.TTNError(f"{who}: weight of shape {w.shape} fits neither ({m},) nor ({batch}, {m})")
    if not np.all(np.isfinite(w)) or not np.all(w > 0.0):
        raise _lib.TTNError(f"{who}: every weight must be finite and > 0")
    return w


def _two_site_eigsolve_(mode, A: DeviceTTO, x0: DeviceTT, x: DeviceTT, tol, sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter,
                        linsolv_tol, itslv_thresh, ortho_to=None, weight=None):
    who = "dmrg_eigsolve" if mode == 1 else "mals_eigsolve"
    if ortho_to is None and weight is not None:
        raise _lib.TTNError(f"{who}: weight without ortho_to")
    ss, rs = _eig_schedules(who, sweep_schedule, rmax_schedule)
    if linsolv_tol is None:
        linsolv_tol = max(math.sqrt(tol), 1.0e-8)                              # dmrg.jl:510, mals.jl:340
    B = x0.batch
    if ortho_to is not None:
        states = _ortho_list(who, ortho_to, DeviceTT)
        w = _ortho_weights(who, weight, B, len(states))
    hl = eigsolve_history_len(mode, len(x0.dims), ss)
    E = np.zeros((B, max(hl, 1)))
    R = np.zeros((B, max(hl, 1)), dtype=np.int64)
    arr = C.c_int64 * len(ss)
    tail = (float(tol), len(ss), arr(*ss), arr(*rs), 1 if it_solver else 0, int(linsolv_maxiter), float(linsolv_tol), int(itslv_thresh), hl,
            E.ctypes.data_as(_lib.p_f64), R.ctypes.data_as(_lib.p_i64))
    hist = lambda: ([list(map(float, E[b, :hl])) for b in range(B)], [list(map(int, R[b, :hl])) for b in range(B)])
    if ortho_to is None:
        fn = _lib.lib().ttn_dmrg_eigsolve if mode == 1 else _lib.lib().ttn_mals_eigsolve
        _lib.check(fn(A.h, x0.h, x.h, *tail))
        return hist()
    m = len(states)
    if getattr(A, "batch", 1) > 1:
        # The penalised entry points take one operator (every entry point outside ttn_opbatch.h's list refuses a batch): an operator
        # batch is solved one operator at a time, train b with A.select(b) on single-train copies, bit for bit the single calls.
        if A.batch != B:
            raise _lib.TTNError(f"{who}: batch sizes differ (the operator batch and the trains)")
        Es, Rs, ovl = [], [], np.zeros((B, m))
        for b in range(B):
            Ab, s0, s = A.select(b), DeviceTT.from_host(x0.download(b)), DeviceTT(x.dims, x.cap)
            sp = [p if p.batch == 1 else DeviceTT.from_host(p.download(b)) for p in states]
            e, r, o = _two_site_eigsolve_(mode, Ab, s0, s, tol, ss, rs, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh, sp,
                                          w[b:b + 1, :m] if m else None)
            s.max_ranks()
            x.upload(b, s.download(0))
            Es.append(e[0]); Rs.append(r[0]); ovl[b] = o[0]
            for h in [Ab, s0, s] + [p for p, q in zip(sp, states) if p is not q]:
                h.free()
        return Es, Rs, ovl
    ovl = np.zeros((B, max(m, 1)))
    phi = (C.c_void_p * max(m, 1))(*[p.h for p in states])
    fn = _lib.lib().ttn_dmrg_eigsolve_ortho if mode == 1 else _lib.lib().ttn_mals_eigsolve_ortho
    _lib.check(fn(A.h, x0.h, x.h, m, phi, w.ctypes.data_as(_lib.p_f64), *tail, ovl.ctypes.data_as(_lib.p_f64)))
    return hist() + (ovl[:, :m].copy(),)


def dmrg_eigsolve_(A: DeviceTTO, x0: DeviceTT, x: DeviceTT, tol: float = 1.0e-12, sweep_schedule: Sequence[int] = (2,),
                   rmax_schedule: Sequence[int] | None = None, it_solver: bool = False, linsolv_maxiter: int = 200,
                   linsolv_tol: float | None = None, itslv_thresh: int = 256, *, ortho_to=None, weight=None):
    """(E_b, r_hist_b) of dmrg_eigsolve(A, x0_b; N = 2, ...) for every train of the batch; x receives the eigenvectors (its capacity
    bounds the adapted ranks).  Returns (E, r_hist): per-train lists.

    ortho_to (a DeviceTT or a sequence of up to 8; batch that of x0, or 1 = shared) with weight (a scalar, one value per state, or a
    (batch, states) array; required) solves A + sum_j weight_j |phi_j><phi_j| / <phi_j, phi_j> instead (csrc/ttn_eig_ortho_kernels.h):
    with the phi_j the levels below and the weights above the gap, the next level.  Returns (E, r_hist, overlaps) then: E holds the
    local eigenvalues of the PENALISED problem (take the energy with device.rayleigh), overlaps (batch, states) the
    <phi_j, x> / ||phi_j|| of the result.  With ortho_to an operator batch is solved one operator at a time (A.select(b) on copies of
    train b, one launch per train: the C entry point takes one operator); eigsolve_stats then holds the last train's figures only."""
    if rmax_schedule is None:
        rmax_schedule = (math.isqrt(math.prod(x0.dims)),)                     # dmrg.jl:507
    return _two_site_eigsolve_(1, A, x0, x, tol, sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh,
                               ortho_to, weight)


def mals_eigsolve_(A: DeviceTTO, x0: DeviceTT, x: DeviceTT, tol: float = 1.0e-12, sweep_schedule: Sequence[int] = (2,),
                   rmax_schedule: Sequence[int] | None = None, it_solver: bool = False, linsolv_maxiter: int = 200,
                   linsolv_tol: float | None = None, itslv_thresh: int = 256, *, ortho_to=None, weight=None):
    """(E_b, r_hist_b) of mals_eigsolve(A, x0_b; ...) for every train of the batch.  itslv_thresh is accepted and, as in the reference
    (mals.jl:383-390, :403-410), not used: the local threshold is 256.  ortho_to / weight as in dmrg_eigsolve_."""
    if rmax_schedule is None:
        rmax_schedule = (int(round(math.sqrt(math.prod(x0.dims)))),)          # mals.jl:338
    return _two_site_eigsolve_(0, A, x0, x, tol, sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh,
                               ortho_to, weight)


def eigsolve_stats(batch: int):
    """(Lanczos operator applications, largest final Lanczos residual) per train of the last eigensolve."""
    it = (C.c_int64 * batch)()
    res = (C.c_double * batch)()
    _lib.check(_lib.lib().ttn_eigsolve_stats(batch, it, res))
    return [int(v) for v in it], [float(v) for v in res]


def _eig_host(mode, A: TToperator, tt_start: TTvector, tol, sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter, linsolv_tol,
              itslv_thresh, ortho_to=None, weight=None):
    who = "dmrg_eigsolve" if mode == 1 else "mals_eigsolve"
    dims = tuple(tt_start.ttv_dims)
    if rmax_schedule is None:
        rmax_schedule = (math.isqrt(math.prod(dims)),) if mode == 1 else (int(round(math.sqrt(math.prod(dims)))),)
    ss, rs = _eig_schedules(who, sweep_schedule, rmax_schedule)       # refusals before anything reaches the device
    if ortho_to is None and weight is not None:
        raise _lib.TTNError(f"{who}: weight without ortho_to")
    if ortho_to is not None:
        states = _ortho_list(who, ortho_to, TTvector)
        weight = _ortho_weights(who, weight, 1, len(states))
    rtop = max(rs)
    cap = dmrg_capacity(dims, tt_start.ttv_rks, rtop)                  # n_i * rank <= 256 (TTNError for start ranks beyond it)
    dA = DeviceTTO(A)
    dx0 = DeviceTT.from_host(tt_start)
    dx = DeviceTT(dims, cap)
    fn = dmrg_eigsolve_ if mode == 1 else mals_eigsolve_
    if ortho_to is None:
        E, R = fn(dA, dx0, dx, tol, ss, rs, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh)
    else:
        dphi = [DeviceTT.from_host(p) for p in states]
        try:
            E, R, _ = fn(dA, dx0, dx, tol, ss, rs, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh, ortho_to=dphi,
                         weight=weight if states else None)
        finally:
            for h in dphi:
                h.free()
    dx.max_ranks()
    return E[0], dx.download(0), R[0]


def dmrg_eigsolve(A: TToperator, tt_start: TTvector, N: int = 2, tol: float = 1.0e-12, sweep_schedule: Sequence[int] = (2,),
                  rmax_schedule: Sequence[int] | None = None, it_solver: bool = False, linsolv_maxiter: int = 200,
                  linsolv_tol: float | None = None, itslv_thresh: int = 256, *, ortho_to=None, weight=None):
    """(E, x, r_hist) = dmrg_eigsolve(A, tt_start; N = 2, ...) (src/solvers/dmrg.jl:501-578) with the reference's keywords and defaults:
    E the eigenvalue of every micro-step, x the normalised eigenvector train, r_hist max(ttv_rks) after every micro-step.  The rank
    capacity is the reference's buffer bound clamped to n_i * rank <= 256 (dmrg_capacity).  ortho_to (a TTvector or a sequence of them)
    with weight (a scalar or one value per state): the penalised solve of dmrg_eigsolve_, E then the penalised local eigenvalues."""
    if N != 2:
        raise _lib.TTNError("dmrg_eigsolve: only the two-site scheme N = 2 is offered")
    return _eig_host(1, A, tt_start, tol, sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh, ortho_to, weight)


def mals_eigsolve(A: TToperator, tt_start: TTvector, tol: float = 1.0e-12, sweep_schedule: Sequence[int] = (2,),
                  rmax_schedule: Sequence[int] | None = None, it_solver: bool = False, linsolv_maxiter: int = 200,
                  linsolv_tol: float | None = None, itslv_thresh: int = 256, *, ortho_to=None, weight=None):
    """(E, x, r_hist) = mals_eigsolve(A, tt_start; ...) (src/solvers/mals.jl:335-425); rmax_schedule defaults to round(sqrt(prod(dims))).
    ortho_to / weight as in dmrg_eigsolve."""
    return _eig_host(0, A, tt_start, tol, sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh, ortho_to, weight)


def _level_weights(who, weight, j: int, batch: int):
    """The weights of level j (against levels 0 .. j-1) from lowest_states' weight: a scalar, one value per state, or (batch, states)."""
    w = np.asarray(weight, dtype=np.float64)
    if w.ndim == 0:
        return float(w)
    if (w.ndim == 1 and w.shape[0] >= j) or (w.ndim == 2 and w.shape[0] == batch and w.shape[1] >= j):
        return w[..., :j]
    raise _lib.TTNError(f"{who}: weight of shape {w.shape} does not cover {j} states")


def lowest_states_(A: DeviceTTO, x0s, k: int, weight, mode: str = "dmrg", **kw):
    """The k lowest eigenpairs of A for every train of a batch, one level after the other: level j is the penalised solve
    (dmrg_eigsolve_ / mals_eigsolve_ with ortho_to) against the results of levels 0 .. j-1.  x0s: one DeviceTT batch of start trains
    per level, or one batch used for every level.  weight: a scalar, one value per state, or a (batch, states) array, above the
    distance from level 0 to level k-1.  mode "dmrg" or "mals"; kw: the keywords of the solver.
    Returns (xs, E, S): the k result handles, the (batch, k) energies device.rayleigh(A, xs[j]) and the (batch, k, k) overlaps
    device.dot(xs[i], xs[j])."""
    if mode not in ("dmrg", "mals"):
        raise _lib.TTNError(f"lowest_states: mode must be 'dmrg' or 'mals', got {mode!r}")
    k = int(k)
    if not 1 <= k <= EIG_ORTHO_MAX + 1:
        raise _lib.TTNError(f"lowest_states: k must lie in 1 .. {EIG_ORTHO_MAX + 1}")
    starts = [x0s] * k if isinstance(x0s, DeviceTT) else list(x0s)
    if len(starts) != k or any(not isinstance(s, DeviceTT) for s in starts):
        raise _lib.TTNError("lowest_states: x0s must be one DeviceTT batch or one per level")
    B = starts[0].batch
    for j in range(1, k):
        _level_weights("lowest_states", weight, j, B)                  # refusals before the first solve
    dims = starts[0].dims
    rs = kw.get("rmax_schedule")
    if rs is None:
        rs = kw["rmax_schedule"] = (math.isqrt(math.prod(dims)),) if mode == "dmrg" else (int(round(math.sqrt(math.prod(dims)))),)
    fn = dmrg_eigsolve_ if mode == "dmrg" else mals_eigsolve_
    xs = []
    for j in range(k):
        x = DeviceTT(dims, dmrg_capacity(dims, starts[j].max_ranks(), max(int(v) for v in rs)), B)
        if j == 0:
            fn(A, starts[j], x, **kw)
        else:
            fn(A, starts[j], x, ortho_to=xs, weight=_level_weights("lowest_states", weight, j, B), **kw)
        xs.append(x)
    E = np.stack([D.rayleigh(A, x) for x in xs], axis=1)
    S = np.empty((B, k, k))
    for i in range(k):
        for j in range(i, k):
            S[:, i, j] = S[:, j, i] = D.dot(xs[i], xs[j])
    return xs, E, S


def lowest_states(A: TToperator, x0s, k: int, weight, mode: str = "dmrg", **kw):
    """Host form of lowest_states_ for one operator: x0s a TTvector (used for every level) or one per level.  Returns (E, xs, S): the k
    energies (Rayleigh quotients of the results), the k TTvectors and their k x k overlap matrix."""
    starts = [x0s] * int(k) if isinstance(x0s, TTvector) else list(x0s)
    if any(not isinstance(s, TTvector) for s in starts):
        raise TypeError("lowest_states: x0s must be a TTvector or a sequence of them")
    if kw.get("N", 2) != 2:
        raise _lib.TTNError("lowest_states: only the two-site scheme N = 2 is offered")
    kw.pop("N", None)
    xs, E, S = lowest_states_(DeviceTTO(A), [DeviceTT.from_host(s) for s in starts], k, weight, mode, **kw)
    for x in xs:
        x.max_ranks()
    return E[0], [x.download(0) for x in xs], S[0]


# ---------------------------------------------------------------------------------------------------------------------
# als_eigsolve (src/solvers/als.jl:251-326) and als_gen_eigsolv (src/solvers/als.jl:344-426) — csrc/ttn_als_eig_kernels.h
# ---------------------------------------------------------------------------------------------------------------------
def _rd_rks(rks, dims, rmax: int = 1024):
    """r_and_d_to_rks (src/tt_tools.jl) on the host: rank k is capped by prod(dims[:k]), prod(dims[k:]) and rmax."""
    return [min(int(r), math.prod(dims[:k]), math.prod(dims[k:]), int(rmax)) if 0 < k < len(dims) else 1 for k, r in enumerate(rks)]


def _als_stages(who, dims, start_rks, sweep_schedule, rmax_schedule, noise_schedule=None):
    """Every refusal of the schedule and the start train, on the host: (ss, rs, ns, ranks of every stage)."""
    ss = [int(v) for v in sweep_schedule]
    rs = [int(min(v, 2 ** 30)) for v in rmax_schedule]
    ns = [float(v) for v in noise_schedule] if noise_schedule is not None else [0.0] * len(rs)
    if not (len(rs) == len(ss) == len(ns)):
        raise _lib.TTNError(f"{who}: Sweep schedule error (the schedules differ in length)")            # als.jl:263
    if not ss or any(v < 1 for v in ss) or any(b <= a for a, b in zip(ss, ss[1:])) or any(v < 1 for v in rs):
        raise _lib.TTNError(f"{who}: sweep_schedule must be positive and strictly increasing, rmax_schedule positive")
    if not all(math.isfinite(v) for v in ns):
        raise _lib.TTNError(f"{who}: noise_schedule is not finite")
    if ss[-1] - 1 > 32:
        raise _lib.TTNError(f"{who}: more than 32 sweeps in one call")
    d = len(dims)
    if d < 2:
        raise _lib.TTNError(f"{who}: needs at least two sites")
    r0 = [int(v) for v in start_rks]
    if _rd_rks(r0, dims) != r0:
        raise _lib.TTNError(f"{who}: the start ranks exceed what orthogonalize keeps")
    if any(dims[i] * r0[i] < r0[i + 1] or dims[i] * r0[i + 1] < r0[i] for i in range(d)):
        raise _lib.TTNError(f"{who}: a core is too flat for the QR core moves")
    stages = [r0]
    for j in range(1, len(ss)):
        if rs[j] <= max(stages[-1]):
            raise _lib.TTNError(f"{who}: New bond dimension too low (a stage's rmax must exceed the current maximum rank)")   # tt_tools.jl:478
        stages.append(_rd_rks([1] + [rs[j]] * (d - 1) + [1], dims, rs[j]))
    return ss, rs, ns, stages


def als_capacity(dims, start_rks, sweep_schedule=(2,), rmax_schedule=None):
    """Rank capacity x needs for a schedule: the largest rank of any stage at every bond."""
    if rmax_schedule is None:
        rmax_schedule = (max(start_rks),)
    _, _, _, stages = _als_stages("als_capacity", list(dims), start_rks, sweep_schedule, rmax_schedule)
    return [max(s[k] for s in stages) for k in range(len(dims) + 1)]


def _als_eig_run(gen, A: DeviceTTO, S, x0: DeviceTT, x: DeviceTT, sweep_schedule, rmax_schedule, noise_schedule, seed, it_solver, maxiter,
                 linsolv_tol, itslv_thresh):
    who = "als_gen_eigsolv" if gen else "als_eigsolve"
    if rmax_schedule is None:
        rmax_schedule = (max(x0.max_ranks()),)
    ss = [int(v) for v in sweep_schedule]
    rs = [int(min(v, 2 ** 30)) for v in rmax_schedule]
    ns = [float(v) for v in noise_schedule] if noise_schedule is not None else [0.0] * len(rs)
    if not (len(rs) == len(ss) == len(ns)):
        raise _lib.TTNError(f"{who}: Sweep schedule error (the schedules differ in length)")
    hl = eigsolve_history_len(2, len(x0.dims), ss) if ss else 0
    B = x0.batch
    E = np.zeros((B, max(hl, 1)))
    n = len(ss)
    arr = C.c_int64 * max(n, 1)
    nrr = C.c_double * max(n, 1)
    if gen:
        _lib.check(_lib.lib().ttn_als_gen_eigsolve(A.h, S.h, x0.h, x.h, n, arr(*ss), arr(*rs), 1 if it_solver else 0, int(itslv_thresh), hl,
                                                   E.ctypes.data_as(_lib.p_f64)))
    else:
        _lib.check(_lib.lib().ttn_als_eigsolve(A.h, x0.h, x.h, n, arr(*ss), arr(*rs), nrr(*ns), int(seed), 1 if it_solver else 0, int(maxiter),
                                               float(linsolv_tol), int(itslv_thresh), hl, E.ctypes.data_as(_lib.p_f64)))
    return [list(map(float, E[b, :hl])) for b in range(B)]


def als_eigsolve_(A: DeviceTTO, x0: DeviceTT, x: DeviceTT, sweep_schedule: Sequence[int] = (2,), rmax_schedule: Sequence[int] | None = None,
                  noise_schedule: Sequence[float] | None = None, it_solver: bool = False, itslv_thresh: int = 1024, maxiter: int = 200,
                  linsolv_tol: float = 1.0e-8, seed: int = 0):
    """E_b of als_eigsolve(A, x0_b; ...) for every train of the batch; x receives the eigenvectors (its capacity must hold the ranks of
    every stage: als_capacity).  rmax_schedule defaults to [max rank of x0], noise_schedule to zeros."""
    return _als_eig_run(0, A, None, x0, x, sweep_schedule, rmax_schedule, noise_schedule, seed, it_solver, maxiter, linsolv_tol, itslv_thresh)


def als_gen_eigsolv_(A: DeviceTTO, S: DeviceTTO, x0: DeviceTT, x: DeviceTT, sweep_schedule: Sequence[int] = (2,),
                     rmax_schedule: Sequence[int] | None = None, tol: float = 1.0e-10, it_solver: bool = False, itslv_thresh: int = 2500):
    """E_b of als_gen_eigsolv(A, S, x0_b; ...) for every train of the batch.  `tol` is accepted and unused, as in the reference."""
    return _als_eig_run(1, A, S, x0, x, sweep_schedule, rmax_schedule, None, 0, it_solver, 1, 1.0e-8, itslv_thresh)


def _als_host(gen, A: TToperator, S, tt_start: TTvector, sweep_schedule, rmax_schedule, noise_schedule, seed, it_solver, maxiter, linsolv_tol,
              itslv_thresh):
    who = "als_gen_eigsolv" if gen else "als_eigsolve"
    dims = tuple(tt_start.ttv_dims)
    if rmax_schedule is None:
        rmax_schedule = (max(tt_start.ttv_rks),)                                  # als.jl:254, :344
    if noise_schedule is None:
        noise_schedule = (0.0,) * len(rmax_schedule)                              # als.jl:255
    ss, rs, ns, stages = _als_stages(who, dims, tt_start.ttv_rks, sweep_schedule, rmax_schedule, noise_schedule)
    cap = [max(s[k] for s in stages) for k in range(len(dims) + 1)]
    dA = DeviceTTO(A)
    dS = DeviceTTO(S) if gen else None
    dx0 = DeviceTT.from_host(tt_start)
    dx = DeviceTT(dims, cap)
    E = _als_eig_run(gen, dA, dS, dx0, dx, ss, rs, ns, seed, it_solver, maxiter, linsolv_tol, itslv_thresh)
    dx.max_ranks()
    return E[0], dx.download(0)


def als_eigsolve(A: TToperator, tt_start: TTvector, sweep_schedule: Sequence[int] = (2,), rmax_schedule: Sequence[int] | None = None,
                 noise_schedule: Sequence[float] | None = None, it_solver: bool = False, itslv_thresh: int = 1024, maxiter: int = 200,
                 linsolv_tol: float = 1.0e-8, seed: int = 0):
    """(E, x) = als_eigsolve(A, tt_start; ...) (src/solvers/als.jl:251-326) with the reference's keywords and defaults: E the eigenvalue of
    every micro-step, x the normalised eigenvector train.  The noise of a rank increase is seeded (`seed`) instead of drawn from the
    global random stream."""
    return _als_host(0, A, None, tt_start, sweep_schedule, rmax_schedule, noise_schedule, seed, it_solver, maxiter, linsolv_tol, itslv_thresh)


def als_gen_eigsolv(A: TToperator, S: TToperator, tt_start: TTvector, sweep_schedule: Sequence[int] = (2,),
                    rmax_schedule: Sequence[int] | None = None, tol: float = 1.0e-10, it_solver: bool = False, itslv_thresh: int = 2500):
    """(E, x) = als_gen_eigsolv(A, S, tt_start; ...) (src/solvers/als.jl:344-426): the smallest eigenpair of A x = lambda S x, x
    S-normalised.  `tol` is accepted and unused, as in the reference (als.jl:344)."""
    return _als_host(1, A, S, tt_start, sweep_schedule, rmax_schedule, None, 0, it_solver, 1, 1.0e-8, itslv_thresh)
