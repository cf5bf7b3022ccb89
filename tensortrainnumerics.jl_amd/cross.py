"""TT-cross interpolation and integration on the device — src/tt_cross_interpolation.jl: tt_cross (MaxVol, DMRG), tt_integrate.

A function f of N coordinates becomes a TTvector from O(d n r^2) of its values.  f is the caller's: it receives the (P, N) coordinate
matrix as a torch tensor on the library's device (float64, or complex128 for a complex domain), is called on the library's stream, and
returns P values, a torch tensor on any device or anything np.asarray accepts (a NumPy function calls `.cpu().numpy()` itself).
Everything else is device work: the index sets (int64, column-major, 1-based, as in the reference) and the cores stay on the device
from the first call of f until the final download.  The pivot search (maxvol), the index matrices with their coordinate gathers and
the evaluation of a train are this library's kernels (csrc/ttn_cross_kernels.h); the QR of the fibre matrices and DMRG's superblock
SVD are ttn_dense_qr / ttn_dense_svd through the TDVP module's helpers; torch is plumbing (memory, index arithmetic on the sets).  A
MaxVol sweep reads the host once, at its validation (the error, the finiteness flag and the maxvol status words together); DMRG also
reads each superblock's singular values to choose the rank.  No CPU fallback: without a GPU these functions raise TTNError.

tt_cross_batch / tt_integrate_batch run MaxVol for many functions at once: f(X, which) receives the coordinates of
every function still running, one workgroup per function does a whole site step (scale, QR, maxvol, core, next index set:
csrc/ttn_cross_batch_kernels.h), a sweep still reads the host once, finished functions leave the active set, and the result is a list
of host trains or one resident DeviceTT batch filled on the device.  Float64 on a real domain, MaxVol only.

Deviations from the reference: the random draws come from a seeded portable stream (`draw_indices`), non-finite
values of f raise TTNError, Greedy is not offered, and a MaxVol run that stops at maxiter after a kick returns the ranks of its cores.
"""
from __future__ import annotations

import ctypes as C
import logging
import math

import numpy as np

from . import _lib
from .constructors import _splitmix64
from .tdvp import _dev, _operands, _own, _p, _qr_j, _svd_j, _svd_rank
from .tt import TTvector

log = logging.getLogger("TensorTrainNumerics")

CROSS_MAXITER = 50
CROSS_TOL = 1.0e-10
CROSS_RMAX = 500
CROSS_KICKRANK = 5
MAXVOL_TOL = 1.05


class MaxVolPivot:
    def __init__(self, tol: float = MAXVOL_TOL, maxiter: int = 100):
        self.tol, self.maxiter = float(tol), int(maxiter)


class RandomPivot:
    def __init__(self, nsamples: int = 1000, seed=None):
        self.nsamples, self.seed = int(nsamples), seed


class _CrossAlgorithm:
    def __init__(self, maxiter, tol, rmax, kickrank, verbose, pivot):
        self.maxiter, self.tol, self.rmax = int(maxiter), float(tol), int(rmax)
        self.kickrank = None if kickrank is None else int(kickrank)
        self.verbose, self.pivot = bool(verbose), pivot


class MaxVol(_CrossAlgorithm):
    def __init__(self, maxiter=CROSS_MAXITER, tol=CROSS_TOL, rmax=CROSS_RMAX, kickrank=CROSS_KICKRANK, verbose=True, pivot=None):
        super().__init__(maxiter, tol, rmax, kickrank, verbose, MaxVolPivot() if pivot is None else pivot)


class DMRG(_CrossAlgorithm):
    def __init__(self, maxiter=CROSS_MAXITER, tol=CROSS_TOL, rmax=CROSS_RMAX, kickrank=CROSS_KICKRANK, verbose=True, pivot=None):
        super().__init__(maxiter, tol, rmax, kickrank, verbose, MaxVolPivot() if pivot is None else pivot)


class Greedy:
    """Constructible with the reference's fields and defaults; tt_cross does not offer it (TTNError)."""

    def __init__(self, maxiter=CROSS_MAXITER, tol=CROSS_TOL, rmax=CROSS_RMAX, verbose=True, nsamples=1000, pivot=None):
        self.maxiter, self.tol, self.rmax = int(maxiter), float(tol), int(rmax)
        self.verbose, self.nsamples = bool(verbose), int(nsamples)
        self.pivot = RandomPivot() if pivot is None else pivot


# ---------------------------------------------------------------------------------------------------------------------------------
# host helpers (integer work and quadrature setup)
# ---------------------------------------------------------------------------------------------------------------------------------
# Sub-seeds of the random draws.  The reference draws from Julia's global RNG; here every draw has its own stream, named by
# (kind, a, b): 1 the initial right index sets of MaxVol (the shared matrix `randint`, :212-214), 2 the validation points (:220, :597),
# 3 the kickrank rows of iteration a at site b (:305), 4 DMRG's I_l[a] (:589), 5 DMRG's I_g[a] (:592).
DRAW_MAXVOL_RSETS, DRAW_VALIDATION, DRAW_KICK, DRAW_DMRG_LEFT, DRAW_DMRG_RIGHT = 1, 2, 3, 4, 5


def _subseed(seed: int, kind: int, a: int = 0, b: int = 0) -> int:
    p = 1000003
    return (((int(seed) * p + kind) * p + a) * p + b) % (1 << 64)


def draw_indices(seed: int, kind: int, a: int, b: int, rows: int, highs) -> np.ndarray:
    """rows x len(highs) matrix of 1-based indices, column c uniform on 1:highs[c], drawn in column-major order from the portable
    splitmix64 stream (constructors.py) of sub-seed (seed, kind, a, b): index = 1 + floor(u n), u = the 53-bit uniform of each word."""
    highs = [int(h) for h in highs]
    n = rows * len(highs)
    if n == 0:
        return np.zeros((rows, len(highs)), dtype=np.int64)
    u = (_splitmix64(n, _subseed(seed, kind, a, b)) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    hi = np.repeat(np.asarray(highs, dtype=np.int64), rows)
    idx = np.minimum(np.floor(u * hi).astype(np.int64), hi - 1) + 1
    return idx.reshape((rows, len(highs)), order="F")


DRAW_SAMPLE = 6      # the uniforms of tt_sample (include/ttn_sample.h): sub-seed (seed, DRAW_SAMPLE, train, 0)


def sample_uniforms(seed: int, batch: int, nsamples: int, d: int) -> np.ndarray:
    """The (batch, nsamples, d) uniforms in [0, 1) that ``tt_sample`` / ``device.sample`` generate on the device for ``u=None``, bit for
    bit: entry (b, s, k) is the 53-bit uniform of word 1 + k + d s of the splitmix64 stream of sub-seed (seed, DRAW_SAMPLE, b, 0), so
    the first S samples of a train do not depend on S."""
    batch, nsamples, d = int(batch), int(nsamples), int(d)
    if batch < 1 or nsamples < 1 or d < 1:
        raise _lib.TTNError(f"sample_uniforms: batch, nsamples and d must be at least 1, got {batch}, {nsamples}, {d}")
    out = np.empty((batch, nsamples, d), dtype=np.float64)
    for b in range(batch):
        words = _splitmix64(nsamples * d, _subseed(seed, DRAW_SAMPLE, b, 0))
        out[b] = ((words >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)).reshape(nsamples, d)
    return out


def _cap_ranks_(Rs, Is, rmax):
    """_cap_ranks! (:106-115) on 1-based lists (Rs[1..N+1], Is[1..N]; index 0 unused)."""
    N = len(Is) - 1
    for n in range(2, N + 1):
        Rs[n] = min(Rs[n - 1] * Is[n - 1], Rs[n], Is[n] * Rs[n + 1], rmax)
    for n in range(N - 1, 0, -1):
        Rs[n + 1] = min(Rs[n] * Is[n], Rs[n + 1], Is[n + 1] * Rs[n + 2], rmax)
    return Rs


def _gauss_legendre(n: int, a, b):
    """nodes and weights of the n-point Gauss-Legendre rule on [a, b] (:695-700): Golub-Welsch on the host."""
    k = np.arange(1, n, dtype=np.float64)
    beta = k / np.sqrt(4.0 * k * k - 1.0)
    J = np.diag(beta, 1) + np.diag(beta, -1)
    lam, V = np.linalg.eigh(J)
    return (b - a) / 2 * lam + (a + b) / 2, (b - a) * V[0, :] ** 2


# ---------------------------------------------------------------------------------------------------------------------------------
# device wrappers.  A Julia matrix (m x n, column-major) is the contiguous torch tensor of shape (n, m).
# ---------------------------------------------------------------------------------------------------------------------------------
def _pow2_scale(V):
    """2^-e, 2^e the binade of max |V| (1 for a zero V), as a device scalar: a QR's Q and an SVD's vectors are unchanged by this
    exact scaling, and the sums of squares inside the dense kernels no longer underflow (values like exp(-400)) or overflow"""
    torch, _ = _dev()
    a = V.abs().amax()
    e = torch.where(a > 0, torch.clamp(torch.floor(torch.log2(a)), -1022.0, 1023.0), torch.zeros_like(a))
    return torch.exp2(-e)


def _d_maxvol(Qt, tol, maxiter, dinfo=None):
    """maxvol!(Q, tol, maxiter) of the Julia matrix Q (m x r) held as Qt (r, m): (piv (r,) 1-based int64, Ct = (Q / Q[piv,:]) as (r, m))
    on the device, asynchronous; dinfo (2 int64, device) receives {status, swaps}."""
    _operands(Qt)
    torch, _ = _dev()
    r, m = Qt.shape
    piv = torch.empty((r,), dtype=torch.int64, device=Qt.device)
    Ct = torch.empty_like(Qt)
    _lib.check(_lib.lib().ttn_cross_maxvol(1 if Qt.is_complex() else 0, m, r, _p(Qt), float(tol), int(maxiter), _p(piv), _p(Ct),
                                           None if dinfo is None else _p(dinfo), None))
    return piv, Ct


def maxvol(A, tol: float = MAXVOL_TOL, maxiter: int = 100):
    """maxvol on a host matrix A (m x r, m >= r) through the device kernel: (piv 1-based, C = A / A[piv,:], swaps).  A zero pivot
    raises TTNError (TTN_ERR_SINGULAR)."""
    torch, stream = _dev()
    A = np.asarray(A)
    dt = np.complex128 if np.iscomplexobj(A) else np.float64
    with torch.cuda.stream(stream):
        At = torch.from_numpy(np.ascontiguousarray(np.asarray(A, dtype=dt).T)).to("cuda")
        r, m = At.shape
        piv = torch.empty((r,), dtype=torch.int64, device="cuda")
        Ct = torch.empty_like(At)
        info = (C.c_int64 * 2)()
        _lib.check(_lib.lib().ttn_cross_maxvol(1 if dt == np.complex128 else 0, m, r, _p(At), float(tol), int(maxiter), _p(piv), _p(Ct),
                                               None, info))
        return piv.cpu().numpy(), Ct.cpu().numpy().T.copy(), int(info[1])


def _core_table(cores):
    ptrs = (C.POINTER(C.c_double) * len(cores))(*[C.cast(C.c_void_p(c.data_ptr()), C.POINTER(C.c_double)) for c in cores])
    dims = (C.c_int64 * len(cores))(*[int(c.shape[2]) for c in cores])
    rks = (C.c_int64 * (len(cores) + 1))(*([int(cores[0].shape[1])] + [int(c.shape[0]) for c in cores]))
    return ptrs, dims, rks


def _check_train(shapes, what):
    """the cores (n, r_left, r_right) chain, with end ranks 1: the kernel reads core k as n_k x r_{k-1} x r_k, so a train that does
    not chain would be read past its end.  Raises TTNError (the reference's DimensionMismatch) before anything is launched."""
    if not shapes or any(len(sh) != 3 or min(sh) < 1 for sh in shapes):
        raise _lib.TTNError(f"{what}: the cores must be non-empty 3-D arrays (n, r_left, r_right)")
    if shapes[0][1] != 1 or shapes[-1][2] != 1:
        raise _lib.TTNError(f"{what}: the end ranks must be 1, got {shapes[0][1]} and {shapes[-1][2]}")
    for k in range(1, len(shapes)):
        if shapes[k][1] != shapes[k - 1][2]:
            raise _lib.TTNError(f"{what}: DimensionMismatch: core {k + 1} has left rank {shapes[k][1]}, core {k} right rank {shapes[k - 1][2]}")


def _d_eval(cores, idx=None, w=None, yref=None, tol=0.0):
    """_evaluate_tt / _contract_with_weights on device cores (each (r_right, r_left, n), one dtype): idx is the index matrix (P x N,
    1-based) held as (N, P); w the concatenated weight vectors.  Returns (values (P,), err (1,) or None)."""
    cplx = _operands(*cores, *([w] if w is not None else []), *([yref] if yref is not None else []))
    torch, _ = _dev()
    N = len(cores)
    _check_train([tuple(reversed(c.shape)) for c in cores], "train evaluation")
    if idx is not None and (idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != N or not idx.is_contiguous()):
        raise _lib.TTNError(f"train evaluation: the index matrix must be int64 (P x {N}), held contiguous as ({N}, P)")
    if w is not None and w.numel() != sum(int(c.shape[2]) for c in cores):
        raise _lib.TTNError("train evaluation: the weight vectors must have the cores' lengths")
    P = 1 if idx is None else int(idx.shape[1])
    if yref is not None and yref.numel() != P:
        raise _lib.TTNError("train evaluation: the reference values must have one entry per point")
    out = torch.empty((P,), dtype=cores[0].dtype, device=cores[0].device)
    err = torch.empty((1,), dtype=torch.float64, device=cores[0].device) if yref is not None else None
    ptrs, dims, rks = _core_table(cores)
    _lib.check(_lib.lib().ttn_cross_eval(cplx, N, P, ptrs, dims, rks, None if idx is None else _p(idx), None if w is None else _p(w), _p(out),
                                         None if yref is None else _p(yref), float(tol), None if err is None else _p(err)))
    return out, err


def _up_cores(cores, dt):
    torch, _ = _dev()
    return [torch.from_numpy(np.ascontiguousarray(np.transpose(np.asarray(c, dtype=dt)))).to("cuda") for c in cores]


def _evaluate_tt(cores, indices, N):
    """_evaluate_tt(cores, indices, N) (:128-142): the train at the rows of the 1-based index matrix, by the device kernel.  Cores
    that do not chain, an index matrix of the wrong width or an index outside 1..n_k raise TTNError (the reference's
    DimensionMismatch / BoundsError) before anything is launched."""
    torch, stream = _dev()
    cores = [np.asarray(c) for c in cores]
    if len(cores) != N:
        raise _lib.TTNError(f"_evaluate_tt: {len(cores)} cores for N = {N}")
    _check_train([c.shape for c in cores], "_evaluate_tt")
    ind = np.asarray(indices, dtype=np.int64)
    if ind.ndim != 2 or ind.shape[1] != N or ind.shape[0] < 1:
        raise _lib.TTNError(f"_evaluate_tt: the index matrix must be P x {N}, got shape {ind.shape}")
    hi = np.array([c.shape[0] for c in cores])
    if np.any(ind < 1) or np.any(ind > hi):
        raise _lib.TTNError("_evaluate_tt: BoundsError: an index lies outside 1..n_k")
    cplx = any(np.iscomplexobj(c) for c in cores)
    dt = np.complex128 if cplx else np.float64
    with torch.cuda.stream(stream):
        ct = _up_cores(cores, dt)
        it = torch.from_numpy(np.ascontiguousarray(ind.T)).to("cuda")
        out, _ = _d_eval(ct, idx=it)
        return out.cpu().numpy()


def _contract_with_weights(cores, weights):
    """_contract_with_weights(cores, weights) (:686-693) by the device kernel; the running row is conjugated before each factor, as
    `result' * contracted` does.  Cores that do not chain or a weight vector of the wrong length raise TTNError."""
    torch, stream = _dev()
    cores = [np.asarray(c) for c in cores]
    weights = [np.asarray(w).reshape(-1) for w in weights]
    _check_train([c.shape for c in cores], "_contract_with_weights")
    if len(weights) != len(cores) or any(len(w) != c.shape[0] for w, c in zip(weights, cores)):
        raise _lib.TTNError("_contract_with_weights: DimensionMismatch: one weight vector of length n_k per core")
    cplx = any(np.iscomplexobj(c) for c in cores) or any(np.iscomplexobj(w) for w in weights)
    dt = np.complex128 if cplx else np.float64
    with torch.cuda.stream(stream):
        ct = _up_cores(cores, dt)
        wt = torch.from_numpy(np.concatenate([np.asarray(w, dtype=dt) for w in weights])).to("cuda")
        out, _ = _d_eval(ct, w=wt)
        v = out.cpu().numpy()[0]
    return complex(v) if cplx else float(v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------------------------
class _Problem:
    """f, its domain on the device, the steps that called f (for error messages) and the device word that records the first call
    with a non-finite value."""

    def __init__(self, f, domain):
        torch, _ = _dev()
        self.f = f
        self.N = len(domain)
        self.Is = [None] + [len(d) for d in domain]
        self.dcplx = any(np.iscomplexobj(d) for d in domain)
        ddt = np.complex128 if self.dcplx else np.float64
        self.dom = torch.from_numpy(np.concatenate([np.asarray(d, dtype=ddt).reshape(-1) for d in domain])).to("cuda")
        self.doff = torch.tensor([0] + list(np.cumsum([len(d) for d in domain])), dtype=torch.int64, device="cuda")
        self.bad = torch.zeros((1,), dtype=torch.int64, device="cuda")
        self.steps = []
        self.vdt = None

    def points(self, mode, site=1, n1=1, n2=1, L=None, R=None, idx=None, want_idx=False):
        """coordinates (N, P) of a fibre (mode 0) / superblock (mode 1) / index matrix idx given as (N, P) (mode 2)"""
        torch, _ = _dev()
        N = self.N
        rl = 1 if L is None or L.shape[0] == 0 else int(L.shape[1])
        rr = 1 if R is None or R.shape[0] == 0 else int(R.shape[1])
        if mode == 0:
            P = rl * n1 * rr
        elif mode == 1:
            P = rl * n1 * n2 * rr
        else:
            P = int(idx.shape[1])
        X = torch.empty((N, P), dtype=self.dom.dtype, device="cuda")
        iout = torch.empty((N, P), dtype=torch.int64, device="cuda") if want_idx else None
        Lp = None if L is None or L.shape[0] == 0 else _p(L)
        Rp = None if R is None or R.shape[0] == 0 else _p(R)
        _lib.check(_lib.lib().ttn_cross_points(1 if self.dcplx else 0, mode, N, site, n1, n2, rl, rr, Lp, Rp,
                                               None if idx is None else _p(idx), P, _p(self.doff), _p(self.dom),
                                               None if iout is None else _p(iout), _p(X)))
        return (X, iout) if want_idx else X

    def call(self, X, step):
        """f at the coordinate rows of X (N, P): P values on the device, in the value type of the probe"""
        torch, _ = _dev()
        P = X.shape[1]
        y = self.f(X.T)
        if isinstance(y, torch.Tensor):
            y = y.to("cuda")
        else:
            y = torch.from_numpy(np.array(y)).to("cuda")
        y = y.reshape(-1)
        if y.numel() != P:
            raise _lib.TTNError(f"tt_cross: f returned {y.numel()} values for {P} points ({step})")
        if self.vdt is None:
            self.vdt = torch.complex128 if y.is_complex() else torch.float64
        elif y.is_complex() and self.vdt == torch.float64:
            raise _lib.TTNError(f"tt_cross: f returned complex values where the probe was real ({step})")
        y = y.to(self.vdt).contiguous()
        self.steps.append(step)
        fin = torch.isfinite(y).all() if P else torch.ones((), dtype=torch.bool, device="cuda")
        self.bad.copy_(torch.where((self.bad == 0) & ~fin, torch.full_like(self.bad, len(self.steps)), self.bad))
        return y

    def probe(self):
        """_infer_value_type (:183-187): f at index (1, ..., 1)"""
        torch, _ = _dev()
        ones = torch.ones((self.N, 1), dtype=torch.int64, device="cuda")
        self.call(self.points(2, idx=ones), "the value-type probe at index (1, ..., 1)")

    def check(self, words):
        """the host read: [bad, maxvol status words ...] as floats; raises on a non-finite value or a singular maxvol"""
        bad = int(words[0])
        if bad:
            raise _lib.TTNError(f"tt_cross: f returned a non-finite value ({self.steps[bad - 1]})")
        if any(int(s) != 0 for s in words[1:]):
            raise _lib.TTNError("tt_cross: maxvol met a zero pivot (a fibre matrix has rank below its size)")


def _validation(pb, seed, val_size):
    torch, _ = _dev()
    Xs = draw_indices(seed, DRAW_VALIDATION, 0, 0, val_size, pb.Is[1:])
    it = torch.from_numpy(np.ascontiguousarray(Xs.T)).to("cuda")
    ys = pb.call(pb.points(2, idx=it), "the validation points")
    return Xs, it, ys


def _dev_set(a):
    """host index matrix (rows x cols) -> device (cols, rows)"""
    torch, _ = _dev()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64).T)).to("cuda")


def _empty_set():
    torch, _ = _dev()
    return torch.zeros((0, 1), dtype=torch.int64, device="cuda")


def _rows(S, n):
    """the first n rows of a device set (cols, rows)"""
    return S if S.shape[1] == n else S[:, :n].contiguous()


_LAST = {}      # diagnostics of the last run (tests, tools/diag_cross.py): per-sweep errors, final index sets, timing split


class _Timer:
    """event pairs around the parts of a half sweep (tools/diag_cross.py); inactive unless _Timer.on"""
    on = False

    def __init__(self):
        self.events = []

    def mark(self, name):
        if not _Timer.on:
            return
        torch, _ = _dev()
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.events.append((name, e))

    def split(self):
        out = {}
        for (name, e0), (_, e1) in zip(self.events, self.events[1:]):
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def _maxvol_cross(pb, alg, ranks, val_size, seed):
    """tt_cross(f, domain, ::MaxVol) (:189-317), statement for statement; 1-based lists"""
    torch, _ = _dev()
    N, Is = pb.N, pb.Is
    Rs = [None, 1] + ([int(ranks)] * (N - 1) if isinstance(ranks, (int, np.integer)) else [int(r) for r in ranks]) + [1]
    if len(Rs) != N + 2:
        raise _lib.TTNError(f"tt_cross: ranks needs N - 1 = {N - 1} entries")
    _cap_ranks_(Rs, Is, alg.rmax)
    cores = [None] * (N + 1)
    lsets, rsets = [None] * (N + 1), [None] * (N + 1)
    lsets[1], rsets[N] = _empty_set(), _empty_set()
    max_R = max(Rs[1:])
    randint = draw_indices(seed, DRAW_MAXVOL_RSETS, 0, 0, max_R, Is[1:])
    for n in range(1, N):
        rsets[n] = _dev_set(randint[: Rs[n + 1], n:])
    Xs_val, it_val, ys_val = _validation(pb, seed, val_size)
    if alg.verbose:
        log.info("MaxVol cross-interpolation over %dD domain with %d grid points", N, int(np.prod(Is[1:], dtype=np.float64)))
    converged, val_eps, hist = False, math.inf, []
    tm = _Timer()
    info = torch.zeros((max(2 * (N - 1), 1), 2), dtype=torch.int64, device="cuda")

    def fibre(j, step):
        tm.mark("gathers")
        X = pb.points(0, j, Is[j], 1, None if j == 1 else _rows(lsets[j], Rs[j]), None if j == N else _rows(rsets[j], Rs[j + 1]))
        tm.mark("f")
        V = pb.call(X, step)
        return V

    for it in range(1, alg.maxiter + 1):
        for j in range(1, N):
            V = fibre(j, f"iteration {it}, left-to-right, site {j}")
            tm.mark("qr")
            Qt, _ = _qr_j(V.reshape(Rs[j + 1], Rs[j] * Is[j]) * _pow2_scale(V))
            tm.mark("maxvol")
            piv, Gt = _d_maxvol(Qt, alg.pivot.tol, alg.pivot.maxiter, info[j - 1])
            tm.mark("gathers")
            r = Gt.shape[0]
            cores[j] = Gt.reshape(r, Rs[j], Is[j])
            local_i = (piv - 1) % Is[j] + 1
            local_r = (piv - 1) // Is[j]
            if j == 1:
                lsets[j + 1] = local_i.reshape(1, r).contiguous()
            else:
                lsets[j + 1] = torch.cat([_rows(lsets[j], Rs[j])[:, local_r], local_i.reshape(1, r)], 0).contiguous()
            Rs[j + 1] = r
        for j in range(N, 1, -1):
            V = fibre(j, f"iteration {it}, right-to-left, site {j}")
            tm.mark("qr")
            Wt = V.reshape(Rs[j + 1], Rs[j], Is[j]).permute(0, 2, 1).reshape(Rs[j + 1] * Is[j], Rs[j])
            Qt, _ = _qr_j(_own(Wt.transpose(0, 1)) * _pow2_scale(V))                      # qr(transpose(V_right))
            tm.mark("maxvol")
            piv, Gt = _d_maxvol(Qt, alg.pivot.tol, alg.pivot.maxiter, info[N - 2 + j - 1])
            tm.mark("gathers")
            r = Gt.shape[0]
            cores[j] = _own(Gt.reshape(r, Rs[j + 1], Is[j]).permute(1, 0, 2))             # permutedims(G_3d, (1, 3, 2))
            local_i = (piv - 1) % Is[j] + 1
            local_r = (piv - 1) // Is[j]
            if j == N:
                rsets[j - 1] = local_i.reshape(1, r).contiguous()
            else:
                rsets[j - 1] = torch.cat([local_i.reshape(1, r), _rows(rsets[j], Rs[j + 1])[:, local_r]], 0).contiguous()
            Rs[j] = r
        V = fibre(1, f"iteration {it}, site 1")
        cores[1] = V.reshape(Rs[2], Rs[1], Is[1])
        tm.mark("evaluation")
        _, err = _d_eval(cores[1:], idx=it_val, yref=ys_val, tol=alg.tol)
        words = torch.cat([err, pb.bad.to(torch.float64), info[:, 0].to(torch.float64)]).tolist()     # the sweep's one host read
        tm.mark("end")
        pb.check(words[1:])
        val_eps = words[0]
        hist.append(val_eps)
        if alg.verbose:
            log.info("Iteration %d: ε = %s, max rank = %d", it, val_eps, max(Rs[1:]))
        if val_eps < alg.tol:
            converged = True
            break
        if alg.kickrank is not None:
            newRs = list(Rs)
            for n in range(2, N + 1):
                newRs[n] = min(newRs[n] + alg.kickrank, alg.rmax)
            _cap_ranks_(newRs, Is, alg.rmax)
            for n in range(1, N):
                if newRs[n + 1] > Rs[n + 1]:
                    extra = draw_indices(seed, DRAW_KICK, it, n, newRs[n + 1] - Rs[n + 1], Is[n + 1:])
                    rsets[n] = torch.cat([_rows(rsets[n], Rs[n + 1]), _dev_set(extra)], 1).contiguous()
            Rs = newRs
    if converged and alg.verbose:
        log.info("Converged: ε = %s < %s", val_eps, alg.tol)
    if not converged and alg.verbose:
        log.warning("Max iterations reached: ε = %s", val_eps)
    _LAST.clear()
    _LAST.update(alg="MaxVol", eps=hist, sweeps=len(hist), split=tm.split(),
                 lsets=[None, None] + [_host_set(lsets[k]) for k in range(2, N + 1)],
                 rsets=[None] + [_host_set(rsets[k]) for k in range(1, N)] + [None])
    return _finish(cores, N, Is)


def _host_set(S):
    return np.ascontiguousarray(S.cpu().numpy().T)


def _finish(cores, N, Is):
    host = [np.asfortranarray(np.transpose(c.cpu().numpy())) for c in cores[1:]]
    rks = [1] + [int(c.shape[2]) for c in host]
    return TTvector(N, host, tuple(Is[1:]), rks, [0] * N)


def _combine_left(I_l_k, s1, I_idx):
    """_combine_indices_left(I_l[k], s1)[I_idx, :] on the device (rows: r_l fastest, then i)"""
    torch, _ = _dev()
    r_l = 1 if I_l_k.shape[0] == 0 else I_l_k.shape[1]
    row = I_idx - 1
    i = (row // r_l + 1).reshape(1, -1)
    if I_l_k.shape[0] == 0:
        return i.contiguous()
    return torch.cat([I_l_k[:, row % r_l], i], 0).contiguous()


def _combine_right(s2, I_g_k, I_idx):
    """_combine_indices_right(s2, I_g[k+1])[I_idx, :] on the device (rows: i fastest, then r_g)"""
    torch, _ = _dev()
    row = I_idx - 1
    i = (row % s2 + 1).reshape(1, -1)
    if I_g_k.shape[0] == 0:
        return i.contiguous()
    return torch.cat([i, I_g_k[:, row // s2]], 0).contiguous()


def _dmrg_cross(pb, alg, ranks, val_size, seed):
    """tt_cross(f, domain, ::DMRG) (:562-658), statement for statement; 1-based lists"""
    torch, _ = _dev()
    N, Is = pb.N, pb.Is
    if N == 1:
        X = pb.points(0, 1, Is[1], 1)
        vals = pb.call(X, "the one-site shortcut")
        words = pb.bad.to(torch.float64).tolist()
        pb.check(words)
        _LAST.clear()
        _LAST.update(alg="DMRG", eps=[], sweeps=0, split={})
        return _finish([None, vals.reshape(1, 1, Is[1])], 1, Is)
    Rs = [None, 1] + ([int(ranks)] * (N - 1) if isinstance(ranks, (int, np.integer)) else [int(r) for r in ranks]) + [1]
    if len(Rs) != N + 2:
        raise _lib.TTNError(f"tt_cross: ranks needs N - 1 = {N - 1} entries")
    _cap_ranks_(Rs, Is, alg.rmax)
    I_l, I_g = [None] * (N + 1), [None] * (N + 1)
    I_l[1], I_g[N] = _empty_set(), _empty_set()
    for k in range(2, N + 1):
        I_l[k] = _dev_set(draw_indices(seed, DRAW_DMRG_LEFT, k, 0, Rs[k], Is[1:k]))
    for k in range(1, N):
        I_g[k] = _dev_set(draw_indices(seed, DRAW_DMRG_RIGHT, k, 0, Rs[k + 1], Is[k + 1:]))
    cores = [None] * (N + 1)
    Xs_val, it_val, ys_val = _validation(pb, seed, val_size)
    if alg.verbose:
        log.info("DMRG cross-interpolation over %dD domain with %d grid points", N, int(np.prod(Is[1:], dtype=np.float64)))
    converged, val_eps, hist = False, math.inf, []
    tm = _Timer()
    infos = []                  # status words of the maxvol calls since the last host read

    def superblock(k, step):
        tm.mark("gathers")
        X = pb.points(1, k, Is[k], Is[k + 1], None if k == 1 else I_l[k], None if k + 1 == N else I_g[k + 1])
        tm.mark("f")
        V = pb.call(X, step)
        r_l = 1 if I_l[k].shape[0] == 0 else I_l[k].shape[1]
        r_g = 1 if I_g[k + 1].shape[0] == 0 else I_g[k + 1].shape[1]
        tm.mark("svd")
        sc = _pow2_scale(V)
        Ut, sd, Vtt = _svd_j(V.reshape(Is[k + 1] * r_g, r_l * Is[k]) * sc)
        sd = sd / sc
        words = torch.cat([sd, pb.bad.to(torch.float64)] + [i[0:1].to(torch.float64) for i in infos]).tolist()   # s for the rank
        pb.check(words[len(sd):])
        infos.clear()                                     # (read and found zero: only the maxvol calls after this read are pending)
        r = _svd_rank(words[: len(sd)], alg.rmax, alg.tol)
        s = sd[:r].to(V.dtype)
        return r_l, r_g, r, Ut[:r, :], s, Vtt[:, :r]

    def validate(name):
        tm.mark("evaluation")
        _, err = _d_eval(cores[1:], idx=it_val, yref=ys_val, tol=alg.tol)
        words = torch.cat([err, pb.bad.to(torch.float64)] + [i[0:1].to(torch.float64) for i in infos]).tolist()
        tm.mark("end")
        pb.check(words[1:])
        infos.clear()
        hist.append(words[0])
        if alg.verbose:
            log.info("Sweep %s: ε = %s, max rank = %d", name, words[0], max(Rs[1:]))
        return words[0]

    def mv(Qt):
        info = torch.zeros((2,), dtype=torch.int64, device="cuda")
        infos.append(info)
        tm.mark("maxvol")
        out = _d_maxvol(Qt, alg.pivot.tol, alg.pivot.maxiter, info)
        tm.mark("gathers")
        return out

    for it in range(1, alg.maxiter + 1):
        for k in range(1, N):
            r_l, r_g, r, U, s, Vt = superblock(k, f"sweep {2 * it - 1} (left-to-right), sites {k}, {k + 1}")
            s1, s2 = Is[k], Is[k + 1]
            if k < N - 1:
                tm.mark("qr")
                Qt, _ = _qr_j(_own(U))
                I_idx, Gt = mv(Qt)
                I_l[k + 1] = _combine_left(I_l[k], s1, I_idx)
                Rs[k + 1] = int(I_idx.shape[0])
                cores[k] = _own(Gt.reshape(Rs[k + 1], s1, r_l).permute(0, 2, 1))
            else:
                cores[k] = _own(U.reshape(r, s1, r_l).permute(0, 2, 1))
                cores[k + 1] = _own((Vt * s.reshape(1, r)).reshape(r_g, s2, r).permute(0, 2, 1))
                Rs[k + 1] = r
        val_eps = validate(f"{2 * it - 1} (L→R)")
        if val_eps < alg.tol:
            converged = True
            break
        for k in range(N - 1, 0, -1):
            r_l, r_g, r, U, s, Vt = superblock(k, f"sweep {2 * it} (right-to-left), sites {k}, {k + 1}")
            s1, s2 = Is[k], Is[k + 1]
            if k > 1:
                tm.mark("qr")
                Qt, _ = _qr_j(_own(Vt.transpose(0, 1).conj()))                             # qr(Vt')
                I_idx, Gt = mv(Qt)
                I_g[k] = _combine_right(s2, I_g[k + 1], I_idx)
                Rs[k + 1] = int(I_idx.shape[0])
                cores[k + 1] = _own(Gt.transpose(0, 1).conj().reshape(r_g, s2, Rs[k + 1]).permute(0, 2, 1))
            else:
                cores[k] = _own((U * s.reshape(r, 1)).reshape(r, s1, r_l).permute(0, 2, 1))
                cores[k + 1] = _own(Vt.reshape(r_g, s2, r).permute(0, 2, 1))
                Rs[k + 1] = r
        val_eps = validate(f"{2 * it} (R→L)")
        if val_eps < alg.tol:
            converged = True
            break
    if converged and alg.verbose:
        log.info("Converged: ε = %s < %s", val_eps, alg.tol)
    if not converged and alg.verbose:
        log.warning("Max iterations reached: ε = %s", val_eps)
    _LAST.clear()
    _LAST.update(alg="DMRG", eps=hist, sweeps=len(hist), split=tm.split(),
                 I_l=[None, None] + [_host_set(I_l[k]) for k in range(2, N + 1)],
                 I_g=[None] + [_host_set(I_g[k]) for k in range(1, N)] + [None])
    return _finish(cores, N, Is)


def _domain(domain):
    if isinstance(domain, (tuple, list)) and len(domain) > 0 and all(isinstance(d, (int, np.integer)) for d in domain):
        return [np.arange(1.0, float(d) + 1.0) for d in domain]            # 1.0:n per axis (:96-104)
    dom = [np.asarray(d) for d in domain]
    if not dom or any(d.ndim != 1 or d.size == 0 for d in dom):
        raise _lib.TTNError("tt_cross: domain must be a non-empty list of non-empty 1-D arrays, or a tuple / list of ints")
    cplx = any(np.iscomplexobj(d) for d in dom)
    return [d.astype(np.complex128 if cplx else np.float64) for d in dom]


def tt_cross(f, domain, alg=None, ranks=2, val_size: int = 1000, seed: int = 0) -> TTvector:
    """tt_cross(f, domain, alg = MaxVol(); ranks = 2, val_size = 1000) (:92-104, :189, :562) on the device; `seed` names the random
    draws (see draw_indices).  Returns a host TTvector (ttv_ot all zeros; complex128 cores when f's values are complex)."""
    alg = MaxVol() if alg is None else alg
    if isinstance(alg, Greedy):
        raise _lib.TTNError("tt_cross: the Greedy algorithm is not offered by this port (use MaxVol or DMRG)")
    if not isinstance(alg, (MaxVol, DMRG)):
        raise _lib.TTNError(f"tt_cross: unknown algorithm {type(alg).__name__}")
    if not isinstance(alg.pivot, MaxVolPivot):
        raise _lib.TTNError(f"tt_cross: {type(alg).__name__} needs a MaxVolPivot (a {type(alg.pivot).__name__} has no tol)")
    dom = _domain(domain)
    torch, stream = _dev()
    with torch.cuda.stream(stream):
        pb = _Problem(f, dom)
        pb.probe()
        if isinstance(alg, MaxVol):
            return _maxvol_cross(pb, alg, ranks, int(val_size), seed)
        return _dmrg_cross(pb, alg, ranks, int(val_size), seed)


def tt_integrate(f, *args, alg=None, nquad: int = 20, lower=0.0, upper=1.0, **kw):
    """tt_integrate(f, lower, upper; alg, nquad, kwargs...) and tt_integrate(f, d; lower = 0.0, upper = 1.0, kwargs...) (:660-684):
    Gauss-Legendre nodes per axis (host), tt_cross on them, the train contracted with the weights on the device."""
    if len(args) == 1 and isinstance(args[0], (int, np.integer)):
        d = int(args[0])
        lo, hi = [lower] * d, [upper] * d
    elif len(args) == 2:
        lo, hi = list(args[0]), list(args[1])
        if len(lo) != len(hi):
            raise AssertionError("lower and upper bounds must have the same length")
    else:
        raise TypeError("tt_integrate(f, lower, upper; ...) or tt_integrate(f, d; lower, upper, ...)")
    nodes, weights = [], []
    for a, b in zip(lo, hi):
        x, w = _gauss_legendre(int(nquad), a, b)
        nodes.append(x)
        weights.append(w)
    tt = tt_cross(f, nodes, alg, **kw)
    return _contract_with_weights(tt.ttv_vec, weights)


# ---------------------------------------------------------------------------------------------------------------------------------
# a batch of functions in one MaxVol cross (csrc/ttn_cross_batch_kernels.h, include/ttn_cross_batch.h)
# ---------------------------------------------------------------------------------------------------------------------------------
# MaxVol's ranks do not depend on the data (r = Rs[j+1] after every site, a kick adds a fixed amount), so every function still running
# has the shapes of every other: a per-function array is one torch tensor with the function axis in front, a Julia (rows x cols) set
# of A functions is (A, cols, rows), a core (n, r_left, r_right) is (A, r_right, r_left, n).
class _BatchProblem:
    """f(X, which), its domain on the device, the steps that called f and, per running function, the first step with a non-finite
    value."""

    def __init__(self, f, domain, batch):
        torch, _ = _dev()
        self.f = f
        self.N = len(domain)
        self.Is = [None] + [len(d) for d in domain]
        self.dom = torch.from_numpy(np.concatenate([np.asarray(d, dtype=np.float64).reshape(-1) for d in domain])).to("cuda")
        self.doff = torch.tensor([0] + list(np.cumsum([len(d) for d in domain])), dtype=torch.int64, device="cuda")
        self.which = torch.arange(batch, dtype=torch.int64, device="cuda")
        self.ids = list(range(batch))                       # the host copy of `which`
        self.bad = torch.zeros((batch,), dtype=torch.int64, device="cuda")
        self.steps = []

    @property
    def A(self):
        return len(self.ids)

    def keep(self, rows, rows_dev):
        """compaction: only the functions at the positions `rows` go on"""
        self.ids = [self.ids[a] for a in rows]
        self.which = self.which[rows_dev].contiguous()
        self.bad = self.bad[rows_dev].contiguous()

    def fibre_points(self, j, n, rl, rr, L, R):
        torch, _ = _dev()
        P = rl * n * rr
        X = torch.empty((self.A, self.N, P), dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib().ttn_cross_batch_points(0, self.A, self.N, j, n, rl, rr, None if L is None else _p(L), None if R is None else _p(R),
                                                     None, P, _p(self.doff), _p(self.dom), None, _p(X)))
        return X

    def shared_points(self, idx):
        """coordinates (A, N, P) of the index matrix idx, held as (N, P), for every running function"""
        torch, _ = _dev()
        P = int(idx.shape[1])
        X = torch.empty((self.A, self.N, P), dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib().ttn_cross_batch_points(2, self.A, self.N, 1, 1, 1, 1, None, None, _p(idx), P, _p(self.doff), _p(self.dom), None, _p(X)))
        return X

    def call(self, X, step):
        """f at the coordinate rows of X (A, N, P): (A, P) float64 values on the device"""
        torch, _ = _dev()
        A, _, P = X.shape
        y = self.f(X.transpose(1, 2), self.which)
        if isinstance(y, torch.Tensor):
            y = y.to("cuda")
        else:
            y = torch.from_numpy(np.array(y)).to("cuda")
        if y.numel() != A * P:
            raise _lib.TTNError(f"tt_cross_batch: f returned {y.numel()} values for {A} functions x {P} points ({step})")
        if y.is_complex():
            raise _lib.TTNError(f"tt_cross_batch: f returned complex values; float64 values on a real domain only ({step})")
        y = y.reshape(A, P).to(torch.float64).contiguous()
        self.steps.append(step)
        if P:
            fin = torch.isfinite(y).all(dim=1)
            self.bad.copy_(torch.where((self.bad == 0) & ~fin, torch.full_like(self.bad, len(self.steps)), self.bad))
        return y

    def probe(self):
        torch, _ = _dev()
        ones = torch.ones((self.N, 1), dtype=torch.int64, device="cuda")
        self.call(self.shared_points(ones), "the value-type probe at index (1, ..., 1)")

    def check(self, bad, status):
        """the host read's words: bad (A), status (2(N-1) x A)"""
        for a, w in enumerate(bad):
            if int(w):
                raise _lib.TTNError(f"tt_cross_batch: f returned a non-finite value for function {self.ids[a]} ({self.steps[int(w) - 1]})")
        for row in status:
            for a, w in enumerate(row):
                if int(w):
                    raise _lib.TTNError(f"tt_cross_batch: maxvol met a zero pivot for function {self.ids[a]} "
                                        "(a fibre is zero, or a fibre matrix has rank below its size)")


def _d_batch_site(direction, N, j, n, rl, rr, V, tol, maxiter, set_in, info):
    """one site step of every running function: (core, next set, pivots).  V (A, rl n rr) as f returned it; set_in (A, cols, rows) or
    None; info (A, 2) int64 receives {status, swaps}."""
    torch, _ = _dev()
    A = V.shape[0]
    r = rr if direction == 0 else rl
    nin = (j - 1) if direction == 0 else (N - j)
    core = torch.empty((A, rr, rl, n), dtype=torch.float64, device="cuda")         # Julia (n, rl, rr) in both directions
    nxt = torch.empty((A, nin + 1, r), dtype=torch.int64, device="cuda")
    piv = torch.empty((A, r), dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().ttn_cross_batch_site(A, direction, N, j, n, rl, rr, _p(V), float(tol), int(maxiter), None if set_in is None else _p(set_in),
                                               _p(nxt), _p(core), _p(piv), _p(info)))
    return core, nxt, piv


def _d_batch_eval(cores, Rs_, Is_, idx=None, w=None, yref=None, tol=0.0):
    """the A trains cores[k] (A, r_right, r_left, n) at the shared index matrix idx (N, P), or against the weights w: (out, err)"""
    torch, _ = _dev()
    N = len(cores)
    A = int(cores[0].shape[0])
    P = 1 if idx is None else int(idx.shape[1])
    out = torch.empty((A, P), dtype=torch.float64, device="cuda")
    err = torch.empty((A,), dtype=torch.float64, device="cuda") if yref is not None else None
    ptrs = (C.POINTER(C.c_double) * N)(*[C.cast(C.c_void_p(c.data_ptr()), C.POINTER(C.c_double)) for c in cores])
    dims = (C.c_int64 * N)(*[int(v) for v in Is_])
    rks = (C.c_int64 * (N + 1))(*[int(v) for v in Rs_])
    _lib.check(_lib.lib().ttn_cross_batch_eval(A, N, P, ptrs, dims, rks, None if idx is None else _p(idx), None if w is None else _p(w), _p(out),
                                               None if yref is None else _p(yref), float(tol), None if err is None else _p(err)))
    return out, err


_LAST_BATCH = {}    # diagnostics of the last batched run: per function eps and sweeps; groups; the timing split; sets through last_batch_sets


def last_batch_sets(b):
    """(lsets, rsets) of function b after the last tt_cross_batch, as host matrices in the lists' 1-based layout of _LAST"""
    for g in _LAST_BATCH["groups"]:
        if b in g["ids"]:
            a = g["ids"].index(b)
            N = len(g["cores"])
            return ([None, None] + [_host_set(g["lsets"][k][a]) for k in range(2, N + 1)],
                    [None] + [_host_set(g["rsets"][k][a]) for k in range(1, N)] + [None])
    raise KeyError(b)


def _maxvol_cross_batch(pb, alg, ranks, val_size, seed):
    """_maxvol_cross for every function of pb at once.  Returns the groups of functions that finished together: dicts with ids, Rs
    (1-based list), cores (list of N device tensors (G, r_right, r_left, n)), lsets, rsets."""
    torch, _ = _dev()
    N, Is = pb.N, pb.Is
    B = pb.A
    Rs = [None, 1] + ([int(ranks)] * (N - 1) if isinstance(ranks, (int, np.integer)) else [int(r) for r in ranks]) + [1]
    if len(Rs) != N + 2:
        raise _lib.TTNError(f"tt_cross_batch: ranks needs N - 1 = {N - 1} entries")
    _cap_ranks_(Rs, Is, alg.rmax)
    if max(Rs[1:]) > 1024 or max(r * n for r, n in zip(Rs[1:], Is[1:])) > (1 << 20):
        raise _lib.TTNError("tt_cross_batch: ranks up to 1024 and fibre matrices of up to 2^20 rows")
    cores = [None] * (N + 1)
    lsets, rsets = [None] * (N + 1), [None] * (N + 1)
    randint = draw_indices(seed, DRAW_MAXVOL_RSETS, 0, 0, max(Rs[1:]), Is[1:])
    for n in range(1, N):
        rsets[n] = _dev_set(randint[: Rs[n + 1], n:]).unsqueeze(0).expand(B, -1, -1).contiguous()
    Xs = draw_indices(seed, DRAW_VALIDATION, 0, 0, val_size, Is[1:])
    it_val = torch.from_numpy(np.ascontiguousarray(Xs.T)).to("cuda")
    ys_val = pb.call(pb.shared_points(it_val), "the validation points")
    if alg.verbose:
        log.info("MaxVol cross-interpolation of %d functions over %dD domain with %d grid points", B, N, int(np.prod(Is[1:], dtype=np.float64)))
    hist = [[] for _ in range(B)]
    groups = []
    tm = _Timer()

    def fibre(j, step):
        tm.mark("gathers")
        X = pb.fibre_points(j, Is[j], Rs[j], Rs[j + 1], None if j == 1 else lsets[j], None if j == N else rsets[j])
        tm.mark("f")
        return pb.call(X, step)

    def finish(rows, rows_dev, core_Rs):
        groups.append(dict(ids=[pb.ids[a] for a in rows], Rs=list(core_Rs), cores=[cores[k][rows_dev].contiguous() for k in range(1, N + 1)],
                           lsets=[None, None] + [lsets[k][rows_dev] for k in range(2, N + 1)],
                           rsets=[None] + [rsets[k][rows_dev] for k in range(1, N)] + [None]))

    for it in range(1, alg.maxiter + 1):
        A = pb.A
        info = torch.zeros((2 * (N - 1), A, 2), dtype=torch.int64, device="cuda")
        for j in range(1, N):
            V = fibre(j, f"iteration {it}, left-to-right, site {j}")
            tm.mark("site")
            cores[j], lsets[j + 1], _ = _d_batch_site(0, N, j, Is[j], Rs[j], Rs[j + 1], V, alg.pivot.tol, alg.pivot.maxiter,
                                                      None if j == 1 else lsets[j], info[j - 1])
        for j in range(N, 1, -1):
            V = fibre(j, f"iteration {it}, right-to-left, site {j}")
            tm.mark("site")
            cores[j], rsets[j - 1], _ = _d_batch_site(1, N, j, Is[j], Rs[j], Rs[j + 1], V, alg.pivot.tol, alg.pivot.maxiter,
                                                      None if j == N else rsets[j], info[N - 2 + j - 1])
        V = fibre(1, f"iteration {it}, site 1")
        cores[1] = V.reshape(A, Rs[2], Rs[1], Is[1])
        tm.mark("evaluation")
        _, err = _d_batch_eval(cores[1:], Rs[1:], Is[1:], idx=it_val, yref=ys_val, tol=alg.tol)
        words = torch.cat([err, pb.bad.to(torch.float64), info[:, :, 0].reshape(-1).to(torch.float64)]).tolist()   # the sweep's one host read
        tm.mark("end")
        pb.check(words[A: 2 * A], [words[2 * A + s * A: 2 * A + (s + 1) * A] for s in range(2 * (N - 1))])
        eps = words[:A]
        for a in range(A):
            hist[pb.ids[a]].append(eps[a])
        if alg.verbose:
            log.info("Iteration %d: %d functions, max ε = %s, max rank = %d", it, A, max(eps), max(Rs[1:]))
        done = [a for a in range(A) if eps[a] < alg.tol]
        rest = [a for a in range(A) if not eps[a] < alg.tol]
        if done:
            finish(done, torch.tensor(done, dtype=torch.int64, device="cuda"), Rs)
        if not rest:
            break
        if done:
            rd = torch.tensor(rest, dtype=torch.int64, device="cuda")
            pb.keep(rest, rd)
            ys_val = ys_val[rd].contiguous()
            for k in range(1, N):
                rsets[k] = rsets[k][rd].contiguous()
            if it == alg.maxiter:                           # (the next sweep would write these anew)
                cores = [None] + [c[rd] for c in cores[1:]]
                for k in range(2, N + 1):
                    lsets[k] = lsets[k][rd]
        core_Rs = list(Rs)
        if alg.kickrank is not None:
            newRs = list(Rs)
            for n in range(2, N + 1):
                newRs[n] = min(newRs[n] + alg.kickrank, alg.rmax)
            _cap_ranks_(newRs, Is, alg.rmax)
            for n in range(1, N):
                if newRs[n + 1] > Rs[n + 1]:
                    extra = _dev_set(draw_indices(seed, DRAW_KICK, it, n, newRs[n + 1] - Rs[n + 1], Is[n + 1:]))
                    rsets[n] = torch.cat([rsets[n], extra.unsqueeze(0).expand(pb.A, -1, -1)], 2).contiguous()
            Rs = newRs
        if it == alg.maxiter:                               # stopped after the kick, as _maxvol_cross: the ranks are those of the cores
            if alg.verbose:
                log.warning("Max iterations reached: functions %s, max ε = %s", pb.ids, max(eps[a] for a in rest))
            finish(list(range(pb.A)), torch.arange(pb.A, dtype=torch.int64, device="cuda"), core_Rs)
    _LAST_BATCH.clear()
    _LAST_BATCH.update(eps=hist, sweeps=[len(h) for h in hist], split=tm.split(), groups=groups)
    return groups


def _batch_checks(alg, domain, batch, who):
    alg = MaxVol() if alg is None else alg
    if isinstance(alg, (DMRG, Greedy)):
        raise _lib.TTNError(f"{who}: MaxVol only; the ranks of {type(alg).__name__} depend on the data, so a batch has no common shapes")
    if not isinstance(alg, MaxVol):
        raise _lib.TTNError(f"{who}: unknown algorithm {type(alg).__name__}")
    if not isinstance(alg.pivot, MaxVolPivot):
        raise _lib.TTNError(f"{who}: MaxVol needs a MaxVolPivot (a {type(alg.pivot).__name__} has no tol)")
    if not isinstance(batch, (int, np.integer)) or batch < 1:
        raise _lib.TTNError(f"{who}: batch must be an integer >= 1, got {batch!r}")
    if batch > 65535:
        raise _lib.TTNError(f"{who}: at most 65535 functions in one call")
    dom = _domain(domain)
    if any(np.iscomplexobj(d) for d in dom):
        raise _lib.TTNError(f"{who}: float64 values on a real domain only (the domain is complex)")
    return alg, dom


def _cross_batch_groups(f, dom, batch, alg, ranks, val_size, seed):
    pb = _BatchProblem(f, dom, int(batch))
    pb.probe()
    return _maxvol_cross_batch(pb, alg, ranks, int(val_size), seed), pb


def tt_cross_batch(f, domain, batch: int, alg=None, ranks=2, val_size: int = 1000, seed: int = 0, resident: bool = False):
    """MaxVol tt_cross of `batch` functions at once.  f(X, which): X is a float64 device tensor (A, P, N), row X[a, p, :] the p-th point
    of function which[a]; which is the int64 device tensor of the A <= batch functions still running; f returns (A, P) values.  One
    `seed` names the draws of all functions: function b sees the draws of tt_cross(f_b, ..., seed=seed) and ends with the
    index sets, ranks and sweep count of that call.  A function whose validation error falls below alg.tol is finished and is not asked of f again.  Returns
    a list of `batch` host TTvectors, or with resident=True one device.DeviceTT of that batch (capacity: the per-bond maximum of the
    final ranks, every train at its own ranks), filled on the device."""
    alg, dom = _batch_checks(alg, domain, batch, "tt_cross_batch")
    torch, stream = _dev()
    with torch.cuda.stream(stream):
        groups, pb = _cross_batch_groups(f, dom, batch, alg, ranks, val_size, seed)
        N, Is = pb.N, pb.Is
        if not resident:
            out = [None] * int(batch)
            for g in groups:
                host = [c.cpu().numpy() for c in g["cores"]]                     # one copy per site and group
                for a, b in enumerate(g["ids"]):
                    cs = [np.asfortranarray(np.transpose(h[a])) for h in host]
                    out[b] = TTvector(N, cs, tuple(Is[1:]), [1] + [int(c.shape[2]) for c in cs], [0] * N)
            return out
        from .device import DeviceTT
        cap = [max(g["Rs"][k] for g in groups) for k in range(1, N + 2)]
        tt = DeviceTT(Is[1:], cap, int(batch))
        for k in range(1, N + 1):
            buf = torch.zeros((int(batch), Is[k] * cap[k - 1] * cap[k]), dtype=torch.float64, device="cuda")
            rk2 = torch.empty((int(batch), 2), dtype=torch.int64, device="cuda")
            for g in groups:
                ids = torch.tensor(g["ids"], dtype=torch.int64, device="cuda")
                rl, rr = g["Rs"][k], g["Rs"][k + 1]
                buf[ids, : Is[k] * rl * rr] = g["cores"][k - 1].reshape(len(g["ids"]), -1)
                rk2[ids] = torch.tensor([rl, rr], dtype=torch.int64, device="cuda")
            _lib.check(_lib.lib().ttn_tt_core_import(tt.h, k, _p(buf), _p(rk2), cap[k - 1], cap[k]))
        return tt


def tt_integrate_batch(f, *args, alg=None, nquad: int = 20, lower=0.0, upper=1.0, **kw):
    """tt_integrate for `batch` functions at once — tt_integrate_batch(f, d, batch; lower, upper, ...) or tt_integrate_batch(f, lower,
    upper, batch; ...), `batch` also as a keyword: Gauss-Legendre nodes per axis, tt_cross_batch on them (f as there; ranks, val_size,
    seed pass through), every train contracted with the weights on the device.  Returns `batch` floats."""
    args = list(args)
    if "batch" in kw:
        args.append(kw.pop("batch"))
    if len(args) == 2 and isinstance(args[0], (int, np.integer)):
        d, batch = int(args[0]), args[1]
        lo, hi = [lower] * d, [upper] * d
    elif len(args) == 3:
        lo, hi, batch = list(args[0]), list(args[1]), args[2]
        if len(lo) != len(hi):
            raise AssertionError("lower and upper bounds must have the same length")
    else:
        raise TypeError("tt_integrate_batch(f, lower, upper, batch; ...) or tt_integrate_batch(f, d, batch; lower, upper, ...)")
    ranks, val_size, seed = kw.pop("ranks", 2), kw.pop("val_size", 1000), kw.pop("seed", 0)
    if kw:
        raise TypeError(f"tt_integrate_batch: unknown keywords {sorted(kw)}")
    nodes, weights = [], []
    for a, b in zip(lo, hi):
        x, w = _gauss_legendre(int(nquad), a, b)
        nodes.append(x)
        weights.append(w)
    alg, dom = _batch_checks(alg, nodes, batch, "tt_integrate_batch")
    torch, stream = _dev()
    with torch.cuda.stream(stream):
        groups, pb = _cross_batch_groups(f, dom, batch, alg, ranks, val_size, seed)
        wt = torch.from_numpy(np.concatenate([np.asarray(w, dtype=np.float64) for w in weights])).to("cuda")
        out = torch.empty((int(batch),), dtype=torch.float64, device="cuda")
        for g in groups:
            v, _ = _d_batch_eval(g["cores"], g["Rs"][1:], pb.Is[1:], w=wt)
            out[torch.tensor(g["ids"], dtype=torch.int64, device="cuda")] = v.reshape(-1)
        return out.cpu().numpy()
