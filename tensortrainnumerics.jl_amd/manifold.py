"""The fixed-rank TT manifold (include/ttn_tangent.h, csrc/ttn_tangent_kernels.h): ``ttvector_manifold`` of the reference's
Manopt extension (ext/TensorTrainNumericsManoptExt) with its methods under their names, and what the extension lacks: the orthogonal
projection onto the tangent space and a retraction that stays at the manifold's ranks.  Float64 only.

A point is held with its two gauges (``TTPoint``: x, U = orthogonalize(x, d), V = orthogonalize(x, 1)).  A tangent is an ordinary
``DeviceTT`` used as a bag of cores dC_k with the point's ranks (as in grad.py) that stands for sum_k U_1 .. U_{k-1} dC_k V_{k+1} .. V_d
with U_k^T dC_k = 0 for k < d; under that gauge condition ``cores_dot`` IS the inner product of the tensors.

    M = ttvector_manifold(x)            dims and ranks (a copy) of a DeviceTT or a host TTvector
    M.gauge(x) -> TTPoint               two orthogonalize calls
    M.project(pt, z) -> (xi, <x, z>)    xi = P_x z for a train z of any ranks (ttn_tangent_project)
    M.to_tt(pt, xi, alpha, beta)        the train alpha x + beta xi at ranks 2 r (ttn_tangent_to_tt)
    M.retract(pt, xi, t, alpha)         alpha x + t xi back at M.ranks: orthogonalize, then the bond step with the cap r_k per bond
    M.transport(pt_new, pt_old, xi)     P_{x_new} of the tangent xi at x_old
    fit_fixed_rank, rayleigh_descent    two drivers on handles

The reference surface (``representation_size``, ``zero_vector``, ``copy``, ``inner``, ``norm``, ``distance``, ``retract_project``) takes
``DeviceTT`` or host ``TTvector`` operands; ``retract_project`` is the reference's own form orthogonalize(p + t X), which grows the ranks.
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import device as _dev
from . import tt as _tt
from ._lib import TTNError
from .device import DeviceTT, DeviceTTO
from .grad import _coef, cores_dot
from .tt import TTvector

ARMIJO_C = 1.0e-4          # sufficient-decrease constant of rayleigh_descent's backtracking
MAX_HALVINGS = 40          # halvings of the step before an iteration gives up and keeps its point


@dataclass
class TTPoint:
    """A point of the manifold with its gauges: U = orthogonalize(x, d), V = orthogonalize(x, 1)."""
    x: DeviceTT
    U: DeviceTT
    V: DeviceTT

    def free(self, keep_x: bool = False) -> None:
        for h in ((self.U, self.V) if keep_x else (self.x, self.U, self.V)):
            h.free()


def _double_ranks(rks: Sequence[int]) -> List[int]:
    return [1] + [2 * int(r) for r in rks[1:-1]] + [1]


class TTManifold:
    """Trains of dims ``dims`` and TT ranks exactly ``ranks``."""

    def __init__(self, dims: Sequence[int], ranks: Sequence[int]):
        self.dims = tuple(int(v) for v in dims)
        self.ranks = [int(r) for r in ranks]
        if len(self.ranks) != len(self.dims) + 1:
            raise TTNError("ttvector_manifold: Dimensions and ranks are not compatible")
        if self.ranks != _tt.r_and_d_to_rks(self.ranks, self.dims):
            raise TTNError(f"ttvector_manifold: ranks {self.ranks} are not feasible for dims {self.dims} (no train of orthonormal cores has them)")

    # ---- the reference's surface (ext/TensorTrainNumericsManoptExt) ------------------------------------------------------------------
    def representation_size(self) -> Tuple[int, ...]:
        return self.dims

    def zero_vector(self, p):
        """The zero train with p's dims and ranks."""
        if isinstance(p, DeviceTT):
            z = DeviceTT(p.dims, p.cap, p.batch)
            _lib.check(_lib.lib().ttn_scale(0.0, p.h, z.h))
            return z
        from .constructors import zeros_tt
        return zeros_tt(p.ttv_dims, p.ttv_rks)

    def copy(self, p):
        if isinstance(p, DeviceTT):
            q = DeviceTT(p.dims, p.cap, p.batch)
            _lib.check(_lib.lib().ttn_tt_copy(q.h, p.h))
            return q
        return p.copy()

    def inner(self, p, X, Y):
        """dot(X, Y) — the extension's metric (p is not read)."""
        if isinstance(X, DeviceTT):
            return _dev.dot(X, Y)
        return float(np.real(_tt.dot(X, Y)))

    def norm(self, p, X):
        return np.sqrt(np.maximum(self.inner(p, X, X), 0.0)) if isinstance(X, DeviceTT) else float(np.sqrt(max(self.inner(p, X, X), 0.0)))

    def distance(self, p, q):
        """norm(p - q)."""
        if isinstance(p, DeviceTT):
            m = _dev.scale(-1.0, q, DeviceTT(q.dims, q.cap, q.batch))
            s = _dev.add(p, m, DeviceTT(p.dims, [a + b for a, b in zip(p.cap, q.cap)], p.batch))
            out = self.norm(p, s)
            m.free()
            s.free()
            return out
        return self.norm(p, _tt.sub(p, q))

    def retract_project(self, p, X, t: float = 1.0):
        """orthogonalize(p + t X) with X a TRAIN: the reference's retraction, ranks r_p + r_X, left exactly as the reference has it."""
        if isinstance(p, DeviceTT):
            tX = _dev.scale(float(t), X, DeviceTT(X.dims, X.cap, X.batch))
            s = _dev.add(p, tX, DeviceTT(p.dims, [a + b for a, b in zip(p.cap, X.cap)], p.batch))
            q = _dev.orthogonalize(s, 1, DeviceTT(s.dims, s.cap, s.batch))
            tX.free()
            s.free()
            return q
        return _tt.orthogonalize(_tt.add(p, _tt.scale(float(t), X)))

    # ---- the fixed-rank surface -------------------------------------------------------------------------------------------------------
    def _check(self, x: DeviceTT, who: str) -> None:
        if not isinstance(x, DeviceTT):
            raise TypeError(f"{who}: expected a DeviceTT, got {type(x).__name__}")
        if x.dtype is np.complex128:
            raise TTNError(f"{who}: Float64 only, a ComplexF64 handle is not supported")
        if tuple(x.dims) != self.dims:
            raise TTNError(f"{who}: dims {tuple(x.dims)} are not the manifold's {self.dims}")

    def gauge(self, x: DeviceTT) -> TTPoint:
        """x with U = orthogonalize(x, d) and V = orthogonalize(x, 1).  Reads the ranks of U back once: a point whose ranks are not the
        manifold's is refused."""
        self._check(x, "TTManifold.gauge")
        d = len(self.dims)
        U = _dev.orthogonalize(x, d, DeviceTT(self.dims, self.ranks, x.batch))
        V = _dev.orthogonalize(x, 1, DeviceTT(self.dims, self.ranks, x.batch))
        got = U.max_ranks()
        if got != self.ranks:
            U.free()
            V.free()
            raise TTNError(f"TTManifold.gauge: the point has ranks {got}, the manifold {self.ranks}")
        return TTPoint(x, U, V)

    def project(self, pt: TTPoint, z: DeviceTT, xi: Optional[DeviceTT] = None, want_value: bool = True):
        """(xi, <x_b, z_b> or None): xi = P_x z.  Without the value the call is asynchronous."""
        self._check(z, "TTManifold.project")
        if xi is None:
            xi = DeviceTT(self.dims, self.ranks, z.batch)
        out = (C.c_double * z.batch)() if want_value else None
        _lib.check(_lib.lib().ttn_tangent_project(pt.U.h, pt.V.h, z.h, xi.h, out))
        return xi, (np.array(out[:]) if want_value else None)

    def to_tt(self, pt: TTPoint, xi: DeviceTT, alpha=1.0, beta=1.0, y: Optional[DeviceTT] = None) -> DeviceTT:
        """The train alpha x + beta xi at ranks 2 r (alpha, beta: a scalar or one value per train)."""
        self._check(xi, "TTManifold.to_tt")
        if y is None:
            y = DeviceTT(self.dims, _double_ranks(self.ranks), xi.batch)
        _lib.check(_lib.lib().ttn_tangent_to_tt(pt.U.h, pt.V.h, xi.h, _coef(alpha, xi.batch), _coef(beta, xi.batch), y.h))
        return y

    def retract(self, pt: TTPoint, xi: DeviceTT, t=1.0, alpha=1.0) -> DeviceTT:
        """alpha x + t xi back at the manifold's ranks: to_tt, orthogonalize(., d), then ttn_bond_truncate with the cap r_k and no
        tolerance for k = d - 1 .. 1 — the reference's own bond step."""
        d = len(self.dims)
        y = self.to_tt(pt, xi, alpha, t)
        q = _dev.orthogonalize(y, d, DeviceTT(self.dims, _double_ranks(self.ranks), y.batch))
        y.free()
        for k in range(d - 1, 0, -1):
            _lib.check(_lib.lib().ttn_bond_truncate(q.h, k, self.ranks[k], 0.0))
        return q

    def transport(self, pt_new: TTPoint, pt_old: TTPoint, xi_old: DeviceTT) -> DeviceTT:
        """The tangent xi_old at pt_old projected onto the tangent space at pt_new."""
        y = self.to_tt(pt_old, xi_old, alpha=0.0)
        xi, _ = self.project(pt_new, y, want_value=False)
        y.free()
        return xi

    @staticmethod
    def tangent_inner(xi: DeviceTT, eta: DeviceTT) -> np.ndarray:
        """<xi, eta> of two tangents at the same point: sum_k <dC_k, dD_k> (``cores_dot``)."""
        return cores_dot(xi, eta)


def ttvector_manifold(x) -> TTManifold:
    """The manifold of trains with x's dims and ranks (x: a DeviceTT or a host TTvector).  The ranks of every train of a batch are read
    once; they must agree between the trains and be feasible (ranks == r_and_d_to_rks(ranks, dims))."""
    if isinstance(x, DeviceTT):
        if x.dtype is np.complex128:
            raise TTNError("ttvector_manifold: Float64 only, a ComplexF64 handle is not supported")
        rks = [x.ranks(b)[0] for b in range(x.batch)]
        if any(r != rks[0] for r in rks):
            raise TTNError("ttvector_manifold: the trains of the batch differ in their ranks")
        return TTManifold(x.dims, rks[0])
    if not hasattr(x, "ttv_rks"):
        raise TypeError(f"ttvector_manifold: expected a DeviceTT or a TTvector, got {type(x).__name__}")
    return TTManifold(x.ttv_dims, list(x.ttv_rks))


# ---- host trains: one upload, the calls, one download -----------------------------------------------------------------------------------
def tangent_project(x: TTvector, z: TTvector) -> Tuple[List[np.ndarray], float]:
    """(cores of P_x z, <x, z>) in the gauges U = orthogonalize(x, d), V = orthogonalize(x, 1)."""
    M = ttvector_manifold(x)
    xd, zd = DeviceTT.from_host(x), DeviceTT.from_host(z)
    pt = M.gauge(xd)
    xi, val = M.project(pt, zd)
    cores = xi.download(0).ttv_vec
    for h in (xi, zd):
        h.free()
    pt.free()
    return cores, float(val[0])


def retract(x: TTvector, cores: Sequence[np.ndarray], t: float = 1.0, alpha: float = 1.0) -> TTvector:
    """alpha x + t xi at x's ranks for the tangent with cores ``cores`` (in the gauges of ``tangent_project``)."""
    M = ttvector_manifold(x)
    xd = DeviceTT.from_host(x)
    pt = M.gauge(xd)
    xi = DeviceTT.from_host(TTvector(x.N, [np.asfortranarray(c) for c in cores], x.ttv_dims, list(x.ttv_rks), [0] * x.N))
    q = M.retract(pt, xi, t, alpha)
    out = q.download(0)
    for h in (xi, q):
        h.free()
    pt.free()
    return out


# ---- drivers on handles -----------------------------------------------------------------------------------------------------------------
def fit_fixed_rank(target: DeviceTT, x0: DeviceTT, iters: int) -> Tuple[DeviceTT, List[np.ndarray]]:
    """The projected fixed point x <- retract(P_x target) (alpha = 0) at the ranks of x0.  Returns (x, [||x - target|| / ||target|| per
    train after every iteration]); x0 is left as it is."""
    M = ttvector_manifold(x0)
    tt = _dev.dot(target, target)
    x, errs = x0, []
    for _ in range(int(iters)):
        pt = M.gauge(x)
        xi, _ = M.project(pt, target, want_value=False)
        xn = M.retract(pt, xi, 1.0, 0.0)
        xi.free()
        pt.free(keep_x=x is x0)
        x = xn
        errs.append(np.sqrt(np.maximum(_dev.dot(x, x) - 2.0 * _dev.dot(x, target) + tt, 0.0)) / np.sqrt(tt))
    return x, errs


def _normalised(y: DeviceTT) -> DeviceTT:
    """y / ||y|| per train, in place."""
    return _dev.scale_batch(1.0 / _dev.norm(y), y, y)


def rayleigh_descent(A: DeviceTTO, x0: DeviceTT, iters: int, step: float, backtrack: bool = True) -> Tuple[DeviceTT, List[np.ndarray]]:
    """Riemannian steepest descent of <x, A x> / <x, x> at the ranks of x0.  Per iteration: z = A x, xi = P_x z, rho = <x, z> / <x, x>;
    the Riemannian gradient is 2 (xi - rho x) / <x, x>, so x - t grad = (1 + 2 t rho / <x, x>) x - (2 t / <x, x>) xi is ONE to_tt,
    retracted and normalised.  With ``backtrack`` the step of a train is halved until E(new) <= E - c t ||grad||^2 with
    ||grad||^2 = 4 (<xi, xi> - rho^2 <x, x>) / <x, x>^2 (at most MAX_HALVINGS times; then that train keeps its point) and the energies
    are the accepted ones, from ``device.rayleigh``.  Returns (x, energies: the start, then one array per iteration)."""
    M = ttvector_manifold(x0)
    B = x0.batch
    t = np.full(B, float(step))
    x = x0
    energies = [_dev.rayleigh(A, x)] if backtrack else []
    zcap = [R * r for R, r in zip(A.rks, M.ranks)]
    for _ in range(int(iters)):
        pt = M.gauge(x)
        z = _dev.apply(A, x, DeviceTT(M.dims, zcap, B))
        xi, xz = M.project(pt, z)
        z.free()
        nn = _dev.dot(x, x)
        rho = xz / nn
        if not backtrack:
            energies.append(rho)
            y = M.retract(pt, xi, -2.0 * t / nn, 1.0 + 2.0 * t * rho / nn)
        else:
            E = energies[-1]
            g2 = 4.0 * (cores_dot(xi, xi) - rho * rho * nn) / (nn * nn)
            todo = np.ones(B, dtype=bool)
            Enew = E.copy()
            y = None
            for _h in range(MAX_HALVINGS):
                # a train accepted in an earlier round keeps its step and its energy: its retraction is recomputed with the same numbers
                cand = M.retract(pt, xi, -2.0 * t / nn, 1.0 + 2.0 * t * rho / nn)
                Etry = _dev.rayleigh(A, cand)
                ok = todo & (Etry <= E - ARMIJO_C * t * g2)
                if y is not None:
                    y.free()
                y = cand
                Enew = np.where(ok, Etry, Enew)
                todo = todo & ~ok
                if not todo.any():
                    break
                t = np.where(todo, t / 2, t)
            if todo.any():                               # those trains keep their point: alpha = 1, t = 0
                y.free()
                tb = np.where(todo, 0.0, -2.0 * t / nn)
                ab = np.where(todo, 1.0, 1.0 + 2.0 * t * rho / nn)
                y = M.retract(pt, xi, tb, ab)
            energies.append(Enew)
        xi.free()
        pt.free(keep_x=x is x0)
        x = _normalised(y)
    if not backtrack:
        energies.append(_dev.rayleigh(A, x))
    return x, energies
