"""Core gradients: the reverse-mode rules of the reference's ChainRulesCore extension (ext/TensorTrainNumericsChainRulesCoreExt.jl) on
the device, and the core-wise linear algebra of their tangents (csrc/ttn_grad_kernels.h).  Float64 only.

On handles (a batch of resident trains; nothing but scalars crosses to the host):

    dot_pullback(a, b, delta, abar, bbar)    rrule of dot(A, B), ChainRulesCoreExt.jl:36-65
    apply_pullback(A, x, ybar, xbar)         rrule of H * psi with respect to psi, :67-88
    cores_axpby(alpha, x, beta, y)           y_k <- alpha_b x_k + beta_b y_k on every core
    cores_dot(x, y)                          sum_k <x_k, y_k>  (test_ad.jl: ladot)
    rayleigh_value_and_grad(A, psi, g)       E = <psi, A psi> / <psi, psi> and its gradient, composed from the calls above and ttn_apply
    sandwich_pullback(x, A, y, delta, ...)   tangents of <x, A y> on the three-layer environments: A y is never formed
    expect_value_and_grad(A, psi, g)         <psi, A psi> and its gradient xbar + ybar
    rayleigh_value_and_grad(..., fused=True) the same E and gradient from sandwich_pullback: no A psi, no cotangent of its size

A tangent is an ordinary ``DeviceTT`` used as a bag of cores with the primal's current ranks; it is never contracted as a train.

On host trains, with the reference's shape: ``dot_rrule``, ``apply_rrule``, ``sandwich_rrule``, ``rayleigh_gradient``.  They run the same kernels on a batch
of one; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .device import DeviceTT, DeviceTTO
from .device import apply as _dev_apply
from .tt import TToperator, TTvector


def _coef(v, batch: int):
    """One double per train as the ABI reads it (None: the library takes 1)."""
    if v is None:
        return None
    arr = np.broadcast_to(np.asarray(v, dtype=np.float64), (batch,))
    return (C.c_double * batch)(*[float(x) for x in arr])


def _like(x: DeviceTT) -> DeviceTT:
    return DeviceTT(x.dims, x.cap, x.batch)


def dot_pullback(a: DeviceTT, b: DeviceTT, delta=None, abar: Optional[DeviceTT] = None, bbar: Optional[DeviceTT] = None,
                 want_value: bool = True, want_abar: bool = True, want_bbar: bool = True):
    """(values or None, abar, bbar): abar_k = delta_b * d dot(a_b, b_b) / d a_k, bbar likewise.  A destination that is not given is
    allocated with its source's capacity unless ``want_abar`` / ``want_bbar`` is False (then it is not computed and None is returned)."""
    if want_abar and abar is None:
        abar = _like(a)
    if want_bbar and bbar is None:
        bbar = _like(b)
    out = (C.c_double * a.batch)() if want_value else None
    _lib.check(_lib.lib().ttn_dot_pullback(a.h, b.h, _coef(delta, a.batch), abar.h if abar is not None else None,
                                           bbar.h if bbar is not None else None, out))
    return (np.array(out[:]) if want_value else None), abar, bbar


def apply_pullback(A: DeviceTTO, x: DeviceTT, ybar: DeviceTT, xbar: Optional[DeviceTT] = None) -> DeviceTT:
    """xbar = (d (A x) / d x)^T ybar, core by core; x only gives the ranks."""
    if xbar is None:
        xbar = _like(x)
    _lib.check(_lib.lib().ttn_apply_pullback(A.h, x.h, ybar.h, xbar.h))
    return xbar


def cores_axpby(alpha, x: DeviceTT, beta, y: DeviceTT) -> DeviceTT:
    """y_k <- alpha_b x_k + beta_b y_k on every core (alpha, beta: a scalar, one value per train, or None = 1)."""
    _lib.check(_lib.lib().ttn_tt_cores_axpby(_coef(alpha, x.batch), x.h, _coef(beta, x.batch), y.h))
    return y


def cores_dot(x: DeviceTT, y: DeviceTT) -> np.ndarray:
    out = (C.c_double * x.batch)()
    _lib.check(_lib.lib().ttn_tt_cores_dot(x.h, y.h, out))
    return np.array(out[:])


def sandwich_pullback(x: DeviceTT, A: DeviceTTO, y: DeviceTT, delta=None, xbar: Optional[DeviceTT] = None, ybar: Optional[DeviceTT] = None,
                      want_value: bool = True, want_xbar: bool = True, want_ybar: bool = True):
    """(values or None, xbar, ybar): xbar_k = delta_b * d <x_b, A y_b> / d x_k, ybar likewise (ttn_sandwich_pullback): one three-layer
    chain from each end, every gradient a contraction of the two environments with the operator core and the other train's core.  A y is
    never formed.  Destinations are allocated as ``dot_pullback`` allocates them; the values are not scaled by delta."""
    if not isinstance(A, DeviceTTO):
        raise TypeError(f"sandwich_pullback: expected a DeviceTTO, got {type(A).__name__}")
    if not isinstance(x, DeviceTT) or not isinstance(y, DeviceTT):
        raise TypeError("sandwich_pullback: expected DeviceTT trains")
    if want_xbar and xbar is None:
        xbar = _like(x)
    if want_ybar and ybar is None:
        ybar = _like(y)
    out = (C.c_double * x.batch)() if want_value else None
    _lib.check(_lib.lib().ttn_sandwich_pullback(x.h, A.h, y.h, _coef(delta, x.batch), xbar.h if xbar is not None else None,
                                                ybar.h if ybar is not None else None, out))
    return (np.array(out[:]) if want_value else None), xbar, ybar


def expect_value_and_grad(A: DeviceTTO, psi: DeviceTT, g: Optional[DeviceTT] = None) -> Tuple[np.ndarray, DeviceTT]:
    """(<psi, A psi>, its gradient with respect to the cores of psi) per train: xbar + ybar of ``sandwich_pullback(psi, A, psi)``."""
    val, g, yb = sandwich_pullback(psi, A, psi, xbar=g)
    cores_axpby(None, yb, None, g)
    yb.free()
    return val, g


def rayleigh_value_and_grad(A: DeviceTTO, psi: DeviceTT, g: Optional[DeviceTT] = None, fused: bool = False) -> Tuple[np.ndarray, DeviceTT]:
    """E_b = <psi, A psi> / <psi, psi> and g = dE / d(cores of psi), per train (test_ad.jl:104-113):
    Y = A psi; (psibar1, Ybar) = pullback of dot(psi, Y) at 1 / <psi, psi>; psibar2 = pullback of Y = A psi at Ybar;
    (p3, p4) = pullback of dot(psi, psi) at -E / <psi, psi>; g = psibar1 + psibar2 + p3 + p4.
    ``fused=True`` takes psibar1 and psibar2 from ``sandwich_pullback`` at 1 / <psi, psi> instead: neither Y nor Ybar exists."""
    from .device import dot as _dot
    if fused:
        nn = _dot(psi, psi)
        num, g, t = sandwich_pullback(psi, A, psi, delta=1.0 / nn, xbar=g)
        E = num / nn
        cores_axpby(None, t, None, g)
        _, p3, p4 = dot_pullback(psi, psi, delta=-E / nn, abar=t, want_value=False)
        cores_axpby(None, p3, None, g)
        cores_axpby(None, p4, None, g)
        for h in (p3, p4):
            h.free()
        return E, g
    Y = DeviceTT(psi.dims, [R * c for R, c in zip(A.rks, psi.cap)], psi.batch)
    _dev_apply(A, psi, Y)
    nn = _dot(psi, psi)
    num, g, Ybar = dot_pullback(psi, Y, delta=1.0 / nn, abar=g)
    E = num / nn
    t = apply_pullback(A, psi, Ybar)
    cores_axpby(None, t, None, g)
    _, p3, p4 = dot_pullback(psi, psi, delta=-E / nn, abar=t, want_value=False)
    cores_axpby(None, p3, None, g)
    cores_axpby(None, p4, None, g)
    for h in (Y, Ybar, p3, p4):
        h.free()
    return E, g


# ---- host trains, the reference's rrule shape -------------------------------------------------------------------------------------
def _cores(t: DeviceTT) -> List[np.ndarray]:
    return t.download(0).ttv_vec


def dot_rrule(A: TTvector, B: TTvector) -> Tuple[float, Callable]:
    """(dot(A, B), pullback) with pullback(delta) -> (Abar cores, Bbar cores) — ChainRulesCoreExt.jl:36-65."""
    a, b = DeviceTT.from_host(A), DeviceTT.from_host(B)
    val, abar, bbar = dot_pullback(a, b)
    value = float(val[0])
    abar.free()
    bbar.free()

    def pullback(delta):
        _, ab, bb = dot_pullback(a, b, delta=float(delta), want_value=False)
        res = (_cores(ab), _cores(bb))
        ab.free()
        bb.free()
        return res

    return value, pullback


def sandwich_rrule(X: TTvector, H: TToperator, Y: TTvector) -> Tuple[float, Callable]:
    """(<X, H Y>, pullback) with pullback(delta) -> (Xbar cores, Ybar cores); H gets no tangent, as in the reference's rule of H * psi.
    The value is one ``ttn_sandwich`` sweep; the chains and the tangents are computed only when the pullback is called."""
    from .device import sandwich as _sandwich
    x, y, Hd = DeviceTT.from_host(X), DeviceTT.from_host(Y), DeviceTTO(H)
    value = float(_sandwich(x, Hd, y)[0])

    def pullback(delta):
        _, xb, yb = sandwich_pullback(x, Hd, y, delta=float(delta), want_value=False)
        res = (_cores(xb), _cores(yb))
        xb.free()
        yb.free()
        return res

    return value, pullback


def apply_rrule(H: TToperator, psi: TTvector) -> Tuple[TTvector, Callable]:
    """(H * psi, pullback) with pullback(Ybar cores or TTvector) -> psibar cores — ChainRulesCoreExt.jl:67-88 (H gets no tangent)."""
    Hd, x = DeviceTTO(H), DeviceTT.from_host(psi)
    yrks = [R * r for R, r in zip(H.tto_rks, psi.ttv_rks)]
    y = DeviceTT(psi.ttv_dims, yrks, 1)
    _dev_apply(Hd, x, y)
    Y = y.download(0)

    def pullback(ybar):
        cores = ybar.ttv_vec if hasattr(ybar, "ttv_vec") else list(ybar)
        yb = DeviceTT.from_host(TTvector(psi.N, cores, psi.ttv_dims, yrks, [0] * psi.N))
        xb = apply_pullback(Hd, x, yb)
        res = _cores(xb)
        yb.free()
        xb.free()
        return res

    return Y, pullback


def rayleigh_gradient(H: TToperator, psi: TTvector, fused: bool = False) -> Tuple[float, List[np.ndarray]]:
    """(E, dE / d cores) of the Rayleigh quotient <psi, H psi> / <psi, psi> — test_ad.jl:104-113 (``fused``: see rayleigh_value_and_grad)."""
    E, g = rayleigh_value_and_grad(DeviceTTO(H), DeviceTT.from_host(psi), fused=fused)
    cores = _cores(g)
    g.free()
    return float(E[0]), cores
