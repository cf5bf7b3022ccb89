"""Host-side mirror of the reference's L1 interface for the hot path, on top of the C ABI.

Julia is not available in this image, so the host side that would be ``julia/TTNBackend.jl``
(shown in INTEGRATION.md) is mirrored here in Python with the reference's names, argument
meaning and error behaviour:

    TTvector / TToperator                    src/tt_tools.jl:23-29, :48-54
    A * v, A(v)                              src/tt_operations.jl:101-111, :151-157
    A * v, A rectangular (one more site)     src/tt_operations.jl:116-148
    dot, norm, euclidean_distance            src/tt_operations.jl:239-250, :452-470
    hadamard (⊕)                             src/tt_operations.jl:343-363
    +, add!, scalar *, -, /                  src/tt_operations.jl:10-66, :256-295
    orthogonalize(x; i=1)                    src/tt_tools.jl:511-543
    ttv_to_tensor                            src/tt_tools.jl (dense tensor of a train)
    _tt_bond_truncate!, tt_compress!         src/tt_tools.jl:743-789   (``!`` -> trailing ``_``)
    r_and_d_to_rks                           src/tt_tools.jl:407-425
    TToperator * TToperator, +, -, scalar *  src/tt_operations.jl:71-95, :162-172, :271-291   (opalg.py)

Every arithmetic function calls libttn_hip.so; nothing here computes on the CPU.
Site numbers (``i``, ``k``) are 1-based like the reference.  Cores are numpy arrays of shape
``(n, r_left, r_right)`` (operator: ``(n, n, R_left, R_right)``; a rectangular operator: ``(n_out, n_in, R_left, R_right)`` with
``tto_dims`` the output dimensions) and are handed to the ABI in column-major order, exactly the reference's memory layout.
"""
from __future__ import annotations

import ctypes as C
import logging
import math
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib

log = logging.getLogger("TensorTrainNumerics")


def _i64(seq) -> "C.Array":
    seq = [int(v) for v in seq]
    return (C.c_int64 * len(seq))(*seq)


def _f(core: np.ndarray) -> np.ndarray:
    """A core as the Float64 entry points read it.  A complex core is refused: the conversion would drop its imaginary part."""
    if np.iscomplexobj(core):
        raise TypeError("this operation is Float64 only: a complex core was passed (ComplexF64 is supported by *, +, -, scalar *, /, "
                        "dot, norm, euclidean_distance, hadamard, _tt_bond_truncate_, tt_compress_ and apply_compress)")
    return np.asfortranarray(core, dtype=np.float64)


def _z(core: np.ndarray) -> np.ndarray:
    """A core as the ComplexF64 entry points read it: column-major, interleaved (re, im)."""
    return np.asfortranarray(core, dtype=np.complex128)


def _is_cplx(*cores_lists) -> bool:
    return any(np.iscomplexobj(c) for cores in cores_lists for c in cores)


def _conv(cores, cplx: bool) -> List[np.ndarray]:
    """The cores of one operand as the entry points read them: ComplexF64 or Float64."""
    return [(_z if cplx else _f)(c) for c in cores]


def _entry(name: str, cplx: bool, c64_name: str = None):
    """What differs between the two element types of a stateless call: the symbol (``ttn_<name>_c64`` / ``ttn_<name>_f64``) and the
    dtype of its result buffers."""
    L = _lib.lib()
    if cplx:
        return getattr(L, c64_name or "ttn_%s_c64" % name), np.complex128
    return getattr(L, "ttn_%s_f64" % name), np.float64


def _ptrs(arrs: Sequence[np.ndarray]):
    return (C.POINTER(C.c_double) * len(arrs))(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs])


def _empty_cores(dims, rks, dtype=np.float64) -> List[np.ndarray]:
    return [np.zeros((int(dims[k]), int(rks[k]), int(rks[k + 1])), order="F", dtype=dtype) for k in range(len(dims))]


class TTvector:
    """mutable struct TTvector{T,M} — src/tt_tools.jl:23-29 (fields keep the reference's names)."""

    def __init__(self, N: int, ttv_vec: List[np.ndarray], ttv_dims: Tuple[int, ...], ttv_rks: List[int], ttv_ot: List[int]):
        self.N = int(N)
        self.ttv_vec = list(ttv_vec)
        self.ttv_dims = tuple(int(v) for v in ttv_dims)
        self.ttv_rks = [int(r) for r in ttv_rks]
        self.ttv_ot = [int(o) for o in ttv_ot]

    def copy(self) -> "TTvector":
        return TTvector(self.N, [c.copy(order="F") for c in self.ttv_vec], self.ttv_dims, list(self.ttv_rks), list(self.ttv_ot))

    # arithmetic operators of the reference
    def __add__(self, other: "TTvector") -> "TTvector":
        return add(self, other)

    def __sub__(self, other: "TTvector") -> "TTvector":
        return sub(self, other)

    def __rmul__(self, a) -> "TTvector":
        return scale(a, self)

    def __mul__(self, a) -> "TTvector":
        return scale(a, self)

    def __truediv__(self, a) -> "TTvector":
        return div(self, a)


class TToperator:
    """struct TToperator{T,M} — src/tt_tools.jl:48-54.  A core may be rectangular, (n_out, n_in, R_l, R_r): ``tto_dims`` are the
    output dimensions, as in the reference (qtto_constant_prolongation, qtto_linear_prolongation)."""

    def __init__(self, N: int, tto_vec: List[np.ndarray], tto_dims: Tuple[int, ...], tto_rks: List[int], tto_ot: List[int]):
        self.N = int(N)
        self.tto_vec = list(tto_vec)
        self.tto_dims = tuple(int(v) for v in tto_dims)
        self.tto_rks = [int(r) for r in tto_rks]
        self.tto_ot = [int(o) for o in tto_ot]

    def __mul__(self, v):
        if isinstance(v, TTvector):
            return apply(self, v)
        from . import opalg
        if isinstance(v, TToperator):
            return opalg.tto_mul(self, v)
        if isinstance(v, (int, float, np.integer, np.floating)):
            return opalg.tto_scale(v, self)
        return NotImplemented

    def __rmul__(self, a):
        from . import opalg
        if isinstance(a, (int, float, np.integer, np.floating)):
            return opalg.tto_scale(a, self)
        return NotImplemented

    def __add__(self, other):
        from . import opalg
        if isinstance(other, TToperator):
            return opalg.tto_add(self, other)
        return NotImplemented

    def __sub__(self, other):
        from . import opalg
        if isinstance(other, TToperator):
            return opalg.tto_sub(self, other)
        return NotImplemented

    def __call__(self, v: TTvector, *_):       # (A::TToperator)(x), src/tt_operations.jl:151-157
        return apply(self, v)


# ---------------------------------------------------------------------------------------------
def r_and_d_to_rks(rks: Sequence[int], dims: Sequence[int], rmax: int = 1024) -> List[int]:
    out = (C.c_int64 * len(rks))()
    _lib.check(_lib.lib().ttn_r_and_d_to_rks(len(dims), _i64(dims), len(rks), _i64(rks), int(rmax), out))
    return [int(v) for v in out]


def increase_ranks(x_tt, max_bond: int, rks: Sequence[int] | None = None, noise: float = 0.0, seed: int = 0):
    """increase_ranks(x_tt, max_bond; rks, noise) — src/tt_tools.jl:480-490: every core zero-padded to
    ``r_and_d_to_rks(rks, dims; rmax=max_bond)``, ``ttv_ot`` all zeros.  ``noise == 0`` is exact zero-padding on the host and needs no
    device; ``noise != 0`` runs k_increase_ranks (``DeviceTT.increase_ranks``), whose orthonormal blocks come from the seeded splitmix64
    stream of als_eigsolve (``seed``) instead of Julia's global RNG.  A QTTvector keeps its metadata."""
    if hasattr(x_tt, "n_dims") and hasattr(x_tt, "ttvector"):                                       # qtt_tools.jl:793
        return x_tt.increase_ranks(max_bond, rks=rks, noise=noise, seed=seed)
    max_bond = int(max_bond)
    assert max_bond > max(x_tt.ttv_rks), "New bond dimension too low"                               # tt_tools.jl:484
    d = x_tt.N
    new = r_and_d_to_rks(list(rks) if rks is not None else [1] + [max_bond] * (d - 1) + [1], x_tt.ttv_dims, rmax=max_bond)
    if any(r < c for r, c in zip(new, x_tt.ttv_rks)):
        raise _lib.TTNError(f"increase_ranks: the new ranks {new} are below the current ranks {list(x_tt.ttv_rks)}")
    if noise != 0.0:
        from .device import DeviceTT
        dx = DeviceTT.from_host(x_tt)
        dy = dx.increase_ranks(max_bond, rks=rks, noise=noise, seed=seed)
        out = dy.download(0)
        dx.free(); dy.free()
        return out
    cores = []
    for k, c in enumerate(x_tt.ttv_vec):
        p = np.zeros((c.shape[0], new[k], new[k + 1]), order="F", dtype=c.dtype)
        p[:, : c.shape[1], : c.shape[2]] = c
        cores.append(p)
    return TTvector(d, cores, x_tt.ttv_dims, new, [0] * d)


def tt_up_rks(x, max_bond: int, eps_wn: float = 0.0, **kw):
    """Deprecated alias of ``increase_ranks`` (the ``eps_wn`` keyword is now ``noise``) — src/tt_tools.jl:493-496."""
    import warnings
    warnings.warn("`tt_up_rks` is deprecated, use `increase_ranks` (the `eps_wn` keyword is now `noise`).", DeprecationWarning, stacklevel=2)
    return increase_ranks(x, max_bond, noise=eps_wn, **kw)


def apply(A: TToperator, v: TTvector) -> TTvector:
    """*(A::TToperator, v::TTvector) — src/tt_operations.jl:101-111.  Complex x complex and the two mixed forms: the real side stays
    real on the device, the result is complex.  An operator with another number of sites than v takes the reference's second method
    (apply_rect)."""
    if A.N != v.N:
        return apply_rect(A, v)
    assert tuple(A.tto_dims) == tuple(v.ttv_dims) and all(c.shape[0] == c.shape[1] for c in A.tto_vec), "Incompatible dimensions"
    d = v.N
    yr = [a * b for a, b in zip(A.tto_rks, v.ttv_rks)]
    ca, cx = _is_cplx(A.tto_vec), _is_cplx(v.ttv_vec)
    fn, dtype = _entry("apply", ca or cx)
    Y = _empty_cores(v.ttv_dims, yr, dtype)
    Ac, Xc = _conv(A.tto_vec, ca), _conv(v.ttv_vec, cx)
    flags = (int(ca), int(cx)) if ca or cx else ()
    _lib.check(fn(d, _i64(v.ttv_dims), _ptrs(Ac), _i64(A.tto_rks), _ptrs(Xc), _i64(v.ttv_rks), _ptrs(Y), *flags))
    return TTvector(d, Y, v.ttv_dims, yr, [0] * d)


def rect_singleton_sites(A: TToperator) -> List[int]:
    """The 1-based sites of A whose input index has a single value (src/tt_operations.jl:118)."""
    return [k + 1 for k, c in enumerate(A.tto_vec) if c.shape[1] == 1]


def apply_rect(A: TToperator, v: TTvector) -> TTvector:
    """*(A::TToperator{T,M}, v::TTvector{T,N}), M == N + 1 — src/tt_operations.jl:116-148: A has one more site than v and exactly one
    site s whose input index is a singleton; that site consumes no input site and the others meet v's sites in order.  With c(b) =
    b - [b >= s] the input sites left of boundary b: ranks y.rks[b] = A.rks[b] * v.rks[c(b)], regular cores as in apply, the singleton
    core Y_s[i, a' + R_l nu', a + R_r nu] = A_s[i, 1, a', a] delta(nu', nu); ttv_ot zeros.  One stateless call (ttn_apply_rect_f64).
    Float64 only."""
    M, N = A.N, v.N
    assert M == N + 1, "Rectangular TToperator must have one additional output site"
    sing = rect_singleton_sites(A)
    assert len(sing) == 1, "Rectangular TToperator must have exactly one singleton input site"
    s = sing[0]
    in_dims = [int(c.shape[1]) for c in A.tto_vec]
    assert tuple(in_dims[:s - 1] + in_dims[s:]) == tuple(v.ttv_dims), "Incompatible input dimensions"
    assert v.ttv_rks[-1] == 1, "Input TTvector must have a closed right boundary rank"
    out_dims = tuple(int(c.shape[0]) for c in A.tto_vec)
    yr = [A.tto_rks[b] * v.ttv_rks[b - (1 if b >= s else 0)] for b in range(M + 1)]
    Ac, Xc = [_f(c) for c in A.tto_vec], [_f(c) for c in v.ttv_vec]
    Y = _empty_cores(out_dims, yr)
    _lib.check(_lib.lib().ttn_apply_rect_f64(M, _i64(out_dims), _i64(in_dims), _ptrs(Ac), _i64(A.tto_rks), _ptrs(Xc), _i64(v.ttv_rks), _ptrs(Y)))
    return TTvector(M, Y, out_dims, yr, [0] * M)


def apply_compress(A: TToperator, v: TTvector, max_bond: int, truncerr: float = 0.0, sweeps: int = 1) -> TTvector:
    """tt_compress!(A * v, max_bond; truncerr, sweeps) — the operator krylov_linsolve and the time steppers iterate
    (src/solvers/euler.jl:55) — as ONE stateless call (ttn_apply_compress_f64): A * v is never materialised, neither in HBM nor over
    PCIe.  Same result as tt_compress_(apply(A, v), max_bond).  ComplexF64: apply, then round, on the device (no fused complex merge)."""
    assert tuple(A.tto_dims) == tuple(v.ttv_dims), "Incompatible dimensions"
    assert sweeps >= 1, "sweeps must be >= 1"
    d = v.N
    max_bond = int(min(max_bond, 2 ** 62))
    cap = (C.c_int64 * (d + 1))()
    _lib.check(_lib.lib().ttn_apply_compress_rank_bound(d, _i64(v.ttv_dims), _i64(A.tto_rks), _i64(v.ttv_rks), max_bond, int(sweeps), cap))
    ca, cx = _is_cplx(A.tto_vec), _is_cplx(v.ttv_vec)
    fn, dtype = _entry("apply_compress", ca or cx)
    bufs = [np.zeros(v.ttv_dims[j] * int(cap[j]) * int(cap[j + 1]), dtype=dtype) for j in range(d)]
    rks = (C.c_int64 * (d + 1))()
    Ac, Xc = _conv(A.tto_vec, ca), _conv(v.ttv_vec, cx)
    flags = (int(ca), int(cx)) if ca or cx else ()
    _lib.check(fn(d, _i64(v.ttv_dims), _ptrs(Ac), _i64(A.tto_rks), _ptrs(Xc), _i64(v.ttv_rks), _ptrs(bufs), rks,
                  max_bond, float(truncerr), int(sweeps), *flags))
    rk = [int(r) for r in rks]
    return TTvector(d, _rewrap(bufs, v.ttv_dims, rk), v.ttv_dims, rk, [0] * d)


def dot(A: TTvector, B: TTvector):
    """dot(A, B) — src/tt_operations.jl:239-250.  With a complex argument the FIRST one is conjugated (:243-248) and the result is a
    ``complex``; a real argument next to a complex one is promoted on the host."""
    assert tuple(A.ttv_dims) == tuple(B.ttv_dims), "TT dimensions are not compatible"
    cplx = _is_cplx(A.ttv_vec, B.ttv_vec)
    fn, _ = _entry("dot", cplx)
    out = (C.c_double * 2)()
    Ac, Bc = _conv(A.ttv_vec, cplx), _conv(B.ttv_vec, cplx)
    _lib.check(fn(A.N, _i64(A.ttv_dims), _ptrs(Ac), _i64(A.ttv_rks), _ptrs(Bc), _i64(B.ttv_rks), out))
    return complex(out[0], out[1]) if cplx else float(out[0])


def sandwich(x: TTvector, A: TToperator, y: TTvector) -> float:
    """<x, A y> = dot(x, A * y) in one sweep over the three cores of every site (ttn_sandwich): A * y is never formed.  The trains and
    the operator are uploaded, the kernel runs, the handles are freed.  Float64 only."""
    from .device import DeviceTT, DeviceTTO, sandwich as dev_sandwich
    assert tuple(A.tto_dims) == tuple(x.ttv_dims) == tuple(y.ttv_dims), "Incompatible dimensions"
    dx = dA = dy = None
    try:
        dx = DeviceTT.from_host(x)
        dy = dx if y is x else DeviceTT.from_host(y)
        dA = DeviceTTO(A)
        return float(dev_sandwich(dx, dA, dy)[0])
    finally:
        for h in (dA, dy if dy is not dx else None, dx):
            if h is not None:
                h.free()


def expect(A: TToperator, x: TTvector) -> float:
    """<x, A x>: ``sandwich(x, A, x)``."""
    return sandwich(x, A, x)


def rayleigh(A: TToperator, x: TTvector) -> float:
    """<x, A x> / <x, x> — the reference's ``real(dot(psi, H * psi)) / real(dot(psi, psi))`` without the train H * psi."""
    return expect(A, x) / dot(x, x)


def braket(x: TTvector, A: TToperator, y: TTvector) -> complex:
    """<x| A |y> = dot(x, A * y), x conjugated, in one sweep over the three cores of every site (ttn_braket): A * y is never formed.  The
    trains and the operator are uploaded, the kernel runs, the handles are freed.  x and y share an element type (a real one next to a
    complex one is promoted on the host, as in ``dot``); the operator keeps its own."""
    from .device import DeviceTT, DeviceTTO, braket as dev_braket
    assert tuple(A.tto_dims) == tuple(x.ttv_dims) == tuple(y.ttv_dims), "Incompatible dimensions"
    dtype = np.complex128 if _is_cplx(x.ttv_vec, y.ttv_vec) else np.float64
    dx = dA = dy = None
    try:
        dx = DeviceTT(x.ttv_dims, x.ttv_rks, 1, dtype=dtype)
        dx.upload(0, x)
        if y is x:
            dy = dx
        else:
            dy = DeviceTT(y.ttv_dims, y.ttv_rks, 1, dtype=dtype)
            dy.upload(0, y)
        dA = DeviceTTO(A)
        return complex(dev_braket(dx, dA, dy)[0])
    finally:
        for h in (dA, dy if dy is not dx else None, dx):
            if h is not None:
                h.free()


def energy(A: TToperator, x: TTvector) -> float:
    """real(<x| A |x>) / real(<x, x>) — the reference's ``real(dot(psi, H * psi)) / real(dot(psi, psi))`` without the train H * psi, for
    real or complex psi and H."""
    return float(np.real(braket(x, A, x)) / np.real(dot(x, x)))


def site_expect(x: TTvector, *ops, normalize: bool = True) -> np.ndarray:
    """The profile <x| O_k |x> / <x, x> of every site (``device.site_expect``): (d,) for one operator, (nops, d) for several.  The train
    is uploaded, the kernels run, the handle is freed.  Float64 only."""
    from .device import DeviceTT, _measure_table, site_expect as dev_site_expect
    for t, op in enumerate(ops):                    # the argument checks, before the upload
        _measure_table("site_expect", f"operator {t}", op, x.ttv_dims)
    dx = None
    try:
        dx = DeviceTT.from_host(x)
        return dev_site_expect(dx, *ops, normalize=normalize)[0]
    finally:
        if dx is not None:
            dx.free()


def correlation_matrix(x: TTvector, P, Q=None, normalize: bool = True, connected: bool = False) -> np.ndarray:
    """C[i, j] = <x| P_i Q_j |x> / <x, x> for all pairs of sites (``device.correlation_matrix``): (d, d).  Upload, call, free.
    Float64 only."""
    from .device import DeviceTT, _measure_table, correlation_matrix as dev_correlation_matrix
    for name, op in (("P", P), ("Q", Q)):           # the argument checks, before the upload
        if op is not None:
            _measure_table("correlation_matrix", name, op, x.ttv_dims)
    dx = None
    try:
        dx = DeviceTT.from_host(x)
        return dev_correlation_matrix(dx, P, Q, normalize=normalize, connected=connected)[0]
    finally:
        if dx is not None:
            dx.free()


def _zmeasure_upload(x: TTvector):
    """x as train 0 of a ComplexF64 handle: a real train is promoted on the host."""
    from .device import DeviceTT
    dx = DeviceTT(x.ttv_dims, x.ttv_rks, 1, dtype=np.complex128)
    try:
        dx.upload(0, x)
    except BaseException:
        dx.free()
        raise
    return dx


def zsite_expect(x: TTvector, *ops, normalize: bool = True) -> np.ndarray:
    """The complex profile <x| O_k |x> / <x|x> of every site (``device.zsite_expect``): complex128, (d,) for one operator, (nops, d) for
    several; the tables may be complex.  The train is uploaded as ComplexF64 — a real train is promoted, which is how it yields its
    sigma_y numbers —, the kernels run, the handle is freed."""
    from .device import _zmeasure_table, zsite_expect as dev_zsite_expect
    if not isinstance(x, TTvector):
        raise TypeError(f"zsite_expect: expected a TTvector, got {type(x).__name__}")
    for t, op in enumerate(ops):                    # the argument checks, before the upload
        _zmeasure_table("zsite_expect", f"operator {t}", op, x.ttv_dims)
    dx = None
    try:
        dx = _zmeasure_upload(x)
        return dev_zsite_expect(dx, *ops, normalize=normalize)[0]
    finally:
        if dx is not None:
            dx.free()


def zcorrelation_matrix(x: TTvector, P, Q=None, normalize: bool = True, connected: bool = False) -> np.ndarray:
    """C[i, j] = <x| P_i Q_j |x> / <x|x> for all pairs of sites (``device.zcorrelation_matrix``): complex128, (d, d); complex tables and
    a complex or real train (promoted).  Upload, call, free."""
    from .device import _zmeasure_table, zcorrelation_matrix as dev_zcorrelation_matrix
    if not isinstance(x, TTvector):
        raise TypeError(f"zcorrelation_matrix: expected a TTvector, got {type(x).__name__}")
    for name, op in (("P", P), ("Q", Q)):           # the argument checks, before the upload
        if op is not None:
            _zmeasure_table("zcorrelation_matrix", name, op, x.ttv_dims)
    dx = None
    try:
        dx = _zmeasure_upload(x)
        return dev_zcorrelation_matrix(dx, P, Q, normalize=normalize, connected=connected)[0]
    finally:
        if dx is not None:
            dx.free()


def tt_sample(x: TTvector, nsamples: int, mode: str = "born", seed: int = 0, u=None):
    """``nsamples`` configurations of the train x drawn on the device (``device.sample``): ``mode="born"`` from x(z)^2 / <x, x>,
    ``mode="density"`` from x(z) / sum x.  Returns ``(idx (S, d) int64, 1-based; logp (S,); info (2,): clamped weights, dead samples)``.
    ``u``: optional (S, d) uniforms in [0, 1) (a leading axis of length 1 is accepted); without it they come from ``seed``
    (``sample_uniforms(seed, 1, S, d)[0]``).  Upload, call, free; the argument checks run before the upload.  Float64 only."""
    from .device import DeviceTT, _sample_args, sample as dev_sample
    if not isinstance(x, TTvector):
        raise TypeError(f"tt_sample: expected a TTvector, got {type(x).__name__}")
    if any(np.iscomplexobj(c) for c in x.ttv_vec):
        raise _lib.TTNError("tt_sample: Float64 only, a ComplexF64 train is not supported")
    if u is not None and not hasattr(u, "data_ptr"):
        u = np.asarray(u)
        if u.ndim == 2:
            u = u[None]
    _sample_args("tt_sample", nsamples, mode, seed, u, 1, x.N)
    dx = None
    try:
        dx = DeviceTT.from_host(x)
        idx, logp, info = dev_sample(dx, nsamples, mode=mode, seed=seed, u=u)
        return idx[0], logp[0], info[0]
    finally:
        if dx is not None:
            dx.free()


def contract_sites(x: TTvector, weights) -> TTvector:
    """The train on the sites ``weights`` (a dict {site: vector of n_k numbers}, sites 1-based) does not name, with the named sites
    contracted against their vectors (``device.contract_sites``): marginals, slices and moments of a function-valued train without its
    dense array.  Upload, call, free; the argument checks run before the upload.  Float64 only."""
    from .device import DeviceTT, _contract_tables
    if not isinstance(x, TTvector):
        raise TypeError(f"contract_sites: expected a TTvector, got {type(x).__name__}")
    if any(np.iscomplexobj(c) for c in x.ttv_vec):
        raise _lib.TTNError("contract_sites: Float64 only, a ComplexF64 train is not supported")
    _contract_tables("contract_sites", x.ttv_dims, 1, weights)
    dx = dy = None
    try:
        dx = DeviceTT.from_host(x)
        dy = dx.contract_sites(weights)
        return dy.download(0)
    finally:
        for h in (dy, dx):
            if h is not None:
                h.free()


def norm(a: TTvector) -> float:
    """norm(a) — src/tt_operations.jl:465-470.  dot(a, a) squares every core, so a core of size 2^+-600 leaves the double range in the
    partial products though the norm itself does not (2^800 in one core and 2^-800 in the next gave 0).  Each core is divided by the
    power of two of its largest entry first and the root gets the powers back: exact, the same bits as sqrt(dot(a, a)) wherever
    that is in range."""
    total, cores = 0, []
    for c in a.ttv_vec:
        m = float(np.max(np.abs(c))) if c.size else 0.0
        k = int(np.frexp(m)[1]) if (m > 0.0 and math.isfinite(m)) else 0
        total += k
        if k == 0:
            cores.append(c)
        elif np.iscomplexobj(c):
            s = np.empty_like(c)
            s.real, s.imag = np.ldexp(c.real, -k), np.ldexp(c.imag, -k)
            cores.append(s)
        else:
            cores.append(np.ldexp(c, -k))
    b = TTvector(a.N, cores, a.ttv_dims, a.ttv_rks, a.ttv_ot)
    v = dot(b, b).real          # norm = sqrt(max(real(dot(a, a)), 0))
    v = 0.0 if v < 0 else v
    return float(np.ldexp(math.sqrt(v), total))


def euclidean_distance(a: TTvector, b: TTvector) -> float:
    """src/tt_operations.jl:452-455."""
    assert tuple(a.ttv_dims) == tuple(b.ttv_dims), "TT dimensions must match"
    return math.sqrt(max((dot(a, a) - 2 * dot(b, a).real + dot(b, b)).real, 0.0))


def _binary(name: str, x: TTvector, y: TTvector, zr: List[int]) -> TTvector:
    """z = x (op) y with result ranks zr through ttn_<name>_f64 / _c64; a real operand next to a complex one is promoted on the host."""
    d = x.N
    cplx = _is_cplx(x.ttv_vec, y.ttv_vec)
    fn, dtype = _entry(name, cplx)
    Z = _empty_cores(x.ttv_dims, zr, dtype)
    Xc, Yc = _conv(x.ttv_vec, cplx), _conv(y.ttv_vec, cplx)
    _lib.check(fn(d, _i64(x.ttv_dims), _ptrs(Xc), _i64(x.ttv_rks), _ptrs(Yc), _i64(y.ttv_rks), _ptrs(Z)))
    return TTvector(d, Z, x.ttv_dims, zr, [0] * d)


def hadamard(x: TTvector, y: TTvector) -> TTvector:
    """hadamard(x, y) / ⊕ — src/tt_operations.jl:343-363 (no conjugation, :343-361)."""
    assert tuple(x.ttv_dims) == tuple(y.ttv_dims), "Incompatible TT dimensions"
    return _binary("hadamard", x, y, [a * b for a, b in zip(x.ttv_rks, y.ttv_rks)])


def add(x: TTvector, y: TTvector) -> TTvector:
    """+(x, y) — src/tt_operations.jl:10-35."""
    assert tuple(x.ttv_dims) == tuple(y.ttv_dims), "Incompatible dimensions"
    zr = [a + b for a, b in zip(x.ttv_rks, y.ttv_rks)]
    zr[0] = 1
    zr[x.N] = 1
    return _binary("add", x, y, zr)


def add_(x: TTvector, y: TTvector) -> TTvector:
    """add!(x, y) — src/tt_operations.jl:37-66: rebinds x's fields and returns x."""
    z = add(x, y)
    x.ttv_vec, x.ttv_rks, x.ttv_ot = z.ttv_vec, z.ttv_rks, z.ttv_ot
    return x


def scale(a: float, A: TTvector) -> TTvector:
    """*(a::Number, A::TTvector) — src/tt_operations.jl:256-266."""
    d = A.N
    cplx = _is_cplx(A.ttv_vec) or isinstance(a, (complex, np.complexfloating))
    fn, dtype = _entry("scale", cplx, "ttn_scale_host_c64")
    factor = (complex(a).real, complex(a).imag) if cplx else (float(a),)
    Y = _empty_cores(A.ttv_dims, A.ttv_rks, dtype)
    Xc = _conv(A.ttv_vec, cplx)
    yot = (C.c_int64 * d)()
    _lib.check(fn(d, _i64(A.ttv_dims), *factor, _ptrs(Xc), _i64(A.ttv_rks), _i64(A.ttv_ot), _ptrs(Y), yot))
    return TTvector(d, Y, A.ttv_dims, list(A.ttv_rks), [int(v) for v in yot])


def sub(A: TTvector, B: TTvector) -> TTvector:
    """-(A, B) = (-1.0)*B + A — src/tt_operations.jl:285-287."""
    return add(scale(-1.0, B), A)


def div(A: TTvector, a: float) -> TTvector:
    """/(A, a) = (1/a)*A — src/tt_operations.jl:293-295."""
    return scale(1 / a, A)


def orthogonalize(x_tt: TTvector, i: int = 1) -> TTvector:
    """orthogonalize(x_tt; i=1) — src/tt_tools.jl:511-543 (non-mutating)."""
    d = x_tt.N
    assert 1 <= i <= d, "Impossible orthogonalization"
    if _is_cplx(x_tt.ttv_vec):
        raise TypeError("orthogonalize: complex trains are not supported (Float64 only)")
    Y = _empty_cores(x_tt.ttv_dims, x_tt.ttv_rks)      # max-size buffers: output ranks never exceed the input's
    Xc = [_f(c) for c in x_tt.ttv_vec]
    yr = (C.c_int64 * (d + 1))()
    yot = (C.c_int64 * d)()
    _lib.check(_lib.lib().ttn_orthogonalize_f64(d, _i64(x_tt.ttv_dims), _ptrs(Xc), _i64(x_tt.ttv_rks), int(i), _ptrs(Y), yr, yot))
    yr = [int(v) for v in yr]
    cores = _rewrap(Y, x_tt.ttv_dims, yr)
    return TTvector(d, cores, x_tt.ttv_dims, yr, [int(v) for v in yot])


def ttv_to_tensor(x: TTvector) -> np.ndarray:
    """ttv_to_tensor(x) — src/tt_tools.jl: the dense tensor of shape ``x.ttv_dims``, contracted on the device (ttn_tt_to_dense)."""
    from .device import DeviceTT
    if _is_cplx(x.ttv_vec):
        raise TypeError("ttv_to_tensor: complex trains are not supported (Float64 only)")
    h = DeviceTT.from_host(x)
    try:
        flat = h.to_dense().cpu().numpy()
    finally:
        h.free()
    return np.reshape(flat[0], x.ttv_dims, order="F")


def _rewrap(bufs: List[np.ndarray], dims, rks) -> List[np.ndarray]:
    """Max-size buffers hold the compact cores of the NEW ranks at their start; re-wrap them as
    exact-size arrays so that size(core) == (n, r_l, r_r) as the reference's tests require."""
    out = []
    for k, buf in enumerate(bufs):
        n, rl, rr = int(dims[k]), int(rks[k]), int(rks[k + 1])
        flat = buf.reshape(-1, order="F")[: n * rl * rr]
        out.append(np.array(flat.reshape((n, rl, rr), order="F"), order="F"))
    return out


def _tt_bond_truncate_(psi: TTvector, k: int, max_bond: int = 2 ** 62, truncerr: float = 0.0) -> TTvector:
    """_tt_bond_truncate!(psi, k; max_bond, truncerr) — src/tt_tools.jl:743-770.  Mutates cores k, k+1
    and ttv_rks[k+1]; ttv_ot untouched.  Returns orthogonalize(psi; i=k) like the reference (:769)."""
    assert 1 <= k < psi.N, "k must be in 1:(N-1)"
    _compress_call(psi, k, max_bond, truncerr, 1)
    if _is_cplx(psi.ttv_vec):
        return psi                 # (orthogonalize is Float64 only: the value the reference returns here is not formed for complex trains)
    return orthogonalize(psi, i=k)


def tt_compress_(psi: TTvector, max_bond: int, truncerr: float = 0.0, sweeps: int = 1, verbose: bool = False) -> TTvector:
    """tt_compress!(psi, max_bond; truncerr=0.0, sweeps=1, verbose=false) — src/tt_tools.jl:772-789.
    Returns the SAME object.  The per-bond `orthogonalize` whose value the reference discards
    (:769, :779, :785) is not computed."""
    assert sweeps >= 1, "sweeps must be >= 1"
    if verbose:
        # the reference logs per sweep (tt_tools.jl:775-783); the whole call is one kernel here
        for sw in range(1, sweeps + 1):
            log.info("TT compress: sweep %d (L→R)", sw)
            log.info("TT compress: sweep %d (R→L)", sw)
    _compress_call(psi, 0, max_bond, truncerr, sweeps)
    return psi


def _compress_call(psi: TTvector, k: int, max_bond: int, truncerr: float, sweeps: int) -> None:
    d = psi.N
    max_bond = int(min(max_bond, 2 ** 62))
    L = _lib.lib()
    # a rank-deficient bond can grow up to min(n r_left, n r_right, max_bond) (the reference keeps
    # min(length(s), max_bond) singular values): size the in/out buffers for that
    need = (C.c_int64 * (d + 1))()
    _lib.check(L.ttn_compress_rank_bound(d, _i64(psi.ttv_dims), _i64(psi.ttv_rks), max_bond, int(sweeps), int(k), need, None))
    cplx = _is_cplx(psi.ttv_vec)
    fn, dtype = _entry("bond_truncate" if k > 0 else "compress", cplx)
    bufs = []
    for j in range(d):
        buf = np.zeros(psi.ttv_dims[j] * int(need[j]) * int(need[j + 1]), dtype=dtype)
        buf[: psi.ttv_vec[j].size] = (_z if cplx else _f)(psi.ttv_vec[j]).reshape(-1, order="F")
        bufs.append(buf)
    rks = _i64(psi.ttv_rks)
    tail = (int(k), max_bond, float(truncerr)) if k > 0 else (max_bond, float(truncerr), int(sweeps))
    rc = fn(d, _i64(psi.ttv_dims), _ptrs(bufs), rks, *tail)
    _lib.check(rc)
    new_rks = [int(v) for v in rks]
    cores = _rewrap(bufs, psi.ttv_dims, new_rks)
    for j in range(d):
        psi.ttv_vec[j] = cores[j]      # in-place slot assignment like the reference (:764-767)
    psi.ttv_rks[:] = new_rks
