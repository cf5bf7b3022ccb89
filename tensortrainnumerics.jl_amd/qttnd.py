"""The multi-dimensional QTT layer (src/qtt_tools.jl:362-972, qtt_laplacian of src/tt_operators.jl:644-703, entanglemententropy of
src/tt_tools.jl:554-587).

    QTTvector / QTToperator, check_compat     src/qtt_tools.jl:370-528    (orderings are the strings "interleaved" / "serial")
    +, -, scalar *, /, hadamard, dot, norm,
    A * q, the mixed forms, copy, orthogonalize,
    tt_compress_                               src/qtt_tools.jl:530-647, :783-786
    reorder                                    src/qtt_tools.jl:732-774, :895-935   (the swap chains of qtt.py)
    function_to_qttv                           src/qtt_tools.jl:805-839
    qttv_to_array                              src/qtt_tools.jl:943-972
    qtt_laplacian                              src/tt_operators.jl:644-703
    entanglemententropy                        src/tt_tools.jl:554-587, src/qtt_tools.jl:472-474

The arithmetic is the existing one of tt.py / opalg.py / qtt.py with the metadata carried along.  What is new underneath runs in
csrc/ttn_grid_kernels.h: the grid never exists on the host (ttn_qtt_grid_points -> f on the library's stream -> ttn_ttv_decomp_dev),
and a train becomes a dense array on the device (ttn_tt_to_dense) with the bit -> grid-index rule folded into the output strides.
Float64 only.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List

import numpy as np

from . import _lib, opalg, qtt
from . import tt as _tt
from .tt import TToperator, TTvector

ORDERINGS = ("interleaved", "serial")
_CHUNK = 1 << 20          # grid points per call of f


def _check_meta(N, dims, n_dims, bits_per_dim, ordering, field):
    """the three checks of src/qtt_tools.jl:437-440 / :457-460"""
    if n_dims * bits_per_dim != N:
        raise _lib.TTNError(f"n_dims * bits_per_dim must equal {field}.N (got {n_dims}*{bits_per_dim}={n_dims * bits_per_dim} ≠ {N})")
    if not all(int(n) == 2 for n in dims):
        raise _lib.TTNError(f"All physical dimensions must be 2 for QTT (got {tuple(dims)})")
    if ordering not in ORDERINGS:
        raise _lib.TTNError(f"ordering must be :interleaved or :serial (got {ordering})")


def _eltype(cores) -> str:
    return "ComplexF64" if any(np.iscomplexobj(c) for c in cores) else "Float64"


def _is_scalar(a) -> bool:
    return isinstance(a, (int, float, complex, np.integer, np.floating, np.complexfloating)) and not isinstance(a, bool)


class QTTvector:
    """mutable struct QTTvector — src/qtt_tools.jl:370-379: the fields of a TTvector plus n_dims, bits_per_dim, ordering."""

    def __init__(self, ttv: TTvector, n_dims: int, bits_per_dim: int, ordering: str):
        if not isinstance(ttv, TTvector):
            raise TypeError(f"QTTvector: expected a TTvector, got {type(ttv).__name__}")
        n_dims, bits_per_dim = int(n_dims), int(bits_per_dim)
        _check_meta(ttv.N, ttv.ttv_dims, n_dims, bits_per_dim, ordering, "ttv")
        self.N = ttv.N
        self.ttv_vec, self.ttv_dims, self.ttv_rks, self.ttv_ot = ttv.ttv_vec, ttv.ttv_dims, ttv.ttv_rks, ttv.ttv_ot
        self.n_dims, self.bits_per_dim, self.ordering = n_dims, bits_per_dim, ordering

    def ttvector(self) -> TTvector:
        """TTvector(q) — src/qtt_tools.jl:469-470: the same cores without the metadata."""
        return TTvector(self.N, self.ttv_vec, self.ttv_dims, self.ttv_rks, self.ttv_ot)

    def _like(self, ttv: TTvector) -> "QTTvector":
        return QTTvector(ttv, self.n_dims, self.bits_per_dim, self.ordering)

    def __repr__(self) -> str:
        return f"QTT-MPS{{{_eltype(self.ttv_vec)}}}({self.N} sites, {self.n_dims}d×{self.bits_per_dim}bits, {self.ordering})"

    def copy(self) -> "QTTvector":
        return self._like(self.ttvector().copy())

    def orthogonalize(self, i: int = 1) -> "QTTvector":
        return self._like(_tt.orthogonalize(self.ttvector(), i=i))

    def increase_ranks(self, max_bond: int, rks=None, noise: float = 0.0, seed: int = 0) -> "QTTvector":
        """increase_ranks(q, max_bond; rks, noise) — src/qtt_tools.jl:793: n_dims, bits_per_dim and ordering are kept."""
        return self._like(_tt.increase_ranks(self.ttvector(), max_bond, rks=rks, noise=noise, seed=seed))

    def reorder(self, new_ordering: str, threshold: float = 0.0) -> "QTTvector":
        return reorder(self, new_ordering, threshold)

    def hadamard(self, other: "QTTvector") -> "QTTvector":
        return hadamard(self, other)

    def dot(self, other):
        return dot(self, other)

    def norm(self) -> float:
        return norm(self)

    def tt_compress_(self, max_bond: int, **kw) -> "QTTvector":
        return tt_compress_(self, max_bond, **kw)

    # a QTTvector next to a QTTvector keeps the metadata; next to a bare TTvector the result is bare (:607-621)
    def __add__(self, other):
        if isinstance(other, QTTvector):
            check_compat(self, other)
            return self._like(_tt.add(self.ttvector(), other.ttvector()))
        if isinstance(other, TTvector):
            return _tt.add(self.ttvector(), other)
        return NotImplemented

    def __radd__(self, other):
        if isinstance(other, TTvector):
            return _tt.add(other, self.ttvector())
        return NotImplemented

    def __sub__(self, other):
        if isinstance(other, QTTvector):
            check_compat(self, other)
            return self._like(_tt.sub(self.ttvector(), other.ttvector()))
        if isinstance(other, TTvector):
            return _tt.sub(self.ttvector(), other)
        return NotImplemented

    def __rsub__(self, other):
        if isinstance(other, TTvector):
            return _tt.sub(other, self.ttvector())
        return NotImplemented

    def __mul__(self, a):
        if _is_scalar(a):
            return self._like(_tt.scale(a, self.ttvector()))
        return NotImplemented

    def __rmul__(self, a):
        if _is_scalar(a):
            return self._like(_tt.scale(a, self.ttvector()))
        if isinstance(a, TToperator):                      # *(A::TToperator, q::QTTvector) = A * TTvector(q), :599-601
            return _tt.apply(a, self.ttvector())
        return NotImplemented

    def __truediv__(self, a):
        if _is_scalar(a):
            return self._like(_tt.div(self.ttvector(), a))
        return NotImplemented


class QTToperator:
    """struct QTToperator — src/qtt_tools.jl:384-393."""

    def __init__(self, tto: TToperator, n_dims: int, bits_per_dim: int, ordering: str):
        if not isinstance(tto, TToperator):
            raise TypeError(f"QTToperator: expected a TToperator, got {type(tto).__name__}")
        n_dims, bits_per_dim = int(n_dims), int(bits_per_dim)
        _check_meta(tto.N, tto.tto_dims, n_dims, bits_per_dim, ordering, "tto")
        self.N = tto.N
        self.tto_vec, self.tto_dims, self.tto_rks, self.tto_ot = tto.tto_vec, tto.tto_dims, tto.tto_rks, tto.tto_ot
        self.n_dims, self.bits_per_dim, self.ordering = n_dims, bits_per_dim, ordering

    def ttoperator(self) -> TToperator:
        """TToperator(q) — src/qtt_tools.jl:481-482."""
        return TToperator(self.N, self.tto_vec, self.tto_dims, self.tto_rks, self.tto_ot)

    def _like(self, tto: TToperator) -> "QTToperator":
        return QTToperator(tto, self.n_dims, self.bits_per_dim, self.ordering)

    def __repr__(self) -> str:
        return f"QTT-MPO{{{_eltype(self.tto_vec)}}}({self.N} sites, {self.n_dims}d×{self.bits_per_dim}bits, {self.ordering})"

    def copy(self) -> "QTToperator":
        return self._like(TToperator(self.N, [np.array(c, order="F") for c in self.tto_vec], self.tto_dims, list(self.tto_rks), list(self.tto_ot)))

    def reorder(self, new_ordering: str, threshold: float = 0.0) -> "QTToperator":
        return reorder(self, new_ordering, threshold)

    def __add__(self, other):
        if isinstance(other, QTToperator):
            check_compat(self, other)
            return self._like(opalg.tto_add(self.ttoperator(), other.ttoperator()))
        if isinstance(other, TToperator):
            return opalg.tto_add(self.ttoperator(), other)
        return NotImplemented

    def __radd__(self, other):
        if isinstance(other, TToperator):
            return opalg.tto_add(other, self.ttoperator())
        return NotImplemented

    def __sub__(self, other):
        if isinstance(other, QTToperator):
            check_compat(self, other)
            return self._like(opalg.tto_sub(self.ttoperator(), other.ttoperator()))
        if isinstance(other, TToperator):
            return opalg.tto_sub(self.ttoperator(), other)
        return NotImplemented

    def __rsub__(self, other):
        if isinstance(other, TToperator):
            return opalg.tto_sub(other, self.ttoperator())
        return NotImplemented

    def __mul__(self, v):
        if isinstance(v, QTTvector):                       # :594-597
            check_compat(self, v)
            return v._like(_tt.apply(self.ttoperator(), v.ttvector()))
        if isinstance(v, TTvector):                        # :603-605
            return _tt.apply(self.ttoperator(), v)
        if _is_scalar(v):
            return self._like(opalg.tto_scale(v, self.ttoperator()))
        return NotImplemented

    def __rmul__(self, a):
        if _is_scalar(a):                                  # :590-592
            return self._like(opalg.tto_scale(a, self.ttoperator()))
        return NotImplemented


def check_compat(a, b) -> None:
    """check_compat — src/qtt_tools.jl:491-528: n_dims, bits_per_dim and ordering of two QTT objects must agree (TTNError); a pair of
    plain TTvector / TToperator objects is always compatible."""
    plain = (TTvector, TToperator)
    if isinstance(a, plain) and isinstance(b, plain):
        return None
    if isinstance(a, QTTvector) and isinstance(b, QTTvector):
        who = "QTTvector"
    elif isinstance(a, QTToperator) and isinstance(b, QTTvector):
        who = "QTToperator/QTTvector"
    elif isinstance(a, QTToperator) and isinstance(b, QTToperator):
        who = "QTToperator"
    else:
        raise TypeError(f"check_compat: no method for ({type(a).__name__}, {type(b).__name__})")
    for field in ("n_dims", "bits_per_dim", "ordering"):
        if getattr(a, field) != getattr(b, field):
            raise _lib.TTNError(f"{who} {field} mismatch: {getattr(a, field)} ≠ {getattr(b, field)}")
    return None


def _bare(x):
    return x.ttvector() if isinstance(x, QTTvector) else x


def hadamard(a: QTTvector, b: QTTvector) -> QTTvector:
    """hadamard(a, b) — src/qtt_tools.jl:560-563."""
    check_compat(a, b)
    return a._like(_tt.hadamard(a.ttvector(), b.ttvector()))


def dot(a, b):
    """dot of two QTTvectors (metadata checked, :565-573) or of a QTTvector and a bare TTvector (:627-631)."""
    if isinstance(a, QTTvector) and isinstance(b, QTTvector):
        check_compat(a, b)
    return _tt.dot(_bare(a), _bare(b))


def norm(q: QTTvector) -> float:
    return _tt.norm(_bare(q))


def orthogonalize(q: QTTvector, i: int = 1) -> QTTvector:
    return q.orthogonalize(i)


def tt_compress_(q: QTTvector, max_bond: int, **kw) -> QTTvector:
    """tt_compress!(q, max_bond; kwargs...) — src/qtt_tools.jl:783-786: q's cores and ranks are rebound to the result; returns q."""
    t = _tt.tt_compress_(q.ttvector(), max_bond, **kw)
    q.ttv_vec, q.ttv_rks, q.ttv_ot = t.ttv_vec, t.ttv_rks, t.ttv_ot
    return q


def reorder(q, new_ordering: str, threshold: float = 0.0):
    """reorder(q, new_ordering; threshold) for a QTTvector (:732-774) or a QTToperator (:895-935) through the device swap chains; with
    the ordering q already has it returns a copy, as the reference does."""
    if new_ordering not in ORDERINGS:
        raise _lib.TTNError("ordering must be :interleaved or :serial")
    if not isinstance(q, (QTTvector, QTToperator)):
        raise TypeError(f"reorder: expected a QTTvector or a QTToperator, got {type(q).__name__}")
    if q.ordering == new_ordering:
        return q.copy()
    if isinstance(q, QTTvector):
        return QTTvector(qtt.reorder(q.ttvector(), q.n_dims, q.bits_per_dim, new_ordering, threshold), q.n_dims, q.bits_per_dim, new_ordering)
    return QTToperator(qtt.reorder_op(q.ttoperator(), q.n_dims, q.bits_per_dim, new_ordering, threshold), q.n_dims, q.bits_per_dim, new_ordering)


# ---- the bit rule ---------------------------------------------------------------------------------------------------------------
def site_dim_level(site: int, n_dims: int, bits_per_dim: int, ordering: str):
    """(dim, level), both 0-based, of the 0-based site — src/qtt_tools.jl:820-829."""
    if ordering == "interleaved":
        return site % n_dims, site // n_dims
    return site // bits_per_dim, site % bits_per_dim


def grid_strides(n_dims: int, bits_per_dim: int, ordering: str) -> List[int]:
    """Output strides that make ttn_tt_to_dense write qttv_to_array's array: strides[site] = 2^(bits-1-level) * (2^bits)^dim, the
    rule of src/qtt_tools.jl:957-968 with dimension 1 fastest (a Julia Array)."""
    if ordering not in ORDERINGS:
        raise _lib.TTNError(f"ordering must be :interleaved or :serial (got {ordering})")
    out = []
    for site in range(n_dims * bits_per_dim):
        dim, level = site_dim_level(site, n_dims, bits_per_dim, ordering)
        out.append(2 ** (bits_per_dim - 1 - level) * (2 ** bits_per_dim) ** dim)
    return out


# ---- function -> QTT, QTT -> array ---------------------------------------------------------------------------------------------------
def function_to_qttv(f, n_dims: int, bits_per_dim: int, ordering: str = "interleaved", a: float = 0.0, b: float = 1.0) -> QTTvector:
    """function_to_qttv(f, n_dims, bits_per_dim; ordering, a, b) — src/qtt_tools.jl:805-839.  f has the cross module's calling
    convention: it receives the coordinates of P grid points as a (P, n_dims) float64 tensor on the library's device and stream and
    returns P values (a torch tensor, or anything np.asarray takes).  The grid is generated chunk by chunk on the device, f's values
    go straight into the tensor buffer, and ttn_ttv_decomp_dev decomposes it there (index = 1, tol = 1e-12, like ttv_decomp(tensor))."""
    from .device import DeviceTT, compress_status
    from .tdvp import _dev
    n_dims, bits_per_dim = int(n_dims), int(bits_per_dim)
    if ordering not in ORDERINGS:
        raise _lib.TTNError(f"ordering must be :interleaved or :serial (got {ordering})")
    if n_dims < 1 or bits_per_dim < 1:
        raise _lib.TTNError("function_to_qttv: n_dims and bits_per_dim must be at least 1")
    N = n_dims * bits_per_dim
    if N > 27:
        raise _lib.TTNError(f"function_to_qttv: 2^{N} grid points; the device decomposition takes at most 2^27")
    torch, stream = _dev()
    total = 1 << N
    L = _lib.lib()
    with torch.cuda.stream(stream):
        tensor = torch.empty((total,), dtype=torch.float64, device="cuda")
        X = torch.empty((n_dims, min(_CHUNK, total)), dtype=torch.float64, device="cuda")
        bad = torch.full((1,), -1, dtype=torch.int64, device="cuda")          # the first chunk with a non-finite value
        for chunk, first in enumerate(range(0, total, _CHUNK)):
            count = min(_CHUNK, total - first)
            Xc = X if count == X.shape[1] else X.reshape(-1)[: n_dims * count].reshape(n_dims, count)
            _lib.check(L.ttn_qtt_grid_points(n_dims, bits_per_dim, 1 if ordering == "interleaved" else 0, float(a), float(b), first, count,
                                             C.c_void_p(Xc.data_ptr())))
            y = f(Xc.T)
            y = y.to("cuda") if isinstance(y, torch.Tensor) else torch.from_numpy(np.array(y)).to("cuda")
            if y.numel() != count:
                raise _lib.TTNError(f"function_to_qttv: f returned {y.numel()} values for {count} points (chunk {chunk}, entries {first}..{first + count - 1})")
            if y.is_complex():
                raise _lib.TTNError(f"function_to_qttv: f returned complex values (chunk {chunk}); Float64 only")
            seg = tensor[first:first + count]
            seg.copy_(y.reshape(-1))
            fin = torch.isfinite(seg).all()
            bad.copy_(torch.where((bad < 0) & ~fin, torch.full_like(bad, chunk), bad))
        nb = int(bad.item())
        if nb >= 0:
            raise _lib.TTNError(f"function_to_qttv: f returned a non-finite value (chunk {nb}, entries {nb * _CHUNK}..{min((nb + 1) * _CHUNK, total) - 1})")
        cap = [1] + [max(1, min(1 << k, 1 << (N - k), 1024)) for k in range(1, N)] + [1]     # the capacity qtt.ttv_decomp chooses
        z = DeviceTT((2,) * N, cap)
        try:
            qtt.ttv_decomp_dev_(z, tensor, 1, 1.0e-12)
            compress_status(z)
            z.max_ranks()
            ttv = z.download(0)
        finally:
            z.free()
    return QTTvector(ttv, n_dims, bits_per_dim, ordering)


def qttv_to_array(q: QTTvector, device: bool = False):
    """qttv_to_array(q) — src/qtt_tools.jl:943-972: the values on the grid, shape (2^bits,) * n_dims with out[g1, ..., gn] the
    reference's out[g1 + 1, ...].  One ttn_tt_to_dense with grid_strides; ``device=True`` returns the torch tensor (a view with the
    same logical indexing) instead of an ndarray."""
    from .device import DeviceTT
    if not isinstance(q, QTTvector):
        raise TypeError(f"qttv_to_array: expected a QTTvector, got {type(q).__name__}")
    shape = (2 ** q.bits_per_dim,) * q.n_dims
    h = DeviceTT.from_host(q.ttvector())
    try:
        flat = h.to_dense(grid_strides(q.n_dims, q.bits_per_dim, q.ordering))[0]
        if device:
            return flat.reshape(shape[::-1]).permute(*range(q.n_dims - 1, -1, -1))      # dimension 1 is the fastest one in memory
        return np.reshape(flat.cpu().numpy(), shape, order="F")
    finally:
        h.free()


def qttv_sample(q: QTTvector, nsamples: int, mode: str = "density", seed: int = 0):
    """``nsamples`` grid points drawn from a QTT vector on the device (``tt.tt_sample``): ``mode="density"`` from q / sum q for a
    non-negative q (a probability density on the grid), ``mode="born"`` from q^2 / <q, q>.  Returns ``(grid, logp)``: ``grid`` is
    (S, n_dims) int64, 0-based, with ``qttv_to_array(q)[tuple(grid[s])]`` the value of the train at the sampled bits (the bits are
    decoded by q's own n_dims / bits_per_dim / ordering), ``logp`` (S,) the log-probability of each point; a dead sample (see
    ``device.sample``) has logp = -inf."""
    from .tt import tt_sample
    if not isinstance(q, QTTvector):
        raise TypeError(f"qttv_sample: expected a QTTvector, got {type(q).__name__}")
    idx, logp, _ = tt_sample(q.ttvector(), nsamples, mode=mode, seed=seed)
    weights = np.array([2 ** (q.bits_per_dim - 1 - site_dim_level(site, q.n_dims, q.bits_per_dim, q.ordering)[1]) for site in range(q.N)], dtype=np.int64)
    dims = np.array([site_dim_level(site, q.n_dims, q.bits_per_dim, q.ordering)[0] for site in range(q.N)])
    grid = np.zeros((idx.shape[0], q.n_dims), dtype=np.int64)
    for dim in range(q.n_dims):
        sel = dims == dim
        grid[:, dim] = (idx[:, sel] - 1) @ weights[sel]
    return grid, logp


# ---- marginals, slices, moments (include/ttn_contract.h) -----------------------------------------------------------------
# What the PDE examples of the reference take from the dense array (sum(P) * h^2, sum(P, dims = 2), P[:, j], the means, variances and
# the covariance) computed on the train: a subset of the sites is contracted against weight vectors (contract_sites) and the rest stays a
# train.  Every function takes a QTTvector and returns QTTvectors, or takes a pair (DeviceTT, (n_dims, bits_per_dim, ordering)) — a
# resident batch with its metadata — and returns such pairs (new handles; per-train numbers as arrays over the batch).  Dimensions and
# grid indices are 0-based, as in site_dim_level and in the array qttv_to_array returns.
def dim_sites(dim: int, n_dims: int, bits_per_dim: int, ordering: str) -> List[int]:
    """The 0-based sites that hold the bits of dimension ``dim``, level 0 (the most significant bit) first."""
    return [s for s in range(n_dims * bits_per_dim) if site_dim_level(s, n_dims, bits_per_dim, ordering)[0] == dim]


def reduced_meta(n_dims: int, bits_per_dim: int, ordering: str, keep):
    """Metadata of the train that is left when only the dimensions ``keep`` remain: they keep their relative order, and both orderings
    stay what they are (interleaved: level-major with the kept dimensions in order inside a level; serial: the kept blocks in order)."""
    return len(_keep_list("reduced_meta", keep, n_dims)), int(bits_per_dim), ordering


def _keep_list(who, keep, n_dims):
    keep = [keep] if isinstance(keep, (int, np.integer)) else list(keep)
    out = sorted({int(k) for k in keep})
    if len(out) != len(keep) or any(not 0 <= k < n_dims for k in out):
        raise _lib.TTNError(f"{who}: keep must hold distinct dimensions in 0:{n_dims - 1} (got {tuple(keep)})")
    return out


def _qtt_parts(who, q):
    """(train, (n_dims, bits_per_dim, ordering), resident)"""
    from .device import DeviceTT
    if isinstance(q, QTTvector):
        if _eltype(q.ttv_vec) != "Float64":
            raise _lib.TTNError(f"{who}: Float64 only, a ComplexF64 train is not supported")
        return q.ttvector(), (q.n_dims, q.bits_per_dim, q.ordering), False
    if isinstance(q, tuple) and len(q) == 2 and isinstance(q[0], DeviceTT):
        n_dims, bits, ordering = q[1]
        _check_meta(q[0].N, q[0].dims, int(n_dims), int(bits), ordering, "x")
        if q[0].dtype is not np.float64:
            raise _lib.TTNError(f"{who}: Float64 only, a ComplexF64 handle is not supported")
        return q[0], (int(n_dims), int(bits), ordering), True
    raise TypeError(f"{who}: expected a QTTvector or a pair (DeviceTT, (n_dims, bits_per_dim, ordering)), got {type(q).__name__}")


def _contract(train, meta, vectors, keep, resident):
    """contract the 0-based sites of ``vectors``; the result carries the metadata of the kept dimensions"""
    weights = {s + 1: v for s, v in vectors.items()}
    new_meta = reduced_meta(*meta, keep)
    if resident:
        return train.contract_sites(weights), new_meta
    return QTTvector(_tt.contract_sites(train, weights), *new_meta)


def _contract_all(train, vectors, resident):
    """every site contracted: dot with the rank-1 train of the weights (a float; an array over the batch for a resident batch)"""
    from .device import DeviceTT, dot as dev_dot
    N = train.N
    batch = train.batch if resident else 1
    vs = [np.broadcast_to(np.asarray(vectors[s], dtype=np.float64), (batch, 2)) for s in range(N)]

    def rank1(b):
        return TTvector(N, [np.asfortranarray(vs[s][b].reshape(2, 1, 1)) for s in range(N)], (2,) * N, [1] * (N + 1), [0] * N)

    if not resident:
        return _tt.dot(train, rank1(0))
    w = DeviceTT((2,) * N, [1] * (N + 1), batch)
    try:
        for b in range(batch):
            w.upload(b, rank1(b))
        return dev_dot(train, w)
    finally:
        w.free()


def marginal(q, keep, h=None):
    """Sum out every dimension that is not in ``keep`` (0-based dimensions; an int or a collection): the rectangle rule of the reference's
    examples, ``sum(P, dims = ...) * h`` per summed dimension when ``h`` is given.  The result lives on the kept dimensions, in their
    order, with q's bits_per_dim and ordering.  ``keep=()`` sums everything and returns the number (the mass ``sum(P) * h^n``) through
    dot with the rank-1 train of the weights; keeping every dimension returns a copy."""
    train, meta, resident = _qtt_parts("marginal", q)
    n_dims, bits, ordering = meta
    keep = _keep_list("marginal", keep, n_dims)
    vectors = {}
    for dim in range(n_dims):
        if dim not in keep:
            for level, s in enumerate(dim_sites(dim, *meta)):
                vectors[s] = np.full(2, float(h) if (h is not None and level == 0) else 1.0)
    if not keep:
        return _contract_all(train, vectors, resident)
    if len(keep) == n_dims:
        if not resident:
            return q.copy()
        from .device import DeviceTT
        y = DeviceTT(train.dims, train.cap, train.batch)
        _lib.check(_lib.lib().ttn_tt_copy(y.h, train.h))
        return y, meta
    return _contract(train, meta, vectors, keep, resident)


def slice_dim(q, dim: int, index):
    """Fix dimension ``dim`` at the grid index ``index`` (both 0-based): ``np.take(qttv_to_array(q), index, axis=dim)`` as a train on the
    other dimensions.  The weight of the site that holds level l of ``dim`` is the unit vector of bit ``(index >> (bits - 1 - l)) & 1``
    (level 0 is the most significant bit, site_dim_level).  For a resident batch ``index`` may hold one index per train: B replicas are
    cut at B positions in one launch.  With one dimension the result is the value itself."""
    train, meta, resident = _qtt_parts("slice_dim", q)
    n_dims, bits, ordering = meta
    dim = int(dim)
    if not 0 <= dim < n_dims:
        raise _lib.TTNError(f"slice_dim: dim must be in 0:{n_dims - 1} (got {dim})")
    idx = np.asarray(index)
    if idx.dtype.kind not in "iu" or idx.ndim > 1 or (idx.ndim == 1 and (not resident or idx.shape[0] != train.batch)):
        raise _lib.TTNError("slice_dim: index must be an integer, or one integer per train of a resident batch")
    if np.any(idx < 0) or np.any(idx >= 2 ** bits):
        raise _lib.TTNError(f"slice_dim: index out of 0:{2 ** bits - 1}")
    vectors = {s: np.eye(2)[(idx >> (bits - 1 - level)) & 1] for level, s in enumerate(dim_sites(dim, *meta))}
    if n_dims == 1:
        return _contract_all(train, vectors, resident)
    return _contract(train, meta, vectors, [k for k in range(n_dims) if k != dim], resident)


def _moments_host(m1, m2, mass, a, b, bits, ordering):
    """means, covariance from the 1-d marginals m1[i] and the 2-d marginals m2[i, j] (i < j), all QTTvectors that carry h per summed dimension"""
    from . import constructors as K
    n = len(m1)
    h = (b - a) / (2 ** bits - 1)
    mean, cov = np.zeros(n), np.zeros((n, n))
    for i in range(n):
        mean[i] = _tt.dot(m1[i].ttvector(), K.qtt_polynom([0.0, 1.0], bits, a, b)) * h
    for i in range(n):
        cov[i, i] = _tt.dot(m1[i].ttvector(), K.qtt_polynom([mean[i] ** 2, -2.0 * mean[i], 1.0], bits, a, b)) * h
        for j in range(i + 1, n):
            w = opalg.kron(K.qtt_polynom([-mean[i], 1.0], bits, a, b), K.qtt_polynom([-mean[j], 1.0], bits, a, b))      # serial: dimension i first
            if ordering == "interleaved":
                w = qtt.reorder(w, 2, bits, "interleaved", 0.0)
            cov[i, j] = cov[j, i] = _tt.dot(m2[i, j].ttvector(), w) * h * h
    return mass, mean, cov


def moments(q, a: float, b: float):
    """(mass, mean, cov) of a density sampled on the grid of [a, b]^n, by the formulas of the reference's Ornstein2D example (rectangle
    rule, h = (b - a) / (2^bits - 1); nothing is divided by the mass):
        mass = sum(P) h^n,   mean[i] = sum(x_i P) h^n,   cov[i, j] = sum((x_i - mean[i]) (x_j - mean[j]) P) h^n
    from the one- and two-dimensional marginals and dot with the trains of qtt_polynom (and their kron): nothing dense is formed.
    For a resident batch the marginals are taken for all trains at once and the three results gain a leading batch axis."""
    train, meta, resident = _qtt_parts("moments", q)
    n, bits, ordering = meta
    if bits < 2:
        raise _lib.TTNError("moments: bits_per_dim must be at least 2 (qtt_polynom)")
    a, b = float(a), float(b)
    h = (b - a) / (2 ** bits - 1)
    mass = marginal(q, (), h)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    m1 = [q if n == 1 else marginal(q, (i,), h) for i in range(n)]
    m2 = {(i, j): (q if n == 2 else marginal(q, (i, j), h)) for (i, j) in pairs}
    if not resident:
        return _moments_host(m1, m2, mass, a, b, bits, ordering)
    try:
        out = []
        for t in range(train.batch):
            h1 = [QTTvector(m[0].download(t), *m[1]) for m in m1]
            h2 = {ij: QTTvector(m[0].download(t), *m[1]) for ij, m in m2.items()}
            out.append(_moments_host(h1, h2, float(mass[t]), a, b, bits, ordering))
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])
    finally:
        for m in list(m1) + list(m2.values()):
            if m[0] is not train:
                m[0].free()


# ---- N-d Laplacian ----------------------------------------------------------------------------------------------------------------
def qtt_laplacian(n_dims: int, bits_per_dim: int, ordering: str = "interleaved", a: float = 0.0, b: float = 1.0, bc: str = "DN") -> QTToperator:
    """qtt_laplacian(n_dims, bits_per_dim; ordering, a, b, bc) — src/tt_operators.jl:644-703: the Kronecker sum
    sum_k I ⊗ … ⊗ Δ_k ⊗ … ⊗ I / h² in serial ordering, assembled on operator handles (kron, scale, add), then the operator swap chain
    for the interleaved ordering."""
    from . import constructors as K
    from .device import DeviceTTO
    n_dims, d = int(n_dims), int(bits_per_dim)
    if ordering not in ORDERINGS:
        raise _lib.TTNError("ordering must be :interleaved or :serial")
    if n_dims < 1:
        raise _lib.TTNError("n_dims must be at least 1")
    if bc not in ("DD", "DN", "ND", "NN"):
        raise _lib.TTNError("bc must be :DD, :DN, :ND, or :NN")
    if bc == "NN" and n_dims > 1:
        raise _lib.TTNError("bc=:NN is only supported for n_dims=1 (the Δ_NN MPO has non-unit boundary ranks, which are incompatible "
                            "with the TToperator Kronecker sum)")
    h = (b - a) / (2 ** d - 1)
    scale = 1.0 / h ** 2
    lap_1d = {"DD": K.Delta, "DN": K.Delta_DN, "ND": K.Delta_ND, "NN": K.Delta_NN}[bc](d)
    if bc == "NN":
        # scale * lap_1d on the host (src/tt_operations.jl:271-281: the first core with ot == 0): an operator handle has end ranks 1
        cores = [np.array(c, order="F") for c in lap_1d.tto_vec]
        i = next((k for k, o in enumerate(lap_1d.tto_ot) if o == 0), 0)
        cores[i] = scale * cores[i]
        return QTToperator(TToperator(d, cores, lap_1d.tto_dims, list(lap_1d.tto_rks), list(lap_1d.tto_ot)), 1, d, ordering)
    hs = []
    try:
        lap = DeviceTTO(lap_1d)
        hs.append(lap)
        if n_dims == 1:
            out = lap.scale(scale)
            hs.append(out)
            return QTToperator(out.download(), 1, d, ordering)
        ident = DeviceTTO(K.id_tto(d))
        hs.append(ident)

        def build_term(k):
            term = lap if k == 0 else ident
            for dim in range(1, n_dims):
                term = term.kron(lap if dim == k else ident)
                hs.append(term)
            return term

        result = build_term(0).scale(scale)
        hs.append(result)
        for k in range(1, n_dims):
            term = build_term(k).scale(scale)
            hs.append(term)
            result = result.add(term)
            hs.append(result)
        serial = QTToperator(result.download(), n_dims, d, "serial")
    finally:
        for x in hs:
            x.free()
    if ordering == "serial":
        return serial
    # The reference reorders with threshold = 0, which keeps every singular value of every swap, zeros included: the ranks grow to
    # min(4 r_left, 4 r_right).  Where that growth outruns the swap chain's rank capacity (n² · rank <= 256), only the directions
    # with a singular value below 1e-14 of the largest are dropped, i.e. numerically zero ones: the operator is the same to
    # rounding, its ranks are smaller than the reference's.
    return reorder(serial, "interleaved", 0.0 if _swaps_fit(serial.tto_rks, n_dims, d, qtt.swap_rank_capacity(4)) else 1.0e-14)


def _swaps_fit(rks, n_dims: int, bits_per_dim: int, cap: int) -> bool:
    """whether the serial -> interleaved swap chain with threshold = 0 (new rank = min(4 r_left, 4 r_right) at every swap of a binary
    operator) stays within the rank capacity `cap` of the swap kernel"""
    r = list(rks)
    for k in qtt.bubble_sort_swaps(qtt.reorder_perm(n_dims, bits_per_dim, "interleaved")):
        r[k] = min(4 * r[k - 1], 4 * r[k + 1])
        if r[k] > cap:
            return False
    return True


# ---- entanglement entropy ----------------------------------------------------------------------------------------------------------
def entanglemententropy(psi, base: float = math.e) -> np.ndarray:
    """entanglemententropy(ψ; base) — src/tt_tools.jl:554-587: entry k is the von Neumann entropy of the cut 1:k | k+1:N.

    On the device with existing calls.  A left-to-right ttn_sweep does NOT give the Schmidt spectra: a bond step splits with sqrt(s) on
    both sides and no gauge step, so after the first bond the part left of the merged pair is no longer orthonormal.  Instead, per
    bond k: ttn_orthogonalize to centre k (everything left of k and right of k + 1 orthonormal), then one untruncated
    ttn_bond_truncate(k) with ttn_sv_capture on — the captured spectrum of that merged pair IS the Schmidt spectrum of the cut."""
    from .device import DeviceTT, compress_rank_bound, compress_status
    from .device import orthogonalize as d_orthogonalize
    if not (base > 0 and base != 1):
        raise _lib.TTNError("base must be positive and not equal to 1")
    x = _bare(psi)
    if not isinstance(x, TTvector):
        raise TypeError(f"entanglemententropy: expected a TTvector or a QTTvector, got {type(psi).__name__}")
    N = x.N
    entropy = np.zeros(max(N - 1, 0))
    if N <= 1:
        return entropy
    if any(np.iscomplexobj(c) for c in x.ttv_vec):
        raise TypeError("entanglemententropy: complex trains are not supported (Float64 only)")
    logscale = math.log(base)
    cap = list(x.ttv_rks)
    for k in range(1, N):
        need, _ = compress_rank_bound(x.ttv_dims, x.ttv_rks, 2 ** 62, 1, k)
        cap = [max(c, n) for c, n in zip(cap, need)]
    dx = DeviceTT.from_host(x)
    dy = DeviceTT(x.ttv_dims, cap)
    try:
        dy.capture_singular_values(True)
        for k in range(1, N):
            d_orthogonalize(dx, k, dy)
            _lib.check(_lib.lib().ttn_bond_truncate(dy.h, k, 2 ** 62, 0.0))
            s = dy.singular_values(0, 0)
            compress_status(dy)
            p = s * s
            total = float(p.sum())
            if total > 0:
                p = p / total
                p = p[p > 0]
                entropy[k - 1] = -float(np.sum(p * np.log(p))) / logscale
    finally:
        dx.free()
        dy.free()
    return entropy
