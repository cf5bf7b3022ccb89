"""TT operator algebra with the reference's names, on host containers (the stateless forms next to tt.py's).

    A * B (TToperator), ∙                    src/tt_operations.jl:162-172, :226
    A ⨝ B                                    src/tt_operations.jl:198-216
    +, -, scalar * of TToperators            src/tt_operations.jl:71-95, :271-281, :289-291
    kron / ⊗ (operators and vectors)         src/tt_operations.jl:427-450
    concatenate                              src/tt_tools.jl:708-735
    outer_product, ttv_to_diag_tto           src/tt_operations.jl:297-338
    tto_to_ttv, ttv_to_tto                   src/tt_tools.jl:296-333
    tto_to_tensor, tto_decomp                src/tt_tools.jl:338-392
    qtto_to_matrix                           src/qtt_tools.jl:180-188

Everything that computes uploads its operands, runs the device operation (device.DeviceTTO / DeviceTT, csrc/ttn_opalg_kernels.h) and
downloads the result; a chain of several operations should stay on ``DeviceTTO`` handles instead.  kron, concatenate and the two
conversions only regroup cores (the reference's are ``vcat`` and ``reshape``), so they are host code.  The dense bridge
(tto_to_tensor, qtto_to_matrix, tto_decomp) is one upload, one device call (ttn_tto_to_dense / ttn_tto_decomp_dev) and one download.
Float64 only.
"""
from __future__ import annotations

import math

import numpy as np

from .tt import TToperator, TTvector


def _need(x, kind, who):
    if not isinstance(x, kind):
        raise TypeError(f"{who}: expected a {kind.__name__}, got {type(x).__name__}")
    vec = x.tto_vec if kind is TToperator else x.ttv_vec
    if any(np.iscomplexobj(c) for c in vec):
        raise TypeError(f"{who}: complex cores are not supported (Float64 only)")


def _run(fn, *operands):
    """Upload, run fn on the device handles, download, release."""
    from .device import DeviceTT, DeviceTTO
    hs, out = [], None
    try:
        for x in operands:
            hs.append(DeviceTTO(x) if isinstance(x, TToperator) else DeviceTT.from_host(x))
        out = fn(*hs)
        return out.download()
    finally:
        for h in hs + ([out] if out is not None else []):
            h.free()


def tto_mul(A: TToperator, B: TToperator) -> TToperator:
    """*(A::TToperator, B::TToperator) — src/tt_operations.jl:162-172."""
    _need(A, TToperator, "tto_mul"), _need(B, TToperator, "tto_mul")
    assert tuple(A.tto_dims) == tuple(B.tto_dims), "Incompatible dimensions"
    return _run(lambda a, b: a.mul(b), A, B)


def tto_inner(A: TToperator, B: TToperator) -> TToperator:
    """A ⨝ B — src/tt_operations.jl:198-216."""
    _need(A, TToperator, "tto_inner"), _need(B, TToperator, "tto_inner")
    assert A.N == B.N, "Inner core product requires operators with the same number of cores"
    return _run(lambda a, b: a.inner(b), A, B)


def tto_add(A: TToperator, B: TToperator) -> TToperator:
    """+(x::TToperator, y::TToperator) — src/tt_operations.jl:71-95."""
    _need(A, TToperator, "tto_add"), _need(B, TToperator, "tto_add")
    assert tuple(A.tto_dims) == tuple(B.tto_dims), "Incompatible dimensions"
    return _run(lambda a, b: a.add(b), A, B)


def tto_scale(a: float, A: TToperator) -> TToperator:
    """*(a::Number, A::TToperator) — src/tt_operations.jl:271-281."""
    _need(A, TToperator, "tto_scale")
    if isinstance(a, complex):
        raise TypeError("tto_scale: complex factors are not supported (Float64 only)")
    return _run(lambda h: h.scale(float(a)), A)


def tto_sub(A: TToperator, B: TToperator) -> TToperator:
    """-(A::TToperator, B::TToperator) = (-1.0 * B) + A — src/tt_operations.jl:289-291."""
    _need(A, TToperator, "tto_sub"), _need(B, TToperator, "tto_sub")
    assert tuple(A.tto_dims) == tuple(B.tto_dims), "Incompatible dimensions"
    return _run(lambda a, b: a.sub(b), A, B)


def outer_product(x: TTvector, y: TTvector) -> TToperator:
    """outer_product(x, y) — src/tt_operations.jl:297-304."""
    _need(x, TTvector, "outer_product"), _need(y, TTvector, "outer_product")
    assert tuple(x.ttv_dims) == tuple(y.ttv_dims), "Incompatible dimensions"
    return _run(lambda a, b: a.outer(b), x, y)


def ttv_to_diag_tto(x: TTvector) -> TToperator:
    """ttv_to_diag_tto(x) — src/tt_operations.jl:310-338."""
    _need(x, TTvector, "ttv_to_diag_tto")
    return _run(lambda a: a.diag_tto(), x)


def tto_compress_(A: TToperator, max_bond: int = 2 ** 62, truncerr: float = 0.0, sweeps: int = 1) -> TToperator:
    """ttv_to_tto(tt_compress!(tto_to_ttv(A), max_bond; truncerr, sweeps)); A's fields are rebound to the result, which is returned."""
    _need(A, TToperator, "tto_compress_")
    assert sweeps >= 1, "sweeps must be >= 1"
    B = _run(lambda a: a.compress(max_bond, truncerr, sweeps), A)
    A.tto_vec, A.tto_rks, A.tto_ot = B.tto_vec, B.tto_rks, B.tto_ot
    return A


# ---- regrouping of cores: host code, like the reference's vcat / reshape ----------------------------------------------------------
def concatenate(a, b):
    """concatenate(tt1, tt2) — src/tt_tools.jl:708-735: the cores of b behind those of a; the ranks at the joint must agree."""
    if isinstance(a, TToperator) and isinstance(b, TToperator):
        if a.tto_rks[-1] != b.tto_rks[0]:
            raise ValueError("The final rank of the first TToperator must equal the initial rank of the second TToperator.")
        return TToperator(a.N + b.N, [np.asfortranarray(c) for c in a.tto_vec + b.tto_vec], tuple(a.tto_dims) + tuple(b.tto_dims),
                          list(a.tto_rks[:-1]) + list(b.tto_rks), list(a.tto_ot) + list(b.tto_ot))
    if isinstance(a, TTvector) and isinstance(b, TTvector):
        if a.ttv_rks[-1] != b.ttv_rks[0]:
            raise ValueError("The final rank of the first TTvector must equal the initial rank of the second TTvector.")
        return TTvector(a.N + b.N, [np.asfortranarray(c) for c in a.ttv_vec + b.ttv_vec], tuple(a.ttv_dims) + tuple(b.ttv_dims),
                        list(a.ttv_rks[:-1]) + list(b.ttv_rks), list(a.ttv_ot) + list(b.ttv_ot))
    raise TypeError("concatenate: expected two TToperators or two TTvectors")


def kron(a, b):
    """kron(A, B) / A ⊗ B for two operators or two vectors — src/tt_operations.jl:427-450 (the same regrouping as concatenate; the
    reference does not check the ranks at the joint, which are 1 for complete trains)."""
    if not ((isinstance(a, TToperator) and isinstance(b, TToperator)) or (isinstance(a, TTvector) and isinstance(b, TTvector))):
        raise TypeError("kron: expected two TToperators or two TTvectors")
    return concatenate(a, b)


def tto_to_ttv(A: TToperator) -> TTvector:
    """tto_to_ttv(A) — src/tt_tools.jl:296-304."""
    _need(A, TToperator, "tto_to_ttv")
    vec = [np.reshape(np.asfortranarray(c), (A.tto_dims[k] ** 2, A.tto_rks[k], A.tto_rks[k + 1]), order="F") for k, c in enumerate(A.tto_vec)]
    return TTvector(A.N, vec, tuple(n * n for n in A.tto_dims), list(A.tto_rks), list(A.tto_ot))


def ttv_to_tto(x: TTvector) -> TToperator:
    """ttv_to_tto(x) — src/tt_tools.jl:323-333; dimensions that are not perfect squares are refused."""
    _need(x, TTvector, "ttv_to_tto")
    dims = tuple(math.isqrt(n) for n in x.ttv_dims)
    assert tuple(n * n for n in dims) == tuple(x.ttv_dims), "DimensionMismatch"
    vec = [np.reshape(np.asfortranarray(c), (dims[k], dims[k], x.ttv_rks[k], x.ttv_rks[k + 1]), order="F") for k, c in enumerate(x.ttv_vec)]
    return TToperator(x.N, vec, dims, list(x.ttv_rks), list(x.ttv_ot))


# ---- the dense bridge: operator <-> dense array (include/ttn_dense.h) -------------------------------------------------------------------
def operator_strides(dims, layout="tensor"):
    """(xstrides, ystrides) of an operator's dense array: entry (x_1..x_d ; y_1..y_d), 0-based, lies at
    sum_k x_k xstrides[k] + y_k ystrides[k].  ``"tensor"``: tto_to_tensor's array, column-major over [x_1..x_d, y_1..y_d].
    ``"matrix"``: qtto_to_matrix's matrix, column-major N x N with row = sum_k x_k prod_{j>k} n_j (site 1 most significant) and the
    same for the column.  A pair of tables is checked (the digits must form a mixed-radix system) and returned as lists."""
    dims = [int(n) for n in dims]
    d = len(dims)
    N = math.prod(dims)
    if isinstance(layout, str):
        if layout == "tensor":
            xs = [math.prod(dims[:k]) for k in range(d)]
        elif layout == "matrix":
            xs = [math.prod(dims[k + 1:]) for k in range(d)]
        else:
            raise ValueError(f"operator_strides: layout must be 'tensor', 'matrix' or a (xstrides, ystrides) pair, got {layout!r}")
        return xs, [N * s for s in xs]
    try:
        xs, ys = layout
        xs, ys = [int(v) for v in xs], [int(v) for v in ys]
    except (TypeError, ValueError):
        raise ValueError("operator_strides: layout must be 'tensor', 'matrix' or a (xstrides, ystrides) pair") from None
    if len(xs) != d or len(ys) != d:
        raise ValueError(f"operator_strides: {len(xs)} and {len(ys)} strides for {d} sites")
    expect = 1
    for stride, n in sorted((s, n) for s, n in zip(xs + ys, dims + dims) if n > 1):
        if stride != expect:
            raise ValueError("operator_strides: the strides are not a mixed-radix system (smallest 1, each next = previous * its n)")
        expect *= n
    return xs, ys


def _need_square(A, who):
    _need(A, TToperator, who)
    for k, c in enumerate(A.tto_vec):
        if np.ndim(c) != 4 or c.shape[0] != c.shape[1]:
            raise TypeError(f"{who}: core {k + 1} has shape {np.shape(c)}; a rectangular operator has no dense form here (square cores only)")


def tto_to_tensor(A: TToperator) -> np.ndarray:
    """tto_to_tensor(A) — src/tt_tools.jl:375-392: the array of shape dims + dims, contracted on the device (ttn_tto_to_dense)."""
    from .device import DeviceTTO
    _need_square(A, "tto_to_tensor")
    h = DeviceTTO(A)
    try:
        return np.reshape(h.to_dense("tensor").cpu().numpy(), tuple(A.tto_dims) * 2, order="F")
    finally:
        h.free()


def qtto_to_matrix(A: TToperator, device: bool = False):
    """qtto_to_matrix(A) — src/qtt_tools.jl:180-188: the (2^d, 2^d) matrix with site 1 the most significant bit of row and column.
    One ttn_tto_to_dense in the matrix layout; ``device=True`` returns the torch tensor (a view with the same logical indexing)."""
    from .device import DeviceTTO
    _need_square(A, "qtto_to_matrix")
    assert all(n == 2 for n in A.tto_dims), "qtto_to_matrix: all dimensions must be 2"
    N = 2 ** A.N
    h = DeviceTTO(A)
    try:
        flat = h.to_dense("matrix")
        if device:
            return flat.reshape(N, N).T                      # column-major in memory
        return np.reshape(flat.cpu().numpy(), (N, N), order="F")
    finally:
        h.free()


def tto_decomp(tensor, index: int = 1, tol: float = 1.0e-12, rank_cap: int = 1024) -> TToperator:
    """tto_decomp(tensor; index) — src/tt_tools.jl:338-362, with ttv_decomp's absolute threshold ``tol`` exposed: the TT operator of the
    array tensor[x_1..x_d, y_1..y_d], decomposed on the device (ttn_tto_decomp_dev) with the root at site ``index``."""
    from .device import DeviceTTO
    from .tdvp import _dev
    t = np.asarray(tensor)
    if np.iscomplexobj(t):
        raise TypeError("tto_decomp: complex tensors are not supported (Float64 only)")
    assert t.ndim >= 2 and t.ndim % 2 == 0, "tto_decomp: the tensor needs an even number of axes [x_1..x_d, y_1..y_d]"
    d = t.ndim // 2
    assert t.shape[:d] == t.shape[d:], "tto_decomp: the x and y dimensions differ"
    assert 1 <= int(index) <= d, "tto_decomp: index must be in 1:d"
    torch, stream = _dev()
    flat = np.ascontiguousarray(np.ravel(np.asarray(t, dtype=np.float64), order="F"))
    with torch.cuda.stream(stream):
        dt = torch.from_numpy(flat).to("cuda")
    h = DeviceTTO.from_dense(dt, t.shape[:d], index=index, tol=tol, layout="tensor", rank_cap=rank_cap)
    try:
        return h.download()
    finally:
        h.free()
