"""Device-resident batches of trains (the handle half of include/ttn.h).

``DeviceTT`` wraps a ``ttn_tt`` handle: ``batch`` independent TT vectors with common dims and a
per-bond rank capacity, resident in HBM.  ``DeviceTTO`` wraps one TT operator, ``DeviceRectTTO`` one
rectangular operator (grid transfer: one more site than the trains it is applied to).  Chains such as
``tt_compress!(A*x, r)`` then never cross PCIe.  All ops are asynchronous on the
library's HIP stream.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import _lib
from .tt import TToperator, TTvector, _f, _i64, _is_cplx, _ptrs, _z


class DeviceTTO:
    """One TT operator in HBM (``ttn_tto``): immutable, ranks known on the host.  The algebra below (csrc/ttn_opalg_kernels.h) returns a
    NEW ``DeviceTTO`` from every call and never crosses PCIe; ``download()`` brings the cores back.  ``batch`` > 1: an operator batch
    (``stack`` / ``from_tt_batch`` / ``lincomb``), one operator per train of the trains it meets."""

    def __init__(self, A: TToperator):
        _lib.ensure_init()
        self.dims = tuple(A.tto_dims)
        self.rks = list(A.tto_rks)
        self.ot = [int(o) for o in A.tto_ot]
        self.N = A.N
        self.dtype = np.complex128 if _is_cplx(A.tto_vec) else np.float64          # the element type comes from the cores
        h = C.c_void_p()
        if self.dtype is np.complex128:
            cores = [_z(c) for c in A.tto_vec]
            _lib.check(_lib.lib().ttn_tto_create_c64(A.N, _i64(A.tto_dims), _i64(A.tto_rks), _ptrs(cores), C.byref(h)))
        else:
            cores = [_f(c) for c in A.tto_vec]
            _lib.check(_lib.lib().ttn_tto_create(A.N, _i64(A.tto_dims), _i64(A.tto_rks), _ptrs(cores), C.byref(h)))
        self.h = h
        self.batch = 1
        if any(self.ot):
            _lib.check(_lib.lib().ttn_tto_set_ot(self.h, _i64(self.ot)))

    # operator batches (include/ttn_opbatch.h): B operators of equal dims and ranks in one handle, operator b for train b
    @classmethod
    def stack(cls, ops: Sequence[TToperator]) -> "DeviceTTO":
        """A batch of host operators of equal dims and ranks in ONE handle (``ttn_tto_create_batch``): ``apply``, ``apply_axpby``,
        ``sandwich`` / ``expect`` / ``rayleigh``, ``grad.sandwich_pullback``, ``dmrg_eigsolve_`` and ``mals_eigsolve_`` then use operator b
        for train b; every other function refuses the handle (``select(b)`` gives it one operator).  Float64 only; gauge flags: zeros."""
        ops = list(ops)
        if not ops:
            raise _lib.TTNError("stack: an operator batch needs at least one operator")
        A0 = ops[0]
        for b, A in enumerate(ops):
            if _is_cplx(A.tto_vec):
                raise _lib.TTNError(f"stack: operator {b} is complex; an operator batch is Float64 only")
            if tuple(A.tto_dims) != tuple(A0.tto_dims) or A.N != A0.N:
                raise _lib.TTNError(f"stack: the dims of operator {b} differ from those of operator 0; an operator batch holds equal dims")
            if list(A.tto_rks) != list(A0.tto_rks):
                raise _lib.TTNError(f"stack: the ranks of operator {b} differ from those of operator 0; an operator batch holds equal ranks")
        _lib.ensure_init()
        cores = [_f(c) for A in ops for c in A.tto_vec]
        h = C.c_void_p()
        _lib.check(_lib.lib().ttn_tto_create_batch(A0.N, _i64(A0.tto_dims), _i64(A0.tto_rks), len(ops), _ptrs(cores), C.byref(h)))
        return cls._adopt(h)

    @classmethod
    def from_tt_batch(cls, x: "DeviceTT") -> "DeviceTTO":
        """ttv_to_tto of EVERY train of x (dims n_k^2) as one operator batch, on the device (``ttn_tto_from_tt_batch``, one packing
        launch).  The trains must hold equal ranks (``TTNError`` otherwise).  Synchronises to read them."""
        h = C.c_void_p()
        rc = _lib.lib().ttn_tto_from_tt_batch(x.h, C.byref(h))
        if rc:                      # (no assert of the reference stands behind this call: every refusal is a TTNError)
            raise _lib.TTNError(f"ttn error {rc}: {_lib.last_error()}")
        return cls._adopt(h)

    @classmethod
    def lincomb(cls, terms: Sequence["DeviceTTO"], coeffs) -> "DeviceTTO":
        """The operator batch H_b = sum_j coeffs[b, j] * terms[j], assembled on the device: ``to_tt(B)`` -> ``scale_batch`` -> ``add`` ->
        ``from_tt_batch``.  ``coeffs``: (B, J) real numbers.  The ranks are the sums of the terms' ranks, as for ``+`` (nothing is rounded)."""
        terms = list(terms)
        if not terms:
            raise _lib.TTNError("lincomb: no terms")
        for j, T in enumerate(terms):
            if not isinstance(T, DeviceTTO):
                raise TypeError(f"lincomb: term {j} is a {type(T).__name__}, expected a DeviceTTO")
        c = np.asarray(coeffs, dtype=np.float64)
        if c.ndim != 2 or c.shape[1] != len(terms) or c.shape[0] < 1:
            raise _lib.TTNError(f"lincomb: coeffs of shape {c.shape} for {len(terms)} terms (need (B, {len(terms)}) with B >= 1)")
        for j, T in enumerate(terms):
            if T.dims != terms[0].dims:
                raise _lib.TTNError(f"lincomb: the dims of term {j} differ from those of term 0")
            if T.dtype is np.complex128:
                raise _lib.TTNError(f"lincomb: term {j} is complex; an operator batch is Float64 only")
        B, N = int(c.shape[0]), terms[0].N
        dims2 = [n * n for n in terms[0].dims]
        acc = None
        for j, T in enumerate(terms):
            t = T.to_tt(B)                                   # (a term that is itself a batch is refused here)
            s = DeviceTT(dims2, T.rks, B)
            scale_batch(c[:, j], t, s)
            t.free()
            if acc is None:
                acc = s
                continue
            rks = [1] + [acc.cap[m] + s.cap[m] for m in range(1, N)] + [1]
            z = add(acc, s, DeviceTT(dims2, rks, B))
            acc.free()
            s.free()
            acc = z
        out = cls.from_tt_batch(acc)
        acc.free()
        return out

    def select(self, b: int) -> "DeviceTTO":
        """Operator b of the batch as a single ``DeviceTTO`` (one device copy)."""
        h = C.c_void_p()
        _lib.check(_lib.lib().ttn_tto_select(self.h, int(b), C.byref(h)))
        return DeviceTTO._adopt(h)

    @classmethod
    def _adopt(cls, h: C.c_void_p) -> "DeviceTTO":
        """Wrap a handle an operation of the library returned (dims, ranks and gauge flags are read from it)."""
        if not h:
            raise _lib.TTNError("the library returned no operator handle")
        self = cls.__new__(cls)
        self.h = h
        L = _lib.lib()
        d = C.c_int64(0)
        _lib.check(L.ttn_tto_ranks(h, C.byref(d), None, None, None))
        self.N = int(d.value)
        dims, rks, ot = (C.c_int64 * self.N)(), (C.c_int64 * (self.N + 1))(), (C.c_int64 * self.N)()
        _lib.check(L.ttn_tto_ranks(h, None, dims, rks, ot))
        self.dims, self.rks, self.ot = tuple(int(v) for v in dims), [int(v) for v in rks], [int(v) for v in ot]
        cplx = C.c_int(0)
        _lib.check(L.ttn_tto_dtype(h, C.byref(cplx)))
        self.dtype = np.complex128 if cplx.value else np.float64
        nb = C.c_int64(0)
        _lib.check(L.ttn_tto_batch(h, C.byref(nb)))
        self.batch = int(nb.value)
        return self

    def _binary(self, name: str, other: "DeviceTTO") -> "DeviceTTO":
        if not isinstance(other, DeviceTTO):
            raise TypeError(f"{name}: expected a DeviceTTO, got {type(other).__name__}")
        h = C.c_void_p()
        _lib.check(getattr(_lib.lib(), name)(self.h, other.h, C.byref(h)))
        return DeviceTTO._adopt(h)

    def mul(self, B: "DeviceTTO") -> "DeviceTTO":
        """A * B — src/tt_operations.jl:162-172 (ranks multiply)."""
        return self._binary("ttn_tto_mul", B)

    def inner(self, B: "DeviceTTO") -> "DeviceTTO":
        """A ⨝ B, the inner core product — src/tt_operations.jl:198-216 (dims and ranks multiply)."""
        return self._binary("ttn_tto_inner", B)

    def add(self, B: "DeviceTTO") -> "DeviceTTO":
        """A + B — src/tt_operations.jl:71-95 (ranks add, d >= 2)."""
        return self._binary("ttn_tto_add", B)

    def scale(self, a: float) -> "DeviceTTO":
        """a * A — src/tt_operations.jl:271-281."""
        h = C.c_void_p()
        _lib.check(_lib.lib().ttn_tto_scale(float(a), self.h, C.byref(h)))
        return DeviceTTO._adopt(h)

    def sub(self, B: "DeviceTTO") -> "DeviceTTO":
        """A - B = (-1.0 * B) + A, in that order — src/tt_operations.jl:289-291."""
        if not isinstance(B, DeviceTTO):
            raise TypeError(f"sub: expected a DeviceTTO, got {type(B).__name__}")
        return B.scale(-1.0).add(self)

    def kron(self, B: "DeviceTTO") -> "DeviceTTO":
        """kron(A, B) / A ⊗ B — src/tt_operations.jl:427-435; with equal ranks at the joint also concatenate(A, B),
        src/tt_tools.jl:723-735."""
        return self._binary("ttn_tto_kron", B)

    def to_tt(self, batch: int = 1, cap_rks: Sequence[int] | None = None) -> "DeviceTT":
        """tto_to_ttv(A) in every train of a new batch — src/tt_tools.jl:296-304."""
        y = DeviceTT([n * n for n in self.dims], cap_rks if cap_rks is not None else self.rks, batch)
        _lib.check(_lib.lib().ttn_tto_to_tt(self.h, y.h))
        return y

    @classmethod
    def from_tt(cls, x: "DeviceTT", b: int = 0) -> "DeviceTTO":
        """ttv_to_tto of train b with its current ranks — src/tt_tools.jl:323-333."""
        h = C.c_void_p()
        _lib.check(_lib.lib().ttn_tto_from_tt(x.h, int(b), C.byref(h)))
        return cls._adopt(h)

    def compress(self, max_bond: int = 2 ** 62, truncerr: float = 0.0, sweeps: int = 1) -> "DeviceTTO":
        """ttv_to_tto(tt_compress!(tto_to_ttv(A), max_bond; truncerr, sweeps)) without leaving the device."""
        assert sweeps >= 1, "sweeps must be >= 1"
        h = C.c_void_p()
        _lib.check(_lib.lib().ttn_tto_compress(self.h, int(min(max_bond, 2 ** 62)), float(truncerr), int(sweeps), C.byref(h)))
        return DeviceTTO._adopt(h)

    # operator <-> dense array (include/ttn_dense.h)
    def to_dense(self, layout="tensor"):
        """The operator as a dense array on the device: a 1-D float64 torch tensor of prod(dims)^2 entries.  ``layout="tensor"`` is
        tto_to_tensor's array (column-major over [x_1..x_d, y_1..y_d]), ``"matrix"`` is qtto_to_matrix's column-major matrix (site 1 most
        significant), or a ``(xstrides, ystrides)`` pair (opalg.operator_strides).  Asynchronous like ``DeviceTT.to_dense``."""
        from .opalg import operator_strides
        from .tdvp import _dev
        torch, stream = _dev()
        xs, ys = operator_strides(self.dims, layout)
        total = 1
        for n in self.dims:
            total *= n * n
        caller = torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            out = torch.empty((total,), dtype=torch.float64, device="cuda")
            _lib.check(_lib.lib().ttn_tto_to_dense(self.h, _i64(xs), _i64(ys), C.c_void_p(out.data_ptr())))
        if caller != stream:
            caller.wait_stream(stream)
            out.record_stream(caller)
        return out

    @classmethod
    def from_dense(cls, d_tensor, dims: Sequence[int], index: int = 1, tol: float = 1.0e-12, layout="tensor", rank_cap: int = 1024) -> "DeviceTTO":
        """tto_decomp of a dense array on the device — src/tt_tools.jl:338-362: ``d_tensor`` is a float64 CUDA tensor of prod(dims)^2
        entries in ``layout`` (see ``to_dense``), only read; ranks above ``rank_cap`` raise (TTN_ERR_CAPACITY).  Synchronises."""
        from .opalg import operator_strides
        from .tdvp import _dev
        _lib.ensure_init()
        torch, stream = _dev()
        dims = [int(n) for n in dims]
        xs, ys = operator_strides(dims, layout)
        total = 1
        for n in dims:
            total *= n * n
        if not isinstance(d_tensor, torch.Tensor) or not d_tensor.is_cuda:
            raise _lib.TTNError("from_dense: expected a CUDA tensor (upload a host array first)")
        if d_tensor.is_complex():
            raise TypeError("from_dense: complex tensors are not supported (Float64 only)")
        if d_tensor.dtype != torch.float64 or not d_tensor.is_contiguous():
            raise _lib.TTNError("from_dense: expected a contiguous float64 tensor")
        if d_tensor.numel() != total:
            raise _lib.TTNError(f"from_dense: {d_tensor.numel()} entries for dims {tuple(dims)} (need {total})")
        stream.wait_stream(torch.cuda.current_stream())
        h = C.c_void_p()
        _lib.check(_lib.lib().ttn_tto_decomp_dev(len(dims), _i64(dims), C.c_void_p(d_tensor.data_ptr()), _i64(xs), _i64(ys), int(index), float(tol),
                                                 int(min(rank_cap, 2 ** 62)), C.byref(h)))
        return cls._adopt(h)

    def ranks(self) -> List[int]:
        return list(self.rks)

    def download(self, b: int = 0) -> TToperator:
        """The cores on the host; of an operator batch, those of operator b."""
        cores = [np.zeros((self.dims[k], self.dims[k], self.rks[k], self.rks[k + 1]), order="F", dtype=self.dtype) for k in range(self.N)]
        _lib.check(_lib.lib().ttn_tto_download_b(self.h, int(b), _ptrs(cores)))
        return TToperator(self.N, cores, self.dims, list(self.rks), list(self.ot))

    def free(self):
        if self.h:
            _lib.lib().ttn_tto_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceRectTTO:
    """One rectangular TT operator in HBM (``ttn_rtto``, include/ttn_rect.h): cores (n_out, n_in, R_l, R_r), exactly one site with
    n_in == 1 when it is applied (``apply_rect``).  Float64 only, immutable.  A handle type of its own: ``apply`` and the operator
    algebra do not take it."""

    def __init__(self, A: TToperator):
        _lib.ensure_init()
        cores = [_f(c) for c in A.tto_vec]                    # (a complex core: TypeError)
        for k, c in enumerate(cores):
            if c.ndim != 4 or c.shape[2:] != (A.tto_rks[k], A.tto_rks[k + 1]):
                raise _lib.TTNError(f"DeviceRectTTO: core {k + 1} has shape {c.shape}, its ranks are {A.tto_rks[k]}, {A.tto_rks[k + 1]}")
        self.N = A.N
        self.dims = tuple(int(c.shape[0]) for c in cores)      # output dimensions (tto_dims)
        self.in_dims = tuple(int(c.shape[1]) for c in cores)
        self.rks = list(A.tto_rks)
        h = C.c_void_p()
        _lib.check(_lib.lib().ttn_rtto_create(A.N, _i64(self.dims), _i64(self.in_dims), _i64(self.rks), _ptrs(cores), C.byref(h)))
        self.h = h

    def ranks(self) -> List[int]:
        """The operator's ranks as the library holds them (ttn_rtto_ranks)."""
        rks = (C.c_int64 * (self.N + 1))()
        _lib.check(_lib.lib().ttn_rtto_ranks(self.h, None, None, None, rks))
        return [int(v) for v in rks]

    def singleton_sites(self) -> List[int]:
        """1-based sites with a singleton input index; ``apply_rect`` needs exactly one."""
        return [k + 1 for k, n in enumerate(self.in_dims) if n == 1]

    def free(self):
        if self.h:
            _lib.lib().ttn_rtto_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceTT:
    """``batch`` trains in HBM (``ttn_tt``).  ``dtype``: ``np.float64`` or ``np.complex128`` — fixed at creation; a complex handle holds
    the cores interleaved (re, im), as Julia's ``Array{ComplexF64,3}`` lies in memory."""

    def __init__(self, dims: Sequence[int], cap_rks: Sequence[int], batch: int = 1, dtype=np.float64):
        _lib.ensure_init()
        if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.complex128)):
            raise TypeError(f"DeviceTT: dtype must be float64 or complex128, got {np.dtype(dtype)}")
        self.dtype = np.complex128 if np.dtype(dtype) == np.dtype(np.complex128) else np.float64
        self.dims = tuple(int(v) for v in dims)
        self.cap = [int(r) for r in cap_rks]
        self.N = len(self.dims)
        self.batch = int(batch)
        h = C.c_void_p()
        create = _lib.lib().ttn_tt_create_c64 if self.dtype is np.complex128 else _lib.lib().ttn_tt_create
        _lib.check(create(self.N, _i64(self.dims), _i64(self.cap), self.batch, C.byref(h)))
        self.h = h

    @classmethod
    def from_host(cls, x: TTvector, batch: int = 1, cap_rks: Sequence[int] | None = None) -> "DeviceTT":
        """Upload x as train 0 and replicate it over the batch.  The element type is that of x's cores."""
        t = cls(x.ttv_dims, cap_rks if cap_rks is not None else x.ttv_rks, batch, dtype=np.complex128 if _is_cplx(x.ttv_vec) else np.float64)
        t.upload(0, x)
        if batch > 1:
            t.replicate(0)
        return t

    def upload(self, b: int, x: TTvector) -> None:
        # (a real train into a complex handle is promoted on the host; a complex train into a real handle is refused by _f)
        cores = [(_z if self.dtype is np.complex128 else _f)(c) for c in x.ttv_vec]
        _lib.check(_lib.lib().ttn_tt_upload(self.h, int(b), _ptrs(cores), _i64(x.ttv_rks), _i64(x.ttv_ot)))

    def replicate(self, src: int = 0) -> None:
        _lib.check(_lib.lib().ttn_tt_replicate(self.h, int(src)))

    def ranks(self, b: int = 0):
        rks = (C.c_int64 * (self.N + 1))()
        ot = (C.c_int64 * self.N)()
        _lib.check(_lib.lib().ttn_tt_ranks(self.h, int(b), rks, ot))
        return [int(v) for v in rks], [int(v) for v in ot]

    def max_ranks(self):
        """Per-bond maximum of the current ranks over the batch (synchronises; also tightens the library's host-side
        rank bounds)."""
        out = (C.c_int64 * (self.N + 1))()
        _lib.check(_lib.lib().ttn_tt_max_ranks(self.h, out))
        return [int(v) for v in out]

    def download(self, b: int = 0) -> TTvector:
        rks, ot = self.ranks(b)
        cores = [np.zeros((self.dims[k], rks[k], rks[k + 1]), order="F", dtype=self.dtype) for k in range(self.N)]
        _lib.check(_lib.lib().ttn_tt_download(self.h, int(b), _ptrs(cores)))
        return TTvector(self.N, cores, self.dims, rks, ot)

    # operator algebra (csrc/ttn_opalg_kernels.h)
    def kron(self, y: "DeviceTT", cap_rks: Sequence[int] | None = None) -> "DeviceTT":
        """kron(x, y) / x ⊗ y train by train — src/tt_operations.jl:440-450."""
        if not isinstance(y, DeviceTT):
            raise TypeError(f"kron: expected a DeviceTT, got {type(y).__name__}")
        z = DeviceTT(self.dims + y.dims, cap_rks if cap_rks is not None else self.cap[:-1] + y.cap, self.batch)
        _lib.check(_lib.lib().ttn_tt_kron(self.h, y.h, z.h))
        return z

    def outer(self, y: "DeviceTT", b: int = 0) -> DeviceTTO:
        """outer_product(x_b, y_b) — src/tt_operations.jl:297-304."""
        if not isinstance(y, DeviceTT):
            raise TypeError(f"outer: expected a DeviceTT, got {type(y).__name__}")
        h = C.c_void_p()
        _lib.check(_lib.lib().ttn_tt_outer(self.h, y.h, int(b), C.byref(h)))
        return DeviceTTO._adopt(h)

    def diag_tto(self, b: int = 0) -> DeviceTTO:
        """ttv_to_diag_tto(x_b) — src/tt_operations.jl:310-338."""
        h = C.c_void_p()
        _lib.check(_lib.lib().ttn_tt_diag_tto(self.h, int(b), C.byref(h)))
        return DeviceTTO._adopt(h)

    # split / merge sites (csrc/ttn_resite_kernels.h)
    def split_sites(self, split_dims: Sequence[Sequence[int]], threshold: float = 0.0, cap_rks: Sequence[int] | None = None) -> "DeviceTT":
        """to_qtt(x, split_dims; threshold) train by train — src/qtt_tools.jl:254-310: site i becomes len(split_dims[i]) sites, the first
        factor the most significant digit.  Default capacity: the exact bound min(rows, cols) of every SVD, propagated from ``self.cap``.
        Asynchronous; a rank above ``cap_rks`` shows in ``compress_status`` of the result."""
        sd = [[int(v) for v in s] for s in split_dims]
        if len(sd) != self.N or any(len(s) < 1 for s in sd):
            raise _lib.TTNError(f"split_sites: {len(sd)} factor lists for {self.N} sites (every site needs a non-empty list)")
        flat = [v for s in sd for v in s]
        if cap_rks is None:
            cap_rks = split_rank_capacity(self.dims, self.cap, sd)
        z = DeviceTT(flat, cap_rks, self.batch, dtype=self.dtype)
        _lib.check(_lib.lib().ttn_tt_split_sites(self.h, z.h, _i64([len(s) for s in sd]), _i64(flat), float(threshold)))
        return z

    def merge_sites(self, merge_numbers: Sequence[int], cap_rks: Sequence[int] | None = None) -> "DeviceTT":
        """to_ttv(x, merge_numbers) train by train — src/qtt_tools.jl:323-360: every run of merge_numbers[g] consecutive cores becomes one
        core, physical indices merged big-endian.  Default capacity: ``self.cap`` at the kept bonds.  Asynchronous."""
        mn = [int(c) for c in merge_numbers]
        if not mn or any(c < 1 for c in mn) or sum(mn) != self.N:
            raise _lib.TTNError(f"merge_sites: merge_numbers {mn} must be positive and sum to {self.N} (the number of sites)")
        first = [sum(mn[:g]) for g in range(len(mn) + 1)]
        dims = []
        for g, c in enumerate(mn):
            n = 1
            for k in range(first[g], first[g] + c):
                n *= self.dims[k]
            dims.append(n)
        if cap_rks is None:
            cap_rks = [self.cap[k] for k in first]
        z = DeviceTT(dims, cap_rks, self.batch, dtype=self.dtype)
        _lib.check(_lib.lib().ttn_tt_merge_sites(self.h, z.h, _i64(mn), len(mn)))
        return z

    # partial contraction (include/ttn_contract.h)
    def contract_sites(self, weights, cap_rks: Sequence[int] | None = None) -> "DeviceTT":
        """``contract_sites(self, weights)`` into a NEW handle on the kept sites; ``cap_rks``: its rank capacity (default: this handle's
        capacity at the bonds the result keeps, ``contract_rank_capacity``)."""
        sites, _, _ = _contract_tables("contract_sites", self.dims, self.batch, weights)
        kept, _ = contract_kept(self.N, sites)
        y = DeviceTT([self.dims[k] for k in kept], cap_rks if cap_rks is not None else contract_rank_capacity(self.cap, sites), self.batch)
        try:
            return contract_sites(self, weights, y)
        except Exception:
            y.free()
            raise

    # increase_ranks (include/ttn_step.h)
    def increase_ranks(self, max_bond: int, rks: Sequence[int] | None = None, noise: float = 0.0, seed: int = 0,
                       cap_rks: Sequence[int] | None = None) -> "DeviceTT":
        """increase_ranks(x, max_bond; rks, noise) train by train — src/tt_tools.jl:480-490: a NEW handle with every core zero-padded to
        ``r_and_d_to_rks(rks, dims; rmax=max_bond)`` (``rks`` defaults to [1, max_bond, ..., 1]); with ``noise != 0`` the new blocks hold
        noise * Q, Q orthonormal from the seeded splitmix64 stream of als_eigsolve (not Julia's RNG).  Gauge flags: zeros.  Synchronises."""
        from .tt import r_and_d_to_rks
        max_bond = int(max_bond)
        assert max_bond > max(self.max_ranks()), "New bond dimension too low"                       # tt_tools.jl:484
        new = r_and_d_to_rks(list(rks) if rks is not None else [1] + [max_bond] * (self.N - 1) + [1], self.dims, rmax=max_bond)
        y = DeviceTT(self.dims, cap_rks if cap_rks is not None else new, self.batch, dtype=self.dtype)
        _lib.check(_lib.lib().ttn_tt_increase_ranks(self.h, _i64(new), float(noise), int(seed) & (2 ** 64 - 1), y.h))
        return y

    # train -> dense tensor (csrc/ttn_grid_kernels.h)
    def to_dense(self, strides: Sequence[int] | None = None):
        """Every train of the batch as a dense tensor, on the device: a float64 torch tensor (batch, total) with
        out[b, sum_k (i_k - 1) strides[k]] = x_b(i_1..i_N).  ``strides=None`` is Julia column-major (``ttv_to_tensor``); any other table
        must be a mixed-radix system of the dims (ttn_tt_to_dense refuses the rest).  Asynchronous: the kernels run on the library's
        stream, and torch's current stream is made to wait for them, so the tensor can be used there right away."""
        from .tdvp import _dev
        torch, stream = _dev()
        if strides is not None and len(strides) != self.N:
            raise _lib.TTNError(f"to_dense: {len(strides)} strides for {self.N} sites")
        total = 1
        for n in self.dims:
            total *= n
        caller = torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            out = torch.empty((self.batch, total), dtype=torch.float64, device="cuda")
            _lib.check(_lib.lib().ttn_tt_to_dense(self.h, None if strides is None else _i64(strides), C.c_void_p(out.data_ptr())))
        if caller != stream:
            caller.wait_stream(stream)
            out.record_stream(caller)
        return out

    def free(self):
        if self.h:
            _lib.lib().ttn_tt_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    # parity instrumentation
    def capture_singular_values(self, on: bool = True) -> None:
        _lib.check(_lib.lib().ttn_sv_capture(self.h, 1 if on else 0))

    def singular_values(self, b: int, step: int, cap: int = 8192) -> np.ndarray:
        out = (C.c_double * cap)()
        n = C.c_int64(0)
        _lib.check(_lib.lib().ttn_sv_get(self.h, int(b), int(step), out, cap, C.byref(n)))
        return np.array(out[: n.value])


def split_rank_capacity(dims: Sequence[int], rks: Sequence[int], split_dims: Sequence[Sequence[int]]) -> List[int]:
    """Rank bounds of to_qtt at threshold 0 for input ranks (or capacities) ``rks``: every SVD keeps min(rows, cols) directions."""
    cap = [int(rks[0])]
    for i, s in enumerate(split_dims):
        r_prev, r_next, remaining = int(rks[i]), int(rks[i + 1]), int(dims[i])
        for f in s[:-1]:
            remaining //= max(int(f), 1)
            r_prev = max(1, min(r_prev * int(f), remaining * r_next))
            cap.append(r_prev)
        cap.append(r_next)
    return cap


def apply(A: DeviceTTO, x: DeviceTT, y: DeviceTT) -> DeviceTT:
    _lib.check(_lib.lib().ttn_apply(A.h, x.h, y.h))
    return y


def _factors(a, batch: int):
    """None (= 1), a scalar or one value per train as the `batch` doubles ttn_apply_axpby reads (None stays NULL)."""
    if a is None:
        return None
    v = np.broadcast_to(np.asarray(a, dtype=np.float64), (batch,))
    return (C.c_double * batch)(*[float(t) for t in v])


def apply_axpby(alpha, x: DeviceTT, beta, A: DeviceTTO, y: DeviceTT, z: DeviceTT) -> DeviceTT:
    """z_b = alpha_b x_b + beta_b (A y_b) in one streaming launch (ttn_apply_axpby): bit for bit ``apply`` -> ``scale_batch`` ->
    ``scale_batch`` -> ``add``.  alpha / beta: None (= 1), a scalar, or one value per train.  z needs the capacity
    x.rks + A.rks * y.rks; x may be y."""
    if not isinstance(A, DeviceTTO):
        raise TypeError(f"apply_axpby: expected a DeviceTTO, got {type(A).__name__}")
    _lib.check(_lib.lib().ttn_apply_axpby(_factors(alpha, x.batch), x.h, _factors(beta, x.batch), A.h, y.h, z.h))
    return z


def rect_rank_capacity(A_rks: Sequence[int], singleton_site: int, x_cap: Sequence[int]) -> List[int]:
    """Rank capacity of y = A * x for a rectangular A: A_rks[b] * x_cap[c(b)] with c(b) = b - [b >= singleton_site] (1-based site) —
    src/tt_operations.jl:127-130 on capacities."""
    s = int(singleton_site)
    return [int(A_rks[b]) * int(x_cap[b - (1 if b >= s else 0)]) for b in range(len(A_rks))]


def apply_rect(A: DeviceRectTTO, x: DeviceTT, y: DeviceTT) -> DeviceTT:
    """y = A * x for a rectangular A on every train of the batch (ttn_apply_rect); y has A.N = x.N + 1 sites and A's output dims."""
    if not isinstance(A, DeviceRectTTO):
        raise TypeError(f"apply_rect: expected a DeviceRectTTO, got {type(A).__name__}")
    _lib.check(_lib.lib().ttn_apply_rect(A.h, x.h, y.h))
    return y


def contract_kept(N: int, sites: Sequence[int]):
    """(kept, start), both 0-based, for the 1-based contracted ``sites`` of a train of N sites: the kept sites in order, and for each
    the first site of the run of contracted sites in front of it (the kept site itself when there is none)."""
    gone = {int(s) - 1 for s in sites}
    kept, start, run = [], [], 0
    for k in range(N):
        if k not in gone:
            kept.append(k)
            start.append(run)
            run = k + 1
    return kept, start


def contract_rank_capacity(x_cap: Sequence[int], sites: Sequence[int]) -> List[int]:
    """Rank capacity of ``contract_sites``' result: the bond left of a kept site carries x's bond left of the run in front of it, the right
    end x's right end."""
    _, start = contract_kept(len(x_cap) - 1, sites)
    return [int(x_cap[s]) for s in start] + [int(x_cap[-1])]


def _contract_tables(who: str, dims: Sequence[int], batch: int, weights):
    """The argument checks of ``contract_sites`` that need no device, and the C ABI's arguments: (sites, wbatch, table) with ``sites``
    1-based ascending and ``table`` a C-contiguous (wbatch, sum n_k) float64 array."""
    if not isinstance(weights, dict) or not weights:
        raise _lib.TTNError(f"{who}: weights must be a non-empty dict {{site: vector}} (sites are 1-based)")
    N = len(dims)
    for s in weights:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 1 <= int(s) <= N:
            raise _lib.TTNError(f"{who}: site {s!r} is not in 1:{N}")
    sites = sorted(int(s) for s in weights)
    if len(sites) >= N:
        raise _lib.TTNError(f"{who}: no kept site (a full contraction is dot with the rank-1 train of the weights)")
    vecs, wbatch = [], 1
    for s in sites:
        v = np.asarray(weights[s])
        if np.iscomplexobj(v):
            raise _lib.TTNError(f"{who}: the weights of site {s} are complex; Float64 only")
        v = np.asarray(v, dtype=np.float64)
        n = int(dims[s - 1])
        if v.shape == (n,):
            pass
        elif v.shape == (batch, n):
            wbatch = batch
        else:
            raise _lib.TTNError(f"{who}: the weights of site {s} have shape {v.shape}; expected ({n},) or ({batch}, {n})")
        vecs.append(v)
    table = np.ascontiguousarray(np.concatenate([np.broadcast_to(v, (wbatch, v.shape[-1])) for v in vecs], axis=1), dtype=np.float64)
    return sites, wbatch, table


def contract_sites(x: DeviceTT, weights, y: DeviceTT | None = None) -> DeviceTT:
    """Contract the sites ``weights`` names (a dict {site: vector}, sites 1-based, each vector of shape (n_k,) for every train or
    (batch, n_k) for one per train) against their vectors, train by train (ttn_tt_contract_sites): the result is the train on the
    remaining sites — a run of contracted sites is multiplied into the kept site behind it, the run behind the last kept site into that
    one.  Fills ``y`` (the kept dims, a rank capacity, x's batch) or returns a new handle.  Asynchronous; Float64 only."""
    if not isinstance(x, DeviceTT):
        raise TypeError(f"contract_sites: expected a DeviceTT, got {type(x).__name__}")
    if y is None:
        return x.contract_sites(weights)
    if not isinstance(y, DeviceTT):
        raise TypeError(f"contract_sites: expected a DeviceTT as y, got {type(y).__name__}")
    sites, wbatch, table = _contract_tables("contract_sites", x.dims, x.batch, weights)
    _lib.check(_lib.lib().ttn_tt_contract_sites(x.h, len(sites), _i64(sites), wbatch, _p_f64(table), y.h))
    return y


def prolong_compress_(A: DeviceRectTTO, x: DeviceTT, y: DeviceTT, max_bond: int, truncerr: float = 0.0, sweeps: int = 1) -> DeviceTT:
    """tt_compress!(A * x, max_bond; truncerr, sweeps) for a rectangular A, the coarse-to-fine step of the reference's prolongation
    examples: apply_rect into y, then the existing rounding in place on y, within its limits (y's capacity must hold what
    compress_rank_bound says a sweep can reach).  Two launches, no transfer."""
    apply_rect(A, x, y)
    return tt_compress_(y, max_bond, truncerr, sweeps)


def compress_rank_bound(dims, rks, max_bond: int, sweeps: int = 1, k: int = 0):
    """(need, final) rank bounds of tt_compress! / _tt_bond_truncate! — see ttn_compress_rank_bound in include/ttn.h."""
    d = len(dims)
    need = (C.c_int64 * (d + 1))()
    fin = (C.c_int64 * (d + 1))()
    _lib.check(_lib.lib().ttn_compress_rank_bound(d, _i64(dims), _i64(rks), int(min(max_bond, 2 ** 62)), int(sweeps), int(k), need, fin))
    return [int(v) for v in need], [int(v) for v in fin]


def tt_compress_(psi: DeviceTT, max_bond: int, truncerr: float = 0.0, sweeps: int = 1) -> DeviceTT:
    assert sweeps >= 1, "sweeps must be >= 1"
    _lib.check(_lib.lib().ttn_compress(psi.h, int(min(max_bond, 2 ** 62)), float(truncerr), int(sweeps)))
    return psi


def apply_compress(A: DeviceTTO, x: DeviceTT, y: DeviceTT, max_bond: int, truncerr: float = 0.0, sweeps: int = 1) -> DeviceTT:
    _lib.check(_lib.lib().ttn_apply_compress(A.h, x.h, y.h, int(max_bond), float(truncerr), int(sweeps)))
    return y


def compress_status(psi: DeviceTT) -> List[int]:
    """Raises if any Jacobi SVD failed to converge; returns total Jacobi sweeps per train."""
    out = (C.c_int64 * psi.batch)()
    _lib.check(_lib.lib().ttn_compress_status(psi.h, out))
    return [int(v) for v in out]


def status_all() -> None:
    """Raises if any live handle, or a handle freed since the last query, carries a failure code (ttn_status_all): the ONE
    check (one stream sync) a chain of asynchronous ops needs per time step / iteration."""
    _lib.check(_lib.lib().ttn_status_all())


def dot(a: DeviceTT, b: DeviceTT) -> np.ndarray:
    """dot(a_b, b_b) per train; complex handles: the first argument conjugated, a complex128 array."""
    if a.dtype is np.complex128:
        out = (C.c_double * (2 * a.batch))()
        _lib.check(_lib.lib().ttn_dot(a.h, b.h, out))
        return np.array(out[:]).view(np.complex128)
    out = (C.c_double * a.batch)()
    _lib.check(_lib.lib().ttn_dot(a.h, b.h, out))
    return np.array(out[:])


# limits of the on-chip route of ttn_sandwich (TTN_EXPECT_QTT_MAX_RANK / TTN_EXPECT_QTT_MAX_OP_RANK of include/ttn_expect.h): every
# n_k = 2, train ranks and operator ranks up to these; beyond them a train takes the general route — the same number
EXPECT_QTT_MAX_RANK = 64
EXPECT_QTT_MAX_OP_RANK = 5


def _sandwich_args(x: DeviceTT, A: DeviceTTO, y: DeviceTT):
    if not isinstance(A, DeviceTTO):
        raise TypeError(f"sandwich: expected a DeviceTTO, got {type(A).__name__}")
    if not isinstance(x, DeviceTT) or not isinstance(y, DeviceTT):
        raise TypeError("sandwich: expected DeviceTT trains")


def sandwich(x: DeviceTT, A: DeviceTTO, y: DeviceTT) -> np.ndarray:
    """<x_b, A y_b> per train in one sweep over the three cores of every site (ttn_sandwich): what ``dot(x, apply(A, y))`` returns up
    to rounding, without the train A y.  x may be y.  Float64 only.  Synchronises, as ``dot``."""
    _sandwich_args(x, A, y)
    out = (C.c_double * x.batch)()
    _lib.check(_lib.lib().ttn_sandwich(x.h, A.h, y.h, out))
    return np.array(out[:])


def sandwich_dev(x: DeviceTT, A: DeviceTTO, y: DeviceTT, out=None):
    """``sandwich`` into a float64 device tensor of ``batch`` entries (``out``, or a new one), asynchronously on the library stream:
    no number crosses to the host.  The tensor must not be read on another stream before ``sync()``."""
    import torch
    _sandwich_args(x, A, y)
    if out is None:
        out = torch.empty(x.batch, dtype=torch.float64, device="cuda")
    if out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous() or out.numel() != x.batch:
        raise TypeError("sandwich_dev: out must be a contiguous float64 device tensor with one entry per train")
    _lib.check(_lib.lib().ttn_sandwich_dev(x.h, A.h, y.h, C.c_void_p(out.data_ptr())))
    return out


def expect(A: DeviceTTO, x: DeviceTT) -> np.ndarray:
    """<x_b, A x_b> per train: ``sandwich(x, A, x)``."""
    return sandwich(x, A, x)


def rayleigh(A: DeviceTTO, x: DeviceTT) -> np.ndarray:
    """<x_b, A x_b> / <x_b, x_b> per train — the reference's ``real(dot(psi, H * psi)) / real(dot(psi, psi))``."""
    return expect(A, x) / dot(x, x)


# ---- site-resolved measurements (include/ttn_measure.h, csrc/ttn_measure_kernels.h) ---------------------------------
def _header_define(header: str, name: str) -> int:
    import os
    import re
    m = re.search(r"#define\s+%s\s+(\d+)" % re.escape(name), open(os.path.join(_lib.INCLUDE, header)).read())
    if m is None:
        raise RuntimeError(f"{header} does not define {name}")
    return int(m.group(1))


MEASURE_MAX_OPS = _header_define("ttn_measure.h", "TTN_MEASURE_MAX_OPS")     # operator tables per site_expect call


# ---- <x| A |y> with x conjugated, on ComplexF64 or Float64 operands (include/ttn_braket.h, csrc/ttn_braket_kernels.h) -----
# limits of the on-chip route of ttn_braket: every n_k = 2, train ranks and operator ranks up to these; beyond them a train takes the
# general route — the same number
BRAKET_QTT_MAX_RANK = _header_define("ttn_braket.h", "TTN_BRAKET_QTT_MAX_RANK")
BRAKET_QTT_MAX_OP_RANK = _header_define("ttn_braket.h", "TTN_BRAKET_QTT_MAX_OP_RANK")


def _braket_args(x: DeviceTT, A: DeviceTTO, y: DeviceTT):
    if not isinstance(A, DeviceTTO):
        raise TypeError(f"braket: expected a DeviceTTO, got {type(A).__name__}")
    if not isinstance(x, DeviceTT) or not isinstance(y, DeviceTT):
        raise TypeError("braket: expected DeviceTT trains")


def braket(x: DeviceTT, A: DeviceTTO, y: DeviceTT) -> np.ndarray:
    """<x_b| A |y_b> = sum_ij conj(x_b[i]) A[i, j] y_b[j] per train in one sweep over the three cores of every site (ttn_braket): what
    ``dot(x, apply(A, y))`` returns up to rounding, without the train A y.  x and y share an element type, the operator is real or
    complex on its own; x may be y.  A complex128 array of ``batch`` entries (all operands Float64: ``sandwich``'s numbers, imaginary
    parts 0).  Synchronises, as ``dot``."""
    _braket_args(x, A, y)
    out = (C.c_double * (2 * x.batch))()
    _lib.check(_lib.lib().ttn_braket(x.h, A.h, y.h, out))
    return np.array(out[:]).view(np.complex128)


def braket_dev(x: DeviceTT, A: DeviceTTO, y: DeviceTT, out=None):
    """``braket`` into a complex128 device tensor of ``batch`` entries (``out``, or a new one), asynchronously on the library stream:
    no number crosses to the host.  The tensor must not be read on another stream before ``sync()``."""
    import torch
    _braket_args(x, A, y)
    if out is None:
        out = torch.empty(x.batch, dtype=torch.complex128, device="cuda")
    if out.dtype != torch.complex128 or not out.is_cuda or not out.is_contiguous() or out.numel() != x.batch:
        raise TypeError("braket_dev: out must be a contiguous complex128 device tensor with one entry per train")
    _lib.check(_lib.lib().ttn_braket_dev(x.h, A.h, y.h, C.c_void_p(out.data_ptr())))
    return out


def energy(A: DeviceTTO, x: DeviceTT) -> np.ndarray:
    """real(<x_b| A |x_b>) / real(<x_b, x_b>) per train — the reference's ``real(dot(psi, H * psi)) / real(dot(psi, psi))``, for either
    element type."""
    return np.real(braket(x, A, x)) / np.real(dot(x, x))


def _measure_table(who: str, name: str, op, dims: Sequence[int]) -> np.ndarray:
    """One operator table of include/ttn_measure.h from ``op`` — an (n, n) array used at every site, or a sequence of d arrays —: the
    per-site matrices column-major, back to back, float64.  Shape and dtype errors are raised here, before any device call."""
    d = len(dims)
    if isinstance(op, (list, tuple)) and len(op) > 0 and all(np.ndim(o) == 2 for o in op):
        mats = list(op)
    else:
        a = np.asarray(op)
        if a.dtype == object or a.ndim not in (2, 3):
            raise _lib.TTNError(f"{who}: {name} must be an (n, n) array or a sequence of {d} such arrays, got shape {getattr(a, 'shape', None)}")
        mats = [a] * d if a.ndim == 2 else list(a)
    if len(mats) != d:
        raise _lib.TTNError(f"{who}: {name} holds {len(mats)} matrices for {d} sites")
    flat = []
    for k, (m, n) in enumerate(zip(mats, dims)):
        m = np.asarray(m)
        if np.iscomplexobj(m):
            raise _lib.TTNError(f"{who}: {name} at site {k} is complex: Float64 only (for sigma_y use [[0, 1], [-1, 0]] = i sigma_y in a correlator)")
        if m.dtype == object or not (np.issubdtype(m.dtype, np.number) or m.dtype == bool):
            raise _lib.TTNError(f"{who}: {name} at site {k} has dtype {m.dtype}, expected real numbers")
        if m.shape != (n, n):
            raise _lib.TTNError(f"{who}: {name} at site {k} has shape {m.shape}, expected ({n}, {n})")
        flat.append(np.asarray(m, dtype=np.float64).flatten(order="F"))
    return np.concatenate(flat)


def _measure_train(who: str, x) -> None:
    if not isinstance(x, DeviceTT):
        raise TypeError(f"{who}: expected a DeviceTT, got {type(x).__name__}")


def _p_f64(a: np.ndarray):
    return a.ctypes.data_as(_lib.p_f64)


def _site_expect_tables(x: DeviceTT, ops) -> np.ndarray:
    _measure_train("site_expect", x)
    if not ops:
        raise _lib.TTNError("site_expect: no operator given")
    return np.concatenate([_measure_table("site_expect", f"operator {t}", op, x.dims) for t, op in enumerate(ops)])


def site_expect(x: DeviceTT, *ops, normalize: bool = True) -> np.ndarray:
    """The profile E_O[k] = <x_b| O_k |x_b> / <x_b, x_b> of every site and train (ttn_site_expect): (batch, d) for one operator,
    (batch, nops, d) for several (at most ``MEASURE_MAX_OPS``), all from ONE pair of environment chains.  Each ``op`` is an (n, n) array
    used at every site or a sequence of d arrays; its first index meets the bra, as the output index of an operator in ``sandwich``.
    The train is real, so only the symmetric part of an operator is seen: an antisymmetric one ([[0, 1], [-1, 0]] = i sigma_y) gives
    zeros.  ``normalize=False`` leaves the division out; a zero train with ``normalize=True`` gives NaN (0 / 0).  Float64 only.
    Synchronises, as ``dot``."""
    tabs = _site_expect_tables(x, ops)
    out = np.empty(x.batch * len(ops) * x.N, dtype=np.float64)
    _lib.check(_lib.lib().ttn_site_expect(x.h, len(ops), _p_f64(tabs), 1 if normalize else 0, _p_f64(out)))
    res = out.reshape(x.batch, len(ops), x.N)
    return res[:, 0, :].copy() if len(ops) == 1 else res


def site_expect_dev(x: DeviceTT, *ops, normalize: bool = True, out=None):
    """``site_expect`` into a float64 device tensor (batch, nops, d) (``out``, or a new one), asynchronously on the library stream.  The
    tensor must not be read on another stream before ``sync()``."""
    import torch
    tabs = _site_expect_tables(x, ops)
    shape = (x.batch, len(ops), x.N)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device="cuda")
    if out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != shape:
        raise TypeError(f"site_expect_dev: out must be a contiguous float64 device tensor of shape {shape}")
    _lib.check(_lib.lib().ttn_site_expect_dev(x.h, len(ops), _p_f64(tabs), 1 if normalize else 0, C.c_void_p(out.data_ptr())))
    return out


def _correlation_tables(x: DeviceTT, P, Q):
    _measure_train("correlation_matrix", x)
    tp = _measure_table("correlation_matrix", "P", P, x.dims)
    tq = tp if (Q is None or Q is P) else _measure_table("correlation_matrix", "Q", Q, x.dims)
    return tp, tq


def correlation_matrix(x: DeviceTT, P, Q=None, normalize: bool = True, connected: bool = False) -> np.ndarray:
    """C[b, i, j] = <x_b| P_i Q_j |x_b> / <x_b, x_b> for ALL pairs of sites (ttn_correlation): (batch, d, d).  ``P`` and ``Q`` are given
    as in ``site_expect``; ``Q=None`` means Q = P.  The diagonal is the matrix product P_i Q_i on one site; off the diagonal the two
    act on different sites and commute; the matrix is in general not symmetric when P != Q.  A correlator sees antisymmetric factors:
    P = Q = [[0, 1], [-1, 0]] (= i sigma_y) gives MINUS <sigma_y sigma_y> — how a Float64 train yields its YY correlations.
    ``connected=True`` subtracts E_P[i] E_Q[j] (on the diagonal E_P[i] E_Q[i]) with the profiles of ``site_expect`` at the same
    ``normalize`` (a connected correlator is meant for ``normalize=True``).  Cost: the two chains, then one short walk per site and
    triangle — one triangle when P and Q are equal bit for bit, the other mirrored.  Reproducible to rounding, not bitwise.
    Synchronises."""
    tp, tq = _correlation_tables(x, P, Q)
    d = x.N
    out = np.empty(x.batch * d * d, dtype=np.float64)
    _lib.check(_lib.lib().ttn_correlation(x.h, _p_f64(tp), _p_f64(tq), 1 if normalize else 0, _p_f64(out)))
    res = np.ascontiguousarray(out.reshape(x.batch, d, d).transpose(0, 2, 1))       # the ABI stores C[i, j] at i + d j
    if connected:
        ep = site_expect(x, P, normalize=normalize)
        eq = ep if (Q is None or Q is P) else site_expect(x, Q, normalize=normalize)
        res -= ep[:, :, None] * eq[:, None, :]
    return res


def correlation_matrix_dev(x: DeviceTT, P, Q=None, normalize: bool = True, out=None):
    """``correlation_matrix`` (not connected) asynchronously on the library stream: returns the (batch, d, d) VIEW C[b, i, j] of a
    float64 device tensor in the layout of the ABI (``out``, contiguous (batch, d, d) holding C[b, j, i], or a new one)."""
    import torch
    tp, tq = _correlation_tables(x, P, Q)
    shape = (x.batch, x.N, x.N)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device="cuda")
    if out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != shape:
        raise TypeError(f"correlation_matrix_dev: out must be a contiguous float64 device tensor of shape {shape}")
    _lib.check(_lib.lib().ttn_correlation_dev(x.h, _p_f64(tp), _p_f64(tq), 1 if normalize else 0, C.c_void_p(out.data_ptr())))
    return out.transpose(1, 2)


# ---- site-resolved measurements on ComplexF64 trains (include/ttn_zmeasure.h, csrc/ttn_zmeasure_kernels.h) -------------
ZMEASURE_MAX_OPS = _header_define("ttn_zmeasure.h", "TTN_ZMEASURE_MAX_OPS")     # operator tables per zsite_expect call


def _zmeasure_table(who: str, name: str, op, dims: Sequence[int]) -> np.ndarray:
    """One operator table of include/ttn_zmeasure.h from ``op`` — an (n, n) array used at every site, or a sequence of d arrays, real
    or complex —: the per-site matrices column-major, back to back, complex128.  Shape and dtype errors are raised here, before any
    device call."""
    d = len(dims)
    if isinstance(op, (list, tuple)) and len(op) > 0 and all(np.ndim(o) == 2 for o in op):
        mats = list(op)
    else:
        a = np.asarray(op)
        if a.dtype == object or a.ndim not in (2, 3):
            raise _lib.TTNError(f"{who}: {name} must be an (n, n) array or a sequence of {d} such arrays, got shape {getattr(a, 'shape', None)}")
        mats = [a] * d if a.ndim == 2 else list(a)
    if len(mats) != d:
        raise _lib.TTNError(f"{who}: {name} holds {len(mats)} matrices for {d} sites")
    flat = []
    for k, (m, n) in enumerate(zip(mats, dims)):
        m = np.asarray(m)
        if m.dtype == object or not (np.issubdtype(m.dtype, np.number) or m.dtype == bool):
            raise _lib.TTNError(f"{who}: {name} at site {k} has dtype {m.dtype}, expected real or complex numbers")
        if m.shape != (n, n):
            raise _lib.TTNError(f"{who}: {name} at site {k} has shape {m.shape}, expected ({n}, {n})")
        flat.append(np.asarray(m, dtype=np.complex128).flatten(order="F"))
    return np.concatenate(flat)


def _zmeasure_train(who: str, x) -> None:
    if not isinstance(x, DeviceTT):
        raise TypeError(f"{who}: expected a DeviceTT, got {type(x).__name__}")
    if x.dtype is not np.complex128:
        raise _lib.TTNError(f"{who}: ComplexF64 only; a Float64 handle is measured by site_expect / correlation_matrix")


def _p_c128(a: np.ndarray):
    return a.view(np.float64).ctypes.data_as(_lib.p_f64)


def _zsite_expect_tables(who: str, x: DeviceTT, ops) -> np.ndarray:
    _zmeasure_train(who, x)
    if not ops:
        raise _lib.TTNError(f"{who}: no operator given")
    if len(ops) > ZMEASURE_MAX_OPS:
        raise _lib.TTNError(f"{who}: {len(ops)} operators, at most {ZMEASURE_MAX_OPS} per call")
    return np.concatenate([_zmeasure_table(who, f"operator {t}", op, x.dims) for t, op in enumerate(ops)])


def zsite_expect(x: DeviceTT, *ops, normalize: bool = True) -> np.ndarray:
    """The complex profile E_O[k] = <x_b| O_k |x_b> / <x_b|x_b> of every site and train of a ComplexF64 handle (ttn_zsite_expect):
    complex128, (batch, d) for one operator, (batch, nops, d) for several (at most ``ZMEASURE_MAX_OPS``), all from ONE pair of
    environment chains.  Each ``op`` is an (n, n) array used at every site or a sequence of d arrays, real or complex; its first index
    meets the conjugated bra, as the output index of an operator in ``braket``.  A lone sigma_y is measured as it stands; a Hermitian
    table gives a real profile up to rounding.  ``normalize=False`` leaves the division by real(<x|x>) out; a zero train with
    ``normalize=True`` gives NaN (0 / 0).  Reproducible to rounding, not bitwise.  Synchronises, as ``dot``."""
    tabs = _zsite_expect_tables("zsite_expect", x, ops)
    out = np.empty(x.batch * len(ops) * x.N, dtype=np.complex128)
    _lib.check(_lib.lib().ttn_zsite_expect(x.h, len(ops), _p_c128(tabs), 1 if normalize else 0, _p_c128(out)))
    res = out.reshape(x.batch, len(ops), x.N)
    return res[:, 0, :].copy() if len(ops) == 1 else res


def zsite_expect_dev(x: DeviceTT, *ops, normalize: bool = True, out=None):
    """``zsite_expect`` into a complex128 device tensor (batch, nops, d) (``out``, or a new one), asynchronously on the library stream.
    The tensor must not be read on another stream before ``sync()``."""
    import torch
    tabs = _zsite_expect_tables("zsite_expect_dev", x, ops)
    shape = (x.batch, len(ops), x.N)
    if out is None:
        out = torch.empty(shape, dtype=torch.complex128, device="cuda")
    if out.dtype != torch.complex128 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != shape:
        raise TypeError(f"zsite_expect_dev: out must be a contiguous complex128 device tensor of shape {shape}")
    _lib.check(_lib.lib().ttn_zsite_expect_dev(x.h, len(ops), _p_c128(tabs), 1 if normalize else 0, C.c_void_p(out.data_ptr())))
    return out


def _zcorrelation_tables(who: str, x: DeviceTT, P, Q):
    _zmeasure_train(who, x)
    tp = _zmeasure_table(who, "P", P, x.dims)
    tq = tp if (Q is None or Q is P) else _zmeasure_table(who, "Q", Q, x.dims)
    return tp, tq


def zcorrelation_matrix(x: DeviceTT, P, Q=None, normalize: bool = True, connected: bool = False) -> np.ndarray:
    """C[b, i, j] = <x_b| P_i Q_j |x_b> / <x_b|x_b> for ALL pairs of sites of a ComplexF64 handle (ttn_zcorrelation): complex128,
    (batch, d, d).  ``P`` and ``Q`` are given as in ``zsite_expect``; ``Q=None`` means Q = P.  The diagonal is the matrix product
    P_i Q_i on one site; off the diagonal the two act on different sites and commute.  ``connected=True`` subtracts E_P[i] E_Q[j] (on
    the diagonal E_P[i] E_Q[i]) with the profiles of ``zsite_expect`` at the same ``normalize``.  Cost: the two chains, then one short
    walk per site and triangle — one triangle when P and Q are equal bit for bit, the other its plain copy.  Reproducible to rounding,
    not bitwise.  Synchronises."""
    tp, tq = _zcorrelation_tables("zcorrelation_matrix", x, P, Q)
    d = x.N
    out = np.empty(x.batch * d * d, dtype=np.complex128)
    _lib.check(_lib.lib().ttn_zcorrelation(x.h, _p_c128(tp), _p_c128(tq), 1 if normalize else 0, _p_c128(out)))
    res = np.ascontiguousarray(out.reshape(x.batch, d, d).transpose(0, 2, 1))       # the ABI stores C[i, j] at i + d j
    if connected:
        ep = zsite_expect(x, P, normalize=normalize)
        eq = ep if (Q is None or Q is P) else zsite_expect(x, Q, normalize=normalize)
        res -= ep[:, :, None] * eq[:, None, :]
    return res


def zcorrelation_matrix_dev(x: DeviceTT, P, Q=None, normalize: bool = True, out=None):
    """``zcorrelation_matrix`` (not connected) asynchronously on the library stream: returns the (batch, d, d) VIEW C[b, i, j] of a
    complex128 device tensor in the layout of the ABI (``out``, contiguous (batch, d, d) holding C[b, j, i], or a new one)."""
    import torch
    tp, tq = _zcorrelation_tables("zcorrelation_matrix_dev", x, P, Q)
    shape = (x.batch, x.N, x.N)
    if out is None:
        out = torch.empty(shape, dtype=torch.complex128, device="cuda")
    if out.dtype != torch.complex128 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != shape:
        raise TypeError(f"zcorrelation_matrix_dev: out must be a contiguous complex128 device tensor of shape {shape}")
    _lib.check(_lib.lib().ttn_zcorrelation_dev(x.h, _p_c128(tp), _p_c128(tq), 1 if normalize else 0, C.c_void_p(out.data_ptr())))
    return out.transpose(1, 2)


# ---- sampling (include/ttn_sample.h, csrc/ttn_sample_kernels.h) ----------------------------------------------------------
SAMPLE_MODES = {"born": _header_define("ttn_sample.h", "TTN_SAMPLE_BORN"), "density": _header_define("ttn_sample.h", "TTN_SAMPLE_DENSITY")}


def _sample_args(who: str, nsamples, mode, seed, u, batch: int, d: int):
    """The argument checks of a sampling call that need no device: (S, mode code, seed as int64, u).  ``u`` stays what it was (a NumPy
    array is made float64 and contiguous); only its shape (batch, S, d) and its range are examined."""
    if isinstance(nsamples, bool) or not isinstance(nsamples, (int, np.integer)) or nsamples < 1:
        raise _lib.TTNError(f"{who}: nsamples must be an integer >= 1, got {nsamples!r}")
    if not isinstance(mode, str) or mode not in SAMPLE_MODES:
        raise _lib.TTNError(f"{who}: mode must be 'born' or 'density', got {mode!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise _lib.TTNError(f"{who}: seed must be an integer, got {seed!r}")
    seed = int(seed) % (1 << 64)
    seed = seed - (1 << 64) if seed >= (1 << 63) else seed                # the same 64 bits as an int64
    if u is not None:
        shape = (batch, int(nsamples), d)
        if isinstance(u, np.ndarray) or not hasattr(u, "data_ptr"):
            u = np.ascontiguousarray(np.asarray(u), dtype=np.float64)
            if u.shape != shape:
                raise _lib.TTNError(f"{who}: u has shape {u.shape}, expected {shape}")
            if u.size and not (np.all(u >= 0.0) and np.all(u < 1.0)):
                raise _lib.TTNError(f"{who}: u must lie in [0, 1)")
        elif tuple(u.shape) != shape or str(u.dtype) != "torch.float64" or not u.is_cuda or not u.is_contiguous():
            raise _lib.TTNError(f"{who}: a device u must be a contiguous float64 tensor of shape {shape}, got {tuple(u.shape)} {u.dtype}")
    return int(nsamples), SAMPLE_MODES[mode], seed, u


def sample_dev(x: DeviceTT, nsamples: int, mode: str = "born", seed: int = 0, u=None):
    """``sample`` into device tensors (idx (B, S, d) int64, logp (B, S) float64, info (B, 2) int64), asynchronously on the library
    stream: they must not be read on another stream before ``sync()``."""
    import torch
    _measure_train("sample", x)
    S, code, seed, u = _sample_args("sample", nsamples, mode, seed, u, x.batch, x.N)
    if isinstance(u, np.ndarray):
        u = torch.from_numpy(u).to("cuda")
    idx = torch.empty((x.batch, S, x.N), dtype=torch.int64, device="cuda")
    logp = torch.empty((x.batch, S), dtype=torch.float64, device="cuda")
    info = torch.empty((x.batch, 2), dtype=torch.int64, device="cuda")
    if u is not None:
        torch.cuda.current_stream().synchronize()                         # u was produced on the caller's stream, not the library's
    _lib.check(_lib.lib().ttn_tt_sample_dev(x.h, code, S, seed, C.c_void_p(u.data_ptr()) if u is not None else None,
                                            C.c_void_p(idx.data_ptr()), C.c_void_p(logp.data_ptr()), C.c_void_p(info.data_ptr())))
    return idx, logp, info


def sample(x: DeviceTT, nsamples: int, mode: str = "born", seed: int = 0, u=None):
    """``nsamples`` configurations of every train of the batch (ttn_tt_sample), drawn by the conditional sweep over the sites:
    ``mode="born"`` from p(z) = x(z)^2 / <x, x>, ``mode="density"`` from p(z) = x(z) / sum x for a train that represents a non-negative
    function.  Returns NumPy arrays: ``idx`` (B, S, d) int64 with 1-based indices, ``logp`` (B, S) with log p(z) of each sample, and
    ``info`` (B, 2): the weights that were negative and clamped to 0, and the DEAD samples — those that met a total weight of 0 or a
    non-finite one; their remaining indices are 1 and their logp is -inf (nothing is raised).  ``u`` gives the uniforms, (B, S, d) in
    [0, 1), as a NumPy array or a float64 device tensor; ``u=None`` generates them on the device from ``seed``, the numbers of
    ``sample_uniforms(seed, B, S, d)``.  Reproducible to rounding: two calls can differ only in a sample whose draw lies within rounding
    of a cumulative weight.  Float64 only.  Synchronises."""
    _measure_train("sample", x)
    S, code, seed, u = _sample_args("sample", nsamples, mode, seed, u, x.batch, x.N)
    if isinstance(u, np.ndarray):
        import torch
        u = torch.from_numpy(u).to("cuda")
    if u is not None:
        import torch
        torch.cuda.current_stream().synchronize()
    idx = np.empty((x.batch, S, x.N), dtype=np.int64)
    logp = np.empty((x.batch, S), dtype=np.float64)
    info = np.empty((x.batch, 2), dtype=np.int64)
    _lib.check(_lib.lib().ttn_tt_sample(x.h, code, S, seed, C.c_void_p(u.data_ptr()) if u is not None else None,
                                        idx.ctypes.data_as(_lib.p_i64), _p_f64(logp), info.ctypes.data_as(_lib.p_i64)))
    return idx, logp, info


def sample_last_ms():
    """(environment ms, sweep ms) of the last ``sample`` / ``sample_dev`` call on the device (ttn_tt_sample_last_ms); synchronises."""
    a, b = C.c_double(0.0), C.c_double(0.0)
    _lib.check(_lib.lib().ttn_tt_sample_last_ms(C.byref(a), C.byref(b)))
    return float(a.value), float(b.value)


def norm(a: DeviceTT) -> np.ndarray:
    out = (C.c_double * a.batch)()
    _lib.check(_lib.lib().ttn_norm(a.h, out))
    return np.array(out[:])


def hadamard(x: DeviceTT, y: DeviceTT, z: DeviceTT) -> DeviceTT:
    _lib.check(_lib.lib().ttn_hadamard(x.h, y.h, z.h))
    return z


def add(x: DeviceTT, y: DeviceTT, z: DeviceTT) -> DeviceTT:
    _lib.check(_lib.lib().ttn_add(x.h, y.h, z.h))
    return z


def scale(a, x: DeviceTT, y: DeviceTT) -> DeviceTT:
    if x.dtype is np.complex128 or isinstance(a, (complex, np.complexfloating)):       # (a complex factor on real handles is refused by the library)
        a = complex(a)
        _lib.check(_lib.lib().ttn_scale_c64(a.real, a.imag, x.h, y.h))
        return y
    _lib.check(_lib.lib().ttn_scale(float(a), x.h, y.h))
    return y


def scale_batch(a, x: DeviceTT, y: DeviceTT) -> DeviceTT:
    """y_b = a[b] * x_b (one scalar per train; complex handles take complex factors)."""
    if x.dtype is np.complex128:
        flat = np.ascontiguousarray(np.asarray(a, dtype=np.complex128).reshape(x.batch)).view(np.float64)
        _lib.check(_lib.lib().ttn_scale_batch_c64((C.c_double * (2 * x.batch))(*flat.tolist()), x.h, y.h))
        return y
    arr = (C.c_double * x.batch)(*[float(v) for v in a])
    _lib.check(_lib.lib().ttn_scale_batch(arr, x.h, y.h))
    return y


def orthogonalize(x: DeviceTT, i: int, y: DeviceTT) -> DeviceTT:
    _lib.check(_lib.lib().ttn_orthogonalize(x.h, int(i), y.h))
    return y


def last_launch_ms() -> float:
    """HIP-event time of the kernel of the last dot / norm / orthogonalize call alone (ttn_last_launch_ms)."""
    ms = C.c_float(0.0)
    _lib.check(_lib.lib().ttn_last_launch_ms(C.byref(ms)))
    return float(ms.value)


def sync() -> None:
    _lib.check(_lib.lib().ttn_sync())


class StreamTimer:
    """HIP-event timer on the library stream (the stream the kernels are launched on)."""

    def __enter__(self):
        _lib.check(_lib.lib().ttn_timer_begin())
        self.ms = None
        return self

    def __exit__(self, *exc):
        ms = C.c_float(0.0)
        _lib.check(_lib.lib().ttn_timer_end(C.byref(ms)))
        self.ms = float(ms.value)
        return False


def event_record(slot: int) -> None:
    _lib.check(_lib.lib().ttn_event_record(int(slot)))


def event_elapsed_ms(a: int, b: int) -> float:
    ms = C.c_float(0.0)
    _lib.check(_lib.lib().ttn_event_elapsed(int(a), int(b), C.byref(ms)))
    return float(ms.value)
