# TTNBackend.jl — the Julia-side binding a TensorTrainNumerics.jl maintainer would add to route the
# Float64 hot path through libttn_hip.so (include/ttn.h).  NOT executed in this repository: the build
# image has no Julia runtime (see DESIGN.md §2); the same C ABI is exercised through ctypes by
# tensortrainnumerics.jl_amd/tt.py, which mirrors this file function for function.
#
# `TTvector{Float64}` / `TToperator{Float64}` methods are overloaded, and for ComplexF64 `*` (with the two mixed forms), `+`, `dot`
# and `tt_compress!`; every other eltype (Float32, Int — test/test_tt_tools.jl:576-596) and every other ComplexF64 method falls
# through to the generic Julia methods.
module TTNBackend

using TensorTrainNumerics
import TensorTrainNumerics: TTvector, TToperator, dmrg_eigsolve, mals_eigsolve, als_eigsolve, als_gen_eigsolv, orthogonalize, tt_compress!, _tt_bond_truncate!, hadamard, add!, r_and_d_to_rks, zeros_tt,
    _applyH1_lsr, _applyH0, _update_left_env, _update_right_env, _applyH2_lsr
import Base: *, +

const LIB = get(ENV, "TTN_LIB", joinpath(@__DIR__, "..", "tensortrainnumerics.jl_amd", "libttn_hip.so"))

# return-code contract of include/ttn.h: 0 ok, <0 argument error (AssertionError in the reference), >0 HIP error
function _chk(rc::Cint)
    rc == 0 && return nothing
    msg = unsafe_string(ccall((:ttn_last_error_string, LIB), Cstring, ()))
    (-4 <= rc <= -1) && throw(AssertionError(msg))      # tt_operations.jl:11,102,240,344; tt_tools.jl:513,744,773
    error("ttn error $rc: $msg")
end

_ptrs(v::Vector{<:Array{Float64}}) = Ptr{Float64}[pointer(c) for c in v]
_dims(x) = Int64[x...]

# *(A::TToperator, v::TTvector)  — src/tt_operations.jl:101-111
function *(A::TToperator{Float64, N}, v::TTvector{Float64, N}) where {N}
    @assert A.tto_dims == v.ttv_dims "Incompatible dimensions"
    y = zeros_tt(Float64, A.tto_dims, A.tto_rks .* v.ttv_rks)
    pa, px, py = _ptrs(A.tto_vec), _ptrs(v.ttv_vec), _ptrs(y.ttv_vec)
    GC.@preserve A v y pa px py _chk(ccall((:ttn_apply_f64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}),
        N, _dims(A.tto_dims), pa, A.tto_rks, px, v.ttv_rks, py))
    return y
end

# dot(A, B) — src/tt_operations.jl:239-250
function TensorTrainNumerics.dot(A::TTvector{Float64, N}, B::TTvector{Float64, N}) where {N}
    @assert A.ttv_dims == B.ttv_dims "TT dimensions are not compatible"
    out = Ref{Float64}(0.0)
    pa, pb = _ptrs(A.ttv_vec), _ptrs(B.ttv_vec)
    GC.@preserve A B pa pb _chk(ccall((:ttn_dot_f64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ref{Float64}),
        N, _dims(A.ttv_dims), pa, A.ttv_rks, pb, B.ttv_rks, out))
    return out[]
end

# hadamard(x, y) — src/tt_operations.jl:343-361
function hadamard(x::TTvector{Float64, N}, y::TTvector{Float64, N}) where {N}
    @assert x.ttv_dims == y.ttv_dims "Incompatible TT dimensions"
    z = zeros_tt(Float64, x.ttv_dims, x.ttv_rks .* y.ttv_rks)
    px, py, pz = _ptrs(x.ttv_vec), _ptrs(y.ttv_vec), _ptrs(z.ttv_vec)
    GC.@preserve x y z px py pz _chk(ccall((:ttn_hadamard_f64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}),
        N, _dims(x.ttv_dims), px, x.ttv_rks, py, y.ttv_rks, pz))
    return z
end

# +(x, y) — src/tt_operations.jl:10-35
function +(x::TTvector{Float64, N}, y::TTvector{Float64, N}) where {N}
    @assert x.ttv_dims == y.ttv_dims "Incompatible dimensions"
    rks = x.ttv_rks + y.ttv_rks; rks[1] = 1; rks[end] = 1
    z = zeros_tt(Float64, x.ttv_dims, rks)
    px, py, pz = _ptrs(x.ttv_vec), _ptrs(y.ttv_vec), _ptrs(z.ttv_vec)
    GC.@preserve x y z px py pz _chk(ccall((:ttn_add_f64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}),
        N, _dims(x.ttv_dims), px, x.ttv_rks, py, y.ttv_rks, pz))
    return z
end

# add!(x, y) — src/tt_operations.jl:37-66 (rebinds the fields of x)
function add!(x::TTvector{Float64, N}, y::TTvector{Float64, N}) where {N}
    z = x + y
    x.ttv_vec = z.ttv_vec; x.ttv_rks = z.ttv_rks; x.ttv_ot = z.ttv_ot
    return x
end

# a * x — src/tt_operations.jl:256-266 (`x * a`, `-`, `/` are one-liners on top of it in the reference, :268-295, and keep dispatching
# here).  a == 0 gives zeros_tt(...) with ot reset; otherwise the first core with ot == 0 (else core 1) is scaled and ot is copied.
function *(a::Float64, x::TTvector{Float64, N}) where {N}
    y = zeros_tt(Float64, x.ttv_dims, x.ttv_rks)
    yot = zeros(Int64, N)
    px, py = _ptrs(x.ttv_vec), _ptrs(y.ttv_vec)
    GC.@preserve x y px py _chk(ccall((:ttn_scale_f64, LIB), Cint,
        (Int64, Ptr{Int64}, Float64, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}),
        N, _dims(x.ttv_dims), a, px, x.ttv_rks, x.ttv_ot, py, yot))
    y.ttv_ot .= yot
    return y
end

# _tt_bond_truncate!(ψ, k; max_bond, truncerr) — src/tt_tools.jl:743-770: mutates cores k, k+1 and ψ.ttv_rks[k+1] in place and
# RETURNS orthogonalize(ψ; i=k) (:769) like the reference (tt_compress! discards that value, so ttn_compress_f64 never computes it).
function _tt_bond_truncate!(ψ::TTvector{Float64, N}, k::Int; max_bond::Int = typemax(Int), truncerr::Real = 0.0) where {N}
    @assert(1 ≤ k < N, "k must be in 1:(N-1)")
    mb = min(max_bond, typemax(Int64) >> 1)
    need = zeros(Int64, N + 1)                      # the rank of a rank-deficient bond may grow to min(n r_left, n r_right, max_bond)
    _chk(ccall((:ttn_compress_rank_bound, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}),
        N, _dims(ψ.ttv_dims), ψ.ttv_rks, mb, 1, k, need, C_NULL))
    bufs = [zeros(Float64, ψ.ttv_dims[j] * need[j] * need[j + 1]) for j in 1:N]
    for j in 1:N
        copyto!(bufs[j], vec(ψ.ttv_vec[j]))
    end
    rks = copy(ψ.ttv_rks)
    pb = Ptr{Float64}[pointer(c) for c in bufs]
    GC.@preserve bufs pb _chk(ccall((:ttn_bond_truncate_f64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Int64, Int64, Float64),
        N, _dims(ψ.ttv_dims), pb, rks, k, mb, Float64(truncerr)))
    for j in (k, k + 1)                             # only these two slots change (:764-767)
        n = ψ.ttv_dims[j]
        ψ.ttv_vec[j] = reshape(bufs[j][1:(n * rks[j] * rks[j + 1])], n, rks[j], rks[j + 1])
    end
    ψ.ttv_rks[k + 1] = rks[k + 1]
    return orthogonalize(ψ; i = k)
end

# orthogonalize(x; i=1) — src/tt_tools.jl:511-543
function orthogonalize(x::TTvector{Float64, N}; i = 1::Int) where {N}
    @assert(1 ≤ i ≤ x.N, DimensionMismatch("Impossible orthogonalization"))
    y = zeros_tt(Float64, x.ttv_dims, x.ttv_rks)    # max-size buffers (output ranks never exceed the input's)
    yr = zeros(Int64, N + 1); yot = zeros(Int64, N)
    px, py = _ptrs(x.ttv_vec), _ptrs(y.ttv_vec)
    GC.@preserve x y px py _chk(ccall((:ttn_orthogonalize_f64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Int64, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Int64}),
        N, _dims(x.ttv_dims), px, x.ttv_rks, i, py, yr, yot))
    # the library writes each core compactly with the NEW ranks at the start of its buffer: re-wrap
    for k in 1:N
        n = x.ttv_dims[k]
        y.ttv_vec[k] = reshape(vec(y.ttv_vec[k])[1:(n * yr[k] * yr[k + 1])], n, yr[k], yr[k + 1])
    end
    y.ttv_rks .= yr; y.ttv_ot .= yot
    return y
end

# tt_compress!(ψ, max_bond; truncerr, sweeps, verbose) — src/tt_tools.jl:772-789.
# Mutates ψ.ttv_vec[k] slots and ψ.ttv_rks IN PLACE (QTTvector wrappers share those arrays,
# src/qtt_tools.jl:783-786) and returns ψ itself (test/test_tt_tools.jl:514).
function tt_compress!(ψ::TTvector{Float64, N}, max_bond::Int; truncerr::Real = 0.0, sweeps::Int = 1, verbose::Bool = false) where {N}
    @assert(sweeps ≥ 1, "sweeps must be >= 1")
    if verbose                               # the two log lines test/test_tt_tools.jl:572 asserts on
        for sw in 1:sweeps
            @info "TT compress: sweep $sw (L→R)"
            @info "TT compress: sweep $sw (R→L)"
        end
    end
    # a rank-deficient bond may grow to min(n r_left, n r_right, max_bond): size the in/out buffers for that
    need = zeros(Int64, N + 1)
    _chk(ccall((:ttn_compress_rank_bound, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}),
        N, _dims(ψ.ttv_dims), ψ.ttv_rks, min(max_bond, typemax(Int64) >> 1), sweeps, 0, need, C_NULL))
    bufs = [zeros(Float64, ψ.ttv_dims[k] * need[k] * need[k + 1]) for k in 1:N]
    for k in 1:N
        copyto!(bufs[k], vec(ψ.ttv_vec[k]))
    end
    rks = copy(ψ.ttv_rks)
    pb = Ptr{Float64}[pointer(c) for c in bufs]
    GC.@preserve bufs pb _chk(ccall((:ttn_compress_f64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Int64, Float64, Int64),
        N, _dims(ψ.ttv_dims), pb, rks, min(max_bond, typemax(Int64) >> 1), Float64(truncerr), sweeps))
    for k in 1:N
        n = ψ.ttv_dims[k]
        ψ.ttv_vec[k] = reshape(bufs[k][1:(n * rks[k] * rks[k + 1])], n, rks[k], rks[k + 1])
    end
    ψ.ttv_rks .= rks
    return ψ
end

# ---- ComplexF64 (include/ttn.h, "ComplexF64 trains and operators"): `*` (complex x complex and the two mixed forms), `+`, `dot`,
# `tt_compress!` bound to the stateless _c64 entry points.  A Julia Array{ComplexF64} is interleaved (re, im) in memory, which is what
# the library reads, so the pointers are passed as they are.  Like the rest of this file these lines have NEVER been executed.
const _CF = ComplexF64
_cptrs(v::Vector{<:Array{_CF}}) = Ptr{Float64}[Ptr{Float64}(pointer(c)) for c in v]
_anyptrs(v::Vector{<:Array{Float64}}) = _ptrs(v)
_anyptrs(v::Vector{<:Array{_CF}}) = _cptrs(v)

function _apply_c64(A::TToperator{TA, N}, v::TTvector{TV, N}) where {TA, TV, N}
    @assert A.tto_dims == v.ttv_dims "Incompatible dimensions"
    y = zeros_tt(_CF, A.tto_dims, A.tto_rks .* v.ttv_rks)
    pa, px, py = _anyptrs(A.tto_vec), _anyptrs(v.ttv_vec), _cptrs(y.ttv_vec)
    GC.@preserve A v y pa px py _chk(ccall((:ttn_apply_c64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}, Cint, Cint),
        N, _dims(A.tto_dims), pa, A.tto_rks, px, v.ttv_rks, py, Cint(TA == _CF), Cint(TV == _CF)))
    return y
end
*(A::TToperator{_CF, N}, v::TTvector{_CF, N}) where {N} = _apply_c64(A, v)
*(A::TToperator{Float64, N}, v::TTvector{_CF, N}) where {N} = _apply_c64(A, v)      # Δ * ψ, ψ from real-time TDVP
*(A::TToperator{_CF, N}, v::TTvector{Float64, N}) where {N} = _apply_c64(A, v)      # fourier_qtto * qtt_sin

function +(x::TTvector{_CF, N}, y::TTvector{_CF, N}) where {N}
    @assert x.ttv_dims == y.ttv_dims "Incompatible dimensions"
    rks = x.ttv_rks + y.ttv_rks; rks[1] = 1; rks[end] = 1
    z = zeros_tt(_CF, x.ttv_dims, rks)
    px, py, pz = _cptrs(x.ttv_vec), _cptrs(y.ttv_vec), _cptrs(z.ttv_vec)
    GC.@preserve x y z px py pz _chk(ccall((:ttn_add_c64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}),
        N, _dims(x.ttv_dims), px, x.ttv_rks, py, y.ttv_rks, pz))
    return z
end

# dot(A, B) conjugates its FIRST argument (src/tt_operations.jl:243-248)
function TensorTrainNumerics.dot(A::TTvector{_CF, N}, B::TTvector{_CF, N}) where {N}
    @assert A.ttv_dims == B.ttv_dims "TT dimensions are not compatible"
    out = zeros(Float64, 2)
    pa, pb = _cptrs(A.ttv_vec), _cptrs(B.ttv_vec)
    GC.@preserve A B pa pb out _chk(ccall((:ttn_dot_c64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Float64}),
        N, _dims(A.ttv_dims), pa, A.ttv_rks, pb, B.ttv_rks, out))
    return complex(out[1], out[2])
end

function tt_compress!(ψ::TTvector{_CF, N}, max_bond::Int; truncerr::Real = 0.0, sweeps::Int = 1, verbose::Bool = false) where {N}
    @assert(sweeps ≥ 1, "sweeps must be >= 1")
    if verbose
        for sw in 1:sweeps
            @info "TT compress: sweep $sw (L→R)"
            @info "TT compress: sweep $sw (R→L)"
        end
    end
    mb = min(max_bond, typemax(Int64) >> 1)
    need = zeros(Int64, N + 1)
    _chk(ccall((:ttn_compress_rank_bound, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}),
        N, _dims(ψ.ttv_dims), ψ.ttv_rks, mb, sweeps, 0, need, C_NULL))
    bufs = [zeros(_CF, ψ.ttv_dims[k] * need[k] * need[k + 1]) for k in 1:N]
    for k in 1:N
        copyto!(bufs[k], vec(ψ.ttv_vec[k]))
    end
    rks = copy(ψ.ttv_rks)
    pb = Ptr{Float64}[Ptr{Float64}(pointer(c)) for c in bufs]
    GC.@preserve bufs pb _chk(ccall((:ttn_compress_c64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Int64, Float64, Int64),
        N, _dims(ψ.ttv_dims), pb, rks, mb, Float64(truncerr), sweeps))
    for k in 1:N
        n = ψ.ttv_dims[k]
        ψ.ttv_vec[k] = reshape(bufs[k][1:(n * rks[k] * rks[k + 1])], n, rks[k], rks[k + 1])
    end
    ψ.ttv_rks .= rks
    return ψ
end

# op = x -> tt_compress!(A * x, max_bond) (src/solvers/euler.jl:55: the operator krylov_linsolve hands to KrylovKit, and the pattern of
# every time stepper) as ONE stateless call: A * x is never materialised, neither in HBM nor over PCIe (16.8 ms against 21.9 ms
# for `*` followed by `tt_compress!` on one d = 30 rank-64 train).  Drop-in for the closure at euler.jl:55:
#     op = x -> apply_compress(A, x, max_bond)
function apply_compress(A::TToperator{Float64, N}, v::TTvector{Float64, N}, max_bond::Int; truncerr::Real = 0.0, sweeps::Int = 1) where {N}
    @assert A.tto_dims == v.ttv_dims "Incompatible dimensions"
    @assert(sweeps ≥ 1, "sweeps must be >= 1")
    mb = min(max_bond, typemax(Int64) >> 1)
    cap = zeros(Int64, N + 1)
    _chk(ccall((:ttn_apply_compress_rank_bound, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Int64, Ptr{Int64}),
        N, _dims(v.ttv_dims), A.tto_rks, v.ttv_rks, mb, sweeps, cap))
    bufs = [zeros(Float64, v.ttv_dims[k] * cap[k] * cap[k + 1]) for k in 1:N]
    rks = zeros(Int64, N + 1)
    pa, px = _ptrs(A.tto_vec), _ptrs(v.ttv_vec)
    pb = Ptr{Float64}[pointer(c) for c in bufs]
    GC.@preserve A v bufs pa px pb _chk(ccall((:ttn_apply_compress_f64, LIB), Cint,
        (Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Int64}, Int64, Float64, Int64),
        N, _dims(v.ttv_dims), pa, A.tto_rks, px, v.ttv_rks, pb, rks, mb, Float64(truncerr), sweeps))
    y = zeros_tt(Float64, v.ttv_dims, rks)
    for k in 1:N
        n = v.ttv_dims[k]
        y.ttv_vec[k] = reshape(bufs[k][1:(n * rks[k] * rks[k + 1])], n, rks[k], rks[k + 1])
    end
    return y
end

# Device-resident chains (Krylov / RK4 inner loops, src/solvers/euler.jl:55,199-204) use the handle API:
#   h = Ref{Ptr{Cvoid}}(); ccall((:ttn_tt_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Ptr{Cvoid}}), ...)
#   ccall((:ttn_apply_compress, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Int64), A, x, y, r, 0.0, 1)
# so that tt_compress!(A*x, r) never crosses PCIe (ttn_apply_compress fuses the apply into the first L->R sweep: A*x is
# never written to HBM).
#
# Core-wise sharded chains (one segment of the chain per GPU / Julia worker, INTEGRATION.md §5): a segment is an ordinary
# handle with open boundary ranks; one direction of a sweep over the local bonds and the boundary-core hand-off are
#   ccall((:ttn_sweep, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Int64, Float64), y, k_first, k_last, max_bond, truncerr)
#   ccall((:ttn_tt_core_extent, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), y, k, n, bl, br)
#   ccall((:ttn_tt_core_export, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Int64}), y, k, devbuf, devrks)   # -> ncclSend
#   ccall((:ttn_tt_core_import, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Int64}, Int64, Int64), y, k, devbuf, devrks, bl, br)
# (k, k_first, k_last 1-based like _tt_bond_truncate!; devbuf / devrks are device pointers).
#
# Site-swap chains (INTEGRATION.md §2): hadamard_ttm and reorder run on handles,
#   ccall((:ttn_hadamard_ttm, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Int64, Int64), x, y, z, tol, rmax, work_cap)
#   ccall((:ttn_swap_sites, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Float64), q, length(swaps), swaps, threshold)
# with swaps = _bubble_sort_swaps(perm) exactly as reorder computes it (src/qtt_tools.jl:759); ttn_compress_status reports a
# rank that outgrew its slot (-5) or a Jacobi SVD that hit its sweep limit (-9).
#
# Two-site solvers on handles (INTEGRATION.md §2): x receives the result, its capacity bounds the adapted ranks,
#   ccall((:ttn_mals_linsolve, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Int64), A, b, x0, x, tol, rmax)
#   ccall((:ttn_dmrg_linsolve, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Int64, Ptr{Int64}, Ptr{Int64}),
#         A, b, x0, x, tol, length(sweep_schedule), sweep_schedule, rmax_schedule)      # dmrg_linsolve(...; N = 2), dmrg.jl:388
#   ccall((:ttn_dmrg_linsolve_it, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Int64, Ptr{Int64}, Ptr{Int64}, Cint, Int64, Float64, Int64),
#         A, b, x0, x, tol, length(sweep_schedule), sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh)
# (the keyword form, dmrg.jl:392-396: local systems above itslv_thresh unknowns — or all of them with it_solver — by matrix-free CG).
#
# Status is sticky per handle: ttn_compress_status(h, C_NULL) returns the most severe error any compress / sweep / swap / solver call
# recorded on h since the last query and clears it.  Most severe first: Lanczos exhaustion -9, a non-finite local eigenpair -9,
# singular local system -10, ranks that differ from the start handle -1, capacity -5, Jacobi sweep limit -9.
# ccall((:ttn_status_all, LIB), Cint, ()) answers for every live handle and for handles freed with an unread code, in one synchronisation.

# ---- Two-site eigensolvers (src/solvers/dmrg.jl:501-578, src/solvers/mals.jl:335-425) --------------------------------------------
# One train through the handle API: upload A and tt_start, solve on the device, download the eigenvector.  The rank capacity is the
# reference's buffer bound min(rmax, prod(dims[1:k]), prod(dims[k+1:end])) clamped to n_k * rank <= 256 (the device's SVD core moves).
function _eigsolve_dev(sym::Symbol, mode::Int, A::TToperator{Float64, N}, x0::TTvector{Float64, N}, tol, sweep_schedule, rmax_schedule,
                       it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh) where {N}
    dims = _dims(x0.ttv_dims)
    ss, rs = Int64[sweep_schedule...], Int64[rmax_schedule...]
    length(ss) == length(rs) || throw(AssertionError("Sweep schedule error"))
    rtop = maximum(rs)
    cap = Int64[k == 0 || k == N ? 1 : max(min(rtop, prod(dims[1:k]), prod(dims[(k + 1):end]), div(256, max(dims[k], dims[k + 1]))), x0.ttv_rks[k + 1])
                for k in 0:N]
    hl = Ref{Int64}(0)
    _chk(ccall((:ttn_eigsolve_history_len, LIB), Cint, (Cint, Int64, Int64, Ptr{Int64}, Ref{Int64}), Cint(mode), N, length(ss), ss, hl))
    hA, hx0, hx = Ref{Ptr{Cvoid}}(), Ref{Ptr{Cvoid}}(), Ref{Ptr{Cvoid}}()
    pa, px = _ptrs(A.tto_vec), _ptrs(x0.ttv_vec)
    GC.@preserve A x0 pa px begin
        _chk(ccall((:ttn_tto_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ref{Ptr{Cvoid}}), N, dims, A.tto_rks, pa, hA))
        _chk(ccall((:ttn_tt_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Ptr{Cvoid}}), N, dims, x0.ttv_rks, 1, hx0))
        _chk(ccall((:ttn_tt_upload, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Int64}), hx0[], 0, px, x0.ttv_rks, x0.ttv_ot))
    end
    _chk(ccall((:ttn_tt_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Ptr{Cvoid}}), N, dims, cap, 1, hx))
    E = zeros(Float64, max(hl[], 1))
    r_hist = zeros(Int64, max(hl[], 1))
    _chk(ccall(sym == :dmrg ? (:ttn_dmrg_eigsolve, LIB) : (:ttn_mals_eigsolve, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Int64, Ptr{Int64}, Ptr{Int64}, Cint, Int64, Float64, Int64, Int64, Ptr{Float64}, Ptr{Int64}),
        hA[], hx0[], hx[], tol, length(ss), ss, rs, Cint(it_solver), linsolv_maxiter, linsolv_tol, itslv_thresh, hl[], E, r_hist))
    rks, ot = zeros(Int64, N + 1), zeros(Int64, N)
    _chk(ccall((:ttn_tt_ranks, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}), hx[], 0, rks, ot))
    x = zeros_tt(Float64, x0.ttv_dims, rks)
    px = _ptrs(x.ttv_vec)
    GC.@preserve x px _chk(ccall((:ttn_tt_download, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Ptr{Float64}}), hx[], 0, px))
    x.ttv_ot .= ot
    ccall((:ttn_tt_free, LIB), Cint, (Ptr{Cvoid},), hx0[]); ccall((:ttn_tt_free, LIB), Cint, (Ptr{Cvoid},), hx[])
    ccall((:ttn_tto_free, LIB), Cint, (Ptr{Cvoid},), hA[])
    return E[1:hl[]], x, r_hist[1:hl[]]
end

function dmrg_eigsolve(A::TToperator{Float64, D}, tt_start::TTvector{Float64, D}; N = 2, tol = 1.0e-12, sweep_schedule = [2],
                       rmax_schedule = [isqrt(prod(tt_start.ttv_dims))], it_solver = false, linsolv_maxiter = 200,
                       linsolv_tol = max(sqrt(tol), 1.0e-8), itslv_thresh = 256) where {D}
    N == 2 || error("dmrg_eigsolve: only the two-site scheme N = 2 runs on the device")
    return _eigsolve_dev(:dmrg, 1, A, tt_start, tol, sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh)
end

function mals_eigsolve(A::TToperator{Float64, N}, tt_start::TTvector{Float64, N}; tol = 1.0e-12, sweep_schedule = [2],
                       rmax_schedule = [round(Int, sqrt(prod(tt_start.ttv_dims)))], it_solver = false, linsolv_maxiter = 200,
                       linsolv_tol = max(sqrt(tol), 1.0e-8), itslv_thresh = 256) where {N}
    return _eigsolve_dev(:mals, 0, A, tt_start, tol, sweep_schedule, rmax_schedule, it_solver, linsolv_maxiter, linsolv_tol, itslv_thresh)
end

# ---- One-site eigensolvers (src/solvers/als.jl:251-426) ------------------------------------------------------------------------
# Written against include/ttn.h and not executed (no Julia on the build machines).  The capacity of x is the largest rank any stage
# holds: the start ranks, then r_and_d_to_rks(fill(rmax)) of every later stage.
function _als_eig_dev(gen::Bool, A::TToperator{Float64, N}, S, x0::TTvector{Float64, N}, sweep_schedule, rmax_schedule, noise_schedule,
                      seed, it_solver, maxiter, linsolv_tol, itslv_thresh) where {N}
    dims = _dims(x0.ttv_dims)
    ss, rs = Int64[sweep_schedule...], Int64[rmax_schedule...]
    ns = Float64[noise_schedule...]
    length(ss) == length(rs) == length(ns) || throw(AssertionError("Sweep schedule error"))
    cap = Int64[x0.ttv_rks...]
    for j in 2:length(rs)
        cap = max.(cap, r_and_d_to_rks(vcat(1, fill(rs[j], N - 1), 1), x0.ttv_dims; rmax = rs[j]))
    end
    hl = Ref{Int64}(0)
    _chk(ccall((:ttn_eigsolve_history_len, LIB), Cint, (Cint, Int64, Int64, Ptr{Int64}, Ref{Int64}), Cint(2), N, length(ss), ss, hl))
    hA, hS, hx0, hx = Ref{Ptr{Cvoid}}(), Ref{Ptr{Cvoid}}(C_NULL), Ref{Ptr{Cvoid}}(), Ref{Ptr{Cvoid}}()
    pa, px = _ptrs(A.tto_vec), _ptrs(x0.ttv_vec)
    GC.@preserve A x0 pa px begin
        _chk(ccall((:ttn_tto_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ref{Ptr{Cvoid}}), N, dims, A.tto_rks, pa, hA))
        _chk(ccall((:ttn_tt_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Ptr{Cvoid}}), N, dims, x0.ttv_rks, 1, hx0))
        _chk(ccall((:ttn_tt_upload, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Int64}), hx0[], 0, px, x0.ttv_rks, x0.ttv_ot))
    end
    if gen
        ps = _ptrs(S.tto_vec)
        GC.@preserve S ps _chk(ccall((:ttn_tto_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ref{Ptr{Cvoid}}), N, dims, S.tto_rks, ps, hS))
    end
    _chk(ccall((:ttn_tt_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Ptr{Cvoid}}), N, dims, cap, 1, hx))
    E = zeros(Float64, max(hl[], 1))
    if gen
        _chk(ccall((:ttn_als_gen_eigsolve, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Cint, Int64, Int64, Ptr{Float64}),
            hA[], hS[], hx0[], hx[], length(ss), ss, rs, Cint(it_solver), itslv_thresh, hl[], E))
    else
        _chk(ccall((:ttn_als_eigsolve, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Cint, Int64, Float64, Int64, Int64, Ptr{Float64}),
            hA[], hx0[], hx[], length(ss), ss, rs, ns, Int64(seed), Cint(it_solver), maxiter, linsolv_tol, itslv_thresh, hl[], E))
    end
    rks, ot = zeros(Int64, N + 1), zeros(Int64, N)
    _chk(ccall((:ttn_tt_ranks, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}), hx[], 0, rks, ot))
    x = zeros_tt(Float64, x0.ttv_dims, rks)
    px = _ptrs(x.ttv_vec)
    GC.@preserve x px _chk(ccall((:ttn_tt_download, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Ptr{Float64}}), hx[], 0, px))
    x.ttv_ot .= ot
    ccall((:ttn_tt_free, LIB), Cint, (Ptr{Cvoid},), hx0[]); ccall((:ttn_tt_free, LIB), Cint, (Ptr{Cvoid},), hx[])
    ccall((:ttn_tto_free, LIB), Cint, (Ptr{Cvoid},), hA[])
    gen && ccall((:ttn_tto_free, LIB), Cint, (Ptr{Cvoid},), hS[])
    return E[1:hl[]], x
end

function als_eigsolve(A::TToperator{Float64, N}, tt_start::TTvector{Float64, N}; sweep_schedule = [2],
                      rmax_schedule = [maximum(tt_start.ttv_rks)], noise_schedule = zeros(length(rmax_schedule)), it_solver = false,
                      itslv_thresh = 1024, maxiter = 200, linsolv_tol = 1.0e-8, seed = 0) where {N}
    return _als_eig_dev(false, A, nothing, tt_start, sweep_schedule, rmax_schedule, noise_schedule, seed, it_solver, maxiter, linsolv_tol,
                        itslv_thresh)
end

function als_gen_eigsolv(A::TToperator{Float64, N}, S::TToperator{Float64, N}, tt_start::TTvector{Float64, N}; sweep_schedule = [2],
                         rmax_schedule = [maximum(tt_start.ttv_rks)], tol = 1.0e-10, it_solver = false, itslv_thresh = 2500) where {N}
    return _als_eig_dev(true, A, S, tt_start, sweep_schedule, rmax_schedule, zeros(length(rmax_schedule)), 0, it_solver, 1, 1.0e-8,
                        itslv_thresh)
end

# ---- TDVP local contractions (src/solvers/tdvp.jl:29-43, :205-208) ------------------------------------------------------------
# The five @tensor kernels of tdvp1sweep! / tdvp2sweep!, for Float64 and ComplexF64 arrays in the layouts the sweeps hold
# (sites (l,s,r), operator cores (a,s,b,s')).  KrylovKit's exponentiate keeps calling them as closures, unchanged.
const _TE = Union{Float64, ComplexF64}
_cplx(::Type{Float64}) = Cint(0)
_cplx(::Type{ComplexF64}) = Cint(1)
_f64ptr(X::Array{T}) where {T <: _TE} = Ptr{Float64}(pointer(X))

function _tdvp_contract(op::Int, ::Type{T}, dims7::NTuple{7, Int}, FL, FR, X, M1, M2, out::Array{T}) where {T <: _TE}
    d7 = Int64[dims7...]
    p(Z) = Z === nothing ? Ptr{Float64}(C_NULL) : _f64ptr(Z)
    GC.@preserve FL FR X M1 M2 out d7 _chk(ccall((:ttn_tdvp_contract_f64, LIB), Cint,
        (Cint, Cint, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint),
        op, _cplx(T), 1, d7, p(FL), p(FR), p(X), p(M1), p(M2), _f64ptr(out), 0))
    return out
end

function _applyH1_lsr(AC::Array{T, 3}, FL::Array{T, 3}, FR::Array{T, 3}, M::Array{T, 4}) where {T <: _TE}
    Dl, d, Dr = size(AC); a, b = size(M, 1), size(M, 3)
    return _tdvp_contract(0, T, (Dl, d, Dr, a, b, 1, 1), FL, FR, AC, M, nothing, Array{T}(undef, Dl, d, Dr))
end

function _applyH0(C::Array{T, 2}, FL::Array{T, 3}, FR::Array{T, 3}) where {T <: _TE}
    Dl, Dr = size(C); a = size(FL, 2)
    return _tdvp_contract(1, T, (Dl, 1, Dr, a, 1, 1, 1), FL, FR, C, nothing, nothing, Array{T}(undef, Dl, Dr))
end

function _update_left_env(A::Array{T, 3}, M::Array{T, 4}, FL::Array{T, 3}) where {T <: _TE}
    Dl, d, Dr = size(A); a_in, a_out = size(M, 1), size(M, 3)
    return _tdvp_contract(2, T, (Dl, d, Dr, a_in, a_out, 1, 1), FL, nothing, A, M, nothing, Array{T}(undef, Dr, a_out, Dr))
end

function _update_right_env(A::Array{T, 3}, M::Array{T, 4}, FR::Array{T, 3}) where {T <: _TE}
    Dl, d, Dr = size(A); a_out, a_in = size(M, 1), size(M, 3)
    return _tdvp_contract(3, T, (Dl, d, Dr, a_in, a_out, 1, 1), nothing, FR, A, M, nothing, Array{T}(undef, Dl, a_out, Dl))
end

function _applyH2_lsr(AAC::Array{T, 4}, FL::Array{T, 3}, FR::Array{T, 3}, M1::Array{T, 4}, M2::Array{T, 4}) where {T <: _TE}
    Dl, d1, d2, Dr = size(AAC); a, b, c = size(M1, 1), size(M1, 3), size(M2, 3)
    return _tdvp_contract(4, T, (Dl, d1, Dr, a, b, c, d2), FL, FR, AAC, M1, M2, Array{T}(undef, Dl, d1, d2, Dr))
end

# ---- TT operator algebra (src/tt_operations.jl:71-95, :162-216, :271-338, :427-435; src/tt_tools.jl:296-333, :723-735) -------------
# Written against include/ttn.h and not executed (no Julia on the build machines).  A device operator is immutable, so every entry
# point returns a new handle: the stateless forms below upload their operands, run one operation and download the result.  A chain
# (assemble a generator, then round it) should keep the handles and call `_tto_op` / `ttn_tto_compress` on them instead.
function _tto_up(A::TToperator{Float64, N}) where {N}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    pa = _ptrs(A.tto_vec)
    GC.@preserve A pa _chk(ccall((:ttn_tto_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Float64}}, Ref{Ptr{Cvoid}}),
        N, _dims(A.tto_dims), A.tto_rks, pa, h))
    any(!=(0), A.tto_ot) && _chk(ccall((:ttn_tto_set_ot, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), h[], Int64[A.tto_ot...]))
    return h[]
end

function _ttv_up(x::TTvector{Float64, N}) where {N}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    px = _ptrs(x.ttv_vec)
    GC.@preserve x px begin
        _chk(ccall((:ttn_tt_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Ptr{Cvoid}}), N, _dims(x.ttv_dims), x.ttv_rks, 1, h))
        _chk(ccall((:ttn_tt_upload, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Int64}), h[], 0, px, x.ttv_rks, x.ttv_ot))
    end
    return h[]
end

_tto_free(h) = ccall((:ttn_tto_free, LIB), Cint, (Ptr{Cvoid},), h)
_ttv_free(h) = ccall((:ttn_tt_free, LIB), Cint, (Ptr{Cvoid},), h)

# download a result handle as a TToperator and release it
function _tto_down(h::Ptr{Cvoid})
    d = Ref{Int64}(0)
    _chk(ccall((:ttn_tto_ranks, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), h, d, C_NULL, C_NULL, C_NULL))
    N = Int(d[])
    dims, rks, ot = zeros(Int64, N), zeros(Int64, N + 1), zeros(Int64, N)
    _chk(ccall((:ttn_tto_ranks, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), h, C_NULL, dims, rks, ot))
    vec = [zeros(Float64, dims[k], dims[k], rks[k], rks[k + 1]) for k in 1:N]
    pv = _ptrs(vec)
    GC.@preserve vec pv _chk(ccall((:ttn_tto_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), h, pv))
    _tto_free(h)
    return TToperator{Float64, N}(N, vec, Tuple(dims), rks, ot)
end

# sym in (:ttn_tto_mul, :ttn_tto_inner, :ttn_tto_add, :ttn_tto_kron) on two operator handles
function _tto_op(sym::Symbol, hA::Ptr{Cvoid}, hB::Ptr{Cvoid})
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _chk(ccall((sym, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), hA, hB, out))
    return out[]
end

function _tto_binary(sym::Symbol, A::TToperator{Float64}, B::TToperator{Float64})
    hA, hB = _tto_up(A), _tto_up(B)
    try
        return _tto_down(_tto_op(sym, hA, hB))
    finally
        _tto_free(hA); _tto_free(hB)
    end
end

function *(A::TToperator{Float64, N}, B::TToperator{Float64, N}) where {N}
    @assert A.tto_dims == B.tto_dims "Incompatible dimensions"
    return _tto_binary(:ttn_tto_mul, A, B)
end

function +(A::TToperator{Float64, N}, B::TToperator{Float64, N}) where {N}
    @assert A.tto_dims == B.tto_dims "Incompatible dimensions"
    return _tto_binary(:ttn_tto_add, A, B)
end

function TensorTrainNumerics.:⨝(A::TToperator{Float64, N}, B::TToperator{Float64, N}) where {N}
    return _tto_binary(:ttn_tto_inner, A, B)
end

# kron / ⊗ and concatenate only regroup cores: the reference's vcat stays the host form; on handles it is ttn_tto_kron / ttn_tt_kron.

function *(a::Float64, A::TToperator{Float64, N}) where {N}
    hA = _tto_up(A)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    try
        _chk(ccall((:ttn_tto_scale, LIB), Cint, (Float64, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), a, hA, out))
        return _tto_down(out[])
    finally
        _tto_free(hA)
    end
end

function TensorTrainNumerics.outer_product(x::TTvector{Float64, N}, y::TTvector{Float64, N}) where {N}
    hx, hy = _ttv_up(x), _ttv_up(y)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    try
        _chk(ccall((:ttn_tt_outer, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{Ptr{Cvoid}}), hx, hy, 0, out))
        return _tto_down(out[])
    finally
        _ttv_free(hx); _ttv_free(hy)
    end
end

function TensorTrainNumerics.ttv_to_diag_tto(x::TTvector{Float64, N}) where {N}
    hx = _ttv_up(x)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    try
        _chk(ccall((:ttn_tt_diag_tto, LIB), Cint, (Ptr{Cvoid}, Int64, Ref{Ptr{Cvoid}}), hx, 0, out))
        return _tto_down(out[])
    finally
        _ttv_free(hx)
    end
end

# ttv_to_tto(tt_compress!(tto_to_ttv(A), max_bond; truncerr, sweeps)) without leaving the device (no reference method of this name:
# the examples round operators through tto_to_ttv by hand)
function tto_compress(A::TToperator{Float64, N}, max_bond::Integer = typemax(Int64) >> 1; truncerr::Float64 = 0.0, sweeps::Integer = 1) where {N}
    hA = _tto_up(A)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    try
        _chk(ccall((:ttn_tto_compress, LIB), Cint, (Ptr{Cvoid}, Int64, Float64, Int64, Ref{Ptr{Cvoid}}), hA, max_bond, truncerr, sweeps, out))
        return _tto_down(out[])
    finally
        _tto_free(hA)
    end
end

# handle-level conversions and the vector kron, for chains that stay on the device
_tto_to_tt(hA::Ptr{Cvoid}, hy::Ptr{Cvoid}) = _chk(ccall((:ttn_tto_to_tt, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), hA, hy))
_tt_kron(hx::Ptr{Cvoid}, hy::Ptr{Cvoid}, hz::Ptr{Cvoid}) = _chk(ccall((:ttn_tt_kron, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), hx, hy, hz))
function _tto_from_tt(hx::Ptr{Cvoid}, b::Integer = 0)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _chk(ccall((:ttn_tto_from_tt, LIB), Cint, (Ptr{Cvoid}, Int64, Ref{Ptr{Cvoid}}), hx, b, out))
    return out[]
end

# ---- time steps (include/ttn_step.h; DESIGN.md §4.23) ------------------------------------------------------------------------------
# Written against include/ttn_step.h and not executed (no Julia on the build machines).
# download train 0 of a result handle as a TTvector and release the handle
function _ttv_down(h::Ptr{Cvoid}, dims::NTuple{N, Int64}) where {N}
    rks, ot = zeros(Int64, N + 1), zeros(Int64, N)
    _chk(ccall((:ttn_tt_ranks, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}), h, 0, rks, ot))
    x = zeros_tt(Float64, dims, rks)
    px = _ptrs(x.ttv_vec)
    GC.@preserve x px _chk(ccall((:ttn_tt_download, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Ptr{Float64}}), h, 0, px))
    x.ttv_ot .= ot
    _ttv_free(h)
    return x
end

# alpha * x + beta * (A * y) in one launch: the Crank-Nicolson right-hand side (I + (h/2) A) u is apply_axpby(1.0, u, h / 2, A, u), a
# residual M * sol - u_prev is apply_axpby(-1.0, u_prev, 1.0, M, sol).  Bit for bit alpha * x + beta * (A * y) as the reference's own
# operators evaluate it (scalar * first, then +).
function apply_axpby(alpha::Float64, x::TTvector{Float64, N}, beta::Float64, A::TToperator{Float64, N}, y::TTvector{Float64, N}) where {N}
    hA, hx, hy = _tto_up(A), _ttv_up(x), _ttv_up(y)
    cap = vcat(1, x.ttv_rks[2:N] .+ A.tto_rks[2:N] .* y.ttv_rks[2:N], 1)
    hz = Ref{Ptr{Cvoid}}(C_NULL)
    try
        _chk(ccall((:ttn_tt_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Ptr{Cvoid}}), N, _dims(x.ttv_dims), cap, 1, hz))
        _chk(ccall((:ttn_apply_axpby, LIB), Cint, (Ptr{Float64}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
            Float64[alpha], hx, Float64[beta], hA, hy, hz[]))
        return _ttv_down(hz[], x.ttv_dims)
    finally
        _tto_free(hA); _ttv_free(hx); _ttv_free(hy)
    end
end

# increase_ranks(x, max_bond; rks, noise) (src/tt_tools.jl:480-490) on the device; the noise blocks come from the library's seeded
# splitmix64 stream (`seed`), not from Julia's RNG
function increase_ranks_device(x::TTvector{Float64, N}, max_bond::Int; rks = vcat(1, max_bond * ones(Int, N - 1), 1), noise::Float64 = 0.0,
        seed::Integer = 0) where {N}
    @assert(max_bond > maximum(x.ttv_rks), "New bond dimension too low")
    new = Int64.(r_and_d_to_rks(rks, x.ttv_dims; rmax = max_bond))
    hx = _ttv_up(x)
    hy = Ref{Ptr{Cvoid}}(C_NULL)
    try
        _chk(ccall((:ttn_tt_create, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Ptr{Cvoid}}), N, _dims(x.ttv_dims), new, 1, hy))
        _chk(ccall((:ttn_tt_increase_ranks, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Float64, UInt64, Ptr{Cvoid}), hx, new, noise, UInt64(seed), hy[]))
        return _ttv_down(hy[], x.ttv_dims)
    finally
        _ttv_free(hx)
    end
end

end # module
