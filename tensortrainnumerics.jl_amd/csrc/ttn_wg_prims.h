// ttn_wg_prims.h — workgroup primitives of the one-workgroup-per-train kernels: the bottom layer of the dense family
// (ttn_wg_prims.h <- ttn_wg_gemm.h <- ttn_wg_lq.h / ttn_wg_jacobi.h / ttn_wg_chol.h <- ttn_dense_kernels.h <- ttn_swap_kernels.h;
// the design of the family stands in ttn_dense_kernels.h).
//
// Provides (top to bottom):
//   TTN_SETPRIO_GEMM / TTN_SETPRIO_BASE        wave priorities
//   TTN_LDS_IMG, TTN_LDS_COLS                  size of the LDS image region of either build (1024 / 512 threads)
//   dpp_mov_f64, row16_*, wave_sum / wave_max  DPP wave reductions
//   wg_sum / wg_max                            workgroup reductions
//   lds_f64, lds_i32, lds_i64, gmem_f64, gmem_wf64, mfma_acc_t
//                                              address-space and MFMA accumulator typedefs
//   uni32 / uni64 / unip / unif64 / uniIdx / uniView
//                                              pins of workgroup-uniform values (the rule below)
//   wg_batched, wg_copy_scale, wg_absmax, wg_copy_to_view
//                                              element loops over global memory with several loads in flight
//   fast_rcp, fast_rsqrt2                      Newton-polished v_rcp_f64 / v_rsq_f64
// Needs: ttn_common.h (View, Idx, ix, TTN_WG, TTN_PRIO_BASE).
// Used by: every header of the family, and directly by ttn_densefact_kernels.h and ttn_ortho_fused.h.
#pragma once
#include "ttn_common.h"
#include <float.h>

// Wave priorities (s_setprio, a per-wave hint to the SIMD's issue arbiter): with two workgroups per CU one of them is usually in a
// latency-bound phase (an eigensolver's serial chain, a Cholesky pivot, a Jacobi sweep) while the other streams MFMAs; the
// latency-bound waves issue first.  Levels: TTN_PRIO_BASE for everything that is not a matrix product, 0 inside the matrix-product
// routines, higher inside the eigensolver (ttn_eig_kernels.h).
#define TTN_SETPRIO_GEMM() __builtin_amdgcn_s_setprio(0)
#define TTN_SETPRIO_BASE() __builtin_amdgcn_s_setprio(TTN_PRIO_BASE)

// The LDS IMAGE region (Jacobi / Cholesky / eigensolver images with leading dimension 128, LQ images, staged GEMM operands):
//   1024-thread build: 128 x 128 doubles, one workgroup per CU (its 16 waves at 128 VGPRs fill the register file anyway);
//   512-thread build:   64 x 128 doubles — the whole kernel then needs < 80 KB of LDS and TWO workgroups share a CU (8 waves at 128
//   VGPRs each), so the serial phases of one train (reflectors, pivots, bisection rounds, barriers) overlap the other's work.
//   Images of more than TTN_LDS_COLS columns take the blocked / global-memory forms there.
#if TTN_WG == 512
#define TTN_LDS_IMG (64 * 128)
#else
#define TTN_LDS_IMG (128 * 128)
#endif
#define TTN_LDS_COLS (TTN_LDS_IMG / 128)           // columns of a leading-dimension-128 image

// -------------------------------------------------------------------------------------------------
// workgroup reductions (1024 threads = 16 waves of 64)
// -------------------------------------------------------------------------------------------------
// Wave reductions on DPP row operations + lane reads: __shfl_xor compiles to ds_bpermute (an LDS round trip per step: 1250 clk
// per 64-lane sum measured with the workgroup busy, 440 for this form).  All 64 lanes must be active.
template <int CTRL>
__device__ inline double dpp_mov_f64(double v) {
    union { double d; int i[2]; } a, r;
    a.d = v;
    r.i[0] = __builtin_amdgcn_update_dpp(0, a.i[0], CTRL, 0xF, 0xF, true);
    r.i[1] = __builtin_amdgcn_update_dpp(0, a.i[1], CTRL, 0xF, 0xF, true);
    return r.d;
}
__device__ inline double row16_sum(double v) {
    v += dpp_mov_f64<0xB1>(v);     // quad_perm [1,0,3,2]
    v += dpp_mov_f64<0x4E>(v);     // quad_perm [2,3,0,1]
    v += dpp_mov_f64<0x141>(v);    // row_half_mirror
    v += dpp_mov_f64<0x140>(v);    // row_mirror
    return v;
}
__device__ inline double row16_max(double v) {
    v = fmax(v, dpp_mov_f64<0xB1>(v));
    v = fmax(v, dpp_mov_f64<0x4E>(v));
    v = fmax(v, dpp_mov_f64<0x141>(v));
    v = fmax(v, dpp_mov_f64<0x140>(v));
    return v;
}
__device__ inline double wave64_sum_fast(double v) {
    v = row16_sum(v);                                   // every lane of a 16-lane row holds the row sum
    union { double d; int i[2]; } u;
    u.d = v;
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        union { double d; int i[2]; } w;
        w.i[0] = __builtin_amdgcn_readlane(u.i[0], 16 * r);
        w.i[1] = __builtin_amdgcn_readlane(u.i[1], 16 * r);
        t += w.d;
    }
    return t;
}
__device__ inline double wave64_max_fast(double v) {
    v = row16_max(v);
    union { double d; int i[2]; } u;
    u.d = v;
    double t = -1.7976931348623157e308;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        union { double d; int i[2]; } w;
        w.i[0] = __builtin_amdgcn_readlane(u.i[0], 16 * r);
        w.i[1] = __builtin_amdgcn_readlane(u.i[1], 16 * r);
        t = fmax(t, w.d);
    }
    return t;
}
__device__ inline double wave_sum(double v) { return wave64_sum_fast(v); }
__device__ inline double wave_max(double v) { return wave64_max_fast(v); }
// red: LDS scratch of >= 32 doubles.  All threads get the result.
__device__ inline double wg_sum(double v, double* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    double t = (l < nw) ? red[l] : 0.0;
    __syncthreads();                                   // red is free again: the caller's next routine may write it at once
    t = wave_sum(t);
    return t;
}
__device__ inline double wg_max(double v, double* red) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    double t = (l < nw) ? red[l] : 0.0;
    __syncthreads();                                   // (as above)
    t = wave_max(t);
    return t;
}

// -------------------------------------------------------------------------------------------------
// MFMA accumulator and address-space typedefs: through a generic pointer every access is a FLAT instruction
// -------------------------------------------------------------------------------------------------
typedef double mfma_acc_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) double lds_f64;
typedef __attribute__((address_space(3))) long long lds_i64;
typedef __attribute__((address_space(3))) int lds_i32;
// GEMM A/B operands always live in global memory.  Loading them through the generic `double*` of a View makes the
// compiler emit flat_load, which counts on lgkmcnt as well as vmcnt — every `s_waitcnt lgkmcnt(0)` in front of an MFMA
// group (meant for the LDS fragment reads) then also waits for the global loads of the NEXT chunk: measured 49 % -> 7x %
// of the per-CU MFMA peak for the tiled GEMM once the loads are global_load.
typedef const __attribute__((address_space(1))) double gmem_f64;
typedef __attribute__((address_space(1))) double gmem_wf64;

// -------------------------------------------------------------------------------------------------
// Pins of workgroup-uniform values.
// Rule learnt the hard way: arguments of out-of-line device functions arrive in VGPRs, and anything
// loaded from memory the kernel also writes is a per-lane value to the compiler — pin workgroup-uniform values with
// uni32/uni64/unip, or every derived size, view and pointer occupies VGPRs and ends up in the stack frame.
// -------------------------------------------------------------------------------------------------
// workgroup-uniform values read from LDS land in VGPRs; readfirstlane moves them to SGPRs (the GEMM is VGPR-starved)
__device__ inline int uni32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline long long uni64(long long v) {
    const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffLL));
    const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return ((long long)hi << 32) | (unsigned int)lo;
}
template <typename PT> __device__ inline PT* unip(PT* q_) { return (PT*)uni64((long long)q_); }
__device__ inline double unif64(double v) { union { double d; long long i; } u; u.d = v; u.i = uni64(u.i); return u.d; }
__device__ inline Idx uniIdx(const Idx& d) { return Idx{uni32(d.q), uni64(d.lo), uni64(d.hi)}; }
__device__ inline View uniView(const View& v) { return View{(double*)uni64((long long)v.p), uniIdx(v.r), uniIdx(v.c)}; }

// -------------------------------------------------------------------------------------------------
// Element loops over global memory.  `for (e = tid; e < n; e += TTN_WG) dst[e] = f(src[e])` compiles to load, s_waitcnt vmcnt(0),
// store per trip (no unrolling, possible aliasing): a full memory round trip per ELEMENT of a thread.  wg_batched runs such a loop
// with U loads of a thread in flight before the first is used: load(e) returns what the element needs (index clamped: it must be
// harmless to call it twice for an e < n), use(e, value) consumes it.  It is used inside OUT-OF-LINE leaf routines only: inlined
// into the bond step the same loops cost 300 more spilled VGPRs (the step runs at the 128-register limit) and 19 % of its speed.
// -------------------------------------------------------------------------------------------------
template <int U, typename LoadF, typename UseF>
__device__ __forceinline__ void wg_batched(long long n, LoadF load, UseF use) {
    for (long long e0 = threadIdx.x; e0 < n; e0 += (long long)TTN_WG * U) {
        decltype(load(0LL)) v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { const long long e = e0 + (long long)u * TTN_WG; v[u] = load(e < n ? e : e0); }
#pragma unroll
        for (int u = 0; u < U; ++u) { const long long e = e0 + (long long)u * TTN_WG; if (e < n) use(e, v[u]); }
    }
}
// dst[e] = s * src[e], e < n
__device__ __noinline__ void wg_copy_scale(double* dst, const double* src, long long n, double s_) {
    dst = unip(dst); src = unip(src); n = uni64(n); s_ = unif64(s_);
    wg_batched<8>(n, [&](long long e) { return src[e]; }, [&](long long e, double v) { dst[e] = v * s_; });
}
// max |src[e]|, e < n (all threads get it)
__device__ __noinline__ double wg_absmax(const double* src, long long n, double* red) {
    src = unip(src); n = uni64(n); red = unip(red);
    double m_ = 0.0;
    wg_batched<8>(n, [&](long long e) { return src[e]; }, [&](long long, double v) { m_ = fmax(m_, fabs(v)); });
    return unif64(wg_max(m_, red));
}
// dst(i, j) = (lim_first ? i : j) < lim ? src[i + ld_first... : the commit copy of the factored route: element (row, col) of the rows x cols
// matrix `src` (element stride rs between rows, cs between columns) goes to the View `dst`; entries whose column (col_lim) or row
// (!col_lim) index is >= lim are written as zeros
__device__ __noinline__ void wg_copy_to_view(View dst, const double* src, int rows, int cols, long long rs, long long cs, int lim, int col_lim) {
    dst = uniView(dst); src = unip(src); rows = uni32(rows); cols = uni32(cols); rs = uni64(rs); cs = uni64(cs); lim = uni32(lim); col_lim = uni32(col_lim);
    const bool row_fast = rs <= cs;
    const int fast = row_fast ? rows : cols;                       // 32-bit index arithmetic (rows * cols < 2^31: at most 4096 x 16384)
    wg_batched<8>((long long)rows * cols,
                  [&](long long e) {
                      const int ei = (int)e, lo = ei % fast, hi = ei / fast;
                      const int i = row_fast ? lo : hi, j = row_fast ? hi : lo;
                      return ((col_lim ? j : i) < lim) ? src[i * rs + j * cs] : 0.0;
                  },
                  [&](long long e, double v) {
                      const int ei = (int)e, lo = ei % fast, hi = ei / fast;
                      const int i = row_fast ? lo : hi, j = row_fast ? hi : lo;
                      dst.p[ix(dst.r, i) + ix(dst.c, j)] = v;
                  });
}

// -------------------------------------------------------------------------------------------------
// Reciprocal and reciprocal square root from the hardware seeds
// -------------------------------------------------------------------------------------------------
__device__ inline double fast_rcp(double x) {       // ~2^-50 relative after one Newton step
    double y = __builtin_amdgcn_rcp(x);
    y = fma(fma(-x, y, 1.0), y, y);
    return y;
}
__device__ inline double fast_rsqrt2(double w) {    // two Newton steps on v_rsq_f64: full fp64 accuracy
    double y = __builtin_amdgcn_rsq(w);
    double h = 0.5 * w;
    y = y * fma(-h * y, y, 1.5);
    y = y * fma(-h * y, y, 1.5);
    return y;
}
