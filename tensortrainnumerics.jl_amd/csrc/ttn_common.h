// ttn_common.h — shared host/device declarations of libttn_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef TTN_WG
#define TTN_WG 1024            // threads of the dense (one-workgroup-per-train) kernels (512 is supported for experiments)
#endif
#define TTN_NWAVES (TTN_WG / 64)
// Register budget of the dense kernels: 128 VGPRs per lane in both builds.  1024 threads = 4 waves per SIMD already imply it; the
// 512-thread build asks for 4 waves per SIMD explicitly (second launch-bounds argument = minimum waves per execution unit), i.e.
// two resident workgroups per CU — without it the compiler would take up to 256 registers and one workgroup would own the CU.
#if TTN_WG == 512 && defined(TTN_WG512_ONE_PER_CU)
#define TTN_KERNEL_BOUNDS __launch_bounds__(512)        // experiment: up to 256 VGPRs, no spills, one workgroup per CU
#elif TTN_WG == 512
#define TTN_KERNEL_BOUNDS __launch_bounds__(512, 4)
#else
#define TTN_KERNEL_BOUNDS __launch_bounds__(TTN_WG)
#endif
// Wave priorities of the dense kernels (s_setprio; see ttn_wg_prims.h): matrix-product routines 0, everything else
// TTN_PRIO_BASE, the symmetric eigensolver TTN_EIG_PRIO, the one wave that carries the tridiagonalisation's serial chain
// TTN_TRIDIAG_PRIO.  Only the order matters (3/3/2 and 3/3/1 measure the same).  Without priorities the benchmark ran 556 k
// instead of 583 k cores/s (same box); one train alone on a CU sees no difference.
#define TTN_PRIO_BASE 1
#define TTN_EIG_PRIO 2
#define TTN_TRIDIAG_PRIO 3
#define TTN_MAX_D 64           // max chain length handled by the on-stack tables of the host API
#define TTN_SV_NONE (-1)

// Device view of one batch of TT vectors (see include/ttn.h: ttn_tt).
struct TTDev {
    double*        data;      // arena: train b, core k at data + b*stride + off[k]
    long long      stride;    // doubles per train
    const long long* off;     // [d+1] device, slot offsets from CAPACITY ranks
    long long*     rks;       // [batch][d+1] device, current ranks
    const int*     dims;      // [d] device
    const long long* cap;     // [d+1] device, capacity ranks
    int            d;
    int            batch;
};

// Device view of one TT operator, or of a batch of operators of equal dims and ranks (include/ttn_opbatch.h): operator b, core k at
// data + b*stride + off[k].  stride = 0: one operator serves every train.
struct TTODev {
    const double*  data;
    const long long* off;     // [d+1] device
    const long long* rks;     // [d+1] device
    const int*     dims;      // [d] device
    int            d;
    long long      stride;    // doubles per operator of a batch; 0 for a single operator
};

// A 2-level strided index: idx(i) = q ? (i % q)*lo + (i / q)*hi : i*lo.
// Lets a TT core (n, rl, rr) be read as the matrices the reference forms with
// permutedims+reshape (src/tt_tools.jl:746-752) without any copy.
struct Idx {
    int q;
    long long lo, hi;
};
struct View {
    double* p;
    Idx r, c;
};

__host__ __device__ inline long long ix(const Idx& d, int i) {
    return d.q ? (long long)(i % d.q) * d.lo + (long long)(i / d.q) * d.hi : (long long)i * d.lo;
}
__host__ __device__ inline Idx plain(long long stride) { return Idx{0, stride, 0}; }
__host__ __device__ inline View tview(View v) { return View{v.p, v.c, v.r}; }
__host__ __device__ inline View mkview(double* p, Idx r, Idx c) { return View{p, r, c}; }
__host__ __device__ inline long long minstride(const Idx& d) { return d.q ? (d.lo < d.hi ? d.lo : d.hi) : d.lo; }

// The dense kernels work "in units of s0 = max|M|", but their products do not: a Gram route takes 1 / (s0 s0) and sums squares of
// UNSCALED entries, an unscaled Householder reflector sums squares too, the output GEMM of a bond step multiplies a factor of size
// sqrt(s0) into the unscaled M (s0^1.5), the swap form carries s0^2, the rank rule squares sigma s0.  All of that is in range while
// the size of the matrix is within SCALE_SAFE.  Outside it the fast routes decline and the general routes take an exact power of two
// out of the matrix first and give it back to their outputs: extra passes for such a step only.
#define SCALE_SAFE_MIN 0x1p-256
#define SCALE_SAFE_MAX 0x1p+256
__host__ __device__ inline bool scale_safe(double s) { return s >= SCALE_SAFE_MIN && s <= SCALE_SAFE_MAX; }      // (false for 0, Inf and NaN)
// the exponent e (|e| <= 1020, even if `even`) with s / 2^e in [1/2, 2); 0 when s is within SCALE_SAFE, zero or not finite
__device__ inline int scale_rescue_exponent(double s, bool even) {
    if (!(s > 0.0) || !(s <= 1.7976931348623157e308) || scale_safe(s)) return 0;
    int e;
    (void)frexp(s, &e);
    e = e < -1020 ? -1020 : (e > 1020 ? 1020 : e);
    return even ? (e & ~1) : e;
}

// Per-train failure codes of the dense kernels.  The host maps each to a TTN_ERR_* code and a message (ttn_host_core.h: status_table).
enum TtnStatus : int {
    TTN_ST_JACOBI = 1,           // a Jacobi SVD hit its sweep limit
    TTN_ST_RANK_OVERFLOW = 2,    // a rank grew beyond the capacity of its handle / working slot
    TTN_ST_SINGULAR = 3,         // a local linear system is singular
    TTN_ST_RANKS_DIFFER = 4,     // a train's ranks differ from the bound of its handle (als_linsolve)
    TTN_ST_LANCZOS = 5,          // Lanczos exhausted its restarts with a residual above 1e3 * tol
    TTN_ST_NONFINITE = 6,        // a local eigenvalue or eigenvector entry was NaN or infinite (the sweep stops there)
};

// Per-train failure code of a handle (include/ttn.h: ttn_compress_status): the FIRST condition a train meets is kept — only the
// workgroup that owns train b writes status[b], so a plain test is enough.
__device__ inline void ttn_set_status(int* st, int code) { if (*st == 0) *st = code; }
