// ttn_measure_kernels.h — site-resolved measurements of a train x (include/ttn_measure.h): the profile
//       E_O[k]     = <x| O_k |x> / <x, x>                                 (one real n_k x n_k matrix O_k per site: an operator TABLE)
// and the two-point functions
//       C_PQ[i, j] = <x| P_i Q_j |x> / <x, x>                             for ALL pairs (i, j)
// in O(d) chain work plus O(d^2) short walks per train.  Float64 only; the bra and the ket are the same train.
//
//   phase 0   k_grad_chain (ttn_grad_kernels.h) on (x, x): L_1 .. L_{d+1} and G_{d+1} .. G_1, every state kept; <x, x> = L_{d+1}[1, 1].
//   phase 1   k_measure_open, grid (d * tables, batch): workgroup (k, t, b) runs ONE left-to-right chain site whose ket core is O_k x_k,
//                 V^O_k[c, c'] = sum_{z, z', al, be} L_k[al, be] x_k[z, al, c] O_k[z, z'] x_k[z', be, c']
//             stores it to its slot and reduces E_O[k] = <V^O_k, G_{k+1}>_F / <x, x> in a fixed order.
//   phase 2   k_measure_walk, grid (d - 1, batch, passes), longest walks first: workgroup (j, b) opens
//                 T[a, a'] = sum_{z, z', c, c'} x_j[z, a, c] O1_j[z, z'] x_j[z', a', c'] G_{j+1}[c, c']       (a right-to-left site, ket core O1_j x_j)
//             and carries T right to left through the sites j - 1, j - 2, ... with the plain transfer step; in front of every site i < j
//             it holds the environment of O1_j on bond i + 1, and <V^{O2}_i, T>_F is <O2_i O1_j>.  Pass 0 runs (O1, O2) = (Q, P) and fills
//             the upper triangle, pass 1 runs (P, Q) and fills the lower one; the diagonal is phase 1 with the table P_k Q_k.
//
// Routes, one per SITE as in k_grad_chain: a site of the k_dot_fused class (n = 2, both ranks <= 64) runs with the state in LDS — the
// plain step IS dot_site, the two opening steps are dot_site / grad_site_lr with the 2 x 2 matrix applied to the two physical slices of
// the ket fragment, which arrive together in the 16-byte load (no transformed core is written anywhere) —; any other site forms O x_k
// in workspace and runs the two workgroup GEMMs of dot_site_generic / grad_site_generic_rl on states in workspace.  The walk's state
// moves between the two homes when consecutive sites differ.
//
// Reductions: a Frobenius product is summed per thread over a fixed set of entries, per wave by shuffles, and the 16 wave sums by
// one thread, all in a fixed order.  The states themselves come from dot_site's LDS atomics, whose order is not fixed: results are
// reproducible to rounding, not bitwise.  In the walk the wave sums of step s are collected AFTER the barrier of step s + 1 (two
// alternating rows of 16 words), so a step costs no barrier beyond the one of its site.
#pragma once
#include "ttn_common.h"
#include "ttn_wg_gemm.h"
#include "ttn_dot_kernels.h"
#include "ttn_grad_kernels.h"

#define MEASURE_MAX_OPS 16                                               // tables per call (TTN_MEASURE_MAX_OPS)
#define MEASURE_MAX_D DOT_MAX_D
#define MEASURE_RED_DOUBLES (2 * TTN_NWAVES)                             // behind the images and the per-site table: the wave sums
#define MEASURE_LDS_BYTES(d) (DOT_LDS_BYTES(d) + sizeof(double) * MEASURE_RED_DOUBLES)

struct MeasureArgs {
    TTDev x;                 // the trains of this launch (a chunk of the handle's batch: data and rks advanced by the host)
    const double* env;       // k_grad_chain's [batch][2][d + 1][W]
    long long W;
    const double* tabs;      // [ntab][S]: the operator tables, site k of a table at toff[k], n_k x n_k column-major
    const long long* toff;   // [d]
    long long S;
    int ntab;
    double* V;               // [batch][ntab][d][W]: V^O_k, r_{k+1} x r_{k+1} column-major
    double* work;            // general route: `wstride` doubles per workgroup — the transformed core [0, csz), the GEMM intermediate
    long long wstride, csz, tsz;   //            [csz, csz + tsz), and for a walk two states of W doubles behind them
    double* out;             // device
    long long ob, ot, ok;    // k_measure_open: table t < nemit writes out[b ob + t ot + k ok]
    int nemit;
    int normalize;           // divide by <x, x> (a zero train: IEEE 0 / 0)
    int o1[2], o2[2];        // k_measure_walk, per pass: the table that opens at j, the table whose V it meets
    int mirror;              // P and Q are the same table: the one pass writes both triangles
};

__device__ __forceinline__ double measure_wave_sum(double p) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) p += __shfl_down(p, s, 64);
    return p;
}

// (O v)[z] for the pair v = (v[z' = 0], v[z' = 1]): O[z, z'] at o[z + 2 z']
__device__ __forceinline__ dot_f64x2 measure_apply2(dot_f64x2 v, double o00, double o10, double o01, double o11) {
    dot_f64x2 w;
    w.x = fma(o01, v.y, o00 * v.x);
    w.y = fma(o11, v.y, o10 * v.x);
    return w;
}

// OX[z, f] = sum_z' O[z, z'] X[z', f] over the `fibres` = r_left r_right fibres of a core (the general route)
__device__ __forceinline__ void measure_transform(double* OX, const double* X, const double* O, int n, int fibres) {
    for (int f = threadIdx.x; f < fibres; f += TTN_WG) {
        const double* xf = X + (long long)n * f;
        for (int z = 0; z < n; ++z) {
            double acc = 0.0;
            for (int zz = 0; zz < n; ++zz) acc = fma(O[z + n * zz], xf[zz], acc);
            OX[(long long)n * f + z] = acc;
        }
    }
}

// dot_site<false> of ttn_dot_kernels.h (RIGHT TO LEFT, bra and ket the same core Xk) with the ket fragment transformed:
//   T_z[a, be] = sum_b M[a, b] (O Xk)[z, be, b],   M'[al, be] = sum_{z, a} Xk[z, al, a] T_z[a, be]
//   r: the RIGHT rank (M is r x r at Mcur[DOT_AT(b, a)]);  r2: the LEFT rank (M' into Mnxt, all zero on entry);  Mzero is zeroed here
__device__ __noinline__ void measure_site_rl(const double* Xk, double o00, double o10, double o01, double o11, int r, int r2, const lds_f64* Mcur,
                                             lds_f64* Mnxt, lds_f64* Mzero) {
    Xk = unip(Xk); r = uni32(r); r2 = uni32(r2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int tr = wave & 3, tc = wave >> 2;
    {
        typedef __attribute__((address_space(3))) dot_f64x2 lds_f64x2;
        lds_f64x2* z2 = (lds_f64x2*)Mzero;
        const dot_f64x2 zero2 = {0.0, 0.0};
        for (int e = threadIdx.x; e < DOT_MS_DOUBLES / 2; e += TTN_WG) z2[e] = zero2;
    }
    if (16 * tr < r && 16 * tc < r2) {                                    // wave-uniform
        mfma_acc_t t0 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}, t1 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
        const int bq = 16 * tc + li;
        const int nt = (r + 3) >> 2;                                      // k-steps of four b
        for (int t = 0; t < nt; ++t) {
            const dot_f64x2 bv = measure_apply2(dot_load2(Xk, bq, 4 * t + lk, r2, r, r2), o00, o10, o01, o11);
            const double a = Mcur[DOT_AT(4 * t + lk, 16 * tr + li)];
            t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv.x, t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv.y, t1, 0, 0, 0);
        }
        const int nr = min(4, (r - 16 * tr + 3) >> 2);                    // k-steps of this block that hold rows a < r
        const int nta = (r2 + 15) >> 4;
#pragma unroll
        for (int ta = 0; ta < 4; ++ta) {
            if (ta < nta) {                                               // wave-uniform
                mfma_acc_t m = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
                const int aq = 16 * ta + li;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q < nr) {
                        const dot_f64x2 av = dot_load2(Xk, aq, 16 * tr + 4 * q + lk, r2, r, r2);
                        m = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, t0[q], m, 0, 0, 0);
                        m = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, t1[q], m, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    __hip_atomic_fetch_add(Mnxt + DOT_AT(16 * tc + li, 16 * ta + lk + 4 * reg), m[reg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    dot_lds_barrier();
}

// grad_site_lr of ttn_grad_kernels.h (LEFT TO RIGHT, bra and ket the same core Xk) with the ket fragment transformed:
//   T_z[al, b] = sum_be L[al, be] (O Xk)[z, be, b],   L'[a, b] = sum_{z, al} Xk[z, al, a] T_z[al, b]
//   r: the LEFT rank (L is r x r at Mcur[DOT_AT(be, al)]);  r2: the RIGHT rank (L' into Mnxt, all zero on entry);  Mzero is zeroed here
__device__ __noinline__ void measure_site_lr(const double* Xk, double o00, double o10, double o01, double o11, int r, int r2, const lds_f64* Mcur,
                                             lds_f64* Mnxt, lds_f64* Mzero) {
    Xk = unip(Xk); r = uni32(r); r2 = uni32(r2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int tr = wave & 3, tc = wave >> 2;
    {
        typedef __attribute__((address_space(3))) dot_f64x2 lds_f64x2;
        lds_f64x2* z2 = (lds_f64x2*)Mzero;
        const dot_f64x2 zero2 = {0.0, 0.0};
        for (int e = threadIdx.x; e < DOT_MS_DOUBLES / 2; e += TTN_WG) z2[e] = zero2;
    }
    if (16 * tr < r && 16 * tc < r2) {                                    // wave-uniform
        mfma_acc_t t0 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}, t1 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
        const int bq = 16 * tc + li;
        const int nt = (r + 3) >> 2;                                      // k-steps of four be
        for (int t = 0; t < nt; ++t) {
            const dot_f64x2 bv = measure_apply2(dot_load2(Xk, 4 * t + lk, bq, r, r2, r), o00, o10, o01, o11);     // (O Xk)[., be = 4 t + lk, b = bq]
            const double a = Mcur[DOT_AT(4 * t + lk, 16 * tr + li)];
            t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv.x, t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv.y, t1, 0, 0, 0);
        }
        const int nr = min(4, (r - 16 * tr + 3) >> 2);                    // k-steps of this block that hold rows al < r
        const int nta = (r2 + 15) >> 4;
#pragma unroll
        for (int ta = 0; ta < 4; ++ta) {
            if (ta < nta) {                                               // wave-uniform
                mfma_acc_t m = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
                const int aq = 16 * ta + li;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q < nr) {
                        const dot_f64x2 av = dot_load2(Xk, 16 * tr + 4 * q + lk, aq, r, r2, r);          // Xk[., al = 16 tr + 4 q + lk, a = aq]
                        m = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, t0[q], m, 0, 0, 0);
                        m = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, t1[q], m, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)                        // L'[a = 16 ta + lk + 4 reg, b = 16 tc + li]
                    __hip_atomic_fetch_add(Mnxt + DOT_AT(16 * tc + li, 16 * ta + lk + 4 * reg), m[reg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    dot_lds_barrier();
}

// dot_site<true> out of line: inlined next to the walk's own live values (the prefetched entries of V, the running sums) it left the kernel
// with 68 spilled VGPRs; behind a call it keeps the register allocation it has in k_dot_fused
__device__ __noinline__ void measure_site_full(const double* Ak, const double* Bk, int ra, int ra2, int rb, int rb2, const lds_f64* Mcur, lds_f64* Mnxt,
                                               lds_f64* Mzero) {
    Ak = unip(Ak); Bk = unip(Bk);
    dot_site<true>(Ak, Bk, ra, ra2, rb, rb2, Mcur, Mnxt, Mzero);
}

// Two clean images, then the r x r column-major state `src` into the first: entry (p, q) at DOT_AT(q, p).  Wave w takes the columns
// w, w + 16, ...: r <= 64, so a lane is a row and nothing is divided.
__device__ __forceinline__ void measure_state_to_lds(lds_f64* img, const double* src, int r) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * DOT_MS_DOUBLES; e += TTN_WG) img[e] = 0.0;
    __syncthreads();
    for (int q = wave; q < r; q += TTN_NWAVES)
        if (lane < r) img[DOT_AT(q, lane)] = src[lane + (long long)r * q];
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// phase 1: block (k + d t, b) — V^O_k of table t and its product with G_{k+1}
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TTN_WG) k_measure_open(MeasureArgs P) {
    extern __shared__ double lds[];
    const int d = P.x.d, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x % d, t = blockIdx.x / d, b = blockIdx.y;
    const long long* rk = P.x.rks + (long long)b * (d + 1);
    const int r = uni32((int)rk[k]), r2 = uni32((int)rk[k + 1]), n = uni32(P.x.dims[k]);
    double* Xk = P.x.data + (long long)b * P.x.stride + P.x.off[k];
    const double* Ok = P.tabs + (long long)t * P.S + P.toff[k];
    const double* E = P.env + (long long)b * 2 * (d + 1) * P.W;
    const double* L = E + (long long)k * P.W;                             // L_k, r x r
    const double* G = E + (long long)(d + 1 + k + 1) * P.W;               // G_{k+1}, r2 x r2
    double* Vk = P.V + (((long long)b * P.ntab + t) * d + k) * P.W;
    lds_f64* img = (lds_f64*)lds;
    lds_f64* red = (lds_f64*)((char*)lds + DOT_LDS_BYTES(d));
    double p = 0.0;
    if (n == 2 && r <= DOT_RMAX && r2 <= DOT_RMAX) {
        measure_state_to_lds(img, L, r);
        measure_site_lr(Xk, Ok[0], Ok[1], Ok[2], Ok[3], r, r2, img, img + DOT_MS_DOUBLES, img + 2 * DOT_MS_DOUBLES);
        const lds_f64* done = img + DOT_MS_DOUBLES;
        for (int q = wave; q < r2; q += TTN_NWAVES)
            if (lane < r2) {
                const double v = done[DOT_AT(q, lane)];
                Vk[lane + (long long)r2 * q] = v;
                p = fma(v, G[lane + (long long)r2 * q], p);
            }
    } else {
        double* OX = P.work + ((long long)b * gridDim.x + blockIdx.x) * P.wstride;
        double* Tb = OX + P.csz;
        measure_transform(OX, Xk, Ok, n, r * r2);
        __syncthreads();
        dot_site_generic(Xk, OX, (double*)L, Vk, Tb, n, r, r2, r, r2, lds);
        __syncthreads();
        for (int e = tid; e < r2 * r2; e += TTN_WG) p = fma(Vk[e], G[e], p);
    }
    if (t >= P.nemit) return;                                             // block-uniform
    p = measure_wave_sum(p);
    if (lane == 0) red[wave] = p;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < TTN_NWAVES; ++w) s += red[w];
        if (P.normalize) s /= E[(long long)d * P.W];                      // <x, x> = L_{d+1}[1, 1]
        P.out[(long long)b * P.ob + (long long)t * P.ot + (long long)k * P.ok] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// phase 2: block (d - 1 - j, b, pass) — the walk that opens at site j (0-based, j = d - 1 first: the longest walk) and ends at site 1
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TTN_WG) k_measure_walk(MeasureArgs P) {
    extern __shared__ double lds[];
    const int d = P.x.d, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = d - 1 - (int)blockIdx.x, b = blockIdx.y, pass = blockIdx.z;
    lds_f64* img = (lds_f64*)lds;
    lds_i32* tab = (lds_i32*)((lds_f64*)lds + DOT_LDS_DOUBLES);           // [0] r_k, [2] n_k, [3] off_k (doubles), stride 6 as in k_dot_fused
    lds_f64* red = (lds_f64*)((char*)lds + DOT_LDS_BYTES(d));
    for (int k = tid; k <= d; k += TTN_WG) {
        tab[6 * k + 0] = (int)P.x.rks[(long long)b * (d + 1) + k];
        tab[6 * k + 2] = k < d ? P.x.dims[k] : 0;
        tab[6 * k + 3] = k < d ? (int)P.x.off[k] : 0;                      // a train is far below 2^31 doubles (checked by the host)
    }
    __syncthreads();
    double* Xb = P.x.data + (long long)b * P.x.stride;
    const double* E = P.env + (long long)b * 2 * (d + 1) * P.W;
    const double* Gch = E + (long long)(d + 1) * P.W;                     // G_1 .. G_{d+1}
    const double* V2 = P.V + ((long long)b * P.ntab + P.o2[pass]) * d * P.W;
    const double* O1 = P.tabs + (long long)P.o1[pass] * P.S + P.toff[j];
    double* wk = P.work + (((long long)b * gridDim.z + pass) * gridDim.x + blockIdx.x) * P.wstride;
    double* OX = wk;
    double* Tb = OX + P.csz;
    double* St0 = Tb + P.tsz;
    double* St1 = St0 + P.W;
    double* Cb = P.out + (long long)b * d * d;
    const double nrm = P.normalize ? E[(long long)d * P.W] : 1.0;

    bool in_lds = false;
    int cur = 0;                                                          // image that holds the state while in_lds
    int sidx = -1;                                                        // workspace state that holds it otherwise (-1: the chain's G_{j+1})
    int step = 0;
    for (int i = j; i >= 1; --i, ++step) {
        const int n = uni32(tab[6 * i + 2]);
        const int rr = uni32(tab[6 * i + 6]), rl = uni32(tab[6 * i]);     // the incoming state is rr x rr, the outgoing one rl x rl
        double* Xi = Xb + uni32(tab[6 * i + 3]);
        const double* Vi = V2 + (long long)(i - 1) * P.W;                 // V^{O2}_{i-1}, rl x rl
        const bool fit = n == 2 && rr <= DOT_RMAX && rl <= DOT_RMAX;
        const double* Sin = sidx < 0 ? Gch + (long long)(j + 1) * P.W : (sidx ? St1 : St0);
        double p = 0.0;
        if (fit) {
            // this thread's entries of V, requested before the site: they arrive while it runs
            double vreg[DOT_RMAX / TTN_NWAVES];
#pragma unroll
            for (int u = 0; u < DOT_RMAX / TTN_NWAVES; ++u) {
                const int q = wave + TTN_NWAVES * u;
                vreg[u] = (q < rl && lane < rl) ? Vi[lane + (long long)rl * q] : 0.0;
            }
            if (!in_lds) {
                measure_state_to_lds(img, Sin, rr);
                cur = 0;
                in_lds = true;
            }
            const int nx = cur == 2 ? 0 : cur + 1, sp = nx == 2 ? 0 : nx + 1;
            if (i == j)
                measure_site_rl(Xi, O1[0], O1[1], O1[2], O1[3], rr, rl, img + cur * DOT_MS_DOUBLES, img + nx * DOT_MS_DOUBLES, img + sp * DOT_MS_DOUBLES);
            else if (rr == DOT_RMAX && rl == DOT_RMAX)
                measure_site_full(Xi, Xi, rr, rl, rr, rl, img + cur * DOT_MS_DOUBLES, img + nx * DOT_MS_DOUBLES, img + sp * DOT_MS_DOUBLES);
            else
                dot_site_masked(Xi, Xi, rr, rl, rr, rl, img + cur * DOT_MS_DOUBLES, img + nx * DOT_MS_DOUBLES, img + sp * DOT_MS_DOUBLES);
            cur = nx;
            const lds_f64* done = img + cur * DOT_MS_DOUBLES;
#pragma unroll
            for (int u = 0; u < DOT_RMAX / TTN_NWAVES; ++u) {
                const int q = wave + TTN_NWAVES * u;
                if (q < rl && lane < rl) p = fma(vreg[u], done[DOT_AT(q, lane)], p);
            }
        } else {
            if (in_lds) {                                                 // the state leaves LDS: the GEMMs use the images' memory
                const lds_f64* src = img + cur * DOT_MS_DOUBLES;
                for (int q = wave; q < rr; q += TTN_NWAVES)
                    if (lane < rr) St0[lane + (long long)rr * q] = src[DOT_AT(q, lane)];
                __syncthreads();
                sidx = 0;
                Sin = St0;
                in_lds = false;
            }
            double* Sout = sidx == 0 ? St1 : St0;
            const double* Bk = Xi;
            if (i == j) {
                measure_transform(OX, Xi, O1, n, rl * rr);
                __syncthreads();
                Bk = OX;
            }
            grad_site_generic_rl(Xi, (double*)Bk, (double*)Sin, Sout, Tb, n, rr, rl, rr, rl, lds);
            __syncthreads();
            sidx = sidx == 0 ? 1 : 0;
            for (int e = tid; e < rl * rl; e += TTN_WG) p = fma(Vi[e], Sout[e], p);
        }
        // the sums of the step before: its wave sums were written before the barrier that ended this step's site
        if (tid == 0 && step > 0) {
            double s = 0.0;
            for (int w = 0; w < TTN_NWAVES; ++w) s += red[((step - 1) & 1) * TTN_NWAVES + w];
            s /= nrm;
            const int io = i;                                             // step - 1 met V of site (i + 1) - 1
            if (pass == 0) Cb[io + (long long)d * j] = s; else Cb[j + (long long)d * io] = s;
            if (P.mirror) Cb[j + (long long)d * io] = s;
        }
        p = measure_wave_sum(p);
        if (lane == 0) red[(step & 1) * TTN_NWAVES + wave] = p;
    }
    __syncthreads();
    if (tid == 0 && step > 0) {
        double s = 0.0;
        for (int w = 0; w < TTN_NWAVES; ++w) s += red[((step - 1) & 1) * TTN_NWAVES + w];
        s /= nrm;
        if (pass == 0) Cb[(long long)d * j] = s; else Cb[j] = s;          // the last step met V of site 0
        if (P.mirror) Cb[j] = s;
    }
}
