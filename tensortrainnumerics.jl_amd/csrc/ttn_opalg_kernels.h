// ttn_opalg_kernels.h — TT operator algebra: operator * operator, the inner core product, outer_product, ttv_to_diag_tto.
// Every kernel is launched on grid (tiles, d): blockIdx.y = core.  The output is a NEW operator whose ranks the host knows, written
// as the vector core (n^2, r_l, r_r) an operator core (n, n, r_l, r_r) is byte for byte (tto_to_ttv, src/tt_tools.jl:296-304).
// + of operators and scalar * are k_add / k_scale on that view (ttn_stream_kernels.h); kron and the conversions are device copies.
#pragma once
#include "ttn_common.h"
#include "ttn_stream_kernels.h"

#ifndef TTN_TTOMUL_K
#define TTN_TTOMUL_K 2                    // output columns per thread in k_tto_mul (n = 2); measured on the 1.1 GB product of DESIGN.md §4.16: K = 1 0.37, 2 0.55, 4 0.37, 8 0.32 of 8 TB/s
#endif
#define TTN_TTOMUL_LDS_DOUBLES 4096       // an A core up to this size is staged in LDS (the 28 x 28 generator core: 3136 doubles)

// ---------------------------------------------------------------------------------------------
// operator * operator:  Y_k[i + n j, a + R b, a' + R' b'] = sum_z A_k[i,z,a,a'] * B_k[z,j,b,b']
// (src/tt_operations.jl:162-172; A's bond index fastest in the merged bond, from the reshape at :168).
// HBM-write bound like k_apply: both operand cores are read many times from LDS / cache, every output fibre is written once.
// ---------------------------------------------------------------------------------------------
// n = 2: one thread = one OUTPUT row p = a + R b and TTN_TTOMUL_K consecutive output columns q = a' + R' b' (k_apply's fast mapping).
// An output fibre is the 2 x 2 product of the A slice (a, a') and the B fibre (b, b'): 32 bytes.  For every column the lanes of a wave
// write consecutive rows — 32 bytes per lane, 2 KB per wave, contiguous, non-temporal.  The index decomposition is paid once per K
// fibres; the column pair (a', b') advances by increment; the B fibre is reloaded only when b' changes (every R' columns), the A
// slice changes with every column and comes from LDS when the core fits (lds_a doubles, sized by the host).
__global__ void __launch_bounds__(TTN_STREAM_TB) k_tto_mul(TTODev A, TTODev B, double* Y, const long long* yoff, int lds_a) {
    extern __shared__ double ttomul_smem[];
    const int k = blockIdx.y;
    const int n = A.dims[k];
    const unsigned int R = (unsigned int)A.rks[k], Rr = (unsigned int)A.rks[k + 1];
    const unsigned int r = (unsigned int)B.rks[k], rr = (unsigned int)B.rks[k + 1];
    const unsigned int uP = R * r, uQ = Rr * rr;                      // fewer than 2^31 fibres per core: the host refuses more
    const double* Ak = A.data + A.off[k];
    const double* Bk = B.data + B.off[k];
    double* Yk = Y + yoff[k];
    if (n == 2) {
        const unsigned int cgroups = (uQ + TTN_TTOMUL_K - 1) / TTN_TTOMUL_K;
        const unsigned long long items = (unsigned long long)uP * cgroups;
        if ((unsigned long long)blockIdx.x * blockDim.x >= items) return;
        const int asz = 4 * (int)(R * Rr);
        const bool in_lds = (long long)4 * R * Rr <= (long long)lds_a;
        if (in_lds) {
            for (int e = threadIdx.x; e < asz; e += blockDim.x) ttomul_smem[e] = Ak[e];
            __syncthreads();
        }
        const double* Ap = in_lds ? ttomul_smem : Ak;
        typedef double d2v_t __attribute__((ext_vector_type(2)));
        for (unsigned long long it = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (unsigned long long)gridDim.x * blockDim.x) {
            const unsigned int p = (unsigned int)(it % uP), c0 = (unsigned int)(it / uP) * TTN_TTOMUL_K;
            const unsigned int al = p % R, bl = p / R;
            unsigned int ar = c0 % Rr, br = c0 / Rr;
            d2v_t o0[TTN_TTOMUL_K], o1[TTN_TTOMUL_K];
            // B fibre (z, j) at z + 2 j: b0 = column j = 0, b1 = column j = 1
            d2v_t b0 = {0.0, 0.0}, b1 = {0.0, 0.0};
            if (c0 < uQ) {
                const d2v_t* bp = reinterpret_cast<const d2v_t*>(Bk + 4 * ((long long)bl + (long long)r * br));
                b0 = bp[0]; b1 = bp[1];
            }
#pragma unroll
            for (int j = 0; j < TTN_TTOMUL_K; ++j) {
                if (c0 + j < uQ) {
                    const d2v_t* ap = reinterpret_cast<const d2v_t*>(Ap + 4 * ((long long)al + (long long)R * ar));
                    const d2v_t a0 = ap[0], a1 = ap[1];                 // A[:, z = 0], A[:, z = 1]
                    o0[j].x = fma(a1.x, b0.y, a0.x * b0.x);             // Y[i, 0] = A[i,0] B[0,0] + A[i,1] B[1,0]
                    o0[j].y = fma(a1.y, b0.y, a0.y * b0.x);
                    o1[j].x = fma(a1.x, b1.y, a0.x * b1.x);             // Y[i, 1]
                    o1[j].y = fma(a1.y, b1.y, a0.y * b1.x);
                }
                if (++ar == Rr) {
                    ar = 0; ++br;
                    if (j + 1 < TTN_TTOMUL_K && c0 + j + 1 < uQ) {
                        const d2v_t* bp = reinterpret_cast<const d2v_t*>(Bk + 4 * ((long long)bl + (long long)r * br));
                        b0 = bp[0]; b1 = bp[1];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < TTN_TTOMUL_K; ++j)
                if (c0 + j < uQ) {
                    d2v_t* yo = reinterpret_cast<d2v_t*>(Yk + 4 * ((long long)p + (long long)uP * (c0 + j)));
                    __builtin_nontemporal_store(o0[j], yo);
                    __builtin_nontemporal_store(o1[j], yo + 1);
                }
        }
        return;
    }
    // any n: one thread per output fibre (p, q), the n x n product in the order z = 0 .. n-1
    const unsigned long long total = (unsigned long long)uP * uQ;
    const long long nn = (long long)n * n;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned int p = (unsigned int)(e % uP), q = (unsigned int)(e / uP);
        const unsigned int al = p % R, bl = p / R, ar = q % Rr, br = q / Rr;
        const double* ap = Ak + nn * ((long long)al + (long long)R * ar);
        const double* bp = Bk + nn * ((long long)bl + (long long)r * br);
        double* yo = Yk + nn * (long long)e;
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) {
                double acc = ap[i] * bp[n * j];
                for (int z = 1; z < n; ++z) acc = fma(ap[i + n * z], bp[z + n * j], acc);
                yo[i + n * j] = acc;
            }
    }
}

// ---------------------------------------------------------------------------------------------
// inner core product (src/tt_operations.jl:198-216): physical and bond indices both Kronecker, A major and B minor on every axis:
// Y_k[iB + nB iA, jB + nB jA, bl + rBl al, br + rBr ar] = A_k[iA,jA,al,ar] * B_k[iB,jB,bl,br].  One multiplication per element.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TTN_STREAM_TB) k_tto_inner(TTODev A, TTODev B, double* Y, const long long* yoff) {
    const int k = blockIdx.y;
    const unsigned long long nA = A.dims[k], nB = B.dims[k];
    const unsigned long long rAl = A.rks[k], rAr = A.rks[k + 1], rBl = B.rks[k], rBr = B.rks[k + 1];
    const double* Ak = A.data + A.off[k];
    const double* Bk = B.data + B.off[k];
    double* Yk = Y + yoff[k];
    const unsigned long long total = nA * nB * nA * nB * rAl * rBl * rAr * rBr;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long t = e;
        const unsigned long long iB = t % nB; t /= nB;
        const unsigned long long iA = t % nA; t /= nA;
        const unsigned long long jB = t % nB; t /= nB;
        const unsigned long long jA = t % nA; t /= nA;
        const unsigned long long bl = t % rBl; t /= rBl;
        const unsigned long long al = t % rAl; t /= rAl;
        const unsigned long long br = t % rBr; t /= rBr;
        const unsigned long long ar = t;
        Yk[e] = Ak[iA + nA * (jA + nA * (al + rAl * ar))] * Bk[iB + nB * (jB + nB * (bl + rBl * br))];
    }
}

// ---------------------------------------------------------------------------------------------
// outer_product(x, y) (src/tt_operations.jl:297-304), real: Y_k[i + n j, a + rx b, a' + rx' b'] = x_k[i,a,a'] * y_k[j,b,b'] of train bt.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TTN_STREAM_TB) k_tt_outer(TTDev x, TTDev y, int bt, double* Y, const long long* yoff) {
    const int k = blockIdx.y;
    const unsigned long long n = x.dims[k];
    const long long* xr = x.rks + (long long)bt * (x.d + 1);
    const long long* yr = y.rks + (long long)bt * (y.d + 1);
    const unsigned long long rxl = xr[k], rxr = xr[k + 1], ryl = yr[k], ryr = yr[k + 1];
    const double* Xk = x.data + (long long)bt * x.stride + x.off[k];
    const double* Yin = y.data + (long long)bt * y.stride + y.off[k];
    double* Yk = Y + yoff[k];
    const unsigned long long total = n * n * rxl * ryl * rxr * ryr;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long t = e;
        const unsigned long long i = t % n; t /= n;
        const unsigned long long j = t % n; t /= n;
        const unsigned long long al = t % rxl; t /= rxl;
        const unsigned long long bl = t % ryl; t /= ryl;
        const unsigned long long ar = t % rxr; t /= rxr;
        const unsigned long long br = t;
        Yk[e] = Xk[i + n * (al + rxl * ar)] * Yin[j + n * (bl + ryl * br)];
    }
}

// ---------------------------------------------------------------------------------------------
// ttv_to_diag_tto (src/tt_operations.jl:310-338): D_k[i, j, s1, s2] = (i == j) ? x_k[i, s1, s2] : 0 of train bt.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TTN_STREAM_TB) k_tt_diag(TTDev x, int bt, double* Y, const long long* yoff) {
    const int k = blockIdx.y;
    const unsigned long long n = x.dims[k];
    const long long* xr = x.rks + (long long)bt * (x.d + 1);
    const unsigned long long fibres = (unsigned long long)xr[k] * xr[k + 1];
    const double* Xk = x.data + (long long)bt * x.stride + x.off[k];
    double* Yk = Y + yoff[k];
    const unsigned long long total = n * n * fibres;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long ij = e % (n * n), s = e / (n * n);
        const unsigned long long i = ij % n, j = ij / n;
        Yk[e] = (i == j) ? Xk[i + n * s] : 0.0;
    }
}
