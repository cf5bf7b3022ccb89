// ttn_rect_kernels.h — the rectangular operator apply (src/tt_operations.jl:116-148): an operator of M = N + 1 sites whose cores are
// (n_out, n_in, R_l, R_r), exactly one of them with n_in == 1 (the singleton site s), against trains of N sites.
//   c(b) = b - [b > s]  (s 0-based) input sites left of boundary b;  y.rks[b] = A.rks[b] * x.rks[c(b)]
//   regular site k (input site k or k - 1):  Y_k[i, a' + Rl v', a + Rr v] = sum_j A_k[i, j, a', a] X[j, v', v]
//   singleton site s (nu = x.rks[s]):         Y_s[i, a' + Rl v', a + Rr v] = A_s[i, 0, a', a] [v' == v]    (every entry written)
// Launched on grid (tiles, M, batch) like the other streaming kernels; ranks are read from device memory.  HBM-write bound: the
// linear prolongation writes rank-5 r cores from rank-r ones, 25 times the bytes it reads.
#pragma once
#include "ttn_common.h"
#include "ttn_stream_kernels.h"

#define TTN_RECT_K 4                      // output columns per thread of the n_out = 2 mapping (k_apply's measured optimum, TTN_APPLY_K)

// Device view of one rectangular TT operator (ttn_rtto).
struct RTTODev {
    const double*  data;
    const long long* off;     // [M+1] device
    const long long* rks;     // [M+1] device
    const int*     odims;     // [M] device: n_out
    const int*     idims;     // [M] device: n_in (1 at the singleton site)
    int            d;         // M
    int            s;         // 0-based singleton site
};

// y.rks[b] = A.rks[b] * x.rks[c(b)]  (tt_operations.jl:127-130), one block per train
__global__ void k_ranks_mul_rect(TTDev y, RTTODev A, TTDev x) {
    const int b = blockIdx.x;
    for (int m = threadIdx.x; m <= A.d; m += blockDim.x)
        y.rks[(long long)b * (y.d + 1) + m] = A.rks[m] * x.rks[(long long)b * (x.d + 1) + (m > A.s ? m - 1 : m)];
}

// One thread = one OUTPUT row p = a' + Rl v' and, for n_out == 2 with the operator core staged in LDS, TTN_RECT_K consecutive output
// columns c = a + Rr v (k_apply's mapping): for every column the lanes of a wave write consecutive rows, 16 bytes per lane,
// coalesced and non-temporal; the column pair (a, v) advances by increment and the input fibre is reloaded only when v changes.  The
// singleton site takes the same mapping and reads no train data: the delta is a compare of the two train indices.  Every other
// shape (n_out != 2, n_in > 2, a core beyond lds_a doubles) takes one thread per output fibre (p, c).  32-bit fibre indices: the host
// refuses cores of 2^31 fibres or more.  lds_a: doubles of dynamic LDS, the largest core that is staged.
__global__ void __launch_bounds__(TTN_STREAM_TB) k_apply_rect(RTTODev A, TTDev x, TTDev y, int lds_a) {
    extern __shared__ __attribute__((aligned(16))) double rect_smem[];
    const int k = blockIdx.y, b = blockIdx.z;
    const int no = A.odims[k], ni = A.idims[k];
    const bool single = k == A.s;
    const int kin = k > A.s ? k - 1 : k;                               // input site of a regular site; left boundary of the singleton
    const int Rl = (int)A.rks[k], Rr = (int)A.rks[k + 1];
    const long long* xr = x.rks + (long long)b * (x.d + 1);
    const int rl = (int)xr[kin], rr = single ? rl : (int)xr[kin + 1];
    const unsigned int uP = (unsigned int)Rl * (unsigned int)rl, uQ = (unsigned int)Rr * (unsigned int)rr;
    const double* Ak = A.data + A.off[k];
    const long long asz = (long long)no * ni * Rl * Rr;
    const bool fast = no == 2 && ni == (single ? 1 : 2) && asz <= lds_a;
    const unsigned int cgroups = (uQ + TTN_RECT_K - 1) / TTN_RECT_K;
    const unsigned int items = fast ? uP * cgroups : uP * uQ;
    const unsigned int first = blockIdx.x * blockDim.x;
    if (first >= items) return;                                         // (uniform: a block beyond the work of its site leaves)
    const double* Xk = single ? nullptr : x.data + (long long)b * x.stride + x.off[kin];
    double* Yk = y.data + (long long)b * y.stride + y.off[k];
    if (fast) {
        for (int e = threadIdx.x; e < (int)asz; e += blockDim.x) rect_smem[e] = Ak[e];
        __syncthreads();
        typedef double d2v_t __attribute__((ext_vector_type(2)));
        const d2v_t zero = {0.0, 0.0};
        for (unsigned int it = first + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
            const unsigned int p = it % uP, c0 = (it / uP) * TTN_RECT_K;
            const unsigned int al = p % (unsigned int)Rl, vl = p / (unsigned int)Rl;
            unsigned int ar = c0 % (unsigned int)Rr, vr = c0 / (unsigned int)Rr;
            d2v_t o[TTN_RECT_K];
            if (single) {
#pragma unroll
                for (int j = 0; j < TTN_RECT_K; ++j) {
                    const d2v_t av = *reinterpret_cast<const d2v_t*>(rect_smem + 2 * (al + (unsigned int)Rl * ar));   // A[i, 0, a', a] at i + 2 (a' + Rl a)
                    o[j] = vl == vr ? av : zero;
                    if (++ar == (unsigned int)Rr) { ar = 0; ++vr; }
                }
            } else {
                d2v_t xv = (c0 < uQ) ? *reinterpret_cast<const d2v_t*>(Xk + 2 * ((long long)vl + (long long)rl * vr)) : zero;
#pragma unroll
                for (int j = 0; j < TTN_RECT_K; ++j) {
                    const double* ap = rect_smem + 4 * (al + (unsigned int)Rl * ar);                                  // A[i, j, a', a] at i + 2 j + 4 (a' + Rl a)
                    o[j].x = fma(ap[2], xv.y, ap[0] * xv.x);
                    o[j].y = fma(ap[3], xv.y, ap[1] * xv.x);
                    if (++ar == (unsigned int)Rr) {
                        ar = 0; ++vr;
                        if (j + 1 < TTN_RECT_K && c0 + j + 1 < uQ) xv = *reinterpret_cast<const d2v_t*>(Xk + 2 * ((long long)vl + (long long)rl * vr));
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < TTN_RECT_K; ++j)
                if (c0 + j < uQ) __builtin_nontemporal_store(o[j], reinterpret_cast<d2v_t*>(Yk + 2 * ((long long)p + (long long)uP * (c0 + j))));
        }
        return;
    }
    // generic: one output fibre (p, c) per thread, the operator core read through the caches
    for (unsigned int it = first + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const unsigned int p = it % uP, c = it / uP;
        const unsigned int al = p % (unsigned int)Rl, vl = p / (unsigned int)Rl;
        const unsigned int ar = c % (unsigned int)Rr, vr = c / (unsigned int)Rr;
        const double* ap = Ak + (long long)no * ni * (al + (long long)Rl * ar);
        double* yo = Yk + (long long)no * it;
        if (single) {
            for (int i = 0; i < no; ++i) yo[i] = vl == vr ? ap[i] : 0.0;
        } else {
            const double* xs = Xk + (long long)ni * ((long long)vl + (long long)rl * vr);
            for (int i = 0; i < no; ++i) {
                double acc = ap[i] * xs[0];
                for (int j = 1; j < ni; ++j) acc = fma(ap[i + no * j], xs[j], acc);
                yo[i] = acc;
            }
        }
    }
}
