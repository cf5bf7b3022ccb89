// ttn_step_kernels.h — z = alpha x + beta (A y) in one streaming launch (include/ttn_step.h): what a time step does around its linear
// solve — the Crank-Nicolson right-hand side (I + (h/2) A) u, the explicit Euler update u + h A u, the residuals of return_error.
// The layout is the one the composition ttn_apply -> ttn_scale_batch -> ttn_scale_batch -> ttn_add produces, bit for bit: the product
// block is accumulated as k_apply accumulates it (acc = A[i,0] y_0, then fma over j >= 1), rounded once and only then scaled by beta
// (core 1 of the product), x's block is scaled by alpha in the core ttn_scale_batch would choose, a zero factor writes zero blocks.
#pragma once
#include "ttn_common.h"
#include "ttn_stream_kernels.h"

#ifndef TTN_AXPBY_K
#define TTN_AXPBY_K 4                     // output columns per thread (n = 2): the K of k_apply and k_add, whose two mappings this kernel joins
#endif

// z.rks = x.rks + A.rks .* y.rks, ends forced to 1 (tt_operations.jl:14-16 on top of :103)
__global__ void k_ranks_axpby(TTDev z, TTDev x, TTODev A, TTDev y) {
    int b = blockIdx.x;
    for (int m = threadIdx.x; m <= x.d; m += blockDim.x) {
        long long r = x.rks[(long long)b * (x.d + 1) + m] + A.rks[m] * y.rks[(long long)b * (y.d + 1) + m];
        if (m == 0 || m == x.d) r = 1;
        z.rks[(long long)b * (z.d + 1) + m] = r;
    }
}

// Grid (tiles, d, batch).  Core k of z: first [X~ Y~], middle diag(X~, Y~) with the off-diagonal blocks written as zeros, last [X~; Y~]
// (d >= 2), where Y~[i, a' + Rl v', a + Rr v] = sum_j A_k[i,j,a',a] Y_k[j,v',v] (times beta_b in core 1) and X~ = X_k (times alpha_b in
// core which_b).  ab: device [2][batch] factors, or null for the uniform pair (alpha_u, beta_u).  lds_a: doubles of dynamic LDS for the
// operator core; a larger core is read through the caches.
// n = 2: one thread = one output row and TTN_AXPBY_K consecutive columns, per j the lanes of a wave write consecutive rows (16-byte
// non-temporal stores, coalesced); the column pair (a, v) of the product block advances by increment and the input fibre of y is
// reloaded only when v changes, as in k_apply.  Any other n: one thread per output fibre.
__global__ void __launch_bounds__(TTN_STREAM_TB) k_apply_axpby(TTODev A, TTDev x, TTDev y, TTDev z, double alpha_u, double beta_u, const double* ab,
                                                               int which, const int* which_b, int lds_a) {
    extern __shared__ double axpby_smem[];
    const int k = blockIdx.y, b = blockIdx.z, d = x.d;
    const int n = x.dims[k];
    if (which_b) which = which_b[b];
    const double fa = ab ? ab[b] : alpha_u, fb = ab ? ab[x.batch + b] : beta_u;
    const int Rl = (int)A.rks[k], Rr = (int)A.rks[k + 1];
    const long long* xr = x.rks + (long long)b * (d + 1);
    const long long* yr = y.rks + (long long)b * (d + 1);
    const int rxl = (int)xr[k], rxr = (int)xr[k + 1], ryl = (int)yr[k], ryr = (int)yr[k + 1];
    const bool first = k == 0, last = k == d - 1;
    const int roff = first ? 0 : rxl, coff = last ? 0 : rxr;              // where the product block starts
    const unsigned int uzl = first ? 1u : (unsigned int)(rxl + Rl * ryl), uzr = last ? 1u : (unsigned int)(rxr + Rr * ryr);
    const unsigned int cgroups = (uzr + TTN_AXPBY_K - 1) / TTN_AXPBY_K;
    const unsigned int items = (n == 2) ? uzl * cgroups : uzl * uzr;
    if (blockIdx.x * blockDim.x >= items) return;                         // (block-uniform: before the barrier below)
    const double* Ak = A.data + (long long)b * A.stride + A.off[k];      // (stride 0: one operator for every train)
    const int asz = n * n * Rl * Rr;
    const bool in_lds = asz <= lds_a;
    if (in_lds) {
        for (int e = threadIdx.x; e < asz; e += blockDim.x) axpby_smem[e] = Ak[e];
        __syncthreads();
    }
    const double* Ap = in_lds ? axpby_smem : Ak;
    const double* Xk = x.data + (long long)b * x.stride + x.off[k];
    const double* Yk = y.data + (long long)b * y.stride + y.off[k];
    double* Zk = z.data + (long long)b * z.stride + z.off[k];
    const bool xzero = fa == 0.0, xscale = !xzero && k == which;          // ttn_scale_batch on x: zero train, or core `which` times alpha
    const bool yzero = fb == 0.0, yscale = !yzero && first;               // ... on the fresh product (all gauge flags zero): core 1 times beta
    if (n == 2) {
        typedef double d2v_t __attribute__((ext_vector_type(2)));
        for (unsigned int it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
            const unsigned int a = it % uzl, c0 = (it / uzl) * TTN_AXPBY_K;
            const bool xrow = first || a < (unsigned int)rxl, yrow = first || a >= (unsigned int)rxl;
            const unsigned int p = a - (unsigned int)roff;                // row of the product block (used on its rows only)
            const unsigned int al = yrow ? p % (unsigned int)Rl : 0u, vl = yrow ? p / (unsigned int)Rl : 0u;
            unsigned int ar = 0, vr = 0;
            if (c0 > (unsigned int)coff) { const unsigned int q0 = c0 - (unsigned int)coff; ar = q0 % (unsigned int)Rr; vr = q0 / (unsigned int)Rr; }
            bool reload = true;
            d2v_t yv = (d2v_t){0.0, 0.0};
            d2v_t o[TTN_AXPBY_K];
#pragma unroll
            for (int j = 0; j < TTN_AXPBY_K; ++j) {
                const unsigned int c = c0 + j;
                o[j] = (d2v_t){0.0, 0.0};
                if (c >= uzr) continue;
                const bool xcol = last || c < (unsigned int)rxr;
                if (xrow && xcol) {
                    if (!xzero) {
                        d2v_t v = *reinterpret_cast<const d2v_t*>(Xk + 2 * ((long long)a + (long long)rxl * c));
                        if (xscale) v *= fa;
                        o[j] = v;
                    }
                } else if (yrow && (last || c >= (unsigned int)rxr)) {
                    if (!yzero) {
                        if (reload) { yv = *reinterpret_cast<const d2v_t*>(Yk + 2 * ((long long)vl + (long long)ryl * vr)); reload = false; }
                        const double* ap = Ap + 4 * ((long long)al + (long long)Rl * ar);      // A[i, j, a', a] at i + 2 j + 4 (a' + Rl a)
                        d2v_t v;
                        v.x = fma(ap[2], yv.y, ap[0] * yv.x);
                        v.y = fma(ap[3], yv.y, ap[1] * yv.x);
                        if (yscale) v *= fb;                                                   // rounded once, then scaled
                        o[j] = v;
                    }
                    if (++ar == (unsigned int)Rr) { ar = 0; ++vr; reload = true; }
                }
            }
#pragma unroll
            for (int j = 0; j < TTN_AXPBY_K; ++j)
                if (c0 + j < uzr) __builtin_nontemporal_store(o[j], reinterpret_cast<d2v_t*>(Zk + 2 * ((long long)a + (long long)uzl * (c0 + j))));
        }
        return;
    }
    for (unsigned int e = blockIdx.x * blockDim.x + threadIdx.x; e < items; e += gridDim.x * blockDim.x) {
        const unsigned int a = e % uzl, c = e / uzl;
        const bool xrow = first || a < (unsigned int)rxl, yrow = first || a >= (unsigned int)rxl;
        const bool xcol = last || c < (unsigned int)rxr, ycol = last || c >= (unsigned int)rxr;
        double* zo = Zk + (long long)n * e;
        if (xrow && xcol) {
            const double* xs = Xk + (long long)n * ((long long)a + (long long)rxl * c);
            for (int s = 0; s < n; ++s) zo[s] = xzero ? 0.0 : (xscale ? fa * xs[s] : xs[s]);
        } else if (yrow && ycol) {
            const unsigned int p = a - (unsigned int)roff, q = c - (unsigned int)coff;
            const unsigned int al = p % (unsigned int)Rl, vl = p / (unsigned int)Rl, ar = q % (unsigned int)Rr, vr = q / (unsigned int)Rr;
            const double* ys = Yk + (long long)n * ((long long)vl + (long long)ryl * vr);
            const double* ap = Ap + (long long)n * n * ((long long)al + (long long)Rl * ar);
            for (int i = 0; i < n; ++i) {
                double acc = ap[i] * ys[0];
                for (int j = 1; j < n; ++j) acc = fma(ap[i + n * j], ys[j], acc);
                zo[i] = yzero ? 0.0 : (yscale ? fb * acc : acc);
            }
        } else {
            for (int s = 0; s < n; ++s) zo[s] = 0.0;
        }
    }
}
