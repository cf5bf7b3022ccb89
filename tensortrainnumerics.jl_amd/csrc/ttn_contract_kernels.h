// ttn_contract_kernels.h — partial contraction of a train (include/ttn_contract.h): the sites of a set C are contracted
// against weight vectors, M_k = sum_z w_k[z] X_k[z, :, :], and every run of them is absorbed into a kept site:
//       a run in front of kept site k (behind the kept site p, or from the left end):   Y_k[z] = (M_{p+1} ... M_{k-1}) X_k[z]
//       the run behind the last kept site:                                               Y_k[z] <- Y_k[z] (M_{k+1} ... M_d)
//       a kept site with no run next to it:                                              copied bit for bit
// Every kept site depends on the run in front of it alone (the last one also on the run behind it), so nothing chains across the
// train: the grid is (kept site, train), and the host sorts the kept sites into three launches by what they need:
//   k_contract_copy   no run: a coalesced 16-byte copy of the core.
//   k_contract_vec    only vector chains: the run from the left end (r_0 = 1: p <- p M_i, a row vector) and / or the run behind the last
//                     kept site (r_d = 1: v <- M_i v).  Any n_k, any rank; the vectors live in workspace.  M_i is never stored: the weighted
//                     sum over z is taken on the loaded fibre.
//   k_contract_chip   a run behind another kept site, ON-CHIP route (every n_k = 2, x's rank capacity <= 64): the running product
//                     P = M_{p+1} ... M_i (r_p x r_i) stays in LDS, transposed (PT[c][a'], pitch 80), M_i is formed while its core streams
//                     in (one 16-byte load per fibre yields z = 0 and 1) into an LDS image (pitch 66) and P <- P M_i runs on the fp64 MFMA
//                     with the accumulators in registers; at the kept site both slices X_k[0], X_k[1] are staged the same way and
//                     Y_k[z]^T = X_k[z]^T P^T leaves the accumulators as 16-byte stores, lanes along the contiguous left index.
//   k_contract_gen    the same on the GENERAL route (any n_k, ranks above 64): M_i and P in workspace, the products are wg_gemm calls.
// No atomics; every sum has one fixed order, so two calls give the same bits and a train's result does not depend on its batch.
// 32-bit element indices inside a core: the host refuses slots of 2^31 doubles or more.
#pragma once
#include "ttn_common.h"
#include "ttn_wg_gemm.h"

#define CONTRACT_RMAX 64                         // largest rank of the on-chip route
#define CONTRACT_COPY_TB 256
#define CONTRACT_VEC_TB 256
#define CONTRACT_CHIP_TB 512
#define CONTRACT_PT_LD 80                        // == 16 mod 32: the two k-rows of a half-wave's fragment read fall on different banks
#define CONTRACT_X_LD 66                         // == 2 mod 32: lanes (a, c) of a fragment read at 66 a + c tile the 32 double-banks
#define CONTRACT_PT_DOUBLES (CONTRACT_RMAX * CONTRACT_PT_LD)
#define CONTRACT_X_DOUBLES (CONTRACT_RMAX * CONTRACT_X_LD)
#define CONTRACT_RED_DOUBLES (64 * (TTN_WG / 64))                         // contract_trail's partial sums, for the largest workgroup
#define CONTRACT_CHIP_VEC_DOUBLES (4 * CONTRACT_RMAX)                     // v, v' and u[z + 2 c] of the last kept site
#define CONTRACT_CHIP_LDS_BYTES (sizeof(double) * (CONTRACT_PT_DOUBLES + 2 * CONTRACT_X_DOUBLES + CONTRACT_RED_DOUBLES + CONTRACT_CHIP_VEC_DOUBLES))

typedef double contract_f64x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) contract_f64x2 contract_gmem_f64x2;

struct ContractArgs {
    TTDev x, y;              // the trains of this launch (a chunk of the batch: data and rks advanced by the host)
    const int* kept;         // [K] the kept sites, 0-based, ascending
    const int* start;        // [K] the first site of the run in front of kept site m (== kept[m]: no run)
    const int* list;         // the kept-site numbers m this launch works on: blockIdx.x -> m
    const long long* woff;   // [d] where site k's weights stand in a table (contracted sites)
    const double* w;         // the weight table of the first train of this launch
    long long wstride;       // doubles per table; 0: one table serves every train
    double* work;            // `wsz` doubles per workgroup (blockIdx.x + gridDim.x * blockIdx.y)
    long long wsz;
    int rcap, ncap;          // layout of a workgroup's workspace: the largest rank bound and dimension of x
    int K;
};

// y's ranks: the bond left of kept site m carries x's rank left of the run in front of it; the right end x's right end
__global__ void k_contract_ranks(ContractArgs P) {
    const int b = blockIdx.x;
    const long long* xr = P.x.rks + (long long)b * (P.x.d + 1);
    long long* yr = P.y.rks + (long long)b * (P.K + 1);
    for (int m = threadIdx.x; m <= P.K; m += blockDim.x) yr[m] = m < P.K ? xr[P.start[m]] : xr[P.x.d];
}

__global__ void __launch_bounds__(CONTRACT_COPY_TB) k_contract_copy(ContractArgs P) {
    const int m = P.list[blockIdx.x], b = blockIdx.y, k = P.kept[m];
    const long long* xr = P.x.rks + (long long)b * (P.x.d + 1);
    const int sz = P.x.dims[k] * (int)xr[k] * (int)xr[k + 1];
    const double* X = P.x.data + (long long)b * P.x.stride + P.x.off[k];
    double* Y = P.y.data + (long long)b * P.y.stride + P.y.off[m];
    for (int e = threadIdx.x; e < sz / 2; e += CONTRACT_COPY_TB)            // (slots are 16-byte aligned)
        reinterpret_cast<contract_f64x2*>(Y)[e] = reinterpret_cast<const contract_f64x2*>(X)[e];
    if ((sz & 1) && threadIdx.x == 0) Y[sz - 1] = X[sz - 1];
}

__device__ __forceinline__ double contract_wave_sum(double p) {              // lane 0 receives the sum, in a fixed order
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) p += __shfl_down(p, s, 64);
    return p;
}

// (sum_z w[z] X[z]) of one fibre
__device__ __forceinline__ double contract_fibre(const double* f, const double* w, int n) {
    double m = w[0] * f[0];
    for (int z = 1; z < n; ++z) m = fma(w[z], f[z], m);
    return m;
}

// The row vector p (rl entries) against the core X (n, rl, rr), one wave per output, the lanes along the contiguous left index:
//   w != null:  out[a] = sum_c p[c] (sum_z w[z] X[z, c, a])        (p <- p M)
//   w == null:  out[z + n a] = sum_c p[c] X[z, c, a]               (the kept site: Y[z] = p X[z])
// Ends with a barrier: out is visible to the workgroup.
__device__ __noinline__ void contract_lead(const double* X, int n, int rl, int rr, const double* w, const double* p, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int nout = w ? rr : n * rr;
    for (int j = wave; j < nout; j += nw) {
        const int a = w ? j : j / n, z0 = w ? 0 : j % n;
        const double* Xa = X + (long long)n * rl * a;
        double acc = 0.0;
        for (int c = lane; c < rl; c += 64) acc = fma(p[c], w ? contract_fibre(Xa + (long long)n * c, w, n) : Xa[z0 + (long long)n * c], acc);
        acc = contract_wave_sum(acc);
        if (lane == 0) out[j] = acc;
    }
    __syncthreads();
}

// The core X (n, rl, rr) against the column vector v (rr entries), 64 rows at a time, the lanes along the contiguous left index and
// the waves over a; the waves' partial sums meet in `red` (64 doubles per wave) and are added in wave order:
//   w != null:  out[c] = sum_a (sum_z w[z] X[z, c, a]) v[a]        (v <- M v)
//   w == null:  out[z + n c] = sum_a X[z, c, a] v[a]               (the kept site: Y[z] = X[z] v)
// Ends with a barrier: out is visible to the workgroup.
__device__ __noinline__ void contract_trail(const double* X, int n, int rl, int rr, const double* w, const double* v, double* out, double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int nrow = w ? rl : n * rl;
    for (int r0 = 0; r0 < nrow; r0 += 64) {
        const int row = r0 + lane;
        double acc = 0.0;
        if (row < nrow)
            for (int a = wave; a < rr; a += nw) {
                const double* Xa = X + (long long)n * rl * a;
                acc = fma(w ? contract_fibre(Xa + (long long)n * row, w, n) : Xa[row], v[a], acc);
            }
        red[64 * wave + lane] = acc;
        __syncthreads();
        if (wave == 0 && row < nrow) {
            double s = red[lane];
            for (int q = 1; q < nw; ++q) s += red[64 * q + lane];
            out[row] = s;
        }
        __syncthreads();
    }
}

// What a workgroup reads about its kept site
struct ContractSite {
    int m, k, s, d, n, L, rl, rr;       // kept-site number, its site, the run's first site, sites of x, n_k, r_s, r_k, r_{k+1}
    bool trail;                         // the last kept site with a run behind it
    const long long* xr;
    const double* xb;                   // train b of x
    const double* wb;                   // its weight table
    double* Y;
};
__device__ __forceinline__ ContractSite contract_site(const ContractArgs& P) {
    ContractSite S;
    const int b = blockIdx.y;
    S.m = P.list[blockIdx.x]; S.k = P.kept[S.m]; S.s = P.start[S.m]; S.d = P.x.d;
    S.xr = P.x.rks + (long long)b * (S.d + 1);
    S.xb = P.x.data + (long long)b * P.x.stride;
    S.wb = P.w + (long long)b * P.wstride;
    S.n = P.x.dims[S.k];
    S.L = (int)S.xr[S.s]; S.rl = (int)S.xr[S.k]; S.rr = (int)S.xr[S.k + 1];
    S.trail = S.m == P.K - 1 && S.k < S.d - 1;
    S.Y = P.y.data + (long long)b * P.y.stride + P.y.off[S.m];
    return S;
}

// v <- M_{k+1} ... M_d [1] in v0 / v1 (each holds the largest rank); returns the buffer that holds it
__device__ __forceinline__ double* contract_trail_chain(const ContractArgs& P, const ContractSite& S, double* v0, double* v1, double* red) {
    if (threadIdx.x == 0) v0[0] = 1.0;
    __syncthreads();
    for (int i = S.d - 1; i > S.k; --i) {
        contract_trail(S.xb + P.x.off[i], P.x.dims[i], (int)S.xr[i], (int)S.xr[i + 1], S.wb + P.woff[i], v0, v1, red);
        double* t = v0; v0 = v1; v1 = t;
    }
    return v0;
}

// Sites that need vector chains only: the run in front starts at the left end (or there is none) — workspace: p, p', v, v' (rcap each)
// and u (ncap * rcap)
__global__ void __launch_bounds__(CONTRACT_VEC_TB) k_contract_vec(ContractArgs P) {
    __shared__ double red[64 * (CONTRACT_VEC_TB / 64)];
    const ContractSite S = contract_site(P);
    double* wk = P.work + ((long long)blockIdx.x + (long long)gridDim.x * blockIdx.y) * P.wsz;
    double* p0 = wk; double* p1 = p0 + P.rcap; double* v0 = p1 + P.rcap; double* v1 = v0 + P.rcap; double* u = v1 + P.rcap;
    const bool lead = S.s < S.k;
    const double* Xk = S.xb + P.x.off[S.k];
    if (lead) {
        if (threadIdx.x == 0) p0[0] = 1.0;
        __syncthreads();
        for (int i = S.s; i < S.k; ++i) {
            contract_lead(S.xb + P.x.off[i], P.x.dims[i], (int)S.xr[i], (int)S.xr[i + 1], S.wb + P.woff[i], p0, p1);
            double* t = p0; p0 = p1; p1 = t;
        }
    }
    if (!S.trail) {                                                      // Y[z, 0, a] = sum_c p[c] X[z, c, a]
        contract_lead(Xk, S.n, S.rl, S.rr, nullptr, p0, S.Y);
        return;
    }
    const double* v = contract_trail_chain(P, S, v0, v1, red);
    if (!lead) {                                                         // Y[z, c, 0] = sum_a X[z, c, a] v[a]
        contract_trail(Xk, S.n, S.rl, S.rr, nullptr, v, S.Y, red);
        return;
    }
    contract_trail(Xk, S.n, S.rl, S.rr, nullptr, v, u, red);             // u[z + n c], then Y[z, 0, 0] = sum_c p[c] u[z + n c]
    for (int z = threadIdx.x; z < S.n; z += CONTRACT_VEC_TB) {
        double acc = 0.0;
        for (int c = 0; c < S.rl; ++c) acc = fma(p0[c], u[z + (long long)S.n * c], acc);
        S.Y[z] = acc;
    }
}

// ---- the on-chip route -------------------------------------------------------------------------------------------------------------
// The fibre pairs (z = 0, 1) of a core (2, rl, rr), 8 per thread, element e = c + 64 a of the padded 64 x 64 index space: zero outside
__device__ __forceinline__ void contract_chip_load(const double* X, int rl, int rr, contract_f64x2 (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int e = threadIdx.x + CONTRACT_CHIP_TB * j, c = e & 63, a = e >> 6;
        const bool ok = c < rl && a < rr;
        v[j] = *(contract_gmem_f64x2*)(X + (ok ? 2 * (c + rl * a) : 0));
        if (!ok) { v[j].x = 0.0; v[j].y = 0.0; }
    }
}

// acc[j] += A B for the wave's two column tiles: A[i = a][k = c] from the image at img[c + 66 a] (rows a = 16 tr + .), B[k = c][j = a']
// from PT[80 c + a'] (columns a' = 16 (2 th + j) + .), k over c < 4 nt
__device__ __forceinline__ void contract_chip_mma(const lds_f64* img, const lds_f64* PT, int nt, int tr, int th, mfma_acc_t& acc0, mfma_acc_t& acc1) {
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    const lds_f64* ap = img + CONTRACT_X_LD * (16 * tr + li) + lk;
    const lds_f64* bp = PT + CONTRACT_PT_LD * lk + 32 * th + li;
    for (int t = 0; t < nt; ++t) {
        const double a = ap[4 * t];
        const double b0 = bp[4 * CONTRACT_PT_LD * t], b1 = bp[4 * CONTRACT_PT_LD * t + 16];
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc1, 0, 0, 0);
    }
}

// One workgroup of 8 waves per (kept site, train); wave w owns the rows a = 16 (w & 3) + . and the columns a' = 32 (w >> 2) + . of the
// 64 x 64 product.  The images are zero outside the current ranks, so no fragment read is masked.
__global__ void __launch_bounds__(CONTRACT_CHIP_TB) k_contract_chip(ContractArgs P) {
    extern __shared__ __attribute__((aligned(16))) double contract_smem[];
    lds_f64* PT = (lds_f64*)contract_smem;                               // P^T: P[a', c] at PT[80 c + a']
    lds_f64* X0 = PT + CONTRACT_PT_DOUBLES;                              // M_i[c, a], or X_k[0, c, a], at X0[c + 66 a]
    lds_f64* X1 = X0 + CONTRACT_X_DOUBLES;                               // X_k[1, c, a]
    double* red = contract_smem + CONTRACT_PT_DOUBLES + 2 * CONTRACT_X_DOUBLES;
    double* vec = red + CONTRACT_RED_DOUBLES;
    const ContractSite S = contract_site(P);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int tr = wave & 3, th = wave >> 2;
    const int L = S.L;
    contract_f64x2 v[8];
    {   // P = M_s: element (a', c) of the core of site s, a' the contiguous index
        const double* ws = S.wb + P.woff[S.s];
        const double w0 = ws[0], w1 = ws[1];
        contract_chip_load(S.xb + P.x.off[S.s], L, (int)S.xr[S.s + 1], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = tid + CONTRACT_CHIP_TB * j;
            PT[CONTRACT_PT_LD * (e >> 6) + (e & 63)] = fma(w1, v[j].y, w0 * v[j].x);
        }
    }
    for (int i = S.s + 1; i < S.k; ++i) {                                // P <- P M_i
        const int rl = (int)S.xr[i], rr = (int)S.xr[i + 1];
        const double* wi = S.wb + P.woff[i];
        const double w0 = wi[0], w1 = wi[1];
        contract_chip_load(S.xb + P.x.off[i], rl, rr, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = tid + CONTRACT_CHIP_TB * j;
            X0[(e & 63) + CONTRACT_X_LD * (e >> 6)] = fma(w1, v[j].y, w0 * v[j].x);
        }
        __syncthreads();
        mfma_acc_t acc0 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}, acc1 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
        if (16 * tr < rr) contract_chip_mma(X0, PT, (rl + 3) >> 2, tr, th, acc0, acc1);     // (wave-uniform)
        __syncthreads();                                                 // every read of PT and of the image is done
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {                              // P'[a', a]: row a = 16 tr + lk + 4 reg of the product, zero outside (rr, L)
            const int a = 16 * tr + lk + 4 * reg, ap = 32 * th + li;
            PT[CONTRACT_PT_LD * a + ap] = (a < rr && ap < L) ? acc0[reg] : 0.0;
            PT[CONTRACT_PT_LD * a + ap + 16] = (a < rr && ap + 16 < L) ? acc1[reg] : 0.0;
        }
    }
    const double* Xk = S.xb + P.x.off[S.k];
    if (S.trail) {                                                       // Y[z, a', 0] = sum_c P[a', c] (X_k[z] v)[c]
        __syncthreads();
        const double* vv = contract_trail_chain(P, S, vec, vec + CONTRACT_RMAX, red);
        double* u = vec + 2 * CONTRACT_RMAX;
        contract_trail(Xk, 2, S.rl, S.rr, nullptr, vv, u, red);
        if (tid < 2 * L) {
            const int z = tid & 1, ap = tid >> 1;
            double acc = 0.0;
            for (int c = 0; c < S.rl; ++c) acc = fma((double)PT[CONTRACT_PT_LD * c + ap], u[z + 2 * c], acc);
            S.Y[tid] = acc;
        }
        return;
    }
    contract_chip_load(Xk, S.rl, S.rr, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int e = tid + CONTRACT_CHIP_TB * j, o = (e & 63) + CONTRACT_X_LD * (e >> 6);
        X0[o] = v[j].x; X1[o] = v[j].y;
    }
    __syncthreads();
    if (16 * tr >= S.rr) return;                                         // (wave-uniform; no barrier follows)
    mfma_acc_t y00 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}, y01 = y00, y10 = y00, y11 = y00;
    contract_chip_mma(X0, PT, (S.rl + 3) >> 2, tr, th, y00, y01);
    contract_chip_mma(X1, PT, (S.rl + 3) >> 2, tr, th, y10, y11);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {                                  // Y[., a', a]: 16 bytes per lane, the lanes along a'
        const int a = 16 * tr + lk + 4 * reg, ap = 32 * th + li;
        if (a < S.rr && ap < L) *reinterpret_cast<contract_f64x2*>(S.Y + 2 * (ap + L * a)) = (contract_f64x2){y00[reg], y10[reg]};
        if (a < S.rr && ap + 16 < L) *reinterpret_cast<contract_f64x2*>(S.Y + 2 * (ap + 16 + L * a)) = (contract_f64x2){y01[reg], y11[reg]};
    }
}

// ---- the general route -------------------------------------------------------------------------------------------------------------
// out[f] = sum_z w[z] X[z, f] over the fibres of a core
__device__ __forceinline__ void contract_form(const double* X, int n, int fibres, const double* w, double* out) {
    for (int f = threadIdx.x; f < fibres; f += TTN_WG) out[f] = contract_fibre(X + (long long)n * f, w, n);
}

// Workspace of a workgroup: M (rcap^2), P, P' (rcap^2 each), v, v' (rcap each), u (ncap * rcap)
__global__ void TTN_KERNEL_BOUNDS k_contract_gen(ContractArgs P) {
    extern __shared__ __attribute__((aligned(16))) double contract_smem[];
    double* lds = contract_smem;
    const ContractSite S = contract_site(P);
    double* wk = P.work + ((long long)blockIdx.x + (long long)gridDim.x * blockIdx.y) * P.wsz;
    const long long r2 = (long long)P.rcap * P.rcap;
    double* Mb = wk; double* Pa = Mb + r2; double* Pb = Pa + r2; double* v0 = Pb + r2; double* v1 = v0 + P.rcap; double* u = v1 + P.rcap;
    const int L = S.L;
    contract_form(S.xb + P.x.off[S.s], P.x.dims[S.s], L * (int)S.xr[S.s + 1], S.wb + P.woff[S.s], Pa);      // P = M_s, L x r_{s+1} column-major
    for (int i = S.s + 1; i < S.k; ++i) {
        const int rl = (int)S.xr[i], rr = (int)S.xr[i + 1];
        __syncthreads();                                                 // nobody still reads M in the product before
        contract_form(S.xb + P.x.off[i], P.x.dims[i], rl * rr, S.wb + P.woff[i], Mb);
        wg_gemm(L, rr, rl, mkview(Pa, plain(1), plain(L)), mkview(Mb, plain(1), plain(rl)), mkview(Pb, plain(1), plain(L)), 1.0, 0.0, lds);
        double* t = Pa; Pa = Pb; Pb = t;
    }
    double* Xk = const_cast<double*>(S.xb) + P.x.off[S.k];
    const int n = S.n;
    if (!S.trail) {                                                      // Y[a', (z, a)] = sum_c P[a', c] X_k[c, (z, a)]
        wg_gemm(L, n * S.rr, S.rl, mkview(Pa, plain(1), plain(L)), mkview(Xk, plain(n), Idx{n, 1, (long long)n * S.rl}),
                mkview(S.Y, plain(n), Idx{n, 1, (long long)n * L}), 1.0, 0.0, lds);
        return;
    }
    __syncthreads();
    const double* vv = contract_trail_chain(P, S, v0, v1, lds);
    contract_trail(Xk, n, S.rl, S.rr, nullptr, vv, u, lds);
    for (int e = threadIdx.x; e < n * L; e += TTN_WG) {                  // Y[z, a', 0] = sum_c P[a', c] u[z + n c]
        const int z = e % n, ap = e / n;
        double acc = 0.0;
        for (int c = 0; c < S.rl; ++c) acc = fma(Pa[ap + (long long)L * c], u[z + (long long)n * c], acc);
        S.Y[e] = acc;
    }
}
