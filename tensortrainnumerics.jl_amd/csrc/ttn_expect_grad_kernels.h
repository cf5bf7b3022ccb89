// ttn_expect_grad_kernels.h — the pullback of s = <x, A y> (include/ttn_expect_grad.h: ttn_sandwich_pullback) on the three-layer
// environments, without A y: neither that train (ranks R r) nor a cotangent of its size exists in memory.  Float64 only.
//
//   environments, r^x x R x r^y, column-major [al + r^x (rho + R be)], each computed ONCE per call and every state kept:
//       L_1 = [1],      L_{k+1}[a, rho, b]   = sum L_k[al, rl, bl] x_k[i, al, a] A_k[i, j, rl, rho] y_k[j, bl, b]
//       G_{N+1} = [1],  G_k[al, rl, bl]      = sum G_{k+1}[a, rho, b] x_k[i, al, a] A_k[i, j, rl, rho] y_k[j, bl, b]
//   gradients:          xbar_k[i, al, a]     = delta sum L_k[al, rl, bl] A_k[i, j, rl, rho] y_k[j, bl, b] G_{k+1}[a, rho, b]
//                       ybar_k[j, bl, b]     = delta sum L_k[al, rl, bl] x_k[i, al, a] A_k[i, j, rl, rho] G_{k+1}[a, rho, b]
//
// k_expgrad_chain<RM>   grid (batch, 2): block (t, 0) walks L left to right on expect_site_generic (ttn_expect_kernels.h has no
//                       left-to-right on-chip site), slot k -> slot k + 1; block (t, 1) walks G right to left — a train of the on-chip
//                       class (every n_k = 2, train ranks <= 64, operator ranks <= RM <= 5) on expect_site_qtt, whose state of R 64 x 64
//                       images is copied to the compact slot after every site; any other train on expgrad_site_generic_rl.
// k_expgrad_core<RM>    the on-chip class: grid (4, 2 N, batch), 4 waves.  An output O[z', p, q] = delta sum E1[p, rl, s] c[z', z, rl, rho]
//                       C[z, s, t] E2[q, rho, t] (xbar: p = al, s = bl, C = y_k; ybar: p = bl, s = al, C = x_k, the two physical indices
//                       of A_k swapped) is computed TRANSPOSED so that no intermediate leaves the registers: a block owns 16 rows p,
//                       wave w the block t = 16 w + . of the inner index;
//                         1.  T1_z[t, p; rl] = sum_s C[z, s, t] E1[p, rl, s]          MFMA, 2 R accumulators per wave
//                         2.  T2_z'[t, p; rho] = sum_{z, rl} c[z', z, rl, rho] T1_z   wave-uniform coefficients on the accumulators
//                         3.  O_z'[q, p] += sum_{t in the wave's block} E2[q, rho, t] T2_z'[t, p; rho]   MFMA: register r of T2 IS the B
//                             fragment of k-step r (the observation of k_dot / k_expect), summed over rho in the accumulators
//                       and the (up to) four partial sums over t meet in LDS, each in its own plane, added in the fixed order w = 0 .. 3:
//                       no atomics, the same call gives the same bits.
// k_expgrad_core_gen    every other train: grid (2 N, batch), one workgroup per output, three calls of the workgroup GEMM with T1 and T2
//                       in library workspace (fixed summation order).
// A train takes one route for its whole chain and all its outputs, decided from its rank words as k_expect decides; a batch may mix.
// The decision is made in ONE place: block (t, 1) of k_expgrad_chain writes it to route[t], and the gradient kernels, which run after it
// on the stream, read that word.  The boundary ranks need not be 1 (a segment of a train, constructors.Delta_NN): L_1 and G_{N+1} are
// e_1 over their whole slot, rx R ry entries, so the value and the tangents are those of the [1, 1, 1] boundary entry.
#pragma once
#include "ttn_common.h"
#include "ttn_wg_gemm.h"
#include "ttn_dot_kernels.h"
#include "ttn_expect_kernels.h"

#define EXPGRAD_TB 256                   // threads of k_expgrad_core: 4 waves, wave w owns t = 16 w .. 16 w + 15
#define EXPGRAD_PP 17                    // row pitch (doubles) of a partial-sum plane: O^T[q, p] at q * 17 + p
#define EXPGRAD_PLANE (EXPECT_QTT_RMAX * EXPGRAD_PP)
static_assert(sizeof(double) * 4 * EXPGRAD_PLANE <= 64 * 1024, "k_expgrad_core: four partial-sum planes in static LDS");
static_assert(EXPECT_LDS_BYTES(EXPECT_MAX_D) <= 160 * 1024, "k_expgrad_chain: the LDS of a workgroup is 160 KiB");
static_assert(sizeof(double) * GEMM_LDS_TOTAL <= 160 * 1024, "k_expgrad_core_gen: the LDS of a workgroup is 160 KiB");

struct ExpGradArgs {
    TTDev x, y, xbar, ybar;     // xbar.data / ybar.data null: that output is not wanted
    TTODev A;
    double* env;                // [batch][2][d + 1][W]: L_1 .. L_{N+1}, then G_1 .. G_{N+1}
    double* work;               // [batch][2][wsz]: per chain, U and V of the GEMM sites or the R images of the on-chip G chain
    double* gwork;              // [batch][2 N][2 nmax S]: T1 and T2 of the general gradient route (null when no train can take it)
    int* route;                 // [batch]: 1 the on-chip class, 0 the general route; written by k_expgrad_chain, read by the gradient kernels
    long long W, wsz, S;        // S = rxmax Rmax rymax
    int nmax;
    const double* delta;        // [batch] on the device, or null: 1
    double* out;                // [batch] device: L_{N+1}[1, 1, 1], or null
};

// One site of the general route, RIGHT TO LEFT: rx2, R2, ry2 are the RIGHT ranks (incoming state Gc[a + rx2 (rho + R2 b)]), rx, R, ry the
// left ranks (outgoing Gn[al + rx (rl + R bl)]).  U at a + rx2 (rho + R2 (j + n bl)), V at i + n (a + rx2 (rl + R bl)).
__device__ __noinline__ void expgrad_site_generic_rl(double* Xk, double* Yk, double* Ak, double* Gc, double* Gn, double* U, double* V, int n, int rx, int rx2,
                                                     int R, int R2, int ry, int ry2, double* lds) {
    Xk = unip(Xk); Yk = unip(Yk); Ak = unip(Ak); Gc = unip(Gc); Gn = unip(Gn); U = unip(U); V = unip(V); lds = unip(lds);
    n = uni32(n); rx = uni32(rx); rx2 = uni32(rx2); R = uni32(R); R2 = uni32(R2); ry = uni32(ry); ry2 = uni32(ry2);
    const long long rxR2 = (long long)rx2 * R2;
    // step 1: U[(a, rho), (j, bl)] = sum_b G[(a, rho), b] y_k[j, bl, b]
    wg_gemm(rx2 * R2, n * ry, ry2, mkview(Gc, plain(1), plain(rxR2)), mkview(Yk, plain((long long)n * ry), plain(1)), mkview(U, plain(1), plain(rxR2)), 1.0, 0.0, lds);
    // step 2: V[(a, bl), (i, rl)] = sum_{(rho, j)} U[(a, bl), (rho, j)] A_k[i, j, rl, rho]
    wg_gemm(rx2 * ry, n * R, R2 * n, mkview(U, Idx{rx2, 1, rxR2 * n}, plain(rx2)), mkview(Ak, Idx{R2, (long long)n * n * R, n}, Idx{n, 1, (long long)n * n}),
            mkview(V, Idx{rx2, n, (long long)n * rx2 * R}, Idx{n, 1, (long long)n * rx2}), 1.0, 0.0, lds);
    // step 3: G'[al, (rl, bl)] = sum_{(i, a)} x_k[i, al, a] V[(i, a), (rl, bl)]
    wg_gemm(rx, R * ry, n * rx2, mkview(Xk, plain(n), Idx{n, 1, (long long)n * rx}), mkview(V, plain(1), plain((long long)n * rx2)), mkview(Gn, plain(1), plain(rx)),
            1.0, 0.0, lds);
}

// Block (t, 0): L_1 .. L_{N+1}; block (t, 1): G_{N+1} .. G_1.  RM as in k_expect.
template <int RM>
__global__ void __launch_bounds__(TTN_WG) k_expgrad_chain(ExpGradArgs P) {
    extern __shared__ double lds[];
    const int t = blockIdx.x, dir = blockIdx.y;
    const int tid = threadIdx.x;
    const TTDev& X = P.x; const TTDev& Y = P.y; const TTODev& A = P.A;
    const int d = X.d;
    lds_i32* tab = (lds_i32*)((lds_f64*)lds + EXPECT_LDS_DOUBLES);   // k_expect's table: [0] rx_k [1] ry_k [2] R_k [3] n_k [4] offx_k [5] offy_k [6] offA_k
    for (int k = tid; k <= d; k += TTN_WG) {
        tab[EXPECT_TAB * k + 0] = (int)X.rks[(long long)t * (d + 1) + k];
        tab[EXPECT_TAB * k + 1] = (int)Y.rks[(long long)t * (d + 1) + k];
        tab[EXPECT_TAB * k + 2] = (int)A.rks[k];
        tab[EXPECT_TAB * k + 3] = k < d ? X.dims[k] : 0;
        tab[EXPECT_TAB * k + 4] = k < d ? (int)X.off[k] : 0;              // trains and operator are below 2^31 doubles (checked by the host)
        tab[EXPECT_TAB * k + 5] = k < d ? (int)Y.off[k] : 0;
        tab[EXPECT_TAB * k + 6] = k < d ? (int)A.off[k] : 0;
    }
    __syncthreads();
    double* Xbase = X.data + (long long)t * X.stride;
    double* Ybase = Y.data + (long long)t * Y.stride;
    double* Abase = const_cast<double*>(A.data) + (long long)t * A.stride;      // (stride 0: one operator for every train)
    double* E = P.env + ((long long)t * 2 + dir) * (d + 1) * P.W;
    double* wk = P.work + ((long long)t * 2 + dir) * P.wsz;
    if (dir == 0) {
        double* U = wk; double* V = wk + (long long)P.nmax * P.S;
        const int tot0 = uni32(tab[0]) * uni32(tab[2]) * uni32(tab[1]);  // L_1 = e_1 over the whole slot: the boundary ranks need not be 1
        for (int e = tid; e < tot0; e += TTN_WG) E[e] = (e == 0) ? 1.0 : 0.0;
        __syncthreads();
        for (int k = 0; k < d; ++k) {
            const lds_i32* s = tab + EXPECT_TAB * k;
            expect_site_generic(Xbase + uni32(s[4]), Ybase + uni32(s[5]), Abase + uni32(s[6]), E + (long long)k * P.W, E + (long long)(k + 1) * P.W, U, V,
                                uni32(s[3]), uni32(s[0]), uni32(s[EXPECT_TAB]), uni32(s[2]), uni32(s[EXPECT_TAB + 2]), uni32(s[1]), uni32(s[EXPECT_TAB + 1]), lds);
            __syncthreads();
        }
        if (P.out && tid == 0) P.out[t] = E[(long long)d * P.W];
        return;
    }
    {
        const lds_i32* s = tab + EXPECT_TAB * d;                         // G_{N+1} = e_1 over the whole slot
        const int totd = uni32(s[0]) * uni32(s[2]) * uni32(s[1]);
        double* Ed = E + (long long)d * P.W;
        for (int e = tid; e < totd; e += TTN_WG) Ed[e] = (e == 0) ? 1.0 : 0.0;
    }
    bool fit = RM > 0;                                                   // every n_k = 2 and the operator ranks <= RM: known on the host
    if (RM > 0)
        for (int k = 0; k <= d; ++k) fit = fit && uni32(tab[EXPECT_TAB * k]) <= EXPECT_QTT_RMAX && uni32(tab[EXPECT_TAB * k + 1]) <= EXPECT_QTT_RMAX;
    if (tid == 0) P.route[t] = fit ? 1 : 0;
    if (RM > 0) {
        if (fit) {
            lds_f64* img = (lds_f64*)lds;
            lds_f64* Ac = img + 2 * DOT_MS_DOUBLES;
            const int Rlast = uni32(tab[EXPECT_TAB * d + 2]);
            for (int e = tid; e < 2 * DOT_MS_DOUBLES; e += TTN_WG) img[e] = 0.0;
            for (int e = tid; e < Rlast * EXPECT_IMG_STATE; e += TTN_WG) wk[e] = (e == 0) ? 1.0 : 0.0;
            __syncthreads();
            for (int k = d - 1; k >= 0; --k) {
                const lds_i32* s = tab + EXPECT_TAB * k;
                const int rx2 = uni32(s[0]), R2 = uni32(s[2]), ry2 = uni32(s[1]);                       // the LEFT ranks: the outgoing state
                expect_site_qtt<(RM > 0 ? RM : 1)>(Xbase + uni32(s[4]), Ybase + uni32(s[5]), Abase + uni32(s[6]), wk, uni32(s[EXPECT_TAB]), rx2,
                                                   uni32(s[EXPECT_TAB + 2]), R2, uni32(s[EXPECT_TAB + 1]), ry2, Ac, img);
                // the finished state to its compact slot (expect_site ended on a barrier; the next site only reads the images)
                double* Ek = E + (long long)k * P.W;
                const int tot = rx2 * R2 * ry2;
                for (int e = tid; e < tot; e += TTN_WG) {
                    const int a = e % rx2, f = e / rx2, rho = f % R2, b = f / R2;
                    Ek[e] = wk[a + EXPECT_QTT_RMAX * (b + EXPECT_QTT_RMAX * rho)];
                }
            }
            return;
        }
    }
    double* U = wk; double* V = wk + (long long)P.nmax * P.S;
    __syncthreads();
    for (int k = d - 1; k >= 0; --k) {
        const lds_i32* s = tab + EXPECT_TAB * k;
        expgrad_site_generic_rl(Xbase + uni32(s[4]), Ybase + uni32(s[5]), Abase + uni32(s[6]), E + (long long)(k + 1) * P.W, E + (long long)k * P.W, U, V,
                                uni32(s[3]), uni32(s[0]), uni32(s[EXPECT_TAB]), uni32(s[2]), uni32(s[EXPECT_TAB + 2]), uni32(s[1]), uni32(s[EXPECT_TAB + 1]), lds);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// per-core gradients, the on-chip class
// ---------------------------------------------------------------------------------------------
template <int RM>
__global__ void __launch_bounds__(EXPGRAD_TB) k_expgrad_core(ExpGradArgs P) {
    __shared__ double part[4 * EXPGRAD_PLANE];
    const int k = blockIdx.y >> 1, which = blockIdx.y & 1, t = blockIdx.z;
    const TTDev& dst = which ? P.ybar : P.xbar;
    if (!dst.data) return;
    if (!P.route[t]) return;                                             // k_expgrad_core_gen owns this train
    const int d = P.x.d;
    const long long* xr = P.x.rks + (long long)t * (d + 1);
    const long long* yr = P.y.rks + (long long)t * (d + 1);
    const int rxl = (int)xr[k], rxr = (int)xr[k + 1], ryl = (int)yr[k], ryr = (int)yr[k + 1];
    const int R = (int)P.A.rks[k], R2 = (int)P.A.rks[k + 1];
    // O[z', p, q] = delta sum E1[p, rl, s] c[z', z, rl, rho] C[z, s, t] E2[q, rho, t]
    //   xbar: p = al, q = a, s = bl, t = b, C = y_k, c = A_k[z', z];     ybar: p = bl, q = b, s = al, t = a, C = x_k, c = A_k[z, z']
    const int Pn = which ? ryl : rxl, Q = which ? ryr : rxr, S = which ? rxl : ryl, T = which ? rxr : ryr;
    const int p0 = 16 * blockIdx.x;
    if (p0 >= Pn) return;
    const int e1p = which ? rxl * R : 1, e1r = rxl, e1s = which ? 1 : rxl * R;
    const int e2q = which ? rxr * R2 : 1, e2r = rxr, e2t = which ? 1 : rxr * R2;
    const int cz = which ? 1 : 2, czp = which ? 2 : 1;                   // A_k[i, j] at i + 2 j: strides of z (summed) and z' (output)
    const TTDev& src = which ? P.x : P.y;
    const double* Cc = src.data + (long long)t * src.stride + src.off[k];
    double* O = dst.data + (long long)t * dst.stride + dst.off[k];
    gmem_f64* L = (gmem_f64*)(P.env + ((long long)t * 2) * (d + 1) * P.W + (long long)k * P.W);
    gmem_f64* G = (gmem_f64*)(P.env + ((long long)t * 2 + 1) * (d + 1) * P.W + (long long)(k + 1) * P.W);
    const double* Ak = P.A.data + (long long)t * P.A.stride + P.A.off[k];
    const double dl = P.delta ? P.delta[t] : 1.0;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int nb = (T + 15) >> 4;                                         // waves that own a block of t
    const int ntq = (Q + 15) >> 4;
    mfma_acc_t m[2][4];
#pragma unroll
    for (int zp = 0; zp < 2; ++zp)
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) m[zp][tq] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
    if (w < nb) {                                                         // wave-uniform
        // ---- step 1: T1_z[t = 16 w + ., p = p0 + .; rl] = sum_s C[z, s, t] E1[p, rl, s] ----
        mfma_acc_t u[RM][2];
#pragma unroll
        for (int rl = 0; rl < RM; ++rl) { u[rl][0] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}; u[rl][1] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}; }
        const int tq_ = 16 * w + li;                                      // this lane's row t of the A fragment
        const bool pok = p0 + li < Pn;
        const int ns = (S + 3) >> 2;
        for (int kk = 0; kk < ns; ++kk) {
            const int s = 4 * kk + lk;
            const dot_f64x2 cv = dot_load2(Cc, s, tq_, S, T, S);          // C[., s, t]
            const bool ok = pok && s < S;
            const int eo = ok ? (p0 + li) * e1p + s * e1s : 0;
#pragma unroll
            for (int rl = 0; rl < RM; ++rl) {
                if (rl < R) {                                             // wave-uniform
                    double ev = L[eo + rl * e1r];
                    if (!ok) ev = 0.0;
                    u[rl][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(cv.x, ev, u[rl][0], 0, 0, 0);
                    u[rl][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(cv.y, ev, u[rl][1], 0, 0, 0);
                }
            }
        }
        for (int rho = 0; rho < R2; ++rho) {
            // ---- step 2: T2_z'[t, p; rho] = sum_{z, rl} c[z', z, rl, rho] T1_z[t, p; rl], on the accumulators ----
            mfma_acc_t v0 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}, v1 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int rl = 0; rl < RM; ++rl) {
                if (rl < R) {
                    const double* c = Ak + 4 * (rl + R * rho);
                    const double c00 = c[0], c01 = c[cz], c10 = c[czp], c11 = c[cz + czp];          // c[z'][z]
                    v0 += c00 * u[rl][0] + c01 * u[rl][1];
                    v1 += c10 * u[rl][0] + c11 * u[rl][1];
                }
            }
            // ---- step 3, partial over this wave's t: O_z'[q, p] += sum_r E2[q, rho, t = 16 w + 4 r + lk] T2_z'[t, p; rho] ----
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) {
                if (tq < ntq) {                                           // wave-uniform
                    const int q = 16 * tq + li;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int tt = 16 * w + 4 * r + lk;
                        const bool ok = q < Q && tt < T;
                        double gv = G[ok ? q * e2q + rho * e2r + tt * e2t : 0];
                        if (!ok) gv = 0.0;
                        m[0][tq] = __builtin_amdgcn_mfma_f64_16x16x4f64(gv, v0[r], m[0][tq], 0, 0, 0);
                        m[1][tq] = __builtin_amdgcn_mfma_f64_16x16x4f64(gv, v1[r], m[1][tq], 0, 0, 0);
                    }
                }
            }
        }
    }
    // ---- the partial sums of the waves, each in its own plane, added in the order w = 0 .. nb - 1 ----
    const int n = 2;
#pragma unroll
    for (int zp = 0; zp < 2; ++zp) {
        __syncthreads();                                                  // the readers of the previous z' are done
        if (w < nb) {
#pragma unroll
            for (int tq = 0; tq < 4; ++tq)
                if (tq < ntq)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) part[w * EXPGRAD_PLANE + (16 * tq + 4 * reg + lk) * EXPGRAD_PP + li] = m[zp][tq][reg];
        }
        __syncthreads();
        for (int e = tid; e < 16 * 16 * ntq; e += EXPGRAD_TB) {
            const int p = e & 15, q = e >> 4;
            if (p0 + p < Pn && q < Q) {
                double acc = part[q * EXPGRAD_PP + p];
                for (int ww = 1; ww < nb; ++ww) acc += part[ww * EXPGRAD_PLANE + q * EXPGRAD_PP + p];
                O[zp + n * ((p0 + p) + (long long)Pn * q)] = dl * acc;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// per-core gradients, every other train: one workgroup per output, T1 (U) and T2 (V) in workspace
// ---------------------------------------------------------------------------------------------
template <bool QTT>
__global__ void __launch_bounds__(TTN_WG) k_expgrad_core_gen(ExpGradArgs P) {
    extern __shared__ double lds[];
    const int k = blockIdx.x >> 1, which = blockIdx.x & 1, t = blockIdx.y;
    const TTDev& dst = which ? P.ybar : P.xbar;
    if (!dst.data) return;
    if (QTT && P.route[t]) return;                                       // k_expgrad_core owns this train
    const int d = uni32(P.x.d);
    const long long* xr = P.x.rks + (long long)t * (d + 1);
    const long long* yr = P.y.rks + (long long)t * (d + 1);
    const int rx = uni32((int)xr[k]), rx2 = uni32((int)xr[k + 1]), ry = uni32((int)yr[k]), ry2 = uni32((int)yr[k + 1]);
    const int R = uni32((int)P.A.rks[k]), R2 = uni32((int)P.A.rks[k + 1]);
    const int n = uni32(P.x.dims[k]);
    double* Xk = unip(P.x.data + (long long)t * P.x.stride + P.x.off[k]);
    double* Yk = unip(P.y.data + (long long)t * P.y.stride + P.y.off[k]);
    double* Ak = unip(const_cast<double*>(P.A.data) + (long long)t * P.A.stride + P.A.off[k]);
    double* O = unip(dst.data + (long long)t * dst.stride + dst.off[k]);
    double* L = unip(P.env + ((long long)t * 2) * (d + 1) * P.W + (long long)k * P.W);                    // L_k[al + rx (rl + R bl)]
    double* G = unip(P.env + ((long long)t * 2 + 1) * (d + 1) * P.W + (long long)(k + 1) * P.W);          // G_{k+1}[a + rx2 (rho + R2 b)]
    double* U = unip(P.gwork + ((long long)t * 2 * d + blockIdx.x) * (2LL * P.nmax * P.S));
    double* V = unip(U + (long long)P.nmax * P.S);
    const double dl = P.delta ? P.delta[t] : 1.0;
    const long long rxR = (long long)rx * R, ryR = (long long)ry * R;
    if (!which) {
        // steps 1 and 2 of expect_site_generic: U at al + rx (rl + R (j + n b)), V at i + n (al + rx (rho + R2 b))
        wg_gemm(rx * R, n * ry2, ry, mkview(L, plain(1), plain(rxR)), mkview(Yk, plain(n), Idx{n, 1, (long long)n * ry}), mkview(U, plain(1), plain(rxR)), 1.0, 0.0, lds);
        wg_gemm(rx * ry2, n * R2, R * n, mkview(U, Idx{rx, 1, rxR * n}, plain(rx)), mkview(Ak, Idx{R, (long long)n * n, n}, Idx{n, 1, (long long)n * n * R}),
                mkview(V, Idx{rx, n, (long long)n * rx * R2}, Idx{n, 1, (long long)n * rx}), 1.0, 0.0, lds);
        // step 3: xbar[(i, al), a] = delta sum_{(rho, b)} V[(i, al), (rho, b)] G[a, (rho, b)]
        wg_gemm(n * rx, rx2, R2 * ry2, mkview(V, plain(1), plain((long long)n * rx)), mkview(G, plain(rx2), plain(1)), mkview(O, plain(1), plain((long long)n * rx)),
                dl, 0.0, lds);
    } else {
        // step 1: U[(rl, bl), (i, a)] = sum_al L[al, (rl, bl)] x_k[i, al, a], stored at bl + ry (rl + R (i + n a))
        wg_gemm(R * ry, n * rx2, rx, mkview(L, plain(rx), plain(1)), mkview(Xk, plain(n), Idx{n, 1, (long long)n * rx}), mkview(U, Idx{R, ry, 1}, plain(ryR)), 1.0, 0.0, lds);
        // step 2: V[(bl, a), (j, rho)] = sum_{(rl, i)} U[(bl, a), (rl, i)] A_k[i, j, rl, rho], stored at j + n (bl + ry (rho + R2 a))
        wg_gemm(ry * rx2, n * R2, R * n, mkview(U, Idx{ry, 1, ryR * n}, plain(ry)), mkview(Ak, Idx{R, (long long)n * n, 1}, Idx{n, n, (long long)n * n * R}),
                mkview(V, Idx{ry, n, (long long)n * ry * R2}, Idx{n, 1, (long long)n * ry}), 1.0, 0.0, lds);
        // step 3: ybar[(j, bl), b] = delta sum_{(rho, a)} V[(j, bl), (rho, a)] G[a, rho, b]
        wg_gemm(n * ry, ry2, R2 * rx2, mkview(V, plain(1), plain((long long)n * ry)), mkview(G, Idx{R2, rx2, 1}, plain((long long)rx2 * R2)),
                mkview(O, plain(1), plain((long long)n * ry)), dl, 0.0, lds);
    }
}
