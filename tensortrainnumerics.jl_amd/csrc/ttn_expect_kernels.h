// ttn_expect_kernels.h — <x, A y> (include/ttn_expect.h) without forming A y: the three-layer transfer recurrence over the cores of
// x, A and y, one workgroup per train, the scalar the only thing that is written per train.
//
//   state, RIGHT TO LEFT (ttn_dot_kernels.h says why):  M[a, be, b] over the right ranks of x_k, A_k, y_k; per site
//     1.  U_j[a, be, bl]   = sum_b M[a, be, b] y_k[j, bl, b]                    fp64 MFMA, once per be
//     2.  V_i[a, be', bl]  = sum_{j, be} A_k[i, j, be', be] U_j[a, be, bl]     elementwise in (a, bl): acts on the accumulators
//     3.  M'[al, be', bl]  = sum_{i, a} x_k[i, al, a] V_i[a, be', bl]          fp64 MFMA, once per be'
//   it starts from e_1 e_1^T e_1 at the right end and returns M[1, 1, 1] of the state that leaves site 1 — the number
//   ttn_dot(x, ttn_apply(A, y)) computes, up to the order of the rounding errors.
//
// The QTT route (every n_k = 2, train ranks <= EXPECT_QTT_RMAX, operator ranks <= EXPECT_QTT_OPR_MAX) keeps U and V in registers:
//   * wave w of the 16 owns tile (tr = w & 3, tc = w >> 2) of every U_j[., be, .], as k_dot's waves own a tile of T: 2 R accumulators;
//   * step 2 is 4 R R' wave-uniform coefficients (the operator core, staged in LDS once per site) times those accumulators;
//   * the accumulator layout of V_i is the B-operand layout of step 3 (k_dot's observation), so a wave multiplies its V tiles by
//     x_k's fragments for the four output row blocks and holds PARTIAL sums over its a-block of M'[., be', .];
//   * the four waves of a column block meet in an LDS image (k_dot's swizzled layout, LDS atomics), ONE be' at a time: two images
//     rotate — pass be' adds into one while the other, complete since the barrier that ended pass be' - 1, is written to the state and
//     zeroed.  R images in and R' images out (41 KiB each) do not fit the LDS for R >= 2, which is why the state itself does not live
//     there: it sits in library workspace as R dense 64 x 64 images per train (32 KiB R, written once and read once per site by the
//     same CU: it stays in L2), zero outside the current ranks, so step 1 reads it without masks.
// From HBM a site reads its three cores and nothing else; U and V never exist in memory.
//
// The general route (any n, any ranks, any R) runs the same three steps LEFT TO RIGHT as three calls of the workgroup GEMM per site, the
// state, U and V in library workspace — step 2 as the skinny product [(al, b), (be, j)] x [(be, j), (i, be')].
// One train takes one route for the whole chain (decided per train from its rank words, as k_dot decides).
#pragma once
#include "ttn_common.h"
#include "ttn_wg_gemm.h"
#include "ttn_dot_kernels.h"

#define EXPECT_QTT_RMAX DOT_RMAX                 // largest train rank of the QTT route (= TTN_EXPECT_QTT_MAX_RANK of the public header)
#define EXPECT_QTT_OPR_MAX 5                     // largest operator rank of the QTT route: 2 R accumulators of U live in a wave's registers
#define EXPECT_MAX_D DOT_MAX_D
#define EXPECT_ACORE_DOUBLES 128                 // >= 4 * EXPECT_QTT_OPR_MAX^2, the staged operator core (behind the two images)
// the QTT route's two images and staged core, or the workgroup GEMM's region of the general route — whichever is larger
#define EXPECT_LDS_DOUBLES ((2 * DOT_MS_DOUBLES + EXPECT_ACORE_DOUBLES) > GEMM_LDS_TOTAL ? (2 * DOT_MS_DOUBLES + EXPECT_ACORE_DOUBLES) : GEMM_LDS_TOTAL)
#define EXPECT_TAB 7                             // ints per site of the table (behind that region)
#define EXPECT_LDS_BYTES(d) (sizeof(double) * EXPECT_LDS_DOUBLES + sizeof(int) * EXPECT_TAB * ((d) + 2))
static_assert(EXPECT_LDS_BYTES(EXPECT_MAX_D) <= 160 * 1024, "k_expect: the LDS of a workgroup is 160 KiB");
static_assert(4 * EXPECT_QTT_OPR_MAX * EXPECT_QTT_OPR_MAX <= EXPECT_ACORE_DOUBLES, "k_expect: the staged operator core");
#define EXPECT_IMG_STATE (EXPECT_QTT_RMAX * EXPECT_QTT_RMAX)      // doubles of one be-image of the state in workspace

struct ExpectArgs {
    TTDev x, y;
    TTODev A;
    double* scratch;            // per train: max(Rmax * EXPECT_IMG_STATE, (2 + 2 nmax) * rxmax * Rmax * rymax)
    long long scratch_stride;
    int rxmax, rymax, Rmax, nmax;
    double* out;                // [batch] device
};

// One site of the QTT route.  rx, R, ry: RIGHT ranks of x_k, A_k, y_k (the incoming state); rx2, R2, ry2: their LEFT ranks.
//   Mg : the state, element (a, be, b) at Mg[a + 64 (b + 64 be)], zero outside (rx, R, ry); overwritten with M' (images be' < R2)
//   Ac : LDS, receives the operator core (i, j, be', be) at i + 2 (j + 2 (be' + R2 be))
//   img: two LDS images, all zero on entry and on exit
template <int RM>
__device__ __forceinline__ void expect_site(const double* Xk, const double* Yk, const double* Ak, double* Mg, int rx, int rx2, int R, int R2, int ry, int ry2,
                                            lds_f64* Ac, lds_f64* img) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int tr = wave & 3, tc = wave >> 2;
    if ((int)threadIdx.x < 4 * R * R2) Ac[threadIdx.x] = ((gmem_f64*)Ak)[threadIdx.x];
    const bool active = 16 * tr < rx && 16 * tc < ry2;                   // wave-uniform
    mfma_acc_t u[RM][2];
#pragma unroll
    for (int be = 0; be < RM; ++be) { u[be][0] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}; u[be][1] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}; }
    if (active) {
        // ---- step 1: U_j[a, be, bl] = sum_b M[a, be, b] y_k[j, bl, b]: rows a = 16 tr + ., columns bl = 16 tc + .; the operands of
        //      k-step t + 1 are requested before the MFMAs of k-step t ----
        const int nt = (ry + 3) >> 2;
        const int bq = 16 * tc + li;
        gmem_f64* mrow = (gmem_f64*)Mg + (16 * tr + li) + 64 * lk;              // M[a, be, b = 4 t + lk]: + 256 t + 4096 be
        dot_f64x2 yv = dot_load2(Yk, bq, lk, ry2, ry, ry2);
        double mv[RM];
#pragma unroll
        for (int be = 0; be < RM; ++be) mv[be] = be < R ? mrow[EXPECT_IMG_STATE * be] : 0.0;
        for (int t = 0; t < nt; ++t) {
            const int tn = t + 1 < nt ? t + 1 : t;
            const dot_f64x2 yn = dot_load2(Yk, bq, 4 * tn + lk, ry2, ry, ry2);
            double mn[RM];
#pragma unroll
            for (int be = 0; be < RM; ++be) mn[be] = be < R ? mrow[256 * tn + EXPECT_IMG_STATE * be] : 0.0;
#pragma unroll
            for (int be = 0; be < RM; ++be) {
                if (be < R) {                                             // wave-uniform
                    u[be][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(mv[be], yv.x, u[be][0], 0, 0, 0);
                    u[be][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(mv[be], yv.y, u[be][1], 0, 0, 0);
                }
            }
            yv = yn;
#pragma unroll
            for (int be = 0; be < RM; ++be) mv[be] = mn[be];
        }
    }
    dot_lds_barrier();                                                    // the staged core is visible
    const int nta = (rx2 + 15) >> 4;
    for (int bp = 0; bp < R2; ++bp) {
        lds_f64* cur = img + (bp & 1) * DOT_MS_DOUBLES;
        lds_f64* prv = img + ((bp & 1) ^ 1) * DOT_MS_DOUBLES;
        if (active) {
            // ---- step 2: V_i[a, bp, bl] = sum_{j, be} A_k[i, j, bp, be] U_j[a, be, bl], on the accumulators ----
            mfma_acc_t v0 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}, v1 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int be = 0; be < RM; ++be) {
                if (be < R) {
                    const lds_f64* c = Ac + 4 * (bp + R2 * be);           // (i, j) at i + 2 j
                    const double c00 = c[0], c10 = c[1], c01 = c[2], c11 = c[3];
                    v0 += c00 * u[be][0] + c01 * u[be][1];
                    v1 += c10 * u[be][0] + c11 * u[be][1];
                }
            }
            // ---- step 3, partial over a in this wave's block: sum_{i, r} x_k[i, al, 16 tr + 4 r + lk] V_i[16 tr + 4 r + lk, bp, bl] — register r
            //      of V_i is the B fragment of k-step r as it is; rows a >= rx are masked fragments ----
#pragma unroll
            for (int ta = 0; ta < 4; ++ta) {
                if (ta < nta) {                                           // wave-uniform
                    const int aq = 16 * ta + li;
                    dot_f64x2 xv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) xv[r] = dot_load2(Xk, aq, 16 * tr + 4 * r + lk, rx2, rx, rx2);
                    mfma_acc_t m = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        m = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[r].x, v0[r], m, 0, 0, 0);
                        m = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[r].y, v1[r], m, 0, 0, 0);
                    }
                    // M'[al = 16 ta + lk + 4 reg, bp, bl = 16 tc + li] += m[reg]   (entries beyond (rx2, ry2) are exact zeros)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg)
                        __hip_atomic_fetch_add(cur + DOT_AT(16 * tc + li, 16 * ta + lk + 4 * reg), m[reg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        if (bp > 0) {                                                     // image bp - 1 is complete: to the state, and zero again
            gmem_wf64* dst = (gmem_wf64*)Mg + EXPECT_IMG_STATE * (bp - 1);
            for (int e = threadIdx.x; e < EXPECT_IMG_STATE; e += TTN_WG) {
                const int at = DOT_AT(e >> 6, e & 63);
                dst[e] = prv[at];
                prv[at] = 0.0;
            }
        }
        dot_lds_barrier();
    }
    {
        lds_f64* lst = img + ((R2 - 1) & 1) * DOT_MS_DOUBLES;
        gmem_wf64* dst = (gmem_wf64*)Mg + EXPECT_IMG_STATE * (R2 - 1);
        for (int e = threadIdx.x; e < EXPECT_IMG_STATE; e += TTN_WG) {
            const int at = DOT_AT(e >> 6, e & 63);
            dst[e] = lst[at];
            lst[at] = 0.0;
        }
    }
    __syncthreads();                                                      // the state is in memory before the next site reads it
}

template <int RM>
__device__ __noinline__ void expect_site_qtt(const double* Xk, const double* Yk, const double* Ak, double* Mg, int rx, int rx2, int R, int R2, int ry, int ry2,
                                             lds_f64* Ac, lds_f64* img) {
    Xk = unip(Xk); Yk = unip(Yk); Ak = unip(Ak); Mg = unip(Mg);
    rx = uni32(rx); rx2 = uni32(rx2); R = uni32(R); R2 = uni32(R2); ry = uni32(ry); ry2 = uni32(ry2);
    expect_site<RM>(Xk, Yk, Ak, Mg, rx, rx2, R, R2, ry, ry2, Ac, img);
}

// One site of the general route, LEFT TO RIGHT: rx, R, ry are the LEFT ranks (incoming state Mc[al + rx (be + R bl)]), rx2, R2, ry2 the
// right ranks (outgoing Mn[a + rx2 (be' + R2 b)]).  U at al + rx (be + R (j + n b)), V at i + n (al + rx (be' + R2 b)).
__device__ __noinline__ void expect_site_generic(double* Xk, double* Yk, double* Ak, double* Mc, double* Mn, double* U, double* V, int n, int rx, int rx2,
                                                 int R, int R2, int ry, int ry2, double* lds) {
    Xk = unip(Xk); Yk = unip(Yk); Ak = unip(Ak); Mc = unip(Mc); Mn = unip(Mn); U = unip(U); V = unip(V); lds = unip(lds);
    n = uni32(n); rx = uni32(rx); rx2 = uni32(rx2); R = uni32(R); R2 = uni32(R2); ry = uni32(ry); ry2 = uni32(ry2);
    const long long rxR = (long long)rx * R;
    // step 1: U[(al, be), (j, b)] = sum_bl M[(al, be), bl] y_k[j, bl, b]
    wg_gemm(rx * R, n * ry2, ry, mkview(Mc, plain(1), plain(rxR)), mkview(Yk, plain(n), Idx{n, 1, (long long)n * ry}), mkview(U, plain(1), plain(rxR)), 1.0, 0.0, lds);
    // step 2: V[(al, b), (i, be')] = sum_{(be, j)} U[(al, b), (be, j)] A_k[i, j, be, be']
    wg_gemm(rx * ry2, n * R2, R * n, mkview(U, Idx{rx, 1, rxR * n}, plain(rx)), mkview(Ak, Idx{R, (long long)n * n, n}, Idx{n, 1, (long long)n * n * R}),
            mkview(V, Idx{rx, n, (long long)n * rx * R2}, Idx{n, 1, (long long)n * rx}), 1.0, 0.0, lds);
    // step 3: M'[a, (be', b)] = sum_{(i, al)} x_k[i, al, a] V[(i, al), (be', b)]
    wg_gemm(rx2, R2 * ry2, n * rx, mkview(Xk, plain((long long)n * rx), plain(1)), mkview(V, plain(1), plain((long long)n * rx)), mkview(Mn, plain(1), plain(rx2)),
            1.0, 0.0, lds);
}

// RM: 0 — general route only; 1 .. EXPECT_QTT_OPR_MAX — every n_k is 2 and the operator ranks are <= RM (both known on the host): a train
// whose ranks are all <= EXPECT_QTT_RMAX takes the QTT route with RM register images of U.
template <int RM>
__global__ void __launch_bounds__(TTN_WG) k_expect(ExpectArgs P) {
    extern __shared__ double lds[];
    const int t = blockIdx.x;
    const int tid = threadIdx.x;
    const TTDev& X = P.x; const TTDev& Y = P.y; const TTODev& A = P.A;
    const int d = X.d;
    double* scr = P.scratch + (long long)t * P.scratch_stride;
    lds_i32* tab = (lds_i32*)((lds_f64*)lds + EXPECT_LDS_DOUBLES);   // [0] rx_k [1] ry_k [2] R_k [3] n_k [4] offx_k [5] offy_k [6] offA_k
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
    if (RM > 0) {
        bool fit = true;
        for (int k = 0; k <= d; ++k) fit = fit && uni32(tab[EXPECT_TAB * k]) <= EXPECT_QTT_RMAX && uni32(tab[EXPECT_TAB * k + 1]) <= EXPECT_QTT_RMAX;
        if (fit) {
            lds_f64* img = (lds_f64*)lds;
            lds_f64* Ac = img + 2 * DOT_MS_DOUBLES;
            const int Rlast = uni32(tab[EXPECT_TAB * d + 2]);
            for (int e = tid; e < 2 * DOT_MS_DOUBLES; e += TTN_WG) img[e] = 0.0;
            for (int e = tid; e < Rlast * EXPECT_IMG_STATE; e += TTN_WG) scr[e] = (e == 0) ? 1.0 : 0.0;     // e_1 e_1^T e_1 at the right end
            __syncthreads();
            for (int k = d - 1; k >= 0; --k) {
                const lds_i32* s = tab + EXPECT_TAB * k;
                expect_site_qtt<(RM > 0 ? RM : 1)>(Xbase + uni32(s[4]), Ybase + uni32(s[5]), Abase + uni32(s[6]), scr, uni32(s[EXPECT_TAB]), uni32(s[0]),
                                                   uni32(s[EXPECT_TAB + 2]), uni32(s[2]), uni32(s[EXPECT_TAB + 1]), uni32(s[1]), Ac, img);
            }
            if (tid == 0) P.out[t] = scr[0];
            return;
        }
    }
    const long long S = (long long)P.rxmax * P.Rmax * P.rymax;
    double* Mc = scr; double* Mn = scr + S;
    double* U = Mn + S; double* V = U + (long long)P.nmax * S;
    if (tid == 0) Mc[0] = 1.0;
    __syncthreads();
    for (int k = 0; k < d; ++k) {
        const lds_i32* s = tab + EXPECT_TAB * k;
        expect_site_generic(Xbase + uni32(s[4]), Ybase + uni32(s[5]), Abase + uni32(s[6]), Mc, Mn, U, V, uni32(s[3]), uni32(s[0]), uni32(s[EXPECT_TAB]),
                            uni32(s[2]), uni32(s[EXPECT_TAB + 2]), uni32(s[1]), uni32(s[EXPECT_TAB + 1]), lds);
        double* tmp = Mc; Mc = Mn; Mn = tmp;
        __syncthreads();
    }
    if (tid == 0) P.out[t] = Mc[0];
}
