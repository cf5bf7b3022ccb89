// ttn_wg_gemm.h — the workgroup matrix products of the one-workgroup-per-train kernels (fp64 MFMA, operands through Views).
//
// Provides (top to bottom):
//   GEMM_BK, GEMM_LD, GEMM_LDS_DOUBLES, GEMM_TAB_ENTRIES, GEMM_KSLAB, GEMM_SMALL_KMAX, GEMM_DESC_DOUBLES, GEMM_LDS_TOTAL
//                                   the LDS budget every caller reserves for a product
//   GemmDesc                        the descriptor in LDS through which the out-of-line bodies take their operands
//   wg_gemm                         C = alpha A B + beta C: tiled (wg_gemm_impl: 2 LDS stages, offset tables) and one-shot small form
//                                   (wg_gemm_small_impl)
//   wg_syrk                         G = alpha A A^T, lower triangle computed, both triangles stored
//   wg_syrk2                        two independent Gram products of <= 64 rows in one call, one per half of the workgroup's waves
//   wg_gemm_ra                      C = alpha A B with A held in registers (short m, k; the 512-thread build)
//   wg_gemm_ra2                     two independent register-A products with m, k <= 64 in one call, one per team of four waves
// Needs: ttn_wg_prims.h (reductions, the uniform pins, the address-space typedefs, TTN_LDS_IMG, TTN_SETPRIO_*).
// Used by: ttn_wg_lq.h, ttn_dense_kernels.h (the bond step), ttn_selftest_kernels.h and every kernel header that only multiplies
// matrices: ttn_dot, ttn_grad, ttn_expect, ttn_expect_grad, ttn_tdvp, ttn_eig.
#pragma once
#include "ttn_wg_prims.h"

#define GEMM_BK 16
// LDS leading dimension (doubles) of the staged chunks, 145 = 17 mod 32.  Two access patterns meet here:
//  * a k-fast operand is staged by 16 lanes that walk k (coalesced global reads) and store to As[kk*LD + r]: an even LD
//    puts all 16 stores on ONE bank pair (16-way conflict: measured 49 % of the MFMA peak with LD = 144, stores alone
//    cost 13 points); with LD odd, 2*kk*LD mod 32 = 2*kk: conflict free;
//  * the MFMA fragment reads take two k-rows per 32-lane half (ds_read_b64, 64 banks): LD*8 mod 256 = 136 puts the second
//    row 2 banks short of the other half: one 2-way conflict per read instead of none.
#define GEMM_LD 145
#define GEMM_LDS_DOUBLES (TTN_LDS_IMG + 512)       // LDS region every GEMM may use (the one-shot small GEMM uses all of it): the
                                                   // image + room for the odd leading dimensions of a 64x64x128 one-shot product

// -------------------------------------------------------------------------------------------------
// wg_gemm: C[m x n] = alpha * A[m x k] * B[k x n] + beta * C, all operands through Views.
// fp64 MFMA (v_mfma_f64_16x16x4_f64): the 16 waves form a 4x4 grid, each wave owns a 32x32 block of a
// 128x128 output tile (2x2 MFMA tiles, 16 accumulator doubles per lane).  K is consumed in chunks of
// 16 staged through LDS (k-major, leading dimension GEMM_LD = 145 doubles: the bank arithmetic stands above, at
// its definition); the next chunk's global loads are issued before the MFMAs of
// the current one.  Fragment maps (one f64 per lane): A[i = lane&15][k = lane>>4],
// B[k = lane>>4][j = lane&15], D[row = (lane>>4) + 4*reg][col = lane&15].
// Every thread of the workgroup must call it (it contains barriers).
// -------------------------------------------------------------------------------------------------

struct GemmDesc {
    int m, n, k, pad;
    View A, B, C;
    double alpha, beta;
    unsigned long long* amax;   // null, or an LDS word that receives max |C_ij| over the stored values (bits of a non-negative double)
};
// Behind the LDS tiles: the descriptor (sizeof(GemmDesc) = 208 bytes, 32 doubles reserved; the two-team forms wg_syrk2 / wg_gemm_ra2 put
// TWO descriptors there, 64 doubles, and start their tables behind them) and the OFFSET TABLES.
// Operands are 2-level strided Views, so an element address costs two integer divisions; a GEMM evaluates ix() once per
// row / column / k index into these tables and the staging loops only add table entries.
// (32-bit entries, two per double of the region: element offsets fit 32 bits, operands are at most 4096 x 16384 doubles)
#if TTN_WG == 512
#define GEMM_TAB_ENTRIES 704                     // doubles: tiled 2 x GEMM_KSLAB + BM + BN ints; one-shot 4 x 128 + 2 x 256 ints
#define GEMM_KSLAB 512
#define GEMM_SMALL_KMAX 256
#else
#define GEMM_TAB_ENTRIES 1536
#define GEMM_KSLAB 768                           // k indices tabulated at a time by the tiled GEMM (A and B tables)
#define GEMM_SMALL_KMAX 512                      // one-shot GEMM: k <= GEMM_LDS_DOUBLES / 34
#endif
#define GEMM_DESC_DOUBLES (32 + GEMM_TAB_ENTRIES)
#define GEMM_LDS_TOTAL (GEMM_LDS_DOUBLES + GEMM_DESC_DOUBLES)

// The body is deliberately NOT inlined (17 call sites) and takes its operands through a descriptor in LDS: only two
// pointers cross the call boundary.
// The descriptor lives in LDS: read it through an LDS-address-space pointer (ds_read, ~100 clk and batched) — through the generic
// pointer the ~25 fields were FLAT loads, 3.5 k clk per GEMM call before the first useful instruction.
typedef __attribute__((address_space(3))) GemmDesc lds_gdesc;
__device__ inline Idx ldsIdx(const __attribute__((address_space(3))) Idx* d) { return Idx{uni32(d->q), uni64(d->lo), uni64(d->hi)}; }
__device__ inline View ldsView(const __attribute__((address_space(3))) View* v) { return View{(double*)uni64((long long)v->p), ldsIdx(&v->r), ldsIdx(&v->c)}; }

// max |C_ij| of the values a GEMM stored, for callers that rescale by it: saves a pass over C (wave max, then one LDS
// atomic per wave; non-negative doubles order like their bit patterns)
__device__ inline void gemm_publish_amax(const lds_gdesc* dsc, double cmax) {
    unsigned long long* am = (unsigned long long*)uni64((long long)dsc->amax);
    if (am) {
        cmax = wave_max(cmax);
        if ((threadIdx.x & 63) == 0) atomicMax(am, (unsigned long long)__double_as_longlong(cmax));
    }
}

// WR = wave rows of the 16-wave grid (WR x 16/WR waves, 32x32 outputs per wave): 4 -> 128x128 output tiles, 2 -> 64x256
// (for m <= 64 and wide n, where half the waves of the square grid would idle).
template <int WR>
__device__ __noinline__ void wg_gemm_impl(const GemmDesc* dsc_, double* lds) {
    const lds_gdesc* dsc = (const lds_gdesc*)dsc_;
    constexpr int WCN = TTN_NWAVES / WR;                 // wave columns
    constexpr int BM = 32 * WR, BN = 32 * WCN;
    constexpr int LDA = (BM <= 64) ? 81 : GEMM_LD, LDB = (BN <= 64) ? 81 : (BN <= 128) ? GEMM_LD : 273;     // all == 17 mod 32 (see GEMM_LD)
    constexpr int STAGE = GEMM_BK * (LDA + LDB);
    static_assert(2 * STAGE <= GEMM_LDS_DOUBLES, "two LDS stages must fit");
    const int m = uni32(dsc->m), n = uni32(dsc->n), k = uni32(dsc->k);
    const View A = ldsView(&dsc->A), B = ldsView(&dsc->B), C = ldsView(&dsc->C);
    const double alpha = unif64(dsc->alpha), beta = unif64(dsc->beta);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WCN, wc = wave % WCN;
    const int li = lane & 15, lk = lane >> 4;
    gmem_f64* Ag = (gmem_f64*)A.p;
    gmem_f64* Bg = (gmem_f64*)B.p;
    // element offsets fit 32 bits (operands are at most 4096 x 16384 doubles): half the registers of 64-bit ones
    lds_i32* tabA = (lds_i32*)(lds + GEMM_LDS_DOUBLES + 32);      // ix(A.c, slab0 + j), j < GEMM_KSLAB
    lds_i32* tabB = tabA + GEMM_KSLAB;                            // ix(B.r, slab0 + j)
    const bool a_kfast = minstride(A.c) < minstride(A.r);
    const bool b_kfast = minstride(B.r) < minstride(B.c);
    // staging assignment: element e = tid + TTN_WG*u of the BM x BK (A) and BK x BN (B) chunk; (row, kk) = (e / BK, e % BK) for a k-fast
    // operand, (e % BM, e / BM) otherwise.  TTN_WG is a multiple of BK, BM and BN, so element u of a thread is its element 0 plus
    // u times a uniform step: the indices are DERIVED where they are used (GEMM_IDX: a shift, a mask and a multiply-add on an opaque
    // copy of the thread index) instead of living in 2 (NUA + NUB) registers across the tile loops — there the compiler kept them,
    // the offsets and the masks made from them on the stack and reloaded them tile after tile.
    constexpr int NUA = BM * GEMM_BK / TTN_WG, NUB = BN * GEMM_BK / TTN_WG;
    static_assert(TTN_WG % BM == 0 && TTN_WG % BN == 0 && TTN_WG % GEMM_BK == 0, "the staging steps are uniform");
    const int ars = a_kfast ? TTN_WG / GEMM_BK : 0, aks = a_kfast ? 0 : TTN_WG / BM;      // row / kk step per element of a thread
    const int bcs = b_kfast ? TTN_WG / GEMM_BK : 0, bks = b_kfast ? 0 : TTN_WG / BN;
    // (shift, mask) pairs of element 0, uniform: the k-fast / row-fast choice costs no branch where the indices are derived
    constexpr int LBK = 4, LBM = BM == 64 ? 6 : 7, LBN = BN == 64 ? 6 : BN == 128 ? 7 : 8;
    static_assert((1 << LBK) == GEMM_BK && (1 << LBM) == BM && (1 << LBN) == BN, "powers of two");
    const int arsh = a_kfast ? LBK : 0, armk = a_kfast ? -1 : BM - 1, aksh = a_kfast ? 0 : LBM, akmk = a_kfast ? GEMM_BK - 1 : -1;
    const int bcsh = b_kfast ? LBK : 0, bcmk = b_kfast ? -1 : BN - 1, bksh = b_kfast ? 0 : LBN, bkmk = b_kfast ? GEMM_BK - 1 : -1;
#define GEMM_IDX                                                                                                \
    int t_ = tid;                                                                                               \
    asm volatile("" : "+v"(t_));                                                                                \
    const int ar0 = (t_ >> arsh) & armk, akk0 = (t_ >> aksh) & akmk;                                            \
    const int bc0 = (t_ >> bcsh) & bcmk, bkk0 = (t_ >> bksh) & bkmk;
#define AR(u) (ar0 + ars * (u))
#define AKK(u) (akk0 + aks * (u))
#define BC(u) (bc0 + bcs * (u))
#define BKK(u) (bkk0 + bks * (u))
    double cmax = 0.0;
    const int nch = (k + GEMM_BK - 1) / GEMM_BK;
    int slab0 = -1;                                               // first k index the tables currently hold
    for (int m0 = 0; m0 < m; m0 += BM) {
        for (int n0 = 0; n0 < n; n0 += BN) {
            int aoff[NUA], boff[NUB];
            {
                GEMM_IDX
#pragma unroll
                for (int u = 0; u < NUA; ++u) aoff[u] = (m0 + AR(u)) < m ? (int)ix(A.r, m0 + AR(u)) : 0;
#pragma unroll
                for (int u = 0; u < NUB; ++u) boff[u] = (n0 + BC(u)) < n ? (int)ix(B.c, n0 + BC(u)) : 0;
            }
            const bool live = (m0 + wr * 32 < m) && (n0 + wc * 32 < n);      // wave-uniform
            mfma_acc_t acc[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
            double av[NUA], bv[NUB];
            // Software pipeline over the K chunks, two LDS stages, ONE barrier per chunk:
            //   iteration c:  MFMAs of chunk c (stage c&1) | registers (chunk c+1) -> stage (c+1)&1 | global loads of chunk c+2
#define GEMM_FILL_TAB(K0)                                                                                       \
            {                                                                                                   \
                __syncthreads();                                                                                \
                slab0 = (K0);                                                                                   \
                for (int j = tid; j < GEMM_KSLAB; j += TTN_WG) {                                                \
                    const int kk = slab0 + j;                                                                   \
                    tabA[j] = (kk < k) ? (int)ix(A.c, kk) : 0;                                                     \
                    tabB[j] = (kk < k) ? (int)ix(B.r, kk) : 0;                                                     \
                }                                                                                               \
                __syncthreads();                                                                                \
            }
#define GEMM_LOAD(K0)  /* branch-free: out-of-range elements read element 0 of the operand and are then zeroed */        \
            {                                                                                                   \
                GEMM_IDX                                                                                        \
                int oa_[NUA], ob_[NUB];                                                                         \
                bool va_[NUA], vb_[NUB];                                                                        \
                _Pragma("unroll") for (int u = 0; u < NUA; ++u) {                                               \
                    const int ga = (K0) + AKK(u);                                                               \
                    va_[u] = (m0 + AR(u)) < m && ga < k;                                                        \
                    oa_[u] = va_[u] ? aoff[u] + tabA[ga - slab0] : 0;                                           \
                }                                                                                               \
                _Pragma("unroll") for (int u = 0; u < NUB; ++u) {                                               \
                    const int gb = (K0) + BKK(u);                                                               \
                    vb_[u] = (n0 + BC(u)) < n && gb < k;                                                        \
                    ob_[u] = vb_[u] ? boff[u] + tabB[gb - slab0] : 0;                                           \
                }                                                                                               \
                _Pragma("unroll") for (int u = 0; u < NUA; ++u) av[u] = Ag[oa_[u]];                             \
                _Pragma("unroll") for (int u = 0; u < NUB; ++u) bv[u] = Bg[ob_[u]];                             \
                _Pragma("unroll") for (int u = 0; u < NUA; ++u) av[u] = va_[u] ? av[u] : 0.0;                   \
                _Pragma("unroll") for (int u = 0; u < NUB; ++u) bv[u] = vb_[u] ? bv[u] : 0.0;                   \
            }
#define GEMM_STORE(STG)                                                                                         \
            {                                                                                                   \
                GEMM_IDX                                                                                        \
                lds_f64* As_ = (lds_f64*)lds + (STG) * STAGE;                                                    \
                lds_f64* Bs_ = As_ + GEMM_BK * LDA;                                                             \
                _Pragma("unroll") for (int u = 0; u < NUA; ++u) As_[AKK(u) * LDA + AR(u)] = av[u];              \
                _Pragma("unroll") for (int u = 0; u < NUB; ++u) Bs_[BKK(u) * LDB + BC(u)] = bv[u];              \
            }
            if (slab0 != 0) GEMM_FILL_TAB(0)
            else __syncthreads();                      // the previous tile's MFMAs have consumed both stages
            {   // prologue: the loads of chunk 0 AND chunk 1 are in flight together (one exposed global latency, not two)
                GEMM_LOAD(0)
                double av0[NUA], bv0[NUB];
                _Pragma("unroll") for (int u = 0; u < NUA; ++u) av0[u] = av[u];
                _Pragma("unroll") for (int u = 0; u < NUB; ++u) bv0[u] = bv[u];
                if (nch > 1) GEMM_LOAD(GEMM_BK)
                GEMM_IDX
                lds_f64* As0 = (lds_f64*)lds;
                lds_f64* Bs0 = As0 + GEMM_BK * LDA;
                _Pragma("unroll") for (int u = 0; u < NUA; ++u) As0[AKK(u) * LDA + AR(u)] = av0[u];
                _Pragma("unroll") for (int u = 0; u < NUB; ++u) Bs0[BKK(u) * LDB + BC(u)] = bv0[u];
            }
            __syncthreads();
            for (int c = 0; c < nch; ++c) {
                // The staging work of the other chunks is placed BETWEEN this wave's MFMA groups: an MFMA occupies the
                // matrix pipe for 64 clk, so the VALU/LDS/global instructions issued behind it run under the MFMAs of
                // the SIMD's other waves instead of after them (the waves run in lockstep from barrier to barrier).
                lds_f64* As = (lds_f64*)lds + (c & 1) * STAGE;
                lds_f64* Bs = As + GEMM_BK * LDA;
#define GEMM_MFMA_STEP(T)                                                                                       \
                if (live) {                                                                                     \
                    const int kra = (4 * (T) + lk) * LDA, krb = (4 * (T) + lk) * LDB;                                                 \
                    const double a0 = As[kra + wr * 32 + li], a1 = As[kra + wr * 32 + 16 + li];                 \
                    const double b0 = Bs[krb + wc * 32 + li], b1 = Bs[krb + wc * 32 + 16 + li];                 \
                    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);               \
                    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);               \
                    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);               \
                    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);               \
                }
                GEMM_MFMA_STEP(0)
                if (c + 1 < nch) GEMM_STORE((c + 1) & 1)
                GEMM_MFMA_STEP(1)
                if (c + 2 < nch) {
                    const int k2 = (c + 2) * GEMM_BK;
                    if (k2 >= slab0 + GEMM_KSLAB) GEMM_FILL_TAB(k2)       // workgroup-uniform; rare (k > GEMM_KSLAB)
                    GEMM_LOAD(k2)
                }
                GEMM_MFMA_STEP(2)
                GEMM_MFMA_STEP(3)
#undef GEMM_MFMA_STEP
                __syncthreads();
            }
#undef GEMM_FILL_TAB
#undef GEMM_LOAD
#undef GEMM_STORE
            // C offsets of this tile through tables too (ten ix() per thread otherwise: two integer divisions each)
            lds_i32* rowC = tabB + GEMM_KSLAB;                            // BM entries
            lds_i32* colC = rowC + BM;                                    // BN entries
            for (int i = tid; i < BM + BN; i += TTN_WG) {
                if (i < BM) rowC[i] = (m0 + i < m) ? (int)ix(C.r, m0 + i) : 0;
                else colC[i - BM] = (n0 + i - BM < n) ? (int)ix(C.c, n0 + i - BM) : 0;
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int li_ = wr * 32 + ti * 16 + lk + 4 * reg;
                        if (m0 + li_ >= m) continue;
                        const int ro = rowC[li_];
#pragma unroll
                        for (int tj = 0; tj < 2; ++tj) {
                            const int lj_ = wc * 32 + tj * 16 + li;
                            if (n0 + lj_ >= n) continue;
                            gmem_wf64* cp = (gmem_wf64*)C.p + ((long long)ro + colC[lj_]);      // C is always global memory: global_store, not flat
                            double v = alpha * acc[ti][tj][reg];
                            if (beta != 0.0) v += beta * (*cp);
                            *cp = v;
                            cmax = fmax(cmax, fabs(v));
                        }
                    }
            }
        }
    }
#undef GEMM_IDX
#undef AR
#undef AKK
#undef BC
#undef BKK
    gemm_publish_amax(dsc, cmax);
    __syncthreads();
}

// -------------------------------------------------------------------------------------------------
// One-shot small GEMM: m, n <= 128, m*n <= 8192 (at most 2 MFMA tiles per wave) and the WHOLE K extent of both
// operands fits the LDS region: k*(lda+ldb) <= GEMM_LDS_DOUBLES.  All global loads are issued at once (these GEMMs
// are latency bound: a 64x64x128 product is 1 Mflop), one barrier, k/4 MFMAs per tile, store.  Small register
// footprint on purpose (8 accumulator doubles per tile): the factored route issues ten of these per bond step.
// -------------------------------------------------------------------------------------------------
__device__ inline int small_ld(int x) { const int t = (x + 15) & ~15; return (((t & 31) == 16) ? t : t + 16) + 1; }   // == 17 mod 32 (see GEMM_LD)
__device__ inline int tight_ld(int x) { return ((x + 15) & ~15) + 1; }                                             // odd: conflict-free k-fast stores

__device__ __noinline__ void wg_gemm_small_impl(const GemmDesc* dsc_, double* lds) {
    const lds_gdesc* dsc = (const lds_gdesc*)dsc_;
    const int m = uni32(dsc->m), n = uni32(dsc->n), k = uni32(dsc->k);
    const View A = ldsView(&dsc->A), B = ldsView(&dsc->B), C = ldsView(&dsc->C);
    const double alpha = unif64(dsc->alpha), beta = unif64(dsc->beta);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    // dsc->pad = 1: leading dimensions == 17 mod 32 (fragment reads nearly conflict free); 0: tight (2-way read conflicts, fits more)
    const int lda = uni32(dsc->pad) ? small_ld(m) : tight_ld(m), ldb = uni32(dsc->pad) ? small_ld(n) : tight_ld(n);
    lds_f64* As = (lds_f64*)lds;                       // As[kk*lda + row]
    lds_f64* Bs = As + k * lda;                        // Bs[kk*ldb + col]
    const bool a_kfast = minstride(A.c) < minstride(A.r);
    const bool b_kfast = minstride(B.r) < minstride(B.c);
    const int mp = (m + 15) & ~15, np = (n + 15) & ~15;
    // ---- offset tables (m, n <= 128; k <= 512 because k*(lda+ldb) <= GEMM_LDS_DOUBLES and lda, ldb >= 16) ----
    gmem_f64* Ag = (gmem_f64*)A.p;
    gmem_f64* Bg = (gmem_f64*)B.p;
    lds_i32* rowA = (lds_i32*)(lds + GEMM_LDS_DOUBLES + 32);
    lds_i32* colB = rowA + 128;
    lds_i32* rowC = colB + 128;
    lds_i32* colC = rowC + 128;
    lds_i32* kA = colC + 128;
    lds_i32* kB = kA + GEMM_SMALL_KMAX;
    for (int i = tid; i < 128; i += TTN_WG) {
        rowA[i] = (i < m) ? (int)ix(A.r, i) : 0;
        rowC[i] = (i < m) ? (int)ix(C.r, i) : 0;
        colB[i] = (i < n) ? (int)ix(B.c, i) : 0;
        colC[i] = (i < n) ? (int)ix(C.c, i) : 0;
    }
    for (int i = tid; i < k; i += TTN_WG) { kA[i] = (int)ix(A.c, i); kB[i] = (int)ix(B.r, i); }
    __syncthreads();
    // ---- stage all of A (m x k) and B (k x n), zero padding rows/cols up to the tile edge; 16 lanes walk the
    //      operand's fast (small-stride) index, the 64 lane groups its slow index: no divisions in the loops ----
    const int fx = tid & 15, sy = tid >> 4;
    // The loads of a thread are issued in batches of GS_U before the first of them is awaited (written naively — load, wait, store
    // per element — every element of a thread paid its own global-memory round trip: 16 of them in a row for a 64 x 64 x 128
    // product, most of the time of these latency-bound GEMMs).  Out-of-range elements read element 0 and are zeroed.
#define GS_U 8
#define GEMM_SMALL_STAGE(DST, LDD, SRC, SLOWTAB, FASTTAB, NSLOW, NSLOW_VALID, NFAST, NFAST_VALID, SLOW_IS_K)                      \
    for (int s_ = sy; s_ < (NSLOW); s_ += TTN_WG / 16) {                                                                        \
        const int so_ = (s_ < (NSLOW_VALID)) ? SLOWTAB[s_] : 0;                                                                 \
        for (int f0_ = fx; f0_ < (NFAST); f0_ += 16 * GS_U) {                                                                   \
            double v_[GS_U];                                                                                                    \
            _Pragma("unroll") for (int u_ = 0; u_ < GS_U; ++u_) {                                                               \
                const int f_ = f0_ + 16 * u_;                                                                                   \
                const bool ok_ = (s_ < (NSLOW_VALID)) && (f_ < (NFAST_VALID));                                                  \
                v_[u_] = SRC[ok_ ? so_ + FASTTAB[f_] : 0];                                                                      \
            }                                                                                                                   \
            _Pragma("unroll") for (int u_ = 0; u_ < GS_U; ++u_) {                                                               \
                const int f_ = f0_ + 16 * u_;                                                                                   \
                const bool ok_ = (s_ < (NSLOW_VALID)) && (f_ < (NFAST_VALID));                                                  \
                if (f_ < (NFAST)) DST[(SLOW_IS_K) ? s_ * (LDD) + f_ : f_ * (LDD) + s_] = ok_ ? v_[u_] : 0.0;                    \
            }                                                                                                                   \
        }                                                                                                                       \
    }
    if (a_kfast) { GEMM_SMALL_STAGE(As, lda, Ag, rowA, kA, mp, m, k, k, 0) }          // slow = row, fast = k
    else { GEMM_SMALL_STAGE(As, lda, Ag, kA, rowA, k, k, mp, m, 1) }                  // slow = k, fast = row
    if (b_kfast) { GEMM_SMALL_STAGE(Bs, ldb, Bg, colB, kB, np, n, k, k, 0) }          // slow = column, fast = k
    else { GEMM_SMALL_STAGE(Bs, ldb, Bg, kB, colB, k, k, np, n, 1) }                  // slow = k, fast = column
#undef GEMM_SMALL_STAGE
#undef GS_U
    __syncthreads();
    const int tm = mp >> 4, tn = np >> 4, ntile = tm * tn;
    const int k4 = k >> 2, krem = k & 3;
    double cmax = 0.0;
    for (int tile = wave; tile < ntile; tile += (TTN_WG >> 6)) {
        const int r0 = (tile % tm) << 4, c0 = (tile / tm) << 4;
        mfma_acc_t acc = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
        const lds_f64* ap = As + lk * lda + r0 + li;
        const lds_f64* bp = Bs + lk * ldb + c0 + li;
        int t = 0;
        for (; t + 4 <= k4; t += 4) {                   // four k-steps per trip: the eight LDS reads go out before the MFMAs
            double a_[4], b_[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { a_[q] = ap[(4 * (t + q)) * lda]; b_[q] = bp[(4 * (t + q)) * ldb]; }
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a_[q], b_[q], acc, 0, 0, 0);
        }
        for (; t < k4; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[(4 * t) * lda], bp[(4 * t) * ldb], acc, 0, 0, 0);
        if (krem) {                                     // k not a multiple of 4: pad the last step with zeros
            const double a = (lk < krem) ? ap[(4 * k4) * lda] : 0.0;
            const double b = (lk < krem) ? bp[(4 * k4) * ldb] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int gi = r0 + lk + 4 * reg, gj = c0 + li;
            if (gi < m && gj < n) {
                gmem_wf64* cp = (gmem_wf64*)C.p + ((long long)rowC[gi] + colC[gj]);
                double v = alpha * acc[reg];
                if (beta != 0.0) v += beta * (*cp);
                *cp = v;
                cmax = fmax(cmax, fabs(v));
            }
        }
    }
    gemm_publish_amax(dsc, cmax);
    __syncthreads();
}

__device__ inline void wg_gemm(int m, int n, int k, View A, View B, View C, double alpha, double beta, double* lds,
                               double* amax_lds = nullptr /* LDS word: receives max |C_ij| */) {
    GemmDesc* dsc = reinterpret_cast<GemmDesc*>(lds + GEMM_LDS_DOUBLES);
    __syncthreads();                         // nobody still reads what the tiles / descriptor alias
    if (threadIdx.x == 0) {
        dsc->m = m; dsc->n = n; dsc->k = k; dsc->pad = 0;
        dsc->A = A; dsc->B = B; dsc->C = C;
        dsc->alpha = alpha; dsc->beta = beta;
        dsc->amax = (unsigned long long*)amax_lds;
        if (amax_lds) *amax_lds = 0.0;
    }
    __syncthreads();
    TTN_SETPRIO_GEMM();
    const bool shape_ok = (m <= 128) && (n <= 128) && (((m + 15) >> 4) * ((n + 15) >> 4) <= 32);
    const int wpad = small_ld(m) + small_ld(n), wtight = tight_ld(m) + tight_ld(n);
    if (shape_ok && (long long)k * wpad <= GEMM_LDS_DOUBLES) {
        if (threadIdx.x == 0) dsc->pad = 1;
        __syncthreads();
        wg_gemm_small_impl(dsc, lds);
    } else if (shape_ok && (long long)k * wtight <= GEMM_LDS_DOUBLES) {
        wg_gemm_small_impl(dsc, lds);                    // pad = 0: tight leading dimensions
    } else if (shape_ok && A.c.q == 0 && B.r.q == 0 && k <= 8 * (GEMM_LDS_DOUBLES / wtight)) {
        // few output tiles but a long K: the tiled GEMM would keep most waves idle; run the one-shot kernel over
        // K chunks, accumulating into C.  Plain-stride k indices only: a chunk is addressed by shifting the operands' base pointers,
        // which a two-level k index (the stacked H of the matrix-free two-site operator) does not allow — that takes the tiled form
        const int kcmax = (GEMM_LDS_DOUBLES / wtight) & ~3;
        const int nck = (k + kcmax - 1) / kcmax;
        const int kc = (((k + nck - 1) / nck) + 3) & ~3;                  // balanced chunks, multiples of 4
        for (int k0 = 0; k0 < k; k0 += kc) {
            if (k0 > 0) __syncthreads();
            if (threadIdx.x == 0) {
                dsc->k = (k - k0 < kc) ? k - k0 : kc;
                dsc->A.p = A.p + ix(A.c, k0);
                dsc->B.p = B.p + ix(B.r, k0);
                dsc->beta = (k0 == 0) ? beta : 1.0;
                dsc->amax = (k0 + kc >= k) ? (unsigned long long*)amax_lds : nullptr;     // the last chunk stores the final values
            }
            __syncthreads();
            wg_gemm_small_impl(dsc, lds);
        }
    } else if (m <= 64 && n > 128) {
        wg_gemm_impl<2>(dsc, lds);                       // 64 x 256 output tiles: all 16 waves busy on a short, wide product
    } else {
        wg_gemm_impl<4>(dsc, lds);
    }
    TTN_SETPRIO_BASE();
}

// -------------------------------------------------------------------------------------------------
// wg_syrk: G = alpha * A A^T, A (p x q, p <= 128) and G (p x p, both triangles written) through Views in global memory.
// The Gram products of a bond step (M M^T, the a-posteriori checks Rf Rf^T / Lf^T Lf, route F's A'^T A' and B' B'^T) are
// 64..128 rows x a long K: as general GEMMs they ran the tiled form at 25 % of the matrix pipe (128 x 128 x 384: both operands staged
// although they are the same matrix, a barrier per 16 k) or the chunked one-shot form (64 x 64 x 384: seven K chunks, each read-modify-
// writing C in memory).  Here A is staged ONCE per K chunk (k-major, leading dimension == 17 mod 32 like the GEMM's) and serves both
// fragment operands — frag(tb) = A[16 tb + lane&15][k + lane>>4] is the A fragment of tile row tb and the B fragment of tile column
// tb alike —, only the tiles on and below the diagonal are computed (36 of 64 for p = 128) with the accumulators in registers over all
// of K, and the global loads of chunk c + 1 are in flight (registers) while chunk c is multiplied.
//   KC16 x 16 = k per chunk, JMAX = rows per thread of a chunk, MAXT = tiles per wave (all sized per build by the wrapper below).
// -------------------------------------------------------------------------------------------------
#define SYRK_QMAX (2 * GEMM_TAB_ENTRIES - 128)           // k offsets tabulated once (32-bit entries behind the descriptor)
// The k-steps of one staged chunk for a wave that owns NT tiles (NT is wave-uniform: wg_syrk_impl dispatches on it once per call, so
// no test of "does tile u exist" stands between a fragment read and its MFMA).  The fragments live in a RING of D k-steps x NT tiles
// register pairs: an MFMA reads its operands when it issues, so the pair of (step s + D, tile u) is read into the registers of
// (step s, tile u) right behind that tile's MFMA and has the D NT - 1 MFMAs in between (64 clk each) to arrive.  All reads are
// unconditional, so the waits in front of the MFMAs are counted ones.  (With one register pair per operand, reused by every tile,
// each MFMA sat behind its own two reads and a full lgkmcnt(0) drain.)  D NT fragment pairs, not two whole sets: the 128-row form
// has 40 accumulator and 24 staging registers next to them, and k_compress's own allocation depends on what its callees clobber.
//  * LD is a compile-time constant and rp ONE running address: a fragment's address is rp + its uniform tile offset (ta / tb = 16 tr,
//    16 tc) + an immediate.
//  * ksteps is rounded up to a multiple of D (D divides the steps of a chunk, KS).  The rows of a chunk behind the operand's last k
//    are staged as +0.0, so a step past the end adds +0.0 to accumulators that started at +0.0 and therefore never hold -0.0: the same
//    bits as skipping it.  For every accumulator the order of its MFMAs is that of the plain loop: results are unchanged bit for bit.
template <int NT, int LD, int KS>
__device__ __forceinline__ void syrk_ksteps(mfma_acc_t* acc, const lds_f64* rp, int ksteps, const int* ta, const int* tb) {
    constexpr int D = NT >= 4 ? 1 : NT == 3 ? 2 : NT == 2 ? 3 : 6;
    static_assert(KS % D == 0, "a rounded-up step count stays inside the chunk");
    double a[D][NT], b[D][NT];
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
        for (int u = 0; u < NT; ++u) { a[j][u] = rp[4 * j * LD + ta[u]]; b[j][u] = rp[4 * j * LD + tb[u]]; }
    __builtin_amdgcn_sched_barrier(0);
    const int rounds = (ksteps + D - 1) / D;
    for (int r = 1; r < rounds; ++r) {
        rp += 4 * D * LD;
        asm volatile("" : "+v"(rp));         // ONE running LDS address, not one induction variable per fragment
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j][u], b[j][u], acc[u], 0, 0, 0);
                a[j][u] = rp[4 * j * LD + ta[u]]; b[j][u] = rp[4 * j * LD + tb[u]];
                __builtin_amdgcn_sched_barrier(0);       // keep each refill right behind its MFMA
            }
    }
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j][u], b[j][u], acc[u], 0, 0, 0);
}
template <int N> struct syrk_nt { static constexpr int value = N; };
// TEAMS = 1: the whole workgroup computes the product of descriptor 0.  TEAMS = 2 (wg_syrk2): the workgroup splits into two teams of
// TTN_NWAVES / 2 waves, team t computes the product of descriptor t (p <= 64) in its own half of the LDS region and of the tables, and
// both teams meet at the SAME workgroup barriers: the chunk loop runs the chunk count of the longer product, the team that is done
// stages zeros and skips its MFMAs.  "tid", "wave" and the thread / wave counts below are those of the TEAM.
#define SYRK2_TAB (GEMM_TAB_ENTRIES - 32)                // 32-bit table entries of one team: 64 row + SYRK2_QMAX k offsets
#define SYRK2_QMAX (SYRK2_TAB - 64)
template <int KC16, int JMAX, int MAXT, int TEAMS>
__device__ __forceinline__ void syrk_body(const GemmDesc* dsc_, double* lds) {
    constexpr int TWG = TTN_WG / TEAMS, TNW = TTN_NWAVES / TEAMS, NROW = 128 / TEAMS;      // threads, waves, tabulated rows of a team
    const int team = (TEAMS == 1) ? 0 : uni32((int)threadIdx.x / TWG);
    const lds_gdesc* dsc = (const lds_gdesc*)dsc_ + team;
    constexpr int KC = 16 * KC16, RG = TWG / 16;                    // k per chunk; row groups (16 lanes walk k)
    const int p = uni32(dsc->m), q = uni32(dsc->k);
    int qall = q;                                                   // the k extent the chunk loop (and its barriers) covers
    if constexpr (TEAMS == 2) { const int qo = uni32(((const lds_gdesc*)dsc_ + (1 - team))->k); qall = q > qo ? q : qo; }
    const View A = ldsView(&dsc->A), C = ldsView(&dsc->C);
    const double alpha = unif64(dsc->alpha);
    const int tid = threadIdx.x - team * TWG, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    constexpr int LD = (JMAX * RG > 64) ? GEMM_LD : 81;             // == 17 mod 32 (see GEMM_LD); a constant: syrk_ksteps
    static_assert(LD >= JMAX * RG + 16 && TEAMS * KC * LD <= GEMM_LDS_DOUBLES, "a chunk fits the region");
    static_assert(TEAMS == 1 || (TEAMS == 2 && JMAX * RG == NROW), "two teams: 64 rows each");
    const int pp = (p + 15) & ~15;
    lds_f64* Cs = (lds_f64*)lds + team * (KC * LD);                 // Cs[kk * LD + row]
    // (two descriptors take 52 doubles: the tables of the two-team form start 64 doubles behind the region, not 32)
    lds_i32* rowT = (lds_i32*)(lds + GEMM_LDS_DOUBLES + 32 * TEAMS) + team * SYRK2_TAB;      // NROW entries
    lds_i32* colT = rowT + NROW;                                    // q entries
    gmem_f64* Ag = (gmem_f64*)A.p;
    for (int i = tid; i < NROW; i += TWG) rowT[i] = (i < p) ? (int)ix(A.r, i) : 0;
    for (int i = tid; i < q; i += TWG) colT[i] = (int)ix(A.c, i);
    // tiles of this wave: t = wave, wave + NWAVES, ... over the lower triangle, t = tr (tr + 1) / 2 + tc
    const int nt = pp >> 4, ntile = nt * (nt + 1) / 2;
    int t_r[MAXT], t_c[MAXT], ta[MAXT], tb[MAXT], nlive = 0;        // the live tiles of a wave are u < nlive
#pragma unroll
    for (int u = 0; u < MAXT; ++u) {
        const int t = wave + u * TNW;
        int tr = 0, base = 0;
        while (base + tr + 1 <= t) { base += tr + 1; ++tr; }
        t_r[u] = uni32(tr); t_c[u] = uni32(t - base);
        ta[u] = uni32(16 * tr); tb[u] = uni32(16 * (t - base));
        nlive += (t < ntile) ? 1 : 0;
    }
    nlive = uni32(nlive);
    const int fx = tid & 15, sy = tid >> 4;
    gmem_wf64* Cg = (gmem_wf64*)C.p;
    __syncthreads();
    // Everything from here on is compiled once per number of live tiles NT and the wave picks its copy ONCE (all copies run the same
    // barriers): a wave with fewer tiles than MAXT then has neither the accumulators of the absent ones nor a test per tile and
    // k-step in its loops.
    mfma_acc_t res[MAXT];                                           // the finished tiles: ONE copy of the store loop below
#pragma unroll
    for (int u = 0; u < MAXT; ++u) res[u] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
    auto body = [&](auto ntc) {
        constexpr int NT = decltype(ntc)::value, NA = NT ? NT : 1;
        mfma_acc_t acc[NA];
#pragma unroll
        for (int u = 0; u < NA; ++u) acc[u] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
        double v[JMAX][KC16];
        // The prefetch of a chunk: the row offsets of a thread do not change from chunk to chunk (registers, read once), the k
        // offsets are ONE batch of table reads per chunk, and the loads are unconditional — an out-of-range position reads element 0
        // of the operand (the LDS store below writes its zero).  (Each load once sat behind its own table read and drain, under a
        // branch.)
        int ro[JMAX];
#pragma unroll
        for (int j = 0; j < JMAX; ++j) ro[j] = rowT[sy + RG * j];   // sy + RG j < 128; entries of rows >= p are 0
#define SYRK_LOAD(K0)                                                                                                   \
        {                                                                                                               \
            int co_[KC16];                                                                                              \
            _Pragma("unroll") for (int u = 0; u < KC16; ++u) {                                                           \
                const int kk = (K0) + fx + 16 * u;                                                                      \
                co_[u] = colT[kk < q ? kk : 0];                                                                         \
            }                                                                                                           \
            _Pragma("unroll") for (int j = 0; j < JMAX; ++j) {                                                           \
                const int row = sy + RG * j;                                                                            \
                _Pragma("unroll") for (int u = 0; u < KC16; ++u) {                                                       \
                    const int kk = (K0) + fx + 16 * u;                                                                  \
                    v[j][u] = Ag[(row < p && kk < q) ? ro[j] + co_[u] : 0];                                             \
                }                                                                                                       \
            }                                                                                                           \
        }
        SYRK_LOAD(0)
        for (int k0 = 0; k0 < qall; k0 += KC) {
#pragma unroll
            for (int j = 0; j < JMAX; ++j) {
                const int row = sy + RG * j;
#pragma unroll
                for (int u = 0; u < KC16; ++u) {
                    const int kl = fx + 16 * u;
                    if (row < pp) Cs[kl * LD + row] = (row < p && k0 + kl < q) ? v[j][u] : 0.0;
                }
            }
            __syncthreads();
            if (k0 + KC < q) { SYRK_LOAD(k0 + KC) }
            const int ksteps = (q - k0 < KC) ? (q - k0 + 3) >> 2 : KC / 4;
            if constexpr (NT > 0) {
                if (TEAMS == 1 || ksteps > 0) syrk_ksteps<NT, LD, KC / 4>(acc, Cs + lk * LD + li, ksteps, ta, tb);      // (wave-uniform)
            }
            __syncthreads();
        }
#undef SYRK_LOAD
#pragma unroll
        for (int u = 0; u < NT; ++u) res[u] = acc[u];
    };
    if (nlive == MAXT) body(syrk_nt<MAXT>{});
    else if (MAXT > 1 && nlive == MAXT - 1) body(syrk_nt<(MAXT > 1 ? MAXT - 1 : 0)>{});
    else if (MAXT > 2 && nlive == MAXT - 2) body(syrk_nt<(MAXT > 2 ? MAXT - 2 : 0)>{});
    else if (MAXT > 3 && nlive == MAXT - 3) body(syrk_nt<(MAXT > 3 ? MAXT - 3 : 0)>{});
    else if (MAXT > 4 && nlive == MAXT - 4) body(syrk_nt<(MAXT > 4 ? MAXT - 4 : 0)>{});
    else body(syrk_nt<0>{});
    static_assert(MAXT <= 5, "one copy of the body per number of live tiles");
#pragma unroll
    for (int u = 0; u < MAXT; ++u) {
        if (u >= nlive) continue;                                   // wave-uniform
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int gi = 16 * t_r[u] + lk + 4 * reg, gj = 16 * t_c[u] + li;
            if (gi < p && gj < p) {
                const double val = alpha * res[u][reg];
                Cg[ix(C.r, gi) + ix(C.c, gj)] = val;
                if (t_r[u] != t_c[u]) Cg[ix(C.r, gj) + ix(C.c, gi)] = val;
            }
        }
    }
    __syncthreads();
}
template <int KC16, int JMAX, int MAXT>
__device__ __noinline__ void wg_syrk_impl(const GemmDesc* dsc_, double* lds) { syrk_body<KC16, JMAX, MAXT, 1>(dsc_, lds); }
// the two-team form: descriptors dsc_[0] and dsc_[1], both products <= 64 rows (10 lower-triangle tiles on TTN_NWAVES / 2 waves)
__device__ __noinline__ void wg_syrk2_impl(const GemmDesc* dsc_, double* lds) {
#if TTN_WG == 512
    syrk_body<3, 4, 3, 2>(dsc_, lds);                    // 4 waves: chunks of 48 k (81 x 48 doubles per team), up to 3 tiles per wave
#else
    syrk_body<3, 2, 2, 2>(dsc_, lds);                    // 8 waves: up to 2 tiles per wave
#endif
}

__device__ inline void wg_syrk(int p, int q, View A, View G, double alpha, double* lds) {
    if (p > 128 || q > SYRK_QMAX) { wg_gemm(p, p, q, A, tview(A), G, alpha, 0.0, lds); return; }
    GemmDesc* dsc = reinterpret_cast<GemmDesc*>(lds + GEMM_LDS_DOUBLES);
    __syncthreads();                         // nobody still reads what the tiles / descriptor alias
    if (threadIdx.x == 0) { dsc->m = p; dsc->n = p; dsc->k = q; dsc->pad = 0; dsc->A = A; dsc->C = G; dsc->alpha = alpha; dsc->beta = 0.0; dsc->amax = nullptr; }
    __syncthreads();
    TTN_SETPRIO_GEMM();
#if TTN_WG == 512
    if (p > 64) wg_syrk_impl<3, 4, 5>(dsc, lds);         // 128 rows: chunks of 48 k (145 x 48 doubles), 36 tiles on 8 waves
    else wg_syrk_impl<6, 2, 2>(dsc, lds);                // <= 64 rows: chunks of 96 k (81 x 96), 10 tiles
#else
    if (p > 64) wg_syrk_impl<6, 2, 3>(dsc, lds);         // 145 x 96 doubles, 36 tiles on 16 waves
    else wg_syrk_impl<6, 1, 1>(dsc, lds);
#endif
    TTN_SETPRIO_BASE();
}

// wg_syrk2: G1 = alpha1 A1 A1^T and G2 = alpha2 A2 A2^T, two INDEPENDENT Gram products of at most 64 rows in one call.  Such a product
// is a few microseconds of MFMAs behind its table setup, one global round trip per chunk, two barriers per chunk and the store: run
// back to back, two of them pay that latency twice; here each runs on half of the workgroup's waves and both wait together.  Every
// accumulator sees the MFMAs of its k-steps in ascending order with the operands wg_syrk gives it (the chunks are 48 k instead of 96,
// the accumulators carry over), so the results are those of two wg_syrk calls bit for bit.  Other shapes take the two calls.
// alt2 != 0: the second product's operand is A2alt instead of A2 (the bond step's B' handed over in its staging area); ovr2: it is
// the view THREAD 0 left at that LDS address (Rf, wherever the step put it).  Thread 0 stores either over the descriptor it has just
// written: as a view chosen by the caller (a select on every field of A2) the same choice costs k_compress 64 more spilled VGPRs
// (DESIGN.md section 4.2, r03n).
__device__ inline void wg_syrk2(int p1, int q1, View A1, View G1, double alpha1, int p2, int q2, View A2, View G2, double alpha2, double* lds,
                                int alt2 = 0, View A2alt = View{}, const View* ovr2 = nullptr) {
    if (p1 > 64 || p2 > 64 || q1 > SYRK2_QMAX || q2 > SYRK2_QMAX) {
        if (alt2) A2 = A2alt;
        if (ovr2) { __syncthreads(); A2 = uniView(*ovr2); }
        wg_syrk(p1, q1, A1, G1, alpha1, lds);
        wg_syrk(p2, q2, A2, G2, alpha2, lds);
        return;
    }
    GemmDesc* dsc = reinterpret_cast<GemmDesc*>(lds + GEMM_LDS_DOUBLES);
    static_assert(2 * sizeof(GemmDesc) <= 64 * sizeof(double), "two descriptors in front of the two-team tables");
    __syncthreads();                         // nobody still reads what the tiles / descriptors alias
    if (threadIdx.x == 0) {
        dsc[0].m = p1; dsc[0].n = p1; dsc[0].k = q1; dsc[0].pad = 0; dsc[0].A = A1; dsc[0].C = G1; dsc[0].alpha = alpha1; dsc[0].beta = 0.0; dsc[0].amax = nullptr;
        dsc[1].m = p2; dsc[1].n = p2; dsc[1].k = q2; dsc[1].pad = 0; dsc[1].A = A2; dsc[1].C = G2; dsc[1].alpha = alpha2; dsc[1].beta = 0.0; dsc[1].amax = nullptr;
        if (alt2) dsc[1].A = A2alt;
        if (ovr2) dsc[1].A = *ovr2;
    }
    __syncthreads();
    TTN_SETPRIO_GEMM();
    wg_syrk2_impl(dsc, lds);
    TTN_SETPRIO_BASE();
}

// -------------------------------------------------------------------------------------------------
// wg_gemm_ra: C = alpha * A B for a SHORT, SHALLOW A (m <= 64 rows, k <= 128) and any n — the right factor of a bond step
// (sqrt(S) V^T = X^T M: 64 x 384 x 128), route F's two output products (64 x 128 x 64; the left one is passed transposed).
// Every wave keeps the A fragments of its 16-row tile for ALL of k in registers (k/4 doubles per lane, read once), B streams through
// LDS in chunks of 16 x (NWAVES / 4) columns — all of k at once, so one barrier pair per chunk of k/4 MFMAs per wave instead of
// one per 16 k, no A staging at all, and the loads of the next chunk are in flight (registers) during the MFMAs.  The general
// tiled GEMM ran these shapes at 21 % of the matrix pipe with two workgroups per CU.
// -------------------------------------------------------------------------------------------------
#define GEMM_RA_NMAX (2 * GEMM_TAB_ENTRIES - 320)           // column offsets of B tabulated once
// The MFMAs of one chunk for 8 NB k-steps, straight-line.  The B fragments live in a ring of RA_RING registers: an MFMA reads its
// operands when it issues, so the fragment of k-step ks + RA_RING is read into the register of k-step ks right behind that MFMA and
// has RA_RING - 1 MFMAs (64 clk each) to arrive; the waits in front of the MFMAs are counted ones and no branch stands between
// them.  (Written as 32 steps each under `if (ks < ksteps)`, every MFMA sat behind one ds_read into the same register pair and a
// full drain, with a branch per k-step.)  One accumulator, its MFMAs in k order: results are unchanged.
// RA_RING = 3 is what fits: next to the 64 A registers and the 16 of the prefetch, a ring of 4 or more has the compiler keep A
// fragments on the stack and reload them between the MFMAs (each reload behind a vmcnt(0) that drains the prefetch), or leaves
// k_compress with 60 to 70 more spilled registers of its own (its allocation depends on its callees': DESIGN 4.2).
#define RA_RING 3
template <int NB, int LD>
__device__ __forceinline__ mfma_acc_t ra_ksteps(const double* areg, const lds_f64* bp) {
    mfma_acc_t acc = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
    double b[RA_RING];
#pragma unroll
    for (int t = 0; t < RA_RING; ++t) b[t] = bp[4 * t * LD];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 8 * NB; ++ks) {
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[ks], b[ks % RA_RING], acc, 0, 0, 0);
        if (ks + RA_RING < 8 * NB) b[ks % RA_RING] = bp[4 * (ks + RA_RING) * LD];
        __builtin_amdgcn_sched_barrier(0);               // keep each refill right behind its MFMA
    }
    return acc;
}
__device__ __noinline__ void wg_gemm_ra_impl(const GemmDesc* dsc_, double* lds) {
    const lds_gdesc* dsc = (const lds_gdesc*)dsc_;
    constexpr int CG = TTN_NWAVES / 4, NC = 16 * CG;                // column groups of waves; columns per chunk (32 / 64)
    constexpr int LD = (NC == 32) ? 49 : 81;                       // == 17 mod 32
    constexpr int KR = 128 / (TTN_WG / NC);                         // k rows per thread of a chunk (8)
    static_assert(128 * LD <= GEMM_LDS_DOUBLES, "a chunk holds all of k");
    const int m = uni32(dsc->m), n = uni32(dsc->n), k = uni32(dsc->k);
    const View A = ldsView(&dsc->A), B = ldsView(&dsc->B), C = ldsView(&dsc->C);
    const double alpha = unif64(dsc->alpha);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int rt = uni32(wave & 3), cg = uni32(wave >> 2);
    lds_f64* Bs = (lds_f64*)lds;                                    // Bs[kk * LD + j]
    lds_i32* rowA = (lds_i32*)(lds + GEMM_LDS_DOUBLES + 32);       // 64
    lds_i32* kA = rowA + 64;                                        // 128
    lds_i32* kB = kA + 128;                                         // 128
    lds_i32* colB = kB + 128;                                       // n
    for (int i = tid; i < 64; i += TTN_WG) rowA[i] = (i < m) ? (int)ix(A.r, i) : 0;
    for (int i = tid; i < 128; i += TTN_WG) { kA[i] = (i < k) ? (int)ix(A.c, i) : 0; kB[i] = (i < k) ? (int)ix(B.r, i) : 0; }
    for (int i = tid; i < n; i += TTN_WG) colB[i] = (int)ix(B.c, i);
    __syncthreads();
    gmem_f64* Ag = (gmem_f64*)A.p;
    gmem_f64* Bg = (gmem_f64*)B.p;
    gmem_wf64* Cg = (gmem_wf64*)C.p;
    const int ksteps = (k + 3) >> 2;
    double areg[32];
    {
        const int row = rt * 16 + li, ro = rowA[row < 64 ? row : 0];
#pragma unroll
        for (int ks = 0; ks < 32; ++ks) {
            const int kk = 4 * ks + lk, ka = kA[kk];                // read unconditionally (entries of rows >= k are 0): one batch
            areg[ks] = Ag[(row < m && kk < k) ? ro + ka : 0];
        }
#pragma unroll
        for (int ks = 0; ks < 32; ++ks) { const int kk = 4 * ks + lk; if (!(row < m && kk < k)) areg[ks] = 0.0; }
    }
    const int fx = tid % NC, sy = tid / NC;                         // column of the chunk; first k row (rows sy + (TTN_WG / NC) u)
    double v[KR];
    // The prefetch of a chunk: ONE batch of table reads (the column offset and the KR k offsets: entries of rows >= k are 0), then
    // the loads, unconditional — an out-of-range position reads element 0 of B (the LDS store below writes its zero).  (Each load
    // once sat behind its own table read and drain, under a branch.)  The k offsets are the same for every chunk, but kept in
    // registers across the chunk loop they take this leaf to the last of the 128 VGPRs, and k_compress then spills 50 more of its own.
#define RA_LOAD(C0)                                                                                                     \
    {                                                                                                                   \
        const int col = (C0) + fx;                                                                                      \
        const int co = colB[col < n ? col : 0];                                                                         \
        int kb_[KR];                                                                                                    \
        _Pragma("unroll") for (int u = 0; u < KR; ++u) kb_[u] = kB[sy + (TTN_WG / NC) * u];                             \
        _Pragma("unroll") for (int u = 0; u < KR; ++u) {                                                                 \
            const int kk = sy + (TTN_WG / NC) * u;                                                                      \
            v[u] = Bg[(col < n && kk < k) ? co + kb_[u] : 0];                                                           \
        }                                                                                                               \
    }
    RA_LOAD(0)
    const bool live = rt * 16 < m;                                  // wave-uniform
    // Dispatched ONCE per chunk on the number of eight-step groups (64 and 128 deep are the bond step's), not per k-step.  A k that
    // is no multiple of 32 runs the rest of its last group on the zero padding of areg and Bs (rows k .. 127 of both are +0.0): that
    // adds +0.0 to an accumulator that started at +0.0 and therefore never holds -0.0 — the same bits as skipping those steps.
    const int nb = uni32((ksteps + 7) >> 3);
    for (int c0 = 0; c0 < n; c0 += NC) {
#pragma unroll
        for (int u = 0; u < KR; ++u) {
            const int kk = sy + (TTN_WG / NC) * u;
            Bs[kk * LD + fx] = (c0 + fx < n && kk < k) ? v[u] : 0.0;
        }
        __syncthreads();
        if (c0 + NC < n) RA_LOAD(c0 + NC)
        if (live && c0 + cg * 16 < n) {
            const lds_f64* bp = Bs + lk * LD + cg * 16 + li;
            mfma_acc_t acc;
            if (nb == 4) acc = ra_ksteps<4, LD>(areg, bp);
            else if (nb == 2) acc = ra_ksteps<2, LD>(areg, bp);
            else if (nb == 3) acc = ra_ksteps<3, LD>(areg, bp);
            else acc = ra_ksteps<1, LD>(areg, bp);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int gi = rt * 16 + lk + 4 * reg, gj = c0 + cg * 16 + li;
                if (gi < m && gj < n) Cg[ix(C.r, gi) + ix(C.c, gj)] = alpha * acc[reg];
            }
        }
        __syncthreads();
    }
#undef RA_LOAD
}

// C = alpha A B; takes the register-A form when the shape allows (m <= 64, k <= 128), else the general GEMM
__device__ inline void wg_gemm_ra(int m, int n, int k, View A, View B, View C, double alpha, double* lds) {
#if TTN_WG != 512
    // (measured: inside the 1024-thread kernel — one workgroup per CU, 16 waves — the general forms are as fast or faster)
    wg_gemm(m, n, k, A, B, C, alpha, 0.0, lds);
#else
    if (m > 64 || k > 128 || n > GEMM_RA_NMAX || n < 64) { wg_gemm(m, n, k, A, B, C, alpha, 0.0, lds); return; }
    GemmDesc* dsc = reinterpret_cast<GemmDesc*>(lds + GEMM_LDS_DOUBLES);
    __syncthreads();
    if (threadIdx.x == 0) { dsc->m = m; dsc->n = n; dsc->k = k; dsc->pad = 0; dsc->A = A; dsc->B = B; dsc->C = C; dsc->alpha = alpha; dsc->beta = 0.0; dsc->amax = nullptr; }
    __syncthreads();
    TTN_SETPRIO_GEMM();
    wg_gemm_ra_impl(dsc, lds);
    TTN_SETPRIO_BASE();
#endif
}

// -------------------------------------------------------------------------------------------------
// wg_gemm_ra2: C1 = alpha1 A1 B1 and C2 = alpha2 A2 B2, two INDEPENDENT register-A products with m, k <= 64 in one call (route F's
// two output products, 64 x 128 x 64 each), for the reason wg_syrk2 gives: the single call is table setup, one global round trip
// and two barriers per chunk around 16 MFMAs per wave.  The workgroup's 8 waves split into two teams of 4; team t takes the product
// of descriptor t: wave w of the team keeps the A fragments of row tile w (16 registers for k <= 64, not 32), B streams through the
// team's half of the LDS region in the single form's chunks (all of k x 32 columns, LD 49) and the wave multiplies BOTH 16-column
// groups of a chunk, one after the other, with the single form's straight-line k-step groups (ra_ksteps).  One accumulator per output
// tile, its MFMAs in k order with the operands the single form gives it: the same bits.  Both teams run the chunk count of the wider
// product (the same workgroup barriers); the team that is done stages zeros and skips its MFMAs.
// -------------------------------------------------------------------------------------------------
#if TTN_WG == 512
#define GEMM_RA2_NMAX (SYRK2_TAB - 192)                     // a team's tables: 64 row, 2 x 64 k and n column offsets
__device__ __noinline__ void wg_gemm_ra2_impl(const GemmDesc* dsc_, double* lds) {
    constexpr int TWG = TTN_WG / 2, NC = 32, LD = 49, KMAX = 64;   // threads of a team; columns per chunk; == 17 mod 32; deepest k
    constexpr int KR = KMAX / (TWG / NC);                           // k rows per thread of a chunk (8)
    static_assert(TWG == 256 && 2 * KMAX * LD <= GEMM_LDS_DOUBLES, "one chunk per team holds all of k");
    const int team = uni32((int)threadIdx.x / TWG);
    const lds_gdesc* dsc = (const lds_gdesc*)dsc_ + team;
    const int m = uni32(dsc->m), n = uni32(dsc->n), k = uni32(dsc->k);
    const int no = uni32(((const lds_gdesc*)dsc_ + (1 - team))->n), nall = n > no ? n : no;     // the columns the chunk loop (and its barriers) covers
    const View A = ldsView(&dsc->A), B = ldsView(&dsc->B), C = ldsView(&dsc->C);
    const double alpha = unif64(dsc->alpha);
    const int tid = threadIdx.x - team * TWG, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int rt = uni32(tid >> 6);                                 // row tile of this wave
    lds_f64* Bs = (lds_f64*)lds + team * (KMAX * LD);               // Bs[kk * LD + j]
    lds_i32* rowA = (lds_i32*)(lds + GEMM_LDS_DOUBLES + 64) + team * SYRK2_TAB;      // 64 (behind the two descriptors, as wg_syrk2's)
    lds_i32* kA = rowA + 64;                                        // 64
    lds_i32* kB = kA + KMAX;                                        // 64
    lds_i32* colB = kB + KMAX;                                      // n
    for (int i = tid; i < 64; i += TWG) {
        rowA[i] = (i < m) ? (int)ix(A.r, i) : 0;
        kA[i] = (i < k) ? (int)ix(A.c, i) : 0;
        kB[i] = (i < k) ? (int)ix(B.r, i) : 0;
    }
    for (int i = tid; i < n; i += TWG) colB[i] = (int)ix(B.c, i);
    __syncthreads();
    gmem_f64* Ag = (gmem_f64*)A.p;
    gmem_f64* Bg = (gmem_f64*)B.p;
    gmem_wf64* Cg = (gmem_wf64*)C.p;
    double areg[KMAX / 4];
    {
        const int row = rt * 16 + li, ro = rowA[row];               // row < 64
#pragma unroll
        for (int ks = 0; ks < KMAX / 4; ++ks) {
            const int kk = 4 * ks + lk, ka = kA[kk];                // read unconditionally (entries of rows >= k are 0): one batch
            areg[ks] = Ag[(row < m && kk < k) ? ro + ka : 0];
        }
#pragma unroll
        for (int ks = 0; ks < KMAX / 4; ++ks) { const int kk = 4 * ks + lk; if (!(row < m && kk < k)) areg[ks] = 0.0; }
    }
    const int fx = tid % NC, sy = tid / NC;                         // column of the chunk; first k row (rows sy + (TWG / NC) u)
    double v[KR];
#define RA2_LOAD(C0)        /* as RA_LOAD of the single form: one batch of table reads, unconditional loads from clamped addresses */ \
    {                                                                                                                   \
        const int col = (C0) + fx;                                                                                      \
        const int co = colB[col < n ? col : 0];                                                                         \
        int kb_[KR];                                                                                                    \
        _Pragma("unroll") for (int u = 0; u < KR; ++u) kb_[u] = kB[sy + (TWG / NC) * u];                                \
        _Pragma("unroll") for (int u = 0; u < KR; ++u) {                                                                 \
            const int kk = sy + (TWG / NC) * u;                                                                         \
            v[u] = Bg[(col < n && kk < k) ? co + kb_[u] : 0];                                                           \
        }                                                                                                               \
    }
    RA2_LOAD(0)
    const bool live = rt * 16 < m;                                  // wave-uniform
    const int nb = uni32((((k + 3) >> 2) + 7) >> 3);                // groups of eight k-steps: 1 or 2 (the rest of a group runs on zeros)
    for (int c0 = 0; c0 < nall; c0 += NC) {
#pragma unroll
        for (int u = 0; u < KR; ++u) {
            const int kk = sy + (TWG / NC) * u;
            Bs[kk * LD + fx] = (c0 + fx < n && kk < k) ? v[u] : 0.0;
        }
        __syncthreads();
        if (c0 + NC < n) RA2_LOAD(c0 + NC)
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) {
            if (live && c0 + cg * 16 < n) {                         // wave-uniform
                const lds_f64* bp = Bs + lk * LD + cg * 16 + li;
                mfma_acc_t acc;
                if (nb == 2) acc = ra_ksteps<2, LD>(areg, bp);
                else acc = ra_ksteps<1, LD>(areg, bp);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int gi = rt * 16 + lk + 4 * reg, gj = c0 + cg * 16 + li;
                    if (gi < m && gj < n) Cg[ix(C.r, gi) + ix(C.c, gj)] = alpha * acc[reg];
                }
            }
        }
        __syncthreads();
    }
#undef RA2_LOAD
}
#endif

// two products C_i = alpha_i A_i B_i; the two-team form where both shapes allow it (the 512-thread build, m, k <= 64), else two wg_gemm_ra.
// ovr2: the second product reads ovr2[0] and stores into ovr2[1], the views THREAD 0 left at that LDS address, instead of B2 and C2
// (stored over the descriptor by thread 0, as in wg_syrk2)
__device__ inline void wg_gemm_ra2(int m1, int n1, int k1, View A1, View B1, View C1, double alpha1,
                                   int m2, int n2, int k2, View A2, View B2, View C2, double alpha2, double* lds, const View* ovr2 = nullptr) {
#if TTN_WG == 512
    if (m1 <= 64 && m2 <= 64 && k1 <= 64 && k2 <= 64 && n1 >= 64 && n2 >= 64 && n1 <= GEMM_RA2_NMAX && n2 <= GEMM_RA2_NMAX) {
        GemmDesc* dsc = reinterpret_cast<GemmDesc*>(lds + GEMM_LDS_DOUBLES);
        __syncthreads();                     // nobody still reads what the tiles / descriptors alias
        if (threadIdx.x == 0) {
            dsc[0].m = m1; dsc[0].n = n1; dsc[0].k = k1; dsc[0].pad = 0; dsc[0].A = A1; dsc[0].B = B1; dsc[0].C = C1; dsc[0].alpha = alpha1; dsc[0].beta = 0.0; dsc[0].amax = nullptr;
            dsc[1].m = m2; dsc[1].n = n2; dsc[1].k = k2; dsc[1].pad = 0; dsc[1].A = A2; dsc[1].B = B2; dsc[1].C = C2; dsc[1].alpha = alpha2; dsc[1].beta = 0.0; dsc[1].amax = nullptr;
            if (ovr2) { dsc[1].B = ovr2[0]; dsc[1].C = ovr2[1]; }
        }
        __syncthreads();
        TTN_SETPRIO_GEMM();
        wg_gemm_ra2_impl(dsc, lds);
        TTN_SETPRIO_BASE();
        return;
    }
#endif
    wg_gemm_ra(m1, n1, k1, A1, B1, C1, alpha1, lds);
    if (ovr2) { __syncthreads(); B2 = uniView(ovr2[0]); C2 = uniView(ovr2[1]); }
    wg_gemm_ra(m2, n2, k2, A2, B2, C2, alpha2, lds);
}
