// ttn_wg_chol.h — Cholesky factorisation of a matrix resident in LDS by one workgroup.
//
// Provides:
//   chol_lds128_teams               blocked LDS Cholesky with lookahead, one or two matrices at once
//   wg_chol_lds128, wg_chol2_lds128 its out-of-line instances (one matrix of n <= 128 / two of n <= 64)
// Needs: ttn_wg_prims.h.
// Used by: ttn_dense_kernels.h (routes F and G, CholeskyQR2), ttn_ortho_kernels.h.
#pragma once
#include "ttn_wg_prims.h"

// -------------------------------------------------------------------------------------------------
// Cholesky G = L L^T in LDS (column-major, leading dimension 128, n <= 128), in place: on exit the lower
// triangle holds L and the strict upper triangle is zeroed.  Returns 0, or 1 if a pivot is not safely
// positive (d_j <= n*eps*max_diag): the caller then falls back to the Householder path.
// Blocked right-looking, panel width 16, three workgroup barriers per PANEL (the unblocked form it replaces took one
// per column and ~2.7 k clk per column of LDS read-modify-write traffic: 355 k clk for n = 128):
//   (a) wave 0 factors the 16x16 diagonal block in LDS (wave-level ordering only) and leaves 1/l_kk in red[0..15];
//   (b) one thread per row below the block solves its row of L21 = A21 L11^-T in registers;
//   (c) the trailing matrix gets A22 -= L21 L21^T by fp64 MFMA, one 16x16 tile of the lower triangle per wave and trip,
//       operands read straight from the LDS image.
// -------------------------------------------------------------------------------------------------
// NTEAM = 2 (n <= 64): the workgroup splits into two teams of 8 waves that factor TWO matrices at once (team t: the matrix
// at Gg + t*64*128, scratch red + 32*t, result slot pivmin_out[t]) — the route-F step needs chol(A'^T A') and chol(B' B'^T),
// and a factorisation is dominated by the dependent pivot chain of one wave, so two in parallel cost about what one does.
// The barriers are workgroup-wide: both teams run the same control flow (same n); a bad pivot in either stops both.
template <int NTEAM>
__device__ int chol_lds128_teams(int n, double* Gg, double* red, int* flag, double* pivmin_out /*LDS*/) {
    n = uni32(n); Gg = unip(Gg); red = unip(red); flag = unip(flag); pivmin_out = unip(pivmin_out);     // VGPR arguments -> SGPRs
    constexpr int WPT = TTN_NWAVES / NTEAM;              // waves per team
    const int lane = threadIdx.x & 63;
    const int team = (threadIdx.x >> 6) / WPT, wave = (threadIdx.x >> 6) % WPT, nwaves = WPT;
    const int tid = threadIdx.x - team * WPT * 64;       // thread index inside the team
    const int li = lane & 15, lk = lane >> 4;
    lds_f64* G = (lds_f64*)Gg + team * (TTN_LDS_IMG / 2);
    lds_f64* invd = (lds_f64*)red + 32 * team;           // 1 / l_kk of the current panel ([0..15]) and the column buffer ([16..31])
    double dmax = 0.0;
    if (wave == 0) {
        for (int j = lane; j < n; j += 64) dmax = fmax(dmax, G[j * 128 + j]);
        dmax = wave_max(dmax);
        if (lane == 0) invd[0] = dmax;
    }
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    dmax = invd[0];
    __syncthreads();
    const double dmin = (double)n * DBL_EPSILON * dmax;
    double pmin = dmax;                                  // tracked by wave 0 (every lane sees every pivot)
    int bad = 0;
    // (a) diagonal block j0, wave 0, in REGISTERS: lane (li, lk) holds D[li][lk + 4q], q = 0..3.  Per column one LDS round
    //     trip: the owners publish the unscaled column, every lane reads the pivot, its row's and its columns' entries and
    //     applies the rank-1 update to its four elements.  A lone wave issues one fp64 instruction per ~9 clk, so the step
    //     is written with as few as possible: no per-element predicates.  Entries above the diagonal are PUBLISHED as zero,
    //     which makes the update of an already final column (c < jj) vanish by itself; the unpublished upper entries a lane
    //     holds just carry bounded garbage that is never read or written back.
#define CHOL_DIAG_BLOCK(J0)                                                                                         \
    {                                                                                                               \
        const int jb_ = (n - (J0) < 16) ? n - (J0) : 16;                                                            \
        lds_f64* D = G + (J0) * 128 + (J0);              /* D[c*128 + i] */                                          \
        lds_f64* colbuf = invd + 16;                     /* red[16..31] */                                           \
        double e[4];                                                                                                \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) { const int c = lk + 4 * q; e[q] = (li < jb_ && c <= li) ? D[c * 128 + li] : 0.0; } \
        _Pragma("unroll") for (int jj = 0; jj < 16; ++jj) {                                                         \
            if (jj >= jb_) break;                                                                                   \
            if (lk == (jj & 3)) colbuf[li] = (li >= jj) ? e[jj >> 2] : 0.0;                                         \
            __builtin_amdgcn_wave_barrier();                                                                        \
            const double d = colbuf[jj], ali = colbuf[li];                                                          \
            double ac[4];                                                                                           \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) ac[q] = colbuf[lk + 4 * q];                               \
            if (!(d > dmin)) { if (lane == 0) *flag = 1; break; }                                                   \
            pmin = fmin(pmin, d);                                                                                   \
            const double rs = fast_rsqrt2(d);                                                                       \
            const double lli = ali * rs, nl = -lli * rs;                                                            \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) e[q] = fma(nl, ac[q], e[q]);                              \
            /* column jj is final: l_ij = a_ij / sqrt(d) below the diagonal, sqrt(d) = d * rs on it */              \
            if (lk == (jj & 3) && li >= jj) e[jj >> 2] = lli;                                                       \
            if (lane == 0) invd[jj] = rs;                                                                           \
            __builtin_amdgcn_wave_barrier();                                                                        \
        }                                                                                                           \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) { const int c = lk + 4 * q; if (li < jb_ && c <= li) D[c * 128 + li] = e[q]; } \
    }
    // (c) one 16x16 tile (tr >= tc) of the trailing update A22 -= L21 L21^T of panel j0, by one wave, straight from LDS
#define CHOL_TILE(TILE)                                                                                             \
    {                                                                                                               \
        int tr = 0, base = 0;                                                                                       \
        while (base + tr + 1 <= (TILE)) { base += tr + 1; ++tr; }      /* tile = tr(tr+1)/2 + tc */                  \
        const int tc = (TILE) - base;                                                                               \
        const int r0 = s0 + 16 * tr, c0 = s0 + 16 * tc;                                                             \
        mfma_acc_t acc = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};                                                          \
        _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                                             \
            const lds_f64* col = G + (j0 + 4 * t + lk) * 128;                                                       \
            const double av = (r0 + li < n) ? col[r0 + li] : 0.0;                                                   \
            const double bv = (c0 + li < n) ? col[c0 + li] : 0.0;                                                   \
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);                                       \
        }                                                                                                           \
        _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) {                                                       \
            const int row = r0 + lk + 4 * reg, colj = c0 + li;                                                      \
            if (row < n && colj < n && row >= colj) G[colj * 128 + row] -= acc[reg];                                \
        }                                                                                                           \
    }
    if (wave == 0) CHOL_DIAG_BLOCK(0)
    for (int j0 = 0; j0 < n; j0 += 16) {
        const int jb = (n - j0 < 16) ? n - j0 : 16;
        __syncthreads();                                 // diagonal block j0 factored (by wave 0, during the previous trailing update)
        if (*flag) { bad = 1; break; }
        const int s0 = j0 + jb, sr = n - s0;             // first row / number of rows below the block
        if (sr > 0) {                                    // then jb == 16
            // ---- (b) rows below the block: x L11^T = a, right-looking in registers ----
            if (tid < sr) {
                const int r = s0 + tid;
                double a[16];
#pragma unroll
                for (int c = 0; c < 16; ++c) a[c] = G[(j0 + c) * 128 + r];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    a[k] *= invd[k];
#pragma unroll
                    for (int c = k + 1; c < 16; ++c) a[c] = fma(-a[k], G[(j0 + k) * 128 + j0 + c], a[c]);
                }
#pragma unroll
                for (int c = 0; c < 16; ++c) G[(j0 + c) * 128 + r] = a[c];
            }
            __syncthreads();
            // ---- (c) trailing update with LOOKAHEAD: wave 0 takes tile 0 (= the next diagonal block) and factors it right
            //      away — the long dependent chain of (a) — while the other waves do the remaining tiles ----
            const int nt = (sr + 15) >> 4, ntiles = nt * (nt + 1) / 2;
            if (wave == 0) {
                CHOL_TILE(0)
                CHOL_DIAG_BLOCK(s0)
            } else {
                for (int tile = wave; tile < ntiles; tile += nwaves - 1) CHOL_TILE(tile)
            }
        }
    }
    __syncthreads();
#undef CHOL_DIAG_BLOCK
#undef CHOL_TILE
    // pivots lie between the extreme eigenvalues of G, so dmax/pmin is a LOWER bound of cond(G) = cond(M)^2
    if (tid == 0) pivmin_out[team] = (!bad && pmin > 0.0) ? dmax / pmin : 1.0e300;
    for (int e = tid; e < n * 128; e += WPT * 64) { const int c = e >> 7, i = e & 127; if (i < c) G[c * 128 + i] = 0.0; }
    __syncthreads();
    return bad;
}

__device__ __noinline__ int wg_chol_lds128(int n, double* Gg, double* red, int* flag, double* pivmin_out /*LDS*/) {
    return chol_lds128_teams<1>(n, Gg, red, flag, pivmin_out);
}
// two n x n matrices (n <= TTN_LDS_COLS / 2) at Gg and Gg + TTN_LDS_IMG / 2; red: 64 doubles; pivmin_out: 2 doubles
__device__ __noinline__ int wg_chol2_lds128(int n, double* Gg, double* red64, int* flag, double* pivmin_out2 /*LDS*/) {
    return chol_lds128_teams<2>(n, Gg, red64, flag, pivmin_out2);
}
