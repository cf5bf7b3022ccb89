// ttn_dense_kernels.h — one-workgroup-per-train dense linear algebra for the chain recurrences:
// tt_compress! bond steps (merge GEMM -> LQ -> one-sided Jacobi SVD -> truncate -> split),
// dot (transfer-matrix GEMMs) and orthogonalize (Householder QR/LQ sweeps).
//
// Design: a sweep is strictly sequential along the chain, so ONE 1024-thread workgroup owns one
// train for the whole sweep (no inter-workgroup synchronisation anywhere); a batch of trains fills
// the 256 CUs.  All matrices are addressed through `View`s (2-level strides) so the reference's
// permutedims/reshape copies (src/tt_tools.jl:746-767) become index arithmetic.
//
// This file is the top of a family of layered headers and holds the bond step alone.  The layers below it, each a header that
// includes what it uses: ttn_wg_prims.h (reductions, uniform pins) <- ttn_wg_gemm.h (wg_gemm, wg_syrk, wg_gemm_ra) <- ttn_wg_lq.h
// (Householder LQ); ttn_wg_jacobi.h (one-sided Jacobi SVDs) and ttn_wg_chol.h (LDS Cholesky) on prims.  Above it:
// ttn_swap_kernels.h (k_swap_chain).  ttn_selftest_kernels.h (k_selftest_gemm) needs ttn_wg_gemm.h only.
// Map of this file (top to bottom):
//   CompressArgs, COMPRESS_LDS_BYTES, the FAST_* tolerances, BondCtx
//   wg_img_load, wg_trsm_lower_cols, wg_tril_mul_lds, wg_scale_image, wg_check_diag_tab, wg_check_diag_tab2, wg_diag_test_t3, wg_scale_t12_diag
//                                   out-of-line leaves of the routes (CholeskyQR2 helpers first)
//   wg_svd_cols / wg_rank_rule / wg_check_diag, wg_materialize_core / wg_fused_merge, wg_bond_step, k_compress
//                                   the bond step (routes F / G / H, fused apply) and the persistent sweep kernel
// Sibling headers (included after this one by ttn_api.hip): ttn_eig_kernels.h (symmetric eigensolver of the Gram routes, called
// from the bond step through the forward declarations below), ttn_ortho_kernels.h, ttn_hsvd_kernels.h (ttv_decomp, SVD moves),
// ttn_als_kernels.h (als_linsolve / mals_linsolve).
#pragma once
#include "ttn_wg_prims.h"
#include "ttn_wg_gemm.h"
#include "ttn_wg_lq.h"
#include "ttn_wg_jacobi.h"
#include "ttn_wg_chol.h"

// -------------------------------------------------------------------------------------------------
// Parameters of the compress / bond-truncate kernel
// -------------------------------------------------------------------------------------------------
struct CompressArgs {
    TTDev tt;
    long long max_bond;
    double truncerr;
    int sweeps;
    int k_single;          // 0: full tt_compress! sweeps; > 0: 1-based bond for _tt_bond_truncate!; < 0: the bond range below
    int k_first, k_last;   // k_single < 0: 0-based bonds k_first .. k_last in that order (descending if k_first > k_last)
    double* scratch;       // per-train global scratch
    long long scratch_stride;
    int pmax, qmax;        // bounds on the short / long side of any merged matrix
    double* sv_out;        // [batch][sv_steps][pmax] or null
    int sv_steps;
    int* status;           // [batch] device: 0 ok, 1 = Jacobi did not converge
    int* sweep_stats;      // [batch] device: total Jacobi sweeps (diagnostics)
    int fast;              // 0: Householder route only; odd: try the Gram / factored fast paths (verified a posteriori) first.
                           // Diagnostic bits (TTN_FAST): 2 no eigensolver in route G (Cholesky + Jacobi), 4 none in route F,
                           // 8 no diagonal-left shortcut in route F, 16 no Jacobi polish after a failed conditioning test,
                           // 32 a route-F step whose B' was handed over in the staging area treats its a-posteriori check as failed
                           //    (the restore path of the hand-over: Rf is in the dead core already, then the step falls back)
    // fused apply (ttn_apply_compress): psi = A * x is never materialised.  During the FIRST L->R sweep core k+1 of psi
    // is still virtual (= A_{k+1} applied to x_{k+1}); psi's ranks already hold A.rks .* x.rks.
    int fused;
    TTODev op;
    TTDev x;
    int rank_rule;         // 0: relative tail norm (_svdtrunc, tt_cross_interpolation.jl:149-166); 1: count(s > truncerr * s[1]), at least 1
                           //    (_swap_adjacent_sites, src/qtt_tools.jl:680-685)
    int fused_first_real;  // fused bond range (k_single < 0, ascending): the left core of the first bond is already real (a boundary core
                           // imported from the left neighbour of a core-wise sharded chain); otherwise it is written out first
    int* next_train;       // null: one workgroup per train (grid = batch).  Else a device counter (zeroed before the launch): the grid is
                           // PERSISTENT — workgroup w starts with train w and then pulls train gridDim.x + atomicAdd(next_train, 1)
                           // until the batch is exhausted (dynamic balancing of the data-dependent sweep counts, scratch per slot)
};

#define COMPRESS_LDS_X_DOUBLES (128 * 128)
#define COMPRESS_LDS_BYTES ((GEMM_LDS_TOTAL + 32 + 2 * QR_NB * QR_NB + QR_NB + 8 + 8 + 128) * sizeof(double))
#define FAST_KAPPA_MAX 128.0          // fast paths are used only when sigma_max/sigma_min <= this (error ~ eps*kappa^2)
#define FAST_KAPPA_POLISH 32768.0     // Gram route with a Jacobi polish of U^T M up to this conditioning of the kept block
#define FAST_POLISH_DROP 1.0e-12      // ... and only if the singular values it drops carry at most this share of ||M||_F^2 (i.e. are noise)
#define FAST_DIAG_TOL 2.0e-12         // route F: A'^T A' counts as diagonal below this (relative to sqrt(G_ii G_jj))
#define FAST_CHECK_TOL 2.0e-11        // a-posteriori bound on |Rf Rf^T - Sigma| (and Lf^T Lf - Sigma), relative
// (the size of M itself: SCALE_SAFE of ttn_common.h — outside it route F declines and the general step divides M by an exact, even
// power of two first and multiplies its outputs by the root of it afterwards)

struct BondCtx {
    // LDS
    double *ldsX, *red, *Ts, *Ss, *taus, *scal, *nrm2;
    int* iflag;
    // global scratch
    double *M, *M2, *Vb, *Wb, *Us, *Xg, *sig, *sigs, *Ga, *Gb, *Cc, *T1, *T2, *T3;
    int* perm;
};

// -------------------------------------------------------------------------------------------------
// CholeskyQR2 for the rank-ramp bond steps (short side 16..64, moderately ill-conditioned: kappa 1e2..1e5 on the benchmark's
// L->R step 64 x 384).  The Householder LQ of such a matrix is 64 dependent reflectors over 384 columns (1.75 M clk with two
// workgroups per CU — more than a whole 128-row Gram step); the Gram route alone squares the condition number.  CholeskyQR2:
//   L1 = chol(M M^T);  Q1 = L1^-1 M (forward substitution, backward stable column by column);  L2 = chol(Q1 Q1^T);  L = L1 L2.
// Q1 is orthonormal up to eps kappa^2 << 1, so ITS Gram matrix loses nothing, and M = L1 Q1 + E with |E| <= eps |L1| |Q1|: L is
// the triangular factor of M + dM, ||dM|| ~ eps ||M|| — the backward error of the Householder factorisation — as long as
// eps kappa^2 stays well below 1 (measured: |Q1 Q1^T - I| <= CHOLQR_ORTH_MAX, i.e. kappa up to ~3e6); two MFMA Gram products, two
// 64 x 64 factorisations in LDS and one triangular solve instead of the reflector chain.
// -------------------------------------------------------------------------------------------------
#define CHOLQR_PIVOT_MAX 1.0e11       // first-pass pivot ratio (a lower bound of kappa^2) up to which CholeskyQR2 is taken
#define CHOLQR_ORTH_MAX 1.0e-3        // ... and the second pass must see a nearly orthonormal Q1: max |Q1 Q1^T - I| (~ eps kappa^2)
#define CHOLQR_CHECK_TOL 1.0e-9       // a-posteriori |Rf Rf^T - Sigma| bound of the route (the Householder route it replaces has none)

// p x p block of a leading-dimension-128 matrix in global memory -> rows [row_off, row_off + p) of the first p columns of the LDS image,
// eight loads of a thread in flight; returns max |src - I| (every thread; contains barriers)
__device__ __noinline__ double wg_img_load(double* img, int row_off, const double* src, int p, double* red) {
    img = unip(img); src = unip(src); p = uni32(p); row_off = uni32(row_off); red = unip(red);
    lds_f64* X = (lds_f64*)img;
    double dev = 0.0;
    wg_batched<8>((long long)p * p, [&](long long e) { const int ei = (int)e; return src[ei % p + 128 * (ei / p)]; },
                  [&](long long e, double v) {
                      const int ei = (int)e, i = ei % p, j = ei / p;
                      X[row_off + i + 128 * j] = v;
                      dev = fmax(dev, fabs(v - ((i == j) ? 1.0 : 0.0)));
                  });
    return unif64(wg_max(dev, red));
}

// Q[i][c] = (L^-1 (s M))[i][c], i < p, c < q: one thread per column, 16 rows at a time in registers; L (lower triangular, p <= 64) in
// the LDS image (L[i][k] at img[i + 128 k]), M and Q row-major in global memory.  Ends with a barrier.
__device__ __noinline__ void wg_trsm_lower_cols(int p, int q, const double* img, const double* M, long long ldm, double s_, double* Q, long long ldq) {
    p = uni32(p); q = uni32(q); img = unip(img); M = unip(M); Q = unip(Q); ldm = uni64(ldm); ldq = uni64(ldq); s_ = unif64(s_);
    const lds_f64* L = (const lds_f64*)img;
    gmem_f64* Mg = (gmem_f64*)M;
    gmem_wf64* Qg = (gmem_wf64*)Q;
    for (int c = threadIdx.x; c < q; c += TTN_WG) {
        for (int i0 = 0; i0 < p; i0 += 16) {
            const int nb = (p - i0 < 16) ? p - i0 : 16;
            double v[16];
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) v[ii] = Mg[(long long)(i0 + (ii < nb ? ii : 0)) * ldm + c];
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) v[ii] *= s_;
            for (int j0 = 0; j0 < i0; j0 += 16) {            // the finished blocks of this column (the thread's own stores)
                double qv[16];
#pragma unroll
                for (int jj = 0; jj < 16; ++jj) qv[jj] = Qg[(long long)(j0 + jj) * ldq + c];
#pragma unroll
                for (int jj = 0; jj < 16; ++jj)
#pragma unroll
                    for (int ii = 0; ii < 16; ++ii) v[ii] = fma(-L[(j0 + jj) * 128 + i0 + ii], qv[jj], v[ii]);
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k < nb) {
                    v[k] = v[k] / L[(i0 + k) * 128 + i0 + k];
#pragma unroll
                    for (int ii = k + 1; ii < 16; ++ii) v[ii] = fma(-L[(i0 + k) * 128 + i0 + ii], v[k], v[ii]);
                }
            }
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) if (ii < nb) Qg[(long long)(i0 + ii) * ldq + c] = v[ii];
        }
    }
    __syncthreads();
}

// L = L1 L2 in the LDS image (p <= 64): L2 at img[i + 128 k], L1 at img[64 + i + 128 k] (the rows the p x p Jacobi image pads with
// zeros); on exit the first p columns hold L (lower triangle) and zeros everywhere else.  Ends with a barrier.
__device__ __noinline__ void wg_tril_mul_lds(int p, double* img) {
    p = uni32(p); img = unip(img);
    lds_f64* X = (lds_f64*)img;
    constexpr int NE = (64 * 64 + TTN_WG - 1) / TTN_WG;
    double acc[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) {
        const int e = threadIdx.x + u * TTN_WG, i = e % p, j = e / p;
        double a = 0.0;
        if (e < p * p && i >= j)
            for (int k = j; k <= i; ++k) a = fma(X[64 + i + 128 * k], X[k + 128 * j], a);
        acc[u] = a;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < p * 128; e += TTN_WG) X[e] = 0.0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NE; ++u) {
        const int e = threadIdx.x + u * TTN_WG, i = e % p, j = e / p;
        if (e < p * p && i >= j) X[i + 128 * j] = acc[u];
    }
    __syncthreads();
}

// -------------------------------------------------------------------------------------------------
// Element loops of a bond step that scale the image columns by functions of sigma_j.  Written inline as
// `for (e = tid; e < p * r; e += WG) { row = e % p; j = e / p; ... sqrt(sigs[j]) ... ix(view, row) ... }` they spent ~3 k clk per
// element of a thread on two runtime integer divisions, the two-level index of the output view, an fp64 square root and two fp64
// divisions (57 k clk per 128-row Gram step for 8192 elements).  Out of line: everything that depends on j alone (factors, the
// permutation, column offsets) or on the row alone (row offsets) goes to small LDS tables first, the element loop walks (row = lane,
// j = wave) without divisions.  `tab`: 512 doubles of LDS (the Householder panel matrices S.Ts / S.Ss, dead outside the LQ).
// -------------------------------------------------------------------------------------------------
// Lo[row, j] = keep_j ? X[row, perm_j] f1_j : 0,  Us[j p + row] = keep_j ? X[row, perm_j] f2_j : 0   (row < p <= 128, j < r <= 128)
//   mode 0 (tt_compress!):  f1 = sq0 / sqrt(s_j), f2 = sq0 / (s_j sqrt(s_j));  mode 1 (swap, wide): 1 / s_j, s0 / s_j;  mode 2 (swap, tall): s0, 1 / s_j^2
__device__ __noinline__ void wg_scale_image(const double* X, int ldx, int x_in_lds, const double* sigs, const int* perm, View Lo, double* Us, int p, int r,
                                            double s0, double aneg, int mode, double* tab) {
    X = unip(X); ldx = uni32(ldx); x_in_lds = uni32(x_in_lds); sigs = unip(sigs); perm = unip(perm); Lo = uniView(Lo); Us = unip(Us);
    p = uni32(p); r = uni32(r); s0 = unif64(s0); aneg = unif64(aneg); mode = uni32(mode); tab = unip(tab);
    lds_f64* f1 = (lds_f64*)tab; lds_f64* f2 = f1 + 128;
    lds_i32* pj = (lds_i32*)(f2 + 128); lds_i32* coff = pj + 128; lds_i32* roff = coff + 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double sq0 = sqrt(s0);
    for (int j = tid; j < r; j += TTN_WG) {
        const double sj = sigs[j];
        const bool keep = (sj > 0.0) && (sj * sj > aneg);
        double a, b_;
        if (mode == 0) { const double rs = sqrt(sj); a = sq0 / rs; b_ = sq0 / (sj * rs); }
        else if (mode == 1) { a = 1.0 / sj; b_ = s0 / sj; }
        else { a = s0; b_ = 1.0 / (sj * sj); }
        f1[j] = keep ? a : 0.0; f2[j] = keep ? b_ : 0.0;
        pj[j] = perm[j]; coff[j] = (int)ix(Lo.c, j);
    }
    for (int i = tid; i < p; i += TTN_WG) roff[i] = (int)ix(Lo.r, i);
    __syncthreads();
    gmem_wf64* Lg = (gmem_wf64*)Lo.p;
    gmem_wf64* Ug = (gmem_wf64*)Us;
    for (int j = wave; j < r; j += TTN_NWAVES) {
        const double a = f1[j], b_ = f2[j];
        const int c = pj[j], co = coff[j];
        for (int row = lane; row < p; row += 64) {
            const double xv = x_in_lds ? ((const lds_f64*)X)[c * ldx + row] : X[(long long)c * ldx + row];
            Lg[roff[row] + co] = xv * a;
            Ug[j * p + row] = xv * b_;
        }
    }
    __syncthreads();
}

// max over i, j < r of |D[i + ldd j] - delta_ij sigs[i] s0| / (s0 sqrt(sigs[i] sigs[j]))   (r <= 128; every thread gets it)
__device__ __noinline__ double wg_check_diag_tab(const double* sigs, const double* D, int ldd, int r, double s0, double* tab, double* red) {
    sigs = unip(sigs); D = unip(D); ldd = uni32(ldd); r = uni32(r); s0 = unif64(s0); tab = unip(tab); red = unip(red);
    lds_f64* t = (lds_f64*)tab; lds_f64* ref = t + 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < r; i += TTN_WG) { const double si = sigs[i]; t[i] = 1.0 / sqrt(s0 * si); ref[i] = si * s0; }
    __syncthreads();
    gmem_f64* Dg = (gmem_f64*)D;
    double worst = 0.0;
    for (int j = wave; j < r; j += TTN_NWAVES) {
        const double tj = t[j];
        for (int i = lane; i < r; i += 64) {
            const double dv = Dg[i + ldd * j];
            const double dev = fabs(dv - ((i == j) ? ref[i] : 0.0)) * (t[i] * tj);
            worst = fmax(worst, dev);
        }
    }
    return unif64(wg_max(worst, red));
}

// The same check of TWO matrices D1, D2 against the same sigs in one pass: max of the two results (route F tests both against one
// tolerance).  One table, one reduction, the loads of both matrices in flight together; a maximum does not depend on the order.
__device__ __noinline__ double wg_check_diag_tab2(const double* sigs, const double* D1, const double* D2, int ldd, int r, double s0, double* tab, double* red) {
    sigs = unip(sigs); D1 = unip(D1); D2 = unip(D2); ldd = uni32(ldd); r = uni32(r); s0 = unif64(s0); tab = unip(tab); red = unip(red);
    lds_f64* t = (lds_f64*)tab; lds_f64* ref = t + 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < r; i += TTN_WG) { const double si = sigs[i]; t[i] = 1.0 / sqrt(s0 * si); ref[i] = si * s0; }
    __syncthreads();
    gmem_f64* D1g = (gmem_f64*)D1; gmem_f64* D2g = (gmem_f64*)D2;
    double worst = 0.0;
    for (int j = wave; j < r; j += TTN_NWAVES) {
        const double tj = t[j];
        for (int i = lane; i < r; i += 64) {
            const double d1 = D1g[i + ldd * j], d2 = D2g[i + ldd * j];
            const double rf = (i == j) ? ref[i] : 0.0, sc = t[i] * tj;
            worst = fmax(worst, fmax(fabs(d1 - rf) * sc, fabs(d2 - rf) * sc));
        }
    }
    return unif64(wg_max(worst, red));
}

// Route F with a 64 x 64 left Gram matrix Ga (ld 128): w = max_{i != j} |Ga_ij| / sqrt(Ga_ii Ga_jj) (1 if a diagonal entry is not
// positive) and T3 = D^(1/2) Gb D^(1/2), D = diag(Ga) — one pass over both matrices.  Every thread gets w.
__device__ __noinline__ double wg_diag_test_t3(const double* Ga, const double* Gb, double* T3, double* tab, double* red) {
    Ga = unip(Ga); Gb = unip(Gb); T3 = unip(T3); tab = unip(tab); red = unip(red);
    lds_f64* sd = (lds_f64*)tab; lds_f64* isd = sd + 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    gmem_f64* Gag = (gmem_f64*)Ga; gmem_f64* Gbg = (gmem_f64*)Gb; gmem_wf64* Tg = (gmem_wf64*)T3;
    for (int i = tid; i < 64; i += TTN_WG) { const double d = Gag[i * 129]; const double sq = (d > 0.0) ? sqrt(d) : 0.0; sd[i] = sq; isd[i] = (d > 0.0) ? 1.0 / sq : -1.0; }
    __syncthreads();
    double w = 0.0;
    const double si = sd[lane], ii = isd[lane];
    constexpr int NJ = 64 / TTN_NWAVES;                       // columns per wave (8 / 4)
    double ga[NJ], gb[NJ];
#pragma unroll
    for (int u = 0; u < NJ; ++u) { const int j = wave + TTN_NWAVES * u; ga[u] = Gag[lane + 128 * j]; gb[u] = Gbg[lane + 128 * j]; }
#pragma unroll
    for (int u = 0; u < NJ; ++u) {
        const int j = wave + TTN_NWAVES * u;
        const double ij = isd[j];
        if (lane != j) w = fmax(w, (ii > 0.0 && ij > 0.0) ? fabs(ga[u]) * (ii * ij) : 1.0);
        Tg[lane + 128 * j] = si * gb[u] * sd[j];
    }
    w = unif64(wg_max(w, red));
    return w;
}

// Route F, diagonal-left form: T1[j 128 + row] = X[row, perm_j] fa / (sd_row sqrt(s_j)),  T2[j 128 + row] = X[row, perm_j] sd_row fb / (s_j sqrt(s_j)),
// sd_row = sqrt(Ga[row, row]); row < 64, j < rk <= 64; X = the LDS image (ld 128)
__device__ __noinline__ void wg_scale_t12_diag(const double* img, const double* sigs, const int* perm, const double* Ga, double* T1, double* T2, int rk,
                                               double fa, double fb, double* tab) {
    img = unip(img); sigs = unip(sigs); perm = unip(perm); Ga = unip(Ga); T1 = unip(T1); T2 = unip(T2); rk = uni32(rk); fa = unif64(fa); fb = unif64(fb); tab = unip(tab);
    lds_f64* c1 = (lds_f64*)tab; lds_f64* c2 = c1 + 64; lds_f64* sd = c2 + 64; lds_f64* isd = sd + 64;
    lds_i32* pj = (lds_i32*)(isd + 64);
    const lds_f64* X = (const lds_f64*)img;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < 64; j += TTN_WG) {
        const double d = sqrt(Ga[j * 129]); sd[j] = d; isd[j] = 1.0 / d;
        if (j < rk) { const double sj = sigs[j], rs = sqrt(sj); c1[j] = fa / rs; c2[j] = fb / (sj * rs); pj[j] = perm[j]; }
    }
    __syncthreads();
    gmem_wf64* T1g = (gmem_wf64*)T1; gmem_wf64* T2g = (gmem_wf64*)T2;
    const double sdr = sd[lane], isdr = isd[lane];
    for (int j = wave; j < rk; j += TTN_NWAVES) {
        const double xv = X[pj[j] * 128 + lane];
        T1g[j * 128 + lane] = xv * (c1[j] * isdr);
        T2g[j * 128 + lane] = xv * (sdr * c2[j]);
    }
    __syncthreads();
}

// Jacobi on the pj columns (length pj) of X, then singular values sigma_c = ||x_c|| sorted descending with a
// stable order: perm[pos] = column, sigs[pos] = sigma (scaled units).  Returns the sweep count (<0: limit hit).
__device__ int wg_svd_cols(const CompressArgs& P, const BondCtx& S, int pj, double* X, int ldx, bool in_lds, int mlen = 0) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = TTN_WG >> 6;
    // mlen: column length if it is not pj (LDS image only: the polish step of the Gram route runs r columns of length q)
    const int nsw = (in_lds && mlen) ? wg_jacobi_lds128(mlen, pj, X, S.nrm2, S.iflag, S.red, S.scal)
                  : in_lds ? wg_jacobi_lds128(pj, pj, X, S.nrm2, S.iflag, S.red, S.scal)
#if TTN_LDS_COLS < 128
                  : (pj <= 128) ? wg_jacobi_blocked128(pj, pj, X, ldx, S.ldsX, S.nrm2, S.iflag, S.red, S.scal)
#endif
                  : (pj <= 256) ? wg_jacobi_blocked256(pj, pj, X, ldx, S.ldsX, S.nrm2, S.iflag, S.red, S.scal)
                                : wg_jacobi_cols(pj, pj, X, ldx, S.iflag, S.red, S.scal);
    for (int c = wave; c < pj; c += nwaves) {
        double a = 0.0;
        for (int r = lane; r < (mlen ? mlen : pj); r += 64) { const double v = X[(long long)c * ldx + r]; a = fma(v, v, a); }
        a = wave_sum(a);
        if (lane == 0) S.sig[c] = sqrt(a);
    }
    __syncthreads();
    for (int c = tid; c < pj; c += TTN_WG) {
        const double sc = S.sig[c];
        int pos = 0;
        for (int j = 0; j < pj; ++j) { const double sj = S.sig[j]; pos += (sj > sc) || (sj == sc && j < c); }
        S.perm[pos] = c;
        S.sigs[pos] = sc;
    }
    __syncthreads();
    return nsw;
}

// The effective _svdtrunc rank rule (src/tt_cross_interpolation.jl:149-166) on `ns` computed singular values
// (scaled by s0) padded with zeros to the reference's length `plen` = min(size(M)).  All threads get r.
__device__ __forceinline__ int wg_rank_rule_core(int rank_rule, double truncerr, long long max_bond, const double* sigs, int* iflag, int ns, int plen, double s0) {
    if (threadIdx.x == 0) {
        int r = plen;
        if (rank_rule == 1) {
            if (truncerr > 0.0) {
                r = 0;
                const double thr = truncerr * (sigs[0] * s0);
                for (int i = 0; i < ns; ++i) r += (sigs[i] * s0 > thr) ? 1 : 0;
                if (r < 1) r = 1;
            }
        } else if (truncerr > 0.0) {
            double n2 = 0.0;
            for (int i = 0; i < ns; ++i) { const double s = sigs[i] * s0; n2 = fma(s, s, n2); }
            const double nrm = sqrt(n2);
            double cum = 0.0;
            for (int i = plen; i >= 1; --i) {
                const double s = (i <= ns) ? sigs[i - 1] * s0 : 0.0;
                cum = fma(s, s, cum);
                if (sqrt(cum) > truncerr * nrm) { r = i; break; }
            }
        }
        if ((long long)r > max_bond) r = (int)max_bond;
        iflag[1] = r;
    }
    __syncthreads();
    const int r = uni32(iflag[1]);
    __syncthreads();
    return r;
}
__device__ int wg_rank_rule(const CompressArgs& P, const BondCtx& S, int ns, int plen, double s0) {
    return wg_rank_rule_core(P.rank_rule, P.truncerr, P.max_bond, S.sigs, S.iflag, ns, plen, s0);
}

// max over i,j < r of |D[i + ldd*j] - delta_ij * sigs[i]*s0| / (s0*sqrt(sigs[i]*sigs[j]))
__device__ double wg_check_diag(const BondCtx& S, const double* D, int ldd, int r, double s0) {
    double worst = 0.0;
    for (int e = threadIdx.x; e < r * r; e += TTN_WG) {
        const int i = e % r, j = e / r;
        const double si = S.sigs[i], sj = S.sigs[j];
        const double ref = (i == j) ? si * s0 : 0.0;
        worst = fmax(worst, fabs(D[i + (long long)ldd * j] - ref) / (s0 * sqrt(si * sj)));
    }
    return wg_max(worst, S.red);
}

// Core k of psi = A * x written out (src/tt_operations.jl:101-111): psi_k[s, a' + Rl*nu', a + Rr*nu] = sum_j A_k[s,j,a',a] x_k[j,nu',nu].
// Used by the fused apply+compress for the cores the fused merge does not cover (first core, tall / tiny steps).
__device__ void wg_materialize_core(const CompressArgs& P, int b, int k) {
    const TTDev& T = P.tt;
    const int n = T.dims[k];
    const long long* xr = P.x.rks + (long long)b * (P.x.d + 1);
    const int rl = uni32((int)xr[k]), rr = uni32((int)xr[k + 1]);
    const int Rl = uni32((int)P.op.rks[k]), Rr = uni32((int)P.op.rks[k + 1]);
    const double* xc = P.x.data + (long long)b * P.x.stride + P.x.off[k];
    const double* ac = P.op.data + P.op.off[k];
    double* yc = T.data + (long long)b * T.stride + T.off[k];
    const long long Dl = (long long)Rl * rl, tot = (long long)n * Dl * Rr * rr;
    for (long long e = threadIdx.x; e < tot; e += TTN_WG) {
        const int s = (int)(e % n);
        const long long t1 = e / n;
        const int ga = (int)(t1 % Dl), be = (int)(t1 / Dl);
        const int a1 = ga % Rl, nu1 = ga / Rl, a2 = be % Rr, nu2 = be / Rr;
        double v = 0.0;
        for (int j = 0; j < n; ++j)
            v = fma(ac[s + n * (j + n * (a1 + (long long)Rl * a2))], xc[j + n * (nu1 + (long long)rl * nu2)], v);
        yc[e] = v;
    }
    __syncthreads();
}

// Fused merge of an L->R step whose right core is still virtual (wide case, p = n1*Dl rows):
//   M[row, s2 + n2*(a + Rr*nu)] = sum_{a', nu'} C_k[row, a' + Rl*nu'] * sum_j A[s2, j, a', a] x[j, nu', nu]
// = (i)  T_a'[row, (j, nu)] = sum_nu' C_k[row, a' + Rl*nu'] x[j, nu', nu]      Rl GEMMs  p x (n2*rho_r) x rho_l  (MFMA)
//   (ii) M[row, (s2, a, nu)] = sum_{a', j} T_a'[row, (j, nu)] A[s2, j, a', a]     Rl*n2 terms per output     (VALU)
// 2*p*Rl*rho_l*n2*rho_r flops instead of 2*p*(Rl*rho_l)*(n2*Rr*rho_r) — Rr times fewer — and the core never exists in HBM.
// T lives in `Tbuf` (>= Rl*p*n2*rho_r doubles).  max|M| goes to *amax_lds.  Returns false (nothing done) if the shapes
// do not qualify; the caller then materialises the core.
// ---- the same merge in ONE pass, with the operator contraction in the GEMM epilogue (n2 = 2, small operator ranks) -----------------
// The first version (wg_fused_merge below, still the general path) runs Rl separate GEMMs into a buffer T (Rl p n2 rho_r doubles,
// 393 KB for the benchmark's steps), and a second pass reads T back, contracts with the operator core and writes M: measured inside
// the kernel (cycle counters, 512-thread build, two workgroups per CU) 349 k clk for the three GEMMs — 14 % of the matrix pipe each: K = 64
// is all prologue — plus 191 k clk for the contraction pass, per bond step.  Here a wave keeps the Rl accumulators T_a'[16 rows,
// 16 (j, nu) columns] of its tiles in registers: they share every B fragment (x is read once, not Rl times), and when the K loop is
// done the lane that holds column (j, nu) forms its share sum_a' T_a' A[s, j, a', a] of the n2 Rr outputs of that (row, nu), adds its
// neighbour's (the other j: one DPP quad permutation) and writes M.  T never exists.
// Layout: chunks of FM_BK = 8 values of nu' through two LDS stages (As[(a' FM_BK + kk) LDA + row], Bs[kk LDB + col]); a wave owns
// one 16-row tile and two 16-column tiles ((j, nu) columns: 8 nu each) of a pass over CP = 32 * (waves / row tiles) columns.
#define FM_BK 8
__device__ __noinline__ bool wg_fused_merge_mfma(double* ck, const double* xc, const double* ac, double* M, int p, int q, int n1, int Dl,
                                                 int rhl, int rhr, int Rl, int Rr, double* lds, double* amax_lds, double* red) {
    ck = unip(ck); xc = unip(xc); ac = unip(ac); M = unip(M); lds = unip(lds); amax_lds = unip(amax_lds); red = unip(red);
    p = uni32(p); q = uni32(q); n1 = uni32(n1); Dl = uni32(Dl); rhl = uni32(rhl); rhr = uni32(rhr); Rl = uni32(Rl); Rr = uni32(Rr);
    constexpr int n2 = 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int RT = p >> 4;                                           // row tiles
    const int WR = RT < 8 ? RT : 8;                                  // waves along the rows (the A stage holds 128 rows: LDA = 145)
    const int WC = TTN_NWAVES / WR;                                  // wave columns (>= 1)
    const int CP = 32 * WC;                                          // (j, nu) columns per pass
    const int ncol = n2 * rhr, nin = Rl * n2, nout = n2 * Rr;
    constexpr int LDA = GEMM_LD;
    const int LDB = (CP <= 32) ? 49 : (CP <= 64) ? 81 : GEMM_LD;     // all == 17 mod 32
    const int stage = Rl * FM_BK * LDA + FM_BK * LDB;
    if (Rl < 1 || Rl > 3 || Rr > 4 || (p & 15) || (rhl % FM_BK) || (ncol % CP) || (RT % WR) || WR * WC != TTN_NWAVES || CP > 128 ||
        Rl * FM_BK * 16 * WR > 6 * TTN_WG || FM_BK * CP > 2 * TTN_WG || 2 * stage + 64 > GEMM_LDS_DOUBLES)
        return false;
    lds_f64* opl = (lds_f64*)lds + 2 * stage;                        // operator core: opl[o * nin + i], o = s + n2 a, i = j + n2 a'
    __syncthreads();
    for (int e = tid; e < nin * nout; e += TTN_WG) {
        const int i = e % nin, o = e / nin;
        opl[e] = ac[(o % n2) + n2 * ((i % n2) + n2 * ((i / n2) + (long long)Rl * (o / n2)))];
    }
    const long long ldk = (long long)n1 * Dl;                        // column stride of C_k as a (n1 Dl) x (Rl rho_l) matrix
    const int wr = wave % WR, wc = wave / WR;
    const int nchunk = rhl / FM_BK;
    gmem_f64* Cg = (gmem_f64*)ck;
    gmem_f64* Xg = (gmem_f64*)xc;
    gmem_wf64* Mg = (gmem_wf64*)M;
    double cmax = 0.0;
    // staging assignment: A chunk = Rl * FM_BK * (16 WR) elements, row fastest; B chunk = FM_BK * CP elements, column fastest
    const int arows = 16 * WR;
    const int na_el = Rl * FM_BK * arows, nb_el = FM_BK * CP;
    constexpr int NUA = 6, NUB = 2;                                  // elements per thread and chunk (enough for 3 * 8 * 128 / 512 and 8 * 128 / 512)
    for (int rb = 0; rb < RT; rb += WR) {                            // row blocks of 16 WR rows
        for (int c0 = 0; c0 < ncol; c0 += CP) {                      // column passes
            mfma_acc_t acc[3][2];
#pragma unroll
            for (int a1 = 0; a1 < 3; ++a1) { acc[a1][0] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}; acc[a1][1] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}; }
            int aoff[NUA], alds[NUA], boff[NUB], blds[NUB];
            bool aok[NUA], bok[NUB];
#pragma unroll
            for (int u = 0; u < NUA; ++u) {
                const int e = tid + TTN_WG * u;
                aok[u] = e < na_el;
                const int r = e % arows, rest = e / arows, kk = rest % FM_BK, a1 = rest / FM_BK;
                const int row = 16 * rb + r;
                // C_k[(al, s1), ga] at s1 + n1 (al + Dl ga), row = al + Dl s1, ga = a1 + Rl nu'
                aoff[u] = aok[u] ? (row % Dl) * n1 + row / Dl + (int)(ldk * (a1 + (long long)Rl * kk)) : 0;
                alds[u] = (a1 * FM_BK + kk) * LDA + r;
            }
#pragma unroll
            for (int u = 0; u < NUB; ++u) {
                const int e = tid + TTN_WG * u;
                bok[u] = e < nb_el;
                const int c = e % CP, kk = e / CP, col = c0 + c;
                // x[j, nu', nu] at j + n2 (nu' + rho_l nu), col = j + n2 nu
                boff[u] = bok[u] ? (col & 1) + n2 * (kk + rhl * (col >> 1)) : 0;
                blds[u] = kk * LDB + c;
            }
            const int astep = (int)(ldk * Rl * FM_BK), bstep = n2 * FM_BK;       // address advance per chunk
            double av[NUA], bv[NUB];
#define FM_LOAD(CH)                                                                                                     \
            { _Pragma("unroll") for (int u = 0; u < NUA; ++u) av[u] = Cg[aoff[u] + (CH) * astep];                       \
              _Pragma("unroll") for (int u = 0; u < NUB; ++u) bv[u] = Xg[boff[u] + (CH) * bstep]; }
#define FM_STORE(STG)                                                                                                   \
            { lds_f64* As_ = (lds_f64*)lds + (STG) * stage; lds_f64* Bs_ = As_ + Rl * FM_BK * LDA;                      \
              _Pragma("unroll") for (int u = 0; u < NUA; ++u) if (aok[u]) As_[alds[u]] = av[u];                         \
              _Pragma("unroll") for (int u = 0; u < NUB; ++u) if (bok[u]) Bs_[blds[u]] = bv[u]; }
            __syncthreads();                                         // the previous pass has consumed both stages (and opl is written)
            FM_LOAD(0)
            FM_STORE(0)
            if (nchunk > 1) FM_LOAD(1)
            __syncthreads();
            for (int ch = 0; ch < nchunk; ++ch) {
                const lds_f64* As = (lds_f64*)lds + (ch & 1) * stage;
                const lds_f64* Bs = As + Rl * FM_BK * LDA;
#pragma unroll
                for (int t = 0; t < FM_BK / 4; ++t) {
                    const int kr = 4 * t + lk;
                    const double b0 = Bs[kr * LDB + wc * 32 + li], b1 = Bs[kr * LDB + wc * 32 + 16 + li];
#pragma unroll
                    for (int a1 = 0; a1 < 3; ++a1) {
                        if (a1 < Rl) {
                            const double a = As[(a1 * FM_BK + kr) * LDA + wr * 16 + li];
                            acc[a1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[a1][0], 0, 0, 0);
                            acc[a1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[a1][1], 0, 0, 0);
                        }
                    }
                    if (t == 0 && ch + 1 < nchunk) FM_STORE((ch + 1) & 1)
                }
                if (ch + 2 < nchunk) FM_LOAD(ch + 2)
                __syncthreads();
            }
#undef FM_LOAD
#undef FM_STORE
            // ---- epilogue: lane (li, lk) holds T_a'[row = lk + 4 reg][column li] of its two column tiles; column = j + n2 nu ----
            const int jl = li & 1;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const int nu = (c0 + wc * 32 + ct * 16 + li) >> 1;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = 16 * (rb + wr) + lk + 4 * reg;
                    gmem_wf64* mrow = Mg + ((long long)row * q + (long long)nout * nu);
                    for (int o = 0; o < nout; ++o) {
                        double v = 0.0;
#pragma unroll
                        for (int a1 = 0; a1 < 3; ++a1)
                            if (a1 < Rl) v = fma(acc[a1][ct][reg], opl[o * nin + jl + n2 * a1], v);
                        v += dpp_mov_f64<0xB1>(v);                   // + the other j (quad_perm [1,0,3,2]): both lanes of the pair hold the sum
                        if ((o & 1) == jl) mrow[o] = v;              // the pair shares the stores
                        cmax = fmax(cmax, fabs(v));
                    }
                }
            }
        }
    }
    cmax = wg_max(cmax, red);
    if (tid == 0) *amax_lds = cmax;
    __syncthreads();
    return true;
}

// ---- the one-pass merge without barriers in its main loop ("direct" form) ------------------------------------------------------------
// wg_fused_merge_mfma stages chunks of FM_BK = 8 values of nu' of BOTH operands through LDS: 8 chunks x 4 column passes = 32 barrier
// rounds of 12 MFMAs per wave each for a 128-row step — the barriers and the staging, not the matrix pipe, set its time (29 % of the
// pipe alone, 18 % with two workgroups per CU).  Here the x core (rho_l x n2 rho_r, 64 KB for rank 64) is staged ONCE, whole, and the
// A fragments — lane (li, lk) needs C_k[row 16 rt + li, a' + Rl (4 ks + lk)] — are loaded from global memory (L2) straight into the
// MFMA operand registers, four k-steps ahead of their use: no LDS staging of C_k, no barrier between the staging of x and the epilogue.
// Same tiling (a wave = one 16-row tile x two 16-column tiles x Rl accumulators), same epilogue.
//
// What keeps those loads in flight (the first version compiled to one memory round trip per LOAD: 4 Rl of them in a row per group):
//  * the operator rank Rl is a template parameter of the tile loops (fmd_tiles<RL>, RL = 1, 2, 3; the __noinline__ entry below picks
//    one).  As a run-time value every `a' < Rl` guard was a branch around one load or one MFMA pair, and a wait in front of each;
//  * an A fragment is addressed through a buffer descriptor of C_k (scalar registers) as ONE 32-bit byte offset per lane plus the
//    uniform displacement of its (group, k-step, a') in a scalar register (fmd_ld: buffer_load ... offen).  As 4 Rl 64-bit per-lane
//    addresses they did not fit the 128-VGPR budget next to the accumulators, and each was reloaded from the stack — behind a
//    vmcnt(0) that also drained the global load issued just before.  The displacement is ONE running scalar, advanced by an add
//    per load: left to itself the compiler precomputes all 4 Rl of every group, this leaf then uses every scalar register up to
//    s99, and k_compress — whose register allocation sees which registers its callees use — spills 180 VGPRs instead of 116;
//  * two fragment sets (fa, fb) alternate, the group loop is unrolled by two: no register copies between groups, so the only
//    wait in front of a group's MFMAs is the counted one for its own loads, with the next group's still outstanding.
// The order of the MFMAs and of the epilogue's FMAs is that of the first version: results are bit-identical.
typedef unsigned int fmd_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double fmd_ld(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {   // bytes: voff per lane, soff uniform
    return __builtin_bit_cast(double, (fmd_u32x2)__builtin_amdgcn_raw_buffer_load_b64(rs, (int)voff, (int)soff, 0));
}
template <int RL>
__device__ __forceinline__ double fmd_tiles(gmem_f64* Cg, gmem_wf64* Mg, const lds_f64* Bs, const lds_f64* opl, int p, int q, int n1,
                                            int Dl, int rhl, int rhr, int Rr, int LDB) {
    constexpr int n2 = 2, nin = RL * n2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int RT = p >> 4;
    const int WR = RT < 8 ? RT : 8;
    const int WC = TTN_NWAVES / WR;
    const int CP = 32 * WC;
    const int ncol = n2 * rhr, nout = n2 * Rr;
    const int ldk = n1 * Dl;                                         // column stride of C_k as a (n1 Dl) x (Rl rho_l) matrix
    const int wr = uni32(wave % WR), wc = uni32(wave / WR);          // wave-uniform: scalar registers
    const int ngrp = rhl >> 4;                                       // groups of four k-steps
    const int kstride = ldk * RL;                                    // address advance per nu'
    const unsigned a_step = 8u * (unsigned)ldk, t_step = 8u * (unsigned)(4 * kstride - (RL - 1) * ldk);   // bytes: a' -> a' + 1; (k-step, Rl - 1) -> (k-step + 1, 0)
    double cmax = 0.0;
    // C_k as a buffer: base and size (n1 Dl Rl rho_l doubles, <= 2^26) in scalar registers; a read past the end would return 0
    const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc((void*)Cg, 0, 8 * kstride * rhl, 0x00020000);
    for (int rb = 0; rb < RT; rb += WR) {
        const int arow = 16 * (rb + wr) + li;
        // C_k[(al, s1), ga] at s1 + n1 (al + Dl ga), row = al + Dl s1, ga = a' + Rl nu'
        const unsigned aoff = 8u * (unsigned)((arow % Dl) * n1 + arow / Dl + lk * kstride);
        for (int c0 = 0; c0 < ncol; c0 += CP) {
            mfma_acc_t acc[RL][2];
#pragma unroll
            for (int a1 = 0; a1 < RL; ++a1) { acc[a1][0] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}; acc[a1][1] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}; }
            double fa[4][RL], fb[4][RL];
            const lds_f64* bp = Bs + lk * LDB + c0 + wc * 32 + li;   // B fragments of k-step ks: bp[0], bp[16] at bp = ... + 4 ks LDB
#define FMD_LOAD(DST, G)   /* the uniform displacement runs along in ONE scalar register (opaque to the compiler: see above) */   \
            {                                                                                                           \
                unsigned so_ = 8u * (unsigned)(16 * (G) * kstride);                                                     \
                _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                            \
                    _Pragma("unroll") for (int a1 = 0; a1 < RL; ++a1) {                                                  \
                        DST[t][a1] = fmd_ld(crs, aoff, so_);                                                            \
                        so_ += (a1 + 1 < RL) ? a_step : t_step;                                                         \
                        asm volatile("" : "+s"(so_));                                                                   \
                    }                                                                                                   \
            }
#define FMD_MFMA(SRC, G)                                                                                                \
            _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                                              \
                const double b0 = bp[0], b1 = bp[16];                                                                   \
                bp += 4 * LDB;                                                                                          \
                asm volatile("" : "+v"(bp));         /* ONE running LDS address, not one induction variable per k-step */ \
                _Pragma("unroll") for (int a1 = 0; a1 < RL; ++a1) {                                                      \
                    acc[a1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(SRC[t][a1], b0, acc[a1][0], 0, 0, 0);             \
                    acc[a1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(SRC[t][a1], b1, acc[a1][1], 0, 0, 0);             \
                }                                                                                                       \
            }
            FMD_LOAD(fa, 0)
            // Group g + 1's loads go out before group g's MFMAs.  Loop body and tail are straight-line code: a load under a
            // condition makes the wait in front of the MFMAs behind it a full drain (the compiler merges both paths' counts).
            int g = 0;
            for (; g + 2 < ngrp; g += 2) {
                FMD_LOAD(fb, g + 1)
                FMD_MFMA(fa, g)
                FMD_LOAD(fa, g + 2)
                FMD_MFMA(fb, g + 1)
            }
            {   // one or two groups are left; an odd count loads its last group twice (in bounds, unused) instead of branching
                const bool two = g + 1 < ngrp;
                FMD_LOAD(fb, two ? g + 1 : g)
                FMD_MFMA(fa, g)
                if (two) { FMD_MFMA(fb, g + 1) }
            }
#undef FMD_LOAD
#undef FMD_MFMA
            // ---- epilogue: lane (li, lk) holds T_a'[row = lk + 4 reg][column li] of its two column tiles; column = j + n2 nu.
            // Both lanes of a (j = 0, 1) pair end up with all nout sums of their (row, nu); the pair then writes the nout consecutive
            // doubles M[row, nout nu ...] as two contiguous halves (lane j = 0 the first nout / 2, lane j = 1 the rest), 16 bytes at a
            // time where the address allows: the 16 lanes of a row of lanes cover 8 nu = 8 nout contiguous doubles of one row of M —
            // whole cache lines per store instruction.  (Stored one output at a time, lanes 6 doubles apart and half of them idle,
            // these stores, not the MFMAs, set the time of the merge.) ----
            // What the epilogue needs per lane (LDS addresses of the weights, row offsets into M) is derived HERE from an opaque copy
            // of the thread index — a handful of integer instructions per pass.  Derived from `li` / `lk` it is loop invariant: the
            // compiler computes it once, above the K loop, where it does not fit next to the accumulators and the two fragment sets,
            // and every pass reloads it from the stack.
            int te = tid;
            asm volatile("" : "+v"(te));
            const int lie = te & 15, lke = (te >> 4) & 3, jl = lie & 1;
            const int half = nout >> 1;
            const bool vec_ok = (half == 3) && ((((unsigned long long)Mg) & 15ull) == 0) && ((q & 1) == 0);
            if (RL == 3 && vec_ok) {
                // Operator ranks 3 x 3 (the Laplacian's interior cores): the pair first swaps its raw T values (one DPP move per a'), then
                // each lane forms ITS three outputs from all six inputs — weights w[oo][a'][own / other j] read from LDS once per pass —
                // and stores them as 16 + 8 bytes.
                constexpr int R3 = RL == 3 ? 3 : 1;                  // (this branch is compiled for RL < 3 too, and dropped)
                double w[3][R3][2];
#pragma unroll
                for (int oo = 0; oo < 3; ++oo)
#pragma unroll
                    for (int a1 = 0; a1 < R3; ++a1) {
                        const int o = 3 * jl + oo;
                        w[oo][a1][0] = opl[o * nin + jl + n2 * a1];          // own j
                        w[oo][a1][1] = opl[o * nin + (1 - jl) + n2 * a1];    // the neighbour's j
                    }
                typedef double dbl2 __attribute__((ext_vector_type(2)));
                typedef __attribute__((address_space(1))) dbl2 gmem_wd2;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int nu = (c0 + wc * 32 + ct * 16 + lie) >> 1;
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int row = 16 * (rb + wr) + lke + 4 * reg;
                        gmem_wf64* mrow = Mg + ((long long)row * q + (long long)nout * nu);
                        const double t0 = acc[0][ct][reg], t1 = acc[R3 > 1 ? 1 : 0][ct][reg], t2 = acc[R3 > 2 ? 2 : 0][ct][reg];
                        const double u0 = dpp_mov_f64<0xB1>(t0), u1 = dpp_mov_f64<0xB1>(t1), u2 = dpp_mov_f64<0xB1>(t2);      // quad_perm [1,0,3,2]
                        double v[3];
#pragma unroll
                        for (int oo = 0; oo < 3; ++oo) {
                            double x_ = t0 * w[oo][0][0];
                            x_ = fma(u0, w[oo][0][1], x_);
                            x_ = fma(t1, w[oo][R3 > 1 ? 1 : 0][0], x_); x_ = fma(u1, w[oo][R3 > 1 ? 1 : 0][1], x_);
                            x_ = fma(t2, w[oo][R3 > 2 ? 2 : 0][0], x_); x_ = fma(u2, w[oo][R3 > 2 ? 2 : 0][1], x_);
                            v[oo] = x_;
                            cmax = fmax(cmax, fabs(x_));
                        }
                        // j = 0: (o0, o1) as 16 bytes at +0, o2 at +2;  j = 1: o3 at +3, (o4, o5) as 16 bytes at +4
                        *(gmem_wd2*)(mrow + (jl ? 4 : 0)) = jl ? (dbl2){v[1], v[2]} : (dbl2){v[0], v[1]};
                        mrow[jl ? 3 : 2] = jl ? v[0] : v[2];
                    }
                }
            } else {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int nu = (c0 + wc * 32 + ct * 16 + lie) >> 1;
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int row = 16 * (rb + wr) + lke + 4 * reg;
                        gmem_wf64* mrow = Mg + ((long long)row * q + (long long)nout * nu);
                        for (int o = 0; o < nout; ++o) {
                            double v = 0.0;
#pragma unroll
                            for (int a1 = 0; a1 < RL; ++a1) v = fma(acc[a1][ct][reg], opl[o * nin + jl + n2 * a1], v);
                            v += dpp_mov_f64<0xB1>(v);                   // + the other j (quad_perm [1,0,3,2]): both lanes of the pair hold the sum
                            if ((o >= half) == (jl == 1)) mrow[o] = v;   // the pair shares the stores: each lane a contiguous half
                            cmax = fmax(cmax, fabs(v));
                        }
                    }
                }
            }
        }
    }
    return cmax;
}

// The ONE out-of-line entry (wg_fused_merge, inlined into the bond step, keeps a single call site): checks the shapes, stages the
// operator core and x, and runs the tile loops of its operator rank.
__device__ __noinline__ bool wg_fused_merge_direct(double* ck, const double* xc, const double* ac, double* M, int p, int q, int n1, int Dl,
                                                   int rhl, int rhr, int Rl, int Rr, double* lds, double* amax_lds, double* red) {
    ck = unip(ck); xc = unip(xc); ac = unip(ac); M = unip(M); lds = unip(lds); amax_lds = unip(amax_lds); red = unip(red);
    p = uni32(p); q = uni32(q); n1 = uni32(n1); Dl = uni32(Dl); rhl = uni32(rhl); rhr = uni32(rhr); Rl = uni32(Rl); Rr = uni32(Rr);
    constexpr int n2 = 2;
    const int tid = threadIdx.x;
    const int RT = p >> 4;
    const int WR = RT < 8 ? RT : 8;
    const int WC = TTN_NWAVES / WR;
    const int CP = 32 * WC;
    const int ncol = n2 * rhr, nin = Rl * n2, nout = n2 * Rr;
    const int LDB = ncol + 1;                                        // odd: the four k rows of a fragment read land two banks apart
    if (Rl < 1 || Rl > 3 || Rr > 4 || (p & 15) || (rhl & 15) || (ncol % CP) || (RT % WR) || WR * WC != TTN_NWAVES ||
        (long long)rhl * LDB + 64 > GEMM_LDS_DOUBLES)
        return false;
    lds_f64* Bs = (lds_f64*)lds;                                     // Bs[kk * LDB + col], kk = nu' < rho_l, col = j + n2 nu
    lds_f64* opl = Bs + rhl * LDB;                                   // operator core: opl[o * nin + i], o = s + n2 a, i = j + n2 a'
    gmem_f64* Cg = (gmem_f64*)ck;
    gmem_f64* Xg = (gmem_f64*)xc;
    gmem_wf64* Mg = (gmem_wf64*)M;
    __syncthreads();
    for (int e = tid; e < nin * nout; e += TTN_WG) {
        const int i = e % nin, o = e / nin;
        opl[e] = ac[(o % n2) + n2 * ((i % n2) + n2 * ((i / n2) + (long long)Rl * (o / n2)))];
    }
    // x[j, nu', nu] at j + n2 (nu' + rho_l nu): consecutive threads walk (j, nu') of one nu — contiguous in memory
    {
        const int nx = rhl * ncol, kspan = n2 * rhl;                 // elements of one nu
        for (int e0 = tid; e0 < nx; e0 += 8 * TTN_WG) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + u * TTN_WG; v[u] = Xg[e < nx ? e : e0]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = e0 + u * TTN_WG;
                if (e < nx) { const int nu = e / kspan, w_ = e - nu * kspan, j = w_ & 1, kk = w_ >> 1; Bs[kk * LDB + j + n2 * nu] = v[u]; }
            }
        }
    }
    __syncthreads();
    double cmax;
    if (Rl == 3) cmax = fmd_tiles<3>(Cg, Mg, Bs, opl, p, q, n1, Dl, rhl, rhr, Rr, LDB);
    else if (Rl == 2) cmax = fmd_tiles<2>(Cg, Mg, Bs, opl, p, q, n1, Dl, rhl, rhr, Rr, LDB);
    else cmax = fmd_tiles<1>(Cg, Mg, Bs, opl, p, q, n1, Dl, rhl, rhr, Rr, LDB);
    cmax = wg_max(cmax, red);
    if (tid == 0) *amax_lds = cmax;
    __syncthreads();
    return true;
}


#define FUSE_MAX_TERMS 16
__device__ bool wg_fused_merge(const CompressArgs& P, int b, int k, int p, int q, const View& Am, double* M, double* Tbuf,
                               long long tbuf_doubles, double* lds, double* amax_lds, double* red) {
    const TTDev& T = P.tt;
    const int n1 = T.dims[k], n2 = T.dims[k + 1];
    const long long* rks = T.rks + (long long)b * (T.d + 1);
    const int Dl = uni32((int)rks[k]);
    const long long* xr = P.x.rks + (long long)b * (P.x.d + 1);
    const int rhl = uni32((int)xr[k + 1]), rhr = uni32((int)xr[k + 2]);
    const int Rl = uni32((int)P.op.rks[k + 1]), Rr = uni32((int)P.op.rks[k + 2]);
    const int ncol = n2 * rhr;
    if (Rl * n2 > FUSE_MAX_TERMS || n2 * Rr > FUSE_MAX_TERMS || (long long)Rl * p * ncol > tbuf_doubles) return false;
    if ((long long)Rl * rhl != rks[k + 1] || (long long)n2 * Rr * rhr != q || p != n1 * Dl) return false;
    double* ck = T.data + (long long)b * T.stride + T.off[k];
    double* xc = P.x.data + (long long)b * P.x.stride + P.x.off[k + 1];
    const double* ac = P.op.data + P.op.off[k + 1];
    TTN_SETPRIO_GEMM();
    struct PrioRestore { __device__ ~PrioRestore() { TTN_SETPRIO_BASE(); } } prio_restore_;
    if (n2 == 2 && wg_fused_merge_direct(ck, xc, ac, M, p, q, n1, Dl, rhl, rhr, Rl, Rr, lds, amax_lds, red)) return true;
    if (n2 == 2 && wg_fused_merge_mfma(ck, xc, ac, M, p, q, n1, Dl, rhl, rhr, Rl, Rr, lds, amax_lds, red)) return true;
    const long long ldk = (long long)n1 * Dl;                           // column stride of C_k viewed as (n1*Dl) x r_mid
    for (int a1 = 0; a1 < Rl; ++a1) {
        const View Av = mkview(ck + a1 * ldk, Am.r, plain((long long)Rl * ldk));
        const View Bv = mkview(xc, plain(n2), Idx{n2, 1, (long long)n2 * rhl});
        const View Cv = mkview(Tbuf + (long long)a1 * p * ncol, plain(ncol), plain(1));
        wg_gemm(p, ncol, rhl, Av, Bv, Cv, 1.0, 0.0, lds);
    }
    // (ii): one thread per (row, nu): Rl*n2 inputs, n2*Rr outputs.  The operator core is staged in LDS as opl[o*nin + i]
    // (o = s2 + n2*a, i = j + n2*a'; the GEMM region is free between GEMM calls): the inner product then costs one broadcast
    // LDS read and one FMA per term instead of an indexed global load.
    double mx = 0.0;
    const int nin = Rl * n2, nout = n2 * Rr;
    lds_f64* opl = (lds_f64*)lds;
    for (int e = threadIdx.x; e < nin * nout; e += TTN_WG) {
        const int i = e % nin, o = e / nin;
        opl[e] = ac[(o % n2) + n2 * ((i % n2) + n2 * ((i / n2) + (long long)Rl * (o / n2)))];
    }
    __syncthreads();
    const long long tstride = (long long)p * ncol;                          // doubles between T_a' and T_a'+1
    for (int e = threadIdx.x; e < p * rhr; e += TTN_WG) {
        const int nu = e % rhr, row = e / rhr;
        const double* tp = Tbuf + (long long)row * ncol + n2 * nu;
        double t[FUSE_MAX_TERMS];
#pragma unroll
        for (int i = 0; i < FUSE_MAX_TERMS; ++i) t[i] = (i < nin) ? tp[(i / n2) * tstride + (i % n2)] : 0.0;
        double* mrow = M + (long long)row * q + (long long)nout * nu;
        for (int o = 0; o < nout; ++o) {
            const lds_f64* w = opl + o * nin;
            double v = 0.0;
#pragma unroll
            for (int i = 0; i < FUSE_MAX_TERMS; ++i)
                if (i < nin) v = fma(t[i], w[i], v);
            mrow[o] = v;
            mx = fmax(mx, fabs(v));
        }
    }
    mx = wg_max(mx, red);
    if (threadIdx.x == 0) *amax_lds = mx;
    __syncthreads();
    return true;
}

// -------------------------------------------------------------------------------------------------
// Bond steps with a SHORT side of at most 8 rows (the first and last three steps of each half sweep: p = 2, 4, 8, q <= 256; with
// 12..16 rows the row-wise Jacobi below loses to LQ + Jacobi on the triangle: measured).
// Through the general machinery — GEMM calls, Householder LQ, Jacobi image, output GEMM, each with its descriptor, barriers and
// global round trips — such a step costs 80..300 k clk, almost all of it fixed overhead (a 2 x 24 matrix: 154 k clk; twenty of them
// are 5 % of a train alone on a CU).  Here the merged matrix lives in LDS from the product to the outputs:
//   M = A' B' by one thread per entry;  one-sided Jacobi on the ROWS of M (one wave per pair, round-robin rounds; no LQ first:
//   the rows are at most 256 long) with the same rotations applied to a p x p identity — rows of the result are sigma_i v_i^T, the
//   rotated identity is U^T;  sort, rank rule, and U sqrt(S) / sqrt(S) V^T are written straight from LDS.
// Same conventions as the Householder route: units of s0 = max |M|, negligible rows (norm^2 <= aneg) are left alone and come out as
// exact zeros, convergence when a whole sweep rotates nothing (|g| <= tol sqrt(a b), tol = sqrt(q) eps).
// -------------------------------------------------------------------------------------------------
#define SMALL_STEP_PMAX 8
#define SMALL_STEP_QMAX 256
// (Everything it needs of the kernel's argument block and of the step's context comes BY VALUE in SmallStepArgs: a reference to either
// would force the caller — the force-inlined bond step, at its register limit — to keep them in memory: +280 spilled VGPRs, -6 % measured.)
struct SmallStepArgs {
    double truncerr;
    long long max_bond;
    int rank_rule, pmax;
    double* sv_row;              // null, or the pmax singular values of this (train, step)
    int* status_b;               // the train's status word
    double *red, *scal, *sigs;   // LDS reduction scratch, LDS scalars, singular values out
    int *perm, *iflag;
};
__device__ __noinline__ int wg_bond_small(SmallStepArgs Q, double* ck, double* ck1, int n1, int n2, int Dl, int rm, int Dr, long long* rank_out, double* lds) {
    rm = uni32(rm); n1 = uni32(n1); n2 = uni32(n2); Dl = uni32(Dl); Dr = uni32(Dr);
    ck = unip(ck); ck1 = unip(ck1); rank_out = unip(rank_out); lds = unip(lds);
    // A_mat[(al + Dl*s1), ga] = core_k[s1, al, ga] ; B_mat[ga, (s2 + n2*be)] = core_{k+1}[s2, ga, be]   (as in wg_bond_step_io)
    const int mr = n1 * Dl, mc = n2 * Dr;
    const View Am = mkview(ck, Idx{Dl, (long long)n1, 1}, plain((long long)n1 * Dl));
    const View Bm = mkview(ck1, plain(n2), Idx{n2, 1, (long long)n2 * rm});
    const int wide = (mr <= mc) ? 1 : 0;
    const int p = wide ? mr : mc, q = wide ? mc : mr;
    const View Ap = wide ? Am : tview(Bm);       // p x rm
    const View Bp = wide ? Bm : tview(Am);       // rm x q
    Q.truncerr = unif64(Q.truncerr); Q.max_bond = uni64(Q.max_bond);
    Q.rank_rule = uni32(Q.rank_rule); Q.pmax = uni32(Q.pmax); Q.sv_row = unip(Q.sv_row); Q.status_b = unip(Q.status_b);
    Q.red = unip(Q.red); Q.scal = unip(Q.scal); Q.sigs = unip(Q.sigs); Q.perm = unip(Q.perm); Q.iflag = unip(Q.iflag);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int LDQ = q + 1;
    lds_f64* Ms = (lds_f64*)lds;                                   // Ms[i * LDQ + j]
    lds_f64* Es = Ms + SMALL_STEP_PMAX * (SMALL_STEP_QMAX + 1);    // Es[i * 17 + j]: the rotated identity (row i = U[:, i]^T)
    lds_f64* nr = Es + SMALL_STEP_PMAX * 17;                       // squared row norms (16)
    lds_i32* flg = (lds_i32*)(nr + 16);
    gmem_f64* Ag = (gmem_f64*)Ap.p;
    gmem_f64* Bg = (gmem_f64*)Bp.p;
    __syncthreads();
    // ---- M = A' B' (p x q, inner rm), max |M| ----
    double mx = 0.0;
    for (int e = tid; e < p * q; e += TTN_WG) {
        const int i = e / q, j = e - i * q;
        const long long ao = ix(Ap.r, i), bo = ix(Bp.c, j);
        double acc = 0.0;
        for (int kk = 0; kk < rm; ++kk) acc = fma(Ag[ao + ix(Ap.c, kk)], Bg[bo + ix(Bp.r, kk)], acc);
        Ms[i * LDQ + j] = acc;
        mx = fmax(mx, fabs(acc));
    }
    for (int e = tid; e < p * 17; e += TTN_WG) Es[e] = ((e / 17) == (e % 17)) ? 1.0 : 0.0;
    mx = unif64(wg_max(mx, Q.red));
    const double s0 = (mx > 0.0) ? mx : 1.0, inv_s0 = 1.0 / s0;
    for (int e = tid; e < p * q; e += TTN_WG) { const int i = e / q, j = e - i * q; Ms[i * LDQ + j] *= inv_s0; }
    __syncthreads();
    // ---- squared row norms, negligible threshold ----
    double amax = 0.0;
    for (int i = wave; i < p; i += TTN_NWAVES) {
        double a = 0.0;
        for (int j = lane; j < q; j += 64) { const double v = Ms[i * LDQ + j]; a = fma(v, v, a); }
        a = wave_sum(a);
        if (lane == 0) nr[i] = a;
        amax = fmax(amax, a);
    }
    amax = unif64(wg_max(amax, Q.red));
    const double aneg = (double)q * DBL_EPSILON * DBL_EPSILON * amax;
    const double tol = sqrt((double)q) * DBL_EPSILON, tol2 = tol * tol;
    if (tid == 0) Q.scal[0] = aneg;
    // ---- one-sided Jacobi on the rows ----
    const int pe = p + (p & 1), half = pe >> 1;
    int sweeps = 0, conv = (p < 2);
    for (; !conv && sweeps < JACOBI_MAX_SWEEPS; ++sweeps) {
        if (tid == 0) *flg = 0;
        __syncthreads();
        int rotated = 0;
        for (int round = 0; round < pe - 1; ++round) {
            for (int kk = wave; kk < half; kk += TTN_NWAVES) {
                int i, j;
                if (kk == 0) { i = round; j = pe - 1; }
                else { i = (round + kk) % (pe - 1); j = (round + pe - 1 - kk) % (pe - 1); }
                if (i > j) { const int t = i; i = j; j = t; }
                if (j >= p) continue;                                  // bye
                lds_f64* xi = Ms + i * LDQ;
                lds_f64* xj = Ms + j * LDQ;
                // (rows of up to 256 entries: four per lane in registers between the dot products and the rotation)
                double u[4], v[4];
                double a = 0.0, b_ = 0.0, g = 0.0;
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    const int c = lane + 64 * t4;
                    u[t4] = (c < q) ? xi[c] : 0.0; v[t4] = (c < q) ? xj[c] : 0.0;
                    a = fma(u[t4], u[t4], a); b_ = fma(v[t4], v[t4], b_); g = fma(u[t4], v[t4], g);
                }
                a = wave_sum(a); b_ = wave_sum(b_); g = wave_sum(g);
                if (a <= aneg || b_ <= aneg) continue;
                if (g * g <= tol2 * a * b_) continue;
                // t = tan(theta) = sign(d) h / (|d| + sqrt(d^2 + h^2)), d = b - a, h = 2 g: hardware seeds are enough for t (it only sets the
                // speed of convergence); c = rsqrt(1 + t^2) with Newton steps so that c^2 + s^2 = 1 to rounding (as in the image Jacobi)
                const double dd = b_ - a, hh = g + g;
                const double hyp = __builtin_amdgcn_sqrt(fma(dd, dd, hh * hh));
                const double t = copysign(hh * __builtin_amdgcn_rcp(fabs(dd) + hyp), hh * dd);
                const double cs = fast_rsqrt2(fma(t, t, 1.0)), sn = cs * t;
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    const int c = lane + 64 * t4;
                    if (c < q) { xi[c] = cs * u[t4] - sn * v[t4]; xj[c] = sn * u[t4] + cs * v[t4]; }
                }
                if (lane < p) { const double u = Es[i * 17 + lane], v = Es[j * 17 + lane]; Es[i * 17 + lane] = cs * u - sn * v; Es[j * 17 + lane] = sn * u + cs * v; }
                rotated = 1;
            }
            __syncthreads();
        }
        if (rotated && lane == 0) atomicOr((int*)flg, 1);
        __syncthreads();
        conv = !(*flg);
        __syncthreads();
    }
    // ---- sigma_i = ||row i||, sorted descending (stable) ----
    for (int i = wave; i < p; i += TTN_NWAVES) {
        double a = 0.0;
        for (int j = lane; j < q; j += 64) { const double v = Ms[i * LDQ + j]; a = fma(v, v, a); }
        a = wave_sum(a);
        if (lane == 0) nr[i] = sqrt(a);
    }
    __syncthreads();
    for (int c = tid; c < p; c += TTN_WG) {
        const double sc = nr[c];
        int pos = 0;
        for (int j = 0; j < p; ++j) { const double sj = nr[j]; pos += (sj > sc) || (sj == sc && j < c); }
        Q.perm[pos] = c;
        Q.sigs[pos] = sc;
    }
    __syncthreads();
    const int r = wg_rank_rule_core(Q.rank_rule, Q.truncerr, Q.max_bond, Q.sigs, Q.iflag, p, p, s0);
    if (Q.sv_row)
        for (int i = tid; i < Q.pmax; i += TTN_WG) Q.sv_row[i] = (i < p) ? Q.sigs[i] * s0 : -1.0;
    // ---- outputs: left factor (p x r) = U sqrt(s0 Sigma), right factor (r x q) = sqrt(s0 / Sigma) (sigma v^T) ----
    const View Lfv = mkview(ck, Idx{Dl, (long long)n1, 1}, plain((long long)n1 * Dl));
    const View Rfv = mkview(ck1, plain(n2), Idx{n2, 1, (long long)n2 * r});
    const View Lo = wide ? Lfv : tview(Rfv);
    const View Ro = wide ? Rfv : tview(Lfv);
    const double sq0 = sqrt(s0);
    for (int e = tid; e < p * r; e += TTN_WG) {
        const int row = e % p, j = e / p;
        const double sj = Q.sigs[j];
        const int pj = Q.perm[j];
        const bool keep = (sj > 0.0) && (sj * sj > aneg);
        Lo.p[ix(Lo.r, row) + ix(Lo.c, j)] = keep ? Es[pj * 17 + row] * (sq0 * sqrt(sj)) : 0.0;
    }
    for (int e = tid; e < r * q; e += TTN_WG) {
        const int col = e % q, j = e / q;
        const double sj = Q.sigs[j];
        const int pj = Q.perm[j];
        const bool keep = (sj > 0.0) && (sj * sj > aneg);
        Ro.p[ix(Ro.r, j) + ix(Ro.c, col)] = keep ? Ms[pj * LDQ + col] * (sq0 / sqrt(sj)) : 0.0;
    }
    if (tid == 0) { *rank_out = r; if (!conv) *Q.status_b = TTN_ST_JACOBI; }
    __syncthreads();
    return sweeps;
}

// One bond step on (core_k, core_{k+1}), 0-based k.  src/tt_tools.jl:743-768 with the effective
// _svdtrunc of src/tt_cross_interpolation.jl:149-166.
//
// With A' (p x rm), B' (rm x q) the two cores viewed as matrices (transposed roles when the merged matrix
// is tall) and M = A'B' (p <= q), three numerically distinct routes produce U sqrt(S) and sqrt(S) V^T:
//   F  (rm < p)  factored: Cholesky of A'^T A' and B' B'^T, Jacobi SVD of the rm x rm core L_A^T L_B,
//                outputs by small GEMMs; never forms M.                     [R->L steps of a sweep]
//   G  (q > p)   Gram: L = chol(M M^T), Jacobi on the columns of L.         [L->R steps]
//   H            robust: blocked Householder LQ of M (or M itself if square), Jacobi on its columns.
// F and G square the condition number, so they are taken only if sigma_max/sigma_min <= FAST_KAPPA_MAX and are
// verified a posteriori (Rf Rf^T = Sigma, Lf^T Lf = Sigma to FAST_CHECK_TOL); otherwise the step is redone by H.
// SWAP != 0 is the site-swap variant of the same step (_ttm_swap!, src/tt_operations.jl:365-382, and _swap_adjacent_sites,
// src/qtt_tools.jl:660-695; both cores have the same physical dimension here): the merged matrix takes its row index from
// (left rank, physical index of core k+1) and its column index from (physical index of core k, right rank), and the factors
// are U and S*Vt instead of U sqrt(S), sqrt(S) Vt.  Only route H is used (the swapped matrices are rank deficient by design).
// symmetric eigensolver of the Gram route (ttn_eig_kernels.h, included after this header by the translation unit)
__device__ int wg_eig128(const double* Gg, double* Vst, int r, int nev, double* sig, double* lds, int* iwork, double* dwork);
__device__ int wg_eig64(const double* Gg, int ldg, double* Vst, int r, int nev, double* sig, double* lds, int* iwork, double* dwork);

// Hand-over of the left factor between consecutive right-to-left route-F steps.  Step k stages Lf (p x r,
// column-major) in the slot's scratch; step k-1 reads that core exactly once, as its B', and then overwrites all of it.  With
// p = n2' rm' the staged matrix IS the next step's B' as a plain column-major rm' x q' matrix (ld = rm'), so the producer leaves the
// commit copy out and sets the slot's note: "core k lives in staging area note-1".  S.M is cut in three: two areas of pq/3 doubles that
// alternate (the reader's B' stays intact while it writes its own Lf, and until its commit: a fallback needs it) and the rest for the
// Rf^T of a reader that cannot store Rf straight into the (dead) core k+1.  The READER decides (wg_bond_step): a step that finds the
// note set and will not read from staging first puts the core back (wg_handover_restore), and so does one that read from staging
// and then leaves route F, before its merge.  The producer only hands over to a step of the same loop (handover_next), so no note
// outlives a launch or a train.
__device__ inline long long handover_area(const CompressArgs& P) { return (long long)P.pmax * P.qmax / 3; }
// the reader's B' (rm x q) and its own Lf (p x rk, rk <= rm) each fit an area
__device__ inline bool handover_fits(const CompressArgs& P, int p, int q, int rm) {
    const long long h = handover_area(P);
    return (long long)p * rm <= h && (long long)rm * q <= h;
}
// the step after `step` of k_compress's loop is bond k-1 on real cores
__device__ inline bool handover_next(const CompressArgs& P, int step) {
    if (P.k_single > 0) return false;
    if (P.k_single < 0) return P.k_first > P.k_last && step < P.k_first - P.k_last && !P.fused;
    const int d = P.tt.d, i = step % (2 * (d - 1));
    return i >= d - 1 && i + 1 < 2 * (d - 1);
}
__device__ inline int* handover_note(const CompressArgs& P) {      // the upper half of the slot's `perm` words (perm itself takes pmax ints)
    double* scr = P.scratch + (long long)blockIdx.x * P.scratch_stride;
    const long long pq = (long long)P.pmax * P.qmax;
    double* sigs = scr + 2 * pq + (long long)QR_NB * P.qmax + (long long)P.pmax * QR_NB + 2LL * P.pmax * P.pmax + P.pmax;
    return reinterpret_cast<int*>(sigs + P.pmax) + P.pmax;
}
// core[s2, ga, be] = stage[(ga + rm s2) + n2 rm be]: the commit copy the producer left out; clears the note
__device__ __noinline__ void wg_handover_restore(double* core, const double* stage, int n2, int rm, int Dr, int* note) {
    core = unip(core); stage = unip(stage); n2 = uni32(n2); rm = uni32(rm); Dr = uni32(Dr); note = unip(note);
    __syncthreads();
    wg_copy_to_view(mkview(core, Idx{rm, (long long)n2, 1}, plain((long long)n2 * rm)), stage, n2 * rm, Dr, 1, (long long)n2 * rm, Dr, 1);
    if (threadIdx.x == 0) *note = 0;
    __syncthreads();
}

// SCALE_SAFE (ttn_common.h), out of line so that the bond step's own body gains one call at each end and no live value.
// wg_scale_takeout: the n contiguous doubles of M divided by 2^e in place when amax = max|M| is outside the safe range (e even if
// `even`); e is left in *keep, an LDS word, and max|M| after the division is returned.  Inside the range: e = 0, nothing is touched.
__device__ __noinline__ double wg_scale_takeout(double* M, long long n, double amax, int even, double* keep) {
    M = unip(M); n = uni64(n); keep = unip(keep); amax = unif64(amax);
    const int e = uni32(scale_rescue_exponent(amax, even != 0));
    if (threadIdx.x == 0) *keep = (double)e;
    if (e == 0) return amax;
    __syncthreads();
    wg_copy_scale(M, M, n, ldexp(1.0, -e));
    __syncthreads();
    return ldexp(amax, -e);
}
// wg_scale_giveback: the power of two a step took out (*keep) goes back into its outputs — half of it into each core (tt_compress!:
// U sqrt(S), sqrt(S) Vt; per_rank doubles of a core for each of the *rank kept directions), or all of it into core k+1 (swap:
// S Vt) — and into the captured singular values (sv: p of them, or null).  *keep = 0 or *rank <= 0: nothing is touched.
__device__ __noinline__ void wg_scale_giveback(double* ck, long long per_rank_k, double* ck1, long long per_rank_k1, const long long* rank,
                                               const double* keep, int swap, double* sv, int p) {
    ck = unip(ck); per_rank_k = uni64(per_rank_k); ck1 = unip(ck1); per_rank_k1 = uni64(per_rank_k1); rank = unip(rank); keep = unip(keep);
    swap = uni32(swap); sv = unip(sv); p = uni32(p);
    const int e = uni32((int)*keep);
    if (e == 0) return;
    const long long rr = uni64(*rank);
    if (rr <= 0) return;
    if (!swap) wg_copy_scale(ck, ck, per_rank_k * rr, ldexp(1.0, e / 2));
    wg_copy_scale(ck1, ck1, per_rank_k1 * rr, ldexp(1.0, swap ? e : e / 2));
    if (sv) for (int i = threadIdx.x; i < p; i += TTN_WG) sv[i] = ldexp(sv[i], e);
    __syncthreads();
}

struct BondIO {
    double *ck, *ck1;            // the two cores (slots)
    int n1, n2, Dl, rm, Dr;      // physical dimensions and the three ranks
    long long* rank_out;         // receives the new middle rank (SWAP: -1 if it exceeds `cap`; nothing is written then)
    int cap;                     // SWAP only: largest middle rank the two slots can hold
};
template <int SWAP>
__device__ __forceinline__ void wg_bond_step_io(const CompressArgs& P, int b, const BondIO& io, int k, int step, double* lds, bool virt) {
    const int tid = threadIdx.x;
    const int n1 = io.n1, n2 = io.n2;
    const int Dl = io.Dl, rm = io.rm, Dr = io.Dr;
    const int mr = n1 * Dl, mc = n2 * Dr;
    double* ck = io.ck;
    double* ck1 = io.ck1;
    // A_mat[(al + Dl*s1), ga] = core_k[s1, al, ga] ; B_mat[ga, (s2 + n2*be)] = core_{k+1}[s2, ga, be]
    const View Am = mkview(ck, Idx{Dl, (long long)n1, 1}, plain((long long)n1 * Dl));
    const View Bm = mkview(ck1, plain(n2), Idx{n2, 1, (long long)n2 * rm});
    const bool wide = mr <= mc;
    const int p = wide ? mr : mc, q = wide ? mc : mr;
    const View Ap = wide ? Am : tview(Bm);       // p x rm
    const View Bp = wide ? Bm : tview(Am);       // rm x q

    BondCtx S;
    S.ldsX = lds;                                         // COMPRESS_LDS_X_DOUBLES (aliases the GEMM tiles)
    S.red = lds + GEMM_LDS_TOTAL;                         // 32 (the GEMM descriptor sits right behind the X region)
    S.Ts = S.red + 32;                                    // QR_NB*QR_NB
    S.Ss = S.Ts + QR_NB * QR_NB;                          // QR_NB*QR_NB
    S.taus = S.Ss + QR_NB * QR_NB;                        // QR_NB
    S.scal = S.taus + QR_NB;                              // 8 misc doubles (scal[0] = Jacobi's negligible threshold)
    S.iflag = reinterpret_cast<int*>(S.scal + 8);         // 8 ints
    S.nrm2 = S.scal + 16;                                 // 128 cached squared column norms
    // scratch belongs to the WORKGROUP SLOT, not to the train: a persistent grid (k_compress with a train counter) reuses the slot for
    // every train the workgroup pulls, so the hot footprint is #slots x per_slot whatever the batch size (every other caller
    // launches one workgroup per train: blockIdx.x == b there)
    double* scr = P.scratch + (long long)blockIdx.x * P.scratch_stride;
    const long long pq = (long long)P.pmax * P.qmax;
    S.M = scr;                                            // p x q row-major
    S.M2 = S.M + pq;                                      // copy for LQ (F path: Lf/Rf staging uses M..M2)
    S.Vb = S.M2 + pq;                                     // QR_NB x qmax
    S.Wb = S.Vb + (long long)QR_NB * P.qmax;              // pmax x QR_NB
    S.Us = S.Wb + (long long)P.pmax * QR_NB;              // pmax x pmax
    S.Xg = S.Us + (long long)P.pmax * P.pmax;             // pmax x pmax Jacobi fallback when LDS is too small
    S.sig = S.Xg + (long long)P.pmax * P.pmax;            // pmax
    S.sigs = S.sig + P.pmax;                              // pmax
    S.perm = reinterpret_cast<int*>(S.sigs + P.pmax);     // pmax ints
    S.Ga = S.sigs + 2 * P.pmax;                           // 6 x (128 x 128) fast-path matrices
    S.Gb = S.Ga + 128 * 128;
    S.Cc = S.Gb + 128 * 128;
    S.T1 = S.Cc + 128 * 128;
    S.T2 = S.T1 + 128 * 128;
    S.T3 = S.T2 + 128 * 128;
    if (pq >= 3 * 128 * 128) {
        // the Gram matrix, the reflector store and the check matrix take the place of the fused merge's T buffer / the LQ copy
        // (dead by the time they are written): 288 KB less footprint per train, and the lines are warm
        S.Ga = S.M2; S.Gb = S.M2 + 128 * 128; S.T2 = S.M2 + 2 * 128 * 128;
    }

    // fused apply: the right core is still A_{k+1} x_{k+1}.  Wide steps with r_mid >= p get the fused merge below; the
    // others (first steps of the ramp that are tall, tiny cores) write the core out first and proceed as usual.
    bool virt_live = false;
    if (virt) {
        if (wide && rm >= p) virt_live = true;
        else wg_materialize_core(P, b, k + 1);
    }

    const View Lfv = mkview(ck, Idx{Dl, (long long)n1, 1}, plain((long long)n1 * Dl));     // (mr x r)
    int nsw_total = 0;
    bool done = false;

    // =============================== route F: factored ===============================
    if (SWAP == 0 && P.fast && rm < p && rm <= TTN_LDS_COLS && rm >= 2) {
        // scales
        double sa = 0.0, sb = 0.0;
        sa = wg_absmax(ck, (long long)n1 * Dl * rm, S.red);
        // Handed over (the slot's note is 1 or 2; wg_bond_step has checked that this step is wide, on real cores and that the areas
        // fit): B' is the plain column-major rm x q matrix in that staging area, the left factor as the step before staged it.  The
        // note is READ AGAIN wherever it matters instead of being kept, and the two-team calls take the alternative operand next to the
        // usual one (they store it over the descriptor): a view chosen at run time, field by field, is what the register budget of
        // k_compress cannot take (64 more spilled VGPRs).
#define HANDOVER_PEND() ((SWAP == 0) ? uni32(*handover_note(P)) : 0)
#define HANDOVER_BS(pn) mkview(S.M + ((pn) == 2 ? handover_area(P) : 0), plain(1), plain(rm))       /* the staged B' (pn != 0) */
#define HANDOVER_B(pn) ((pn) ? HANDOVER_BS(pn) : Bp)
        { const int pn = HANDOVER_PEND(); sb = wg_absmax(pn ? S.M + (pn == 2 ? handover_area(P) : 0) : ck1, (long long)n2 * rm * Dr, S.red); }      // (the same set of numbers)
        // (1 / (sA sA), 1 / (sB sB) and the squares behind them, s0 = sA sB in the rank rule: in range or the step is the general one's)
        bool ok = scale_safe(sa) && scale_safe(sb) && scale_safe(sa * sb);
        const double sA = wide ? sa : sb, sB = wide ? sb : sa;       // scale of A', B'
        const double s0 = sA * sB;
        const View Gav = mkview(S.Ga, plain(1), plain(128));
        const View Gbv = mkview(S.Gb, plain(1), plain(128));
        const View Ccv = mkview(S.Cc, plain(1), plain(128));
        bool diagA = false;
        if (ok) {
            // A'^T A' and B' B'^T: independent, one two-team call (two wg_syrk calls where rm > 64)
            { const int pn = HANDOVER_PEND(); wg_syrk2(rm, p, tview(Ap), Gav, 1.0 / (sA * sA), rm, q, Bp, Gbv, 1.0 / (sB * sB), lds, pn, HANDOVER_BS(pn)); }
            // A' = U D^(1/2) with orthonormal U (the left core of a bond step is left as U sqrt(S) by the step before it, so every
            // R->L step of a sweep that follows an L->R sweep sees this): then M = U (D^(1/2) B') and the SVD of M is U times the SVD
            // of the rm x q matrix N = D^(1/2) B' — no Cholesky factors, no core matrix, two output GEMMs instead of five.
            // Detected, not assumed: |G_ij| <= FAST_DIAG_TOL sqrt(G_ii G_jj) for every off-diagonal entry of A'^T A'.
            if (rm == 64 && !(P.fast & 4) && !(P.fast & 8)) {
                const double wmax = wg_diag_test_t3(S.Ga, S.Gb, S.T3, S.Ss, S.red);      // (T3 = D^(1/2) (B' B'^T) D^(1/2), used if the test passes)
                diagA = wmax <= FAST_DIAG_TOL;
            }
            if (diagA) {
                // (the Gram matrix of N = D^(1/2) B', D^(1/2) (B' B'^T) D^(1/2), is in T3 already)
            } else if (rm <= TTN_LDS_COLS / 2) {
                // both Cholesky factorisations at once, one per half of the workgroup (wg_chol2_lds128)
                for (int e = tid; e < rm * 128; e += TTN_WG) if ((e & 127) < rm) { S.ldsX[e] = S.Ga[e]; S.ldsX[TTN_LDS_IMG / 2 + e] = S.Gb[e]; }
                __syncthreads();
                ok = wg_chol2_lds128(rm, S.ldsX, S.Ts, S.iflag, S.scal + 1) == 0;     // Ts: 256 doubles of LDS, free here
                for (int e = tid; e < rm * 128; e += TTN_WG) if ((e & 127) < rm) { S.Ga[e] = S.ldsX[e]; S.Gb[e] = S.ldsX[TTN_LDS_IMG / 2 + e]; }
                __syncthreads();
            } else {
                // L_A
                for (int e = tid; e < rm * 128; e += TTN_WG) if ((e & 127) < rm) S.ldsX[e] = S.Ga[e];
                __syncthreads();
                ok = wg_chol_lds128(rm, S.ldsX, S.red, S.iflag, S.scal + 1) == 0;
                for (int e = tid; e < rm * 128; e += TTN_WG) if ((e & 127) < rm) S.Ga[e] = S.ldsX[e];
                __syncthreads();
                if (ok) {
                    for (int e = tid; e < rm * 128; e += TTN_WG) if ((e & 127) < rm) S.ldsX[e] = S.Gb[e];
                    __syncthreads();
                    ok = wg_chol_lds128(rm, S.ldsX, S.red, S.iflag, S.scal + 1) == 0;
                    for (int e = tid; e < rm * 128; e += TTN_WG) if ((e & 127) < rm) S.Gb[e] = S.ldsX[e];
                    __syncthreads();
                }
            }
        }
        int r = 0, rk = 0;
        if (ok) {
            int nsw = 1;
            if (diagA) {
                ok = wg_eig64(S.T3, 128, S.T2, 64, 64, S.sigs, lds, reinterpret_cast<int*>(S.Ts), S.Ts + 64) == 0;
                for (int j = tid; j < 64; j += TTN_WG) S.perm[j] = j;
                if (tid == 0) S.scal[0] = 64.0 * DBL_EPSILON * DBL_EPSILON * S.sigs[0] * S.sigs[0];
                __syncthreads();
            } else {
            // core C = L_A^T L_B  (rm x rm)
            wg_gemm(rm, rm, rm, tview(Gav), Gbv, Ccv, 1.0, 0.0, lds);
            if (rm == 64 && !(P.fast & 4)) {
                // the 64 x 64 core through the symmetric eigensolver: C C' = U S^2 U' gives the same image x_j = sigma_j u_j the
                // Jacobi on the columns of C leaves (ttn_eig_kernels.h; the a-posteriori check below covers the squared condition)
                wg_gemm(64, 64, 64, Ccv, tview(Ccv), mkview(S.T3, plain(1), plain(128)), 1.0, 0.0, lds);
                ok = wg_eig64(S.T3, 128, S.T2, 64, 64, S.sigs, lds, reinterpret_cast<int*>(S.Ts), S.Ts + 64) == 0;
                for (int j = tid; j < 64; j += TTN_WG) S.perm[j] = j;
                if (tid == 0) S.scal[0] = 64.0 * DBL_EPSILON * DBL_EPSILON * S.sigs[0] * S.sigs[0];
                __syncthreads();
            } else {
                for (int e = tid; e < rm * 128; e += TTN_WG) { const int c = e >> 7, r_ = e & 127; S.ldsX[e] = (r_ < rm) ? S.Cc[c * 128 + r_] : 0.0; }
                __syncthreads();
                nsw = uni32(wg_svd_cols(P, S, rm, S.ldsX, 128, true));
                nsw_total += (nsw < 0 ? -nsw : nsw);
            }
            }
            ok = ok && (nsw > 0) && (S.sigs[rm - 1] * FAST_KAPPA_MAX >= S.sigs[0]) && (S.sigs[rm - 1] * S.sigs[rm - 1] > S.scal[0]);
        }
        if (ok) {
            r = wg_rank_rule(P, S, rm, p, s0);
            rk = r < rm ? r : rm;                                           // columns that carry data
            // X_s[:, j] = x_j * (sqrt(s0)/sA) / sigma_j^2.5 -> T1 ;  X_t[:, j] = x_j * (sqrt(s0)/sB) / sigma_j^1.5 -> T2
            const double fa = sqrt(s0) / sA, fb = sqrt(s0) / sB;
            if (diagA) {
                // x_j = sigma_j w_j (w_j: left singular vector of N).  Lf = A' (D^(-1/2) w_j sqrt(s0 sigma_j) / sA),
                // Rf = (D^(1/2) w_j sqrt(s0) / (sB sqrt(sigma_j)))^T B'
                wg_scale_t12_diag(S.ldsX, S.sigs, S.perm, S.Ga, S.T1, S.T2, rk, fa, fb, S.Ts);
            } else {
                for (int e = tid; e < rm * rk; e += TTN_WG) {
                    const int row = e % rm, j = e / rm;
                    const double sj = S.sigs[j], xv = S.ldsX[S.perm[j] * 128 + row];
                    const double rs = sqrt(sj);
                    S.T1[j * 128 + row] = xv * (fa / (sj * sj * rs));
                    S.T2[j * 128 + row] = xv * (fb / (sj * rs));
                }
                __syncthreads();
            }
            const View T1v = mkview(S.T1, plain(1), plain(128));
            const View T2v = mkview(S.T2, plain(1), plain(128));
            // Lf goes to the staging area that does not hold this step's B'.  B' read from staging: core k+1 holds nothing live, Rf
            // goes straight into it unless zero rows have to follow (a step that leaves route F gets B' put back over it)
#define HANDOVER_LFT(pn) (S.M + ((pn) == 1 ? handover_area(P) : 0))                                  /* p x rk, column-major (ld = p) */
#define HANDOVER_RFT(pn) ((pn) ? S.M + 2 * handover_area(P) : S.M + (long long)p * rk)              /* rk x q, row-major (ld = q) */
#define HANDOVER_RFS(pn) mkview(HANDOVER_RFT(pn), plain(q), plain(1))                                /* Rf^T staged */
#define HANDOVER_RFC() mkview(ck1, plain(n2), Idx{n2, 1, (long long)n2 * r})                         /* Rf in core k+1 (pn != 0, rk == r) */
#define HANDOVER_RF(pn) (((pn) && rk == r) ? HANDOVER_RFC() : HANDOVER_RFS(pn))
            const int pn = HANDOVER_PEND();
            const View Lft = mkview(HANDOVER_LFT(pn), plain(1), plain(p));
            const View Rft = HANDOVER_RF(pn);
            // the operands of the two-team calls below that depend on the hand-over, left in LDS by thread 0 for itself (S.taus is
            // the Householder route's): B' and where Rf goes
            View* hv = reinterpret_cast<View*>(S.taus);
            static_assert(2 * sizeof(View) <= QR_NB * sizeof(double), "two views in S.taus");
            if (tid == 0) { hv[0] = HANDOVER_B(pn); hv[1] = Rft; }
            if (diagA) {
                // Lf^T = T1^T A'^T and Rf = T2^T B': the short operands in registers, both products in one two-team call
                wg_gemm_ra2(rk, p, rm, tview(T1v), tview(Ap), tview(Lft), 1.0, rk, q, rm, tview(T2v), Bp, mkview(S.M + (long long)p * rk, plain(q), plain(1)), 1.0, lds, hv);
            } else {
            // Lf = A' * (L_B * (C^T * X_s))     (ldsX is free again: use it as the second temporary)
            wg_gemm(rm, rk, rm, tview(Ccv), T1v, mkview(S.T3, plain(1), plain(128)), 1.0, 0.0, lds);
            wg_gemm(rm, rk, rm, Gbv, mkview(S.T3, plain(1), plain(128)), T1v, 1.0, 0.0, lds);
            wg_gemm(p, rk, rm, Ap, T1v, Lft, 1.0, 0.0, lds);
            // Rf = (L_A * X_t)^T * B'
            wg_gemm(rm, rk, rm, Gav, T2v, mkview(S.T3, plain(1), plain(128)), 1.0, 0.0, lds);
            wg_gemm(rk, q, rm, tview(mkview(S.T3, plain(1), plain(128))), HANDOVER_B(pn), Rft, 1.0, 0.0, lds);
            }
            // a-posteriori check: Lf^T Lf = Sigma, Rf Rf^T = Sigma
            { const int pc = HANDOVER_PEND();
              wg_syrk2(rk, p, tview(mkview(HANDOVER_LFT(pc), plain(1), plain(p))), mkview(S.T1, plain(1), plain(128)), 1.0, rk, q, mkview(S.M + (long long)p * rk, plain(q), plain(1)), mkview(S.T2, plain(1), plain(128)), 1.0, lds,
                       0, View{}, reinterpret_cast<const View*>(S.taus) + 1); }
            ok = wg_check_diag_tab2(S.sigs, S.T1, S.T2, 128, rk, s0, S.Ts, S.red) <= FAST_CHECK_TOL;       // both checks, one pass
            if ((P.fast & 32) && HANDOVER_PEND()) ok = false;               // diagnostic: the restore path
            if (ok) {
                if (P.sv_out && step < P.sv_steps) {
                    double* so = P.sv_out + ((long long)b * P.sv_steps + step) * P.pmax;
                    for (int i = tid; i < P.pmax; i += TTN_WG) so[i] = (i < rm) ? S.sigs[i] * s0 : (i < p ? 0.0 : -1.0);
                }
                // commit: cores are overwritten only now
                const View Rfv = mkview(ck1, plain(n2), Idx{n2, 1, (long long)n2 * r});
                const View Lo = wide ? Lfv : tview(Rfv);       // p x r
                const View Ro = wide ? Rfv : tview(Lfv);       // r x q
                // the next step can take Lf from its staging area: no copy into core k (wg_bond_step reads the note)
                const bool hand = SWAP == 0 && wide && rk == r && handover_next(P, step);
                const int pc = HANDOVER_PEND();
                __syncthreads();
                if (!hand) wg_copy_to_view(Lo, HANDOVER_LFT(pc), p, r, 1, p, rk, 1);               // Lo[row, j] = LfT[row + p j], columns j >= rk zero
                if (!(pc && rk == r)) wg_copy_to_view(Ro, HANDOVER_RFT(pc), r, q, q, 1, rk, 0);    // Ro[j, col] = RfT[j q + col], rows j >= rk zero
                if (tid == 0) { *io.rank_out = r; if (pc || hand) *handover_note(P) = hand ? (pc == 1 ? 2 : 1) : 0; }
                __syncthreads();
                done = true;
            }
        }
    }

    if (!done) {
        // read B' from staging and leaves route F: the core back in its slot first (the merge writes S.M; core k+1 held nothing live,
        // Rf at most).  core[s2, ga, be] = stage[(ga + rm s2) + n2 rm be], as wg_handover_restore
        if (const int pn = HANDOVER_PEND()) {
            const double* stage = S.M + (pn == 2 ? handover_area(P) : 0);
            __syncthreads();
            for (int e = tid; e < n2 * rm * Dr; e += TTN_WG) { const int s2 = e % n2, ga = (e / n2) % rm, be = e / (n2 * rm); ck1[e] = stage[ga + rm * s2 + n2 * rm * be]; }
            if (tid == 0) *handover_note(P) = 0;
            __syncthreads();
        }
#undef HANDOVER_PEND
#undef HANDOVER_B
#undef HANDOVER_BS
#undef HANDOVER_RFS
#undef HANDOVER_RFC
#undef HANDOVER_LFT
#undef HANDOVER_RFT
#undef HANDOVER_RF
        // ---- merge: M = A' * B'  (p x q), scaled to max|M| = 1 ----
        const View Mv = mkview(S.M, plain(q), plain(1));
        // M stays UNSCALED in memory: max|M| comes out of the GEMM epilogue and the consumers (Gram, LQ copy, output GEMM)
        // apply 1/s0 as their alpha — no extra read-modify-write pass over the p x q matrix.
        bool merged = false;
        if (virt_live) {
            merged = wg_fused_merge(P, b, k, p, q, Am, S.M, S.M2, pq, lds, S.scal + 6, S.red);
            if (!merged) wg_materialize_core(P, b, k + 1);
        }
        double mx_swap = 0.0;
        if (SWAP != 0) {
            // M[(m + Dl*sB), (sA + n1*nn)] = sum_a core_k[sA, m, a] * core_{k+1}[sB, a, nn]: one Dl x Dr x rm product per (sA, sB),
            // written into its strided block of M (transposed when the merged matrix is tall)
            for (int sA = 0; sA < n1; ++sA)
                for (int sB = 0; sB < n2; ++sB) {
                    const View Av = mkview(ck + sA, plain(n1), plain((long long)n1 * Dl));          // Dl x rm
                    const View Bv = mkview(ck1 + sB, plain(n2), plain((long long)n2 * rm));         // rm x Dr
                    if (wide) wg_gemm(Dl, Dr, rm, Av, Bv, mkview(S.M + (long long)Dl * sB * q + sA, plain(q), plain(n1)), 1.0, 0.0, lds, S.scal + 6);
                    else wg_gemm(Dr, Dl, rm, tview(Bv), tview(Av), mkview(S.M + (long long)sA * q + (long long)Dl * sB, plain((long long)n1 * q), plain(1)), 1.0, 0.0, lds, S.scal + 6);
                    mx_swap = fmax(mx_swap, unif64(S.scal[6]));
                    __syncthreads();
                }
        } else if (!merged) wg_gemm(p, q, rm, Ap, Bp, Mv, 1.0, 0.0, lds, S.scal + 6);
        // max|M| outside SCALE_SAFE: M / 2^e in place (e even, so that the sqrt(S) split of the outputs is exact too); the step then runs
        // on a matrix of size 1 and its outputs get the power back at the end (the exponent waits in S.scal[7])
        const double mx = wg_scale_takeout(S.M, (long long)p * q, (SWAP != 0) ? mx_swap : unif64(S.scal[6]), 1, S.scal + 7);
        const double s0 = (mx > 0.0) ? mx : 1.0;
        const double inv_s0 = 1.0 / s0;
        const bool need_lq = q > p;
        const bool x_in_lds = p <= TTN_LDS_COLS;              // fast Jacobi: X in LDS with leading dimension 128
        double* X = x_in_lds ? S.ldsX : S.Xg;
        int ldx = x_in_lds ? 128 : p;

        // small merged matrices (the rank-ramp steps) fit the LDS whole: their Householder LQ needs no GEMM calls and costs
        // about what the Gram + Cholesky do, without the conditioning gamble — route H directly
        const bool lq_in_lds = (long long)p * q <= GEMM_LDS_DOUBLES || GEMM_LDS_DOUBLES / p >= 2 * p;     // whole, or TSQR chunks (wg_lq_blocked)
        const bool eig_ok = SWAP == 0 && P.fast && !(P.fast & 2) && need_lq && ((p > 64 && p <= 128 && P.max_bond <= 64) || (p == 64 && P.max_bond < 64));
        // (the eigensolver leaves its image — at most 64 columns — in LDS whatever p is; the Cholesky + Jacobi form needs the whole L there)
        // CholeskyQR2 (above) instead of the Householder LQ when the plain Gram route finds the matrix too ill-conditioned for itself
        // (only where the Householder LQ cannot keep the whole matrix in LDS — 64 x 384, 32 x 384: there it wins 3x; against the in-LDS
        // LQ of a 64 x 128 step it is a draw, and the R->L ramp matrices are often too ill-conditioned for it anyway)
        const bool cholqr_ok = SWAP == 0 && P.fast && need_lq && x_in_lds && p >= 16 && p <= 64 && (long long)p * q > GEMM_LDS_DOUBLES;
        for (int attempt = (SWAP == 0 && P.fast && need_lq && (eig_ok || cholqr_ok || (x_in_lds && !lq_in_lds)) && p >= 2) ? 1 : 2; attempt <= 2 && !done; ++attempt) {
            bool ok = true;
            bool use_eig = false;
            bool cholqr = false;
            double gram_trace = 0.0;
            X = (x_in_lds || attempt == 1) ? S.ldsX : S.Xg;
            ldx = (x_in_lds || attempt == 1) ? 128 : p;
            if (attempt == 1) {
                // =========================== route G: L = chol(M M^T) ===========================
                wg_syrk(p, q, Mv, mkview(S.Ga, plain(1), plain(128)), inv_s0 * inv_s0, lds);
                // p = 128 with at most 64 vectors kept (the L->R steps of the benchmark sweep): eigen-decomposition of the Gram
                // matrix itself — tridiagonalisation, bisection, twisted factorisations (ttn_eig_kernels.h) — instead of
                // Cholesky + Jacobi on L; same outputs (sigs, perm, X = sigma_j u_j in LDS), same a-posteriori check below
                use_eig = eig_ok;
                if (use_eig) {
                    if (p > 64 && p < 128) {             // 64 < p < 128: the Gram matrix zero-padded to the 128-row solver (the padding adds
                        for (int e = tid; e < 128 * 128; e += TTN_WG)      // exact zero eigenvalues below the wanted ones)
                            if ((e & 127) >= p || (e >> 7) >= p) S.Ga[e] = 0.0;
                        __syncthreads();
                    }
                    const int r0 = (int)P.max_bond;
                    const int nev = (P.truncerr > 0.0 || (P.sv_out && step < P.sv_steps)) ? p : r0;
                    // trace of the Gram matrix = sum of ALL squared singular values: the polish branch below needs the weight of
                    // the part it drops (the solver only computes the kept eigenvalues)
                    { double t_ = 0.0; for (int i = tid; i < p; i += TTN_WG) t_ += S.Ga[i * 129]; gram_trace = unif64(wg_sum(t_, S.red)); }
                    ok = ((p == 64) ? wg_eig64(S.Ga, 128, S.Gb, r0, nev, S.sigs, lds, reinterpret_cast<int*>(S.Ts), S.Ts + 64)
                                    : wg_eig128(S.Ga, S.Gb, r0, nev, S.sigs, lds, reinterpret_cast<int*>(S.Ts), S.Ts + 64)) == 0;
                    for (int j = tid; j < p; j += TTN_WG) { S.perm[j] = j; if (j >= nev) S.sigs[j] = 0.0; }      // (sigs / perm hold pmax entries)
                    if (tid == 0) S.scal[0] = (double)p * DBL_EPSILON * DBL_EPSILON * S.sigs[0] * S.sigs[0];
                    __syncthreads();
                } else {
                wg_img_load(S.ldsX, 0, S.Ga, p, S.red);
                ok = wg_chol_lds128(p, S.ldsX, S.red, S.iflag, S.scal + 1) == 0;
                // with truncerr > 0 the rank rule reads the SMALL singular values too: need cond(M) <= kappa_max overall;
                // likewise when nothing will be truncated (p <= max_bond: every singular value is kept): the pivot ratio is a lower
                // bound of cond(M)^2, so a value above the limit means the a-posteriori test WILL fail — take the factor from
                // CholeskyQR2 (the rank-ramp steps of a sweep are such steps), or go to Householder now instead of after a wasted Jacobi
                // The pivot ratio is only a LOWER bound of cond(M)^2 (unpivoted: orders of magnitude low on the R->L ramp matrices), so a
                // step that may take CholeskyQR2 always does: its second pass measures the conditioning itself.
                if (ok && (P.truncerr > 0.0 || (long long)p <= P.max_bond)) {
                    if (cholqr_ok) { if (unif64(S.scal[1]) <= CHOLQR_PIVOT_MAX) cholqr = true; else ok = false; }
                    else if (unif64(S.scal[1]) > FAST_KAPPA_MAX * FAST_KAPPA_MAX) ok = false;
                }
                if (cholqr) {
                    for (int e = tid; e < p * p; e += TTN_WG) { const int i = e % p, j = e / p; S.T1[i + 128 * j] = S.ldsX[i + 128 * j]; }       // L1 (the GEMM below takes the image)
                    wg_trsm_lower_cols(p, q, S.ldsX, S.M, q, inv_s0, S.M2, q);                                                           // Q1 = L1^-1 M / s0
                    const View Q1v = mkview(S.M2, plain(q), plain(1));
                    wg_syrk(p, q, Q1v, mkview(S.Cc, plain(1), plain(128)), 1.0, lds);
                    // Q1 Q1^T = I + E, |E| ~ eps cond(M)^2: the route needs |E| << 1 (CHOLQR_ORTH_MAX), else Householder
                    const double dev = wg_img_load(S.ldsX, 0, S.Cc, p, S.red);
                    ok = dev <= CHOLQR_ORTH_MAX && wg_chol_lds128(p, S.ldsX, S.red, S.iflag, S.scal + 1) == 0;
                    if (ok) {
                        wg_img_load(S.ldsX, 64, S.T1, p, S.red);
                        wg_tril_mul_lds(p, S.ldsX);
                    }
                }
                for (int e = tid; e < p * 128; e += TTN_WG) if ((e & 127) >= p) S.ldsX[e] = 0.0;      // zero row padding for the Jacobi
                __syncthreads();
                }
            } else {
                // =========================== route H: Householder LQ ===========================
                if (need_lq) {
                    wg_copy_scale(S.M2, S.M, (long long)p * q, inv_s0);
                    __syncthreads();
                    wg_lq_blocked(p, q, S.M2, q, S.Vb, S.Wb, nullptr, nullptr, lds, S.Ts, S.Ss, S.taus, S.red);
                }
                const double* Lsrc = need_lq ? S.M2 : S.M;               // row-major, ld = q
                // columns of L in order of decreasing norm (de Rijk): the rank-deficient L of the ramp steps converges in
                // fewer sweeps that way; any column order is fine for the caller (wg_svd_cols sorts by sigma anyway)
                if (need_lq && x_in_lds) {
                    const int lane_ = tid & 63, wave_ = tid >> 6;
                    for (int c = wave_; c < p; c += TTN_NWAVES) {
                        double a = 0.0;
                        for (int r_ = c + lane_; r_ < p; r_ += 64) { const double v = Lsrc[(long long)r_ * q + c]; a = fma(v, v, a); }
                        a = wave_sum(a);
                        if (lane_ == 0) S.sig[c] = a;
                    }
                    __syncthreads();
                    for (int c = tid; c < p; c += TTN_WG) {
                        const double sc = S.sig[c];
                        int pos = 0;
                        for (int j = 0; j < p; ++j) { const double sj = S.sig[j]; pos += (sj > sc) || (sj == sc && j < c); }
                        S.perm[c] = pos;                                    // column c of L goes to position pos
                    }
                    __syncthreads();
                }
                const bool presort = need_lq && x_in_lds;
                for (int e = tid; e < p * ldx; e += TTN_WG) {
                    const int r_ = e % ldx, c = e / ldx;              // X[r + ldx*c] = L[r][c]; rows >= p are zero padding
                    const double v = (r_ < p) ? Lsrc[(long long)r_ * q + c] * (need_lq ? 1.0 : inv_s0) : 0.0;
                    const int cd = presort ? S.perm[c] : c;
                    X[(long long)cd * ldx + r_] = (need_lq && c > r_) ? 0.0 : v;
                }
                __syncthreads();
            }
            int nsw = 0;
            if (ok && !(attempt == 1 && use_eig)) {
                nsw = uni32(wg_svd_cols(P, S, p, X, ldx, x_in_lds));
                nsw_total += (nsw < 0 ? -nsw : nsw);
                if (attempt == 1) ok = nsw > 0;
                else if (nsw < 0 && tid == 0) ttn_set_status(&P.status[b], TTN_ST_JACOBI);
            }
            if (!ok) continue;
            const int r = wg_rank_rule(P, S, p, p, s0);
            if (SWAP != 0 && r > io.cap) {                                  // would not fit the slots: report, write nothing
                if (tid == 0) { ttn_set_status(&P.status[b], TTN_ST_RANK_OVERFLOW); *io.rank_out = -1; }
                __syncthreads();
                done = true;
                continue;
            }
            if (attempt == 1 && !cholqr) {
                // Gram route: the KEPT block must be well conditioned (error ~ eps*kappa^2, verified below); the discarded
                // singular values only matter to the rank rule, i.e. when truncerr > 0 (then all of them must qualify).
                const int rl = (P.truncerr > 0.0) ? p : r;
                if (__builtin_expect(!((S.sigs[rl - 1] * FAST_KAPPA_MAX >= S.sigs[0]) && (S.sigs[rl - 1] * S.sigs[rl - 1] > S.scal[0])), 0)) {
                    // Moderately ill-conditioned kept block and everything kept fits the LDS image: POLISH instead of starting over.
                    // The eigenvectors U of the Gram matrix span the dominant subspace up to an angle theta ~ eps kappa^2 / relgap; the
                    // r x q matrix B = U^T M is then nearly row-orthogonal, and a one-sided Jacobi on its rows (2-3 sweeps) delivers the
                    // singular values and right vectors of M restricted to that subspace to Jacobi accuracy; the left vectors follow as
                    // M v / sigma — one step of subspace iteration, so the product of the two outputs is M projected on the computed
                    // right vectors and the singular values are off by theta^2 / 2 only (<= 5e-11 at FAST_KAPPA_POLISH).
                    // That bound needs a GAP behind the kept block: the error of the product is theta * sigma_{r+1} / sigma_1, so the
                    // branch is taken only when what it drops is noise — dropped weight trace(G) - sum of the kept eigenvalues at most
                    // FAST_POLISH_DROP of the trace (sigma_{r+1} <= 1e-6 sigma_1: relgap = 1, theta <= eps kappa^2 = 1e-7, product
                    // error <= 1e-13).  The rank-deficient ramp step of a sweep that was just truncated on its other bond is such a
                    // step (its dropped part is rounding noise); a matrix with a smooth spectrum goes to the Householder route.
                    bool polish = use_eig && SWAP == 0 && !(P.fast & 16) && P.truncerr == 0.0 && q <= 128 && r <= 64 && r >= 2 &&
                                  (S.sigs[r - 1] * FAST_KAPPA_POLISH >= S.sigs[0]) && (S.sigs[r - 1] * S.sigs[r - 1] > S.scal[0]);
                    if (polish) {
                        double kept = 0.0;
                        for (int j = tid; j < r; j += TTN_WG) kept = fma(S.sigs[j], S.sigs[j], kept);
                        kept = unif64(wg_sum(kept, S.red));
                        polish = (gram_trace - kept) <= FAST_POLISH_DROP * gram_trace;
                    }
                    if (!polish) continue;
                    const double aneg0 = S.scal[0];
                    for (int e = tid; e < p * r; e += TTN_WG) {
                        const int row = e % p, j = e / p;
                        const double sj = S.sigs[j], xv = X[(long long)S.perm[j] * ldx + row];
                        S.Us[(long long)j * p + row] = ((sj > 0.0) && (sj * sj > aneg0)) ? xv / sj : 0.0;
                    }
                    __syncthreads();
                    wg_gemm_ra(r, q, p, mkview(S.Us, plain(p), plain(1)), Mv, mkview(S.M2, plain(q), plain(1)), inv_s0, lds);
                    for (int e = tid; e < r * 128; e += TTN_WG) { const int c = e & 127, j = e >> 7; S.ldsX[e] = (c < q) ? S.M2[(long long)j * q + c] : 0.0; }
                    __syncthreads();
                    const int nsp = uni32(wg_svd_cols(P, S, r, S.ldsX, 128, true, q));
                    nsw_total += (nsp < 0 ? -nsp : nsp);
                    if (nsp <= 0) continue;                                     // not converged: Householder route (M is intact)
                    const View Rfv = mkview(ck1, plain(n2), Idx{n2, 1, (long long)n2 * r});
                    const View Lo = wide ? Lfv : tview(Rfv);       // p x r
                    const View Ro = wide ? Rfv : tview(Lfv);       // r x q
                    const double sq0 = sqrt(s0), aneg = S.scal[0];
                    for (int e = tid; e < r * q; e += TTN_WG) {
                        const int col = e % q, j = e / q;
                        const double sj = S.sigs[j], xv = S.ldsX[S.perm[j] * 128 + col];
                        const bool keep = (sj > 0.0) && (sj * sj > aneg);
                        Ro.p[ix(Ro.r, j) + ix(Ro.c, col)] = keep ? xv * (sq0 / sqrt(sj)) : 0.0;          // sqrt(s0 sigma_j) v_j
                        S.M2[(long long)j * q + col] = keep ? xv * (sq0 / (sj * sqrt(sj))) : 0.0;
                    }
                    __syncthreads();
                    wg_gemm(p, r, q, Mv, mkview(S.M2, plain(1), plain(q)), Lo, inv_s0, 0.0, lds);          // M v_j sqrt(s0) / (s0 sqrt(sigma_j))
                    if (P.sv_out && step < P.sv_steps) {
                        double* so = P.sv_out + ((long long)b * P.sv_steps + step) * P.pmax;
                        for (int i = tid; i < P.pmax; i += TTN_WG) so[i] = (i < p) ? S.sigs[i] * s0 : -1.0;
                    }
                    if (tid == 0) *io.rank_out = r;
                    __syncthreads();
                    done = true;
                    continue;
                }
            }
            if (attempt == 2 && P.sv_out && step < P.sv_steps) {
                double* so = P.sv_out + ((long long)b * P.sv_steps + step) * P.pmax;
                for (int i = tid; i < P.pmax; i += TTN_WG) so[i] = (i < p) ? S.sigs[i] * s0 : -1.0;
            }
            // ---- outputs.  left factor (p x r): x_j * sqrt(s0)/sqrt(sig_j) ; right factor (r x q):
            //      (x_j^T M / s0) * sqrt(s0) / (sig_j*sqrt(sig_j)).  Columns the Jacobi left alone as numerically
            //      zero (norm^2 <= aneg) are not singular vectors relative to their own size: written as exact zeros.
            const View Rfv = mkview(ck1, plain(n2), Idx{n2, 1, (long long)n2 * r});                 // (r x mc)
            const View Lo = wide ? Lfv : tview(Rfv);       // p x r
            const View Ro = wide ? Rfv : tview(Lfv);       // r x q
            const double sq0 = sqrt(s0);
            const double aneg = S.scal[0];
            if (p <= 128 && r <= 128) {
                wg_scale_image(X, ldx, (x_in_lds || attempt == 1) ? 1 : 0, S.sigs, S.perm, Lo, S.Us, p, r, s0, aneg, (SWAP == 0) ? 0 : (wide ? 1 : 2), S.Ts);
            } else {
            for (int e = tid; e < p * r; e += TTN_WG) {
                const int row = e % p, j = e / p;
                const double sj = S.sigs[j];
                const double xv = X[(long long)S.perm[j] * ldx + row];
                const bool keep = (sj > 0.0) && (sj * sj > aneg);
                // x_j = sigma_j * (singular vector of the short side), in units of s0.  Compress: sqrt(S) on both sides.
                // Swap: the LEFT core gets U, the right one S*Vt — the short side is the left one iff the matrix is wide.
                double lf, us;
                if (SWAP == 0) { lf = keep ? xv * (sq0 / sqrt(sj)) : 0.0; us = keep ? xv * (sq0 / (sj * sqrt(sj))) : 0.0; }
                else if (wide) { lf = keep ? xv / sj : 0.0; us = keep ? xv * (s0 / sj) : 0.0; }
                else { lf = keep ? xv * s0 : 0.0; us = keep ? xv / (sj * sj) : 0.0; }
                Lo.p[ix(Lo.r, row) + ix(Lo.c, j)] = lf;
                S.Us[(long long)j * p + row] = us;            // Us^T stored: (r x p) row-major
            }
            }
            __syncthreads();
            wg_gemm_ra(r, q, p, mkview(S.Us, plain(p), plain(1)), Mv, Ro, inv_s0, lds);
            if (attempt == 1) {
                wg_syrk(r, q, Ro, mkview(S.T2, plain(1), plain(128)), 1.0, lds);
                const double e2 = (r <= 128) ? wg_check_diag_tab(S.sigs, S.T2, 128, r, s0, S.Ts, S.red) : unif64(wg_check_diag(S, S.T2, 128, r, s0));
                if (!(e2 <= (cholqr ? CHOLQR_CHECK_TOL : FAST_CHECK_TOL))) continue;                     // redo with Householder (M is intact)
                if (P.sv_out && step < P.sv_steps) {
                    double* so = P.sv_out + ((long long)b * P.sv_steps + step) * P.pmax;
                    for (int i = tid; i < P.pmax; i += TTN_WG) so[i] = (i < p) ? S.sigs[i] * s0 : -1.0;
                }
            }
            if (tid == 0) *io.rank_out = r;
            __syncthreads();
            done = true;
        }
        if (done)
            wg_scale_giveback(ck, (long long)n1 * Dl, ck1, (long long)n2 * Dr, io.rank_out, S.scal + 7, SWAP != 0,
                              (P.sv_out && step < P.sv_steps) ? P.sv_out + ((long long)b * P.sv_steps + step) * P.pmax : nullptr, p);
    }
    if (tid == 0) P.sweep_stats[b] += nsw_total;
    __syncthreads();
}

// tt_compress! form of the step: cores k, k+1 of train b of P.tt
__device__ __forceinline__ void wg_bond_step(const CompressArgs& P, int b, int k, int step, double* lds, bool virt = false /* core k+1 is A_{k+1} x_{k+1}, not yet written */) {
    const TTDev& T = P.tt;
    long long* rks = T.rks + (long long)b * (T.d + 1);
    // the ranks are read from memory this kernel also writes, so the compiler treats them (and every view, size and pointer
    // derived from them) as per-lane values: readfirstlane pins them to SGPRs — the bond step is full of calls, and every
    // VGPR that is live across a call costs a slot of the stack frame (HBM traffic, profiles/README.md "traffic by step")
    BondIO io;
    io.n1 = uni32(T.dims[k]); io.n2 = uni32(T.dims[k + 1]);
    io.Dl = uni32((int)rks[k]); io.rm = uni32((int)rks[k + 1]); io.Dr = uni32((int)rks[k + 2]);
    io.ck = T.data + (long long)b * T.stride + T.off[k];
    io.ck1 = T.data + (long long)b * T.stride + T.off[k + 1];
    io.rank_out = rks + k + 1;
    const int mr = io.n1 * io.Dl, mc = io.n2 * io.Dr;
    const int p = mr <= mc ? mr : mc, q = mr <= mc ? mc : mr;
    const bool small = P.fast && p >= 2 && p <= SMALL_STEP_PMAX && q <= SMALL_STEP_QMAX && P.pmax >= p;
    // the hand-over note of the step before (see handover_area): taken by a wide route-F step on real cores whose areas fit.  Every
    // other step puts the core back in its slot before anything reads it.  (A step that took it and then leaves route F puts it
    // back itself, with a plain loop: a call site inside the force-inlined step is what its register budget cannot take.)
    int pend = uni32(*handover_note(P));
    {
        const bool take = !small && !virt && P.fast && mr <= mc && io.rm < p && io.rm <= TTN_LDS_COLS && io.rm >= 2 && handover_fits(P, p, q, io.rm);
        if (pend && !take) {
            wg_handover_restore(io.ck1, P.scratch + (long long)blockIdx.x * P.scratch_stride + (pend == 2 ? handover_area(P) : 0), io.n2, io.rm, io.Dr, handover_note(P));
            pend = 0;
        }
        // tiny steps (short side <= 8): everything in LDS, no GEMM / LQ / image machinery.  Dispatched HERE, not inside the force-inlined
        // step: one more call site with live views in that function cost it 280 spilled VGPRs (-7 % on the whole benchmark, measured).
        if (small) {
            if (virt) wg_materialize_core(P, b, k + 1);
            SmallStepArgs Q;
            Q.truncerr = P.truncerr; Q.max_bond = P.max_bond; Q.rank_rule = P.rank_rule; Q.pmax = P.pmax;
            Q.sv_row = (P.sv_out && step < P.sv_steps) ? P.sv_out + ((long long)b * P.sv_steps + step) * P.pmax : nullptr;
            Q.status_b = P.status + b;
            // the step's LDS / scratch map (wg_bond_step_io): reduction scratch, scalars, flags; singular values and their order
            Q.red = lds + GEMM_LDS_TOTAL;
            Q.scal = Q.red + 32 + 2 * QR_NB * QR_NB + QR_NB;
            Q.iflag = reinterpret_cast<int*>(Q.scal + 8);
            double* scr = P.scratch + (long long)blockIdx.x * P.scratch_stride;
            const long long pq = (long long)P.pmax * P.qmax;
            double* sig = scr + 2 * pq + (long long)QR_NB * P.qmax + (long long)P.pmax * QR_NB + 2LL * P.pmax * P.pmax;
            Q.sigs = sig + P.pmax;
            Q.perm = reinterpret_cast<int*>(Q.sigs + P.pmax);
            const int nsw = wg_bond_small(Q, io.ck, io.ck1, io.n1, io.n2, io.Dl, io.rm, io.Dr, io.rank_out, lds);
            if (threadIdx.x == 0) P.sweep_stats[b] += nsw;
            __syncthreads();
            return;
        }
    }
    wg_bond_step_io<0>(P, b, io, k, step, lds, virt);
}

__global__ void TTN_KERNEL_BOUNDS k_compress(CompressArgs P) {
    TTN_SETPRIO_BASE();
    extern __shared__ double lds[];
    const int d = P.tt.d;
    // ONE call site of the (force-inlined) bond step: as an out-of-line function it received its arguments in VGPRs, so
    // every size, view and pointer derived from them was a per-lane value and the step carried a 512-byte stack frame per
    // lane across its ~25 calls.  Inlined here everything uniform sits in SGPRs.
    const int per_sweep = 2 * (d - 1);
    const int nsteps = (P.k_single > 0) ? 1 : (P.k_single < 0) ? ((P.k_first <= P.k_last ? P.k_last - P.k_first : P.k_first - P.k_last) + 1)
                                                               : P.sweeps * per_sweep;
    int b = blockIdx.x;
    while (b < P.tt.batch) {
        if (threadIdx.x == 0) { P.sweep_stats[b] = 0; *handover_note(P) = 0; }        // (P.status is sticky: only failures are stored, the host clears on read)
        __syncthreads();
        // fused apply: the left core of the first bond is written out (unless it was imported), every core to its right stays
        // virtual until the front of the first L->R pass reaches it
        if (P.fused && !(P.k_single < 0 && P.fused_first_real)) wg_materialize_core(P, b, (P.k_single < 0) ? P.k_first : 0);
        for (int step = 0; step < nsteps; ++step) {
            int k;
            bool virt = false;
            if (P.k_single > 0) k = P.k_single - 1;                                  // _tt_bond_truncate!
            else if (P.k_single < 0) { k = (P.k_first <= P.k_last) ? P.k_first + step : P.k_first - step; virt = P.fused != 0; }   // ttn_sweep / ttn_apply_sweep
            else {                                                                   // tt_compress!: L->R then R->L per sweep
                const int i = step % per_sweep;
                k = (i < d - 1) ? i : per_sweep - 1 - i;
                virt = P.fused && step < d - 1;                                      // first L->R sweep of the fused op
            }
            wg_bond_step(P, b, k, step, lds, virt);
        }
        if (!P.next_train) break;
        // next train of this slot: one atomic per train, broadcast through LDS (the bond step ends with a barrier, so nobody still
        // reads the words behind the image)
        int* nb = reinterpret_cast<int*>(lds + GEMM_LDS_TOTAL);
        if (threadIdx.x == 0) *nb = (int)gridDim.x + atomicAdd(P.next_train, 1);
        __syncthreads();
        b = uni32(*nb);
        __syncthreads();
    }
}
