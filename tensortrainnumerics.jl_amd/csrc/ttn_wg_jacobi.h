// ttn_wg_jacobi.h — one-sided (Hestenes) Jacobi SVD by one workgroup, in three forms.
//
// Provides (top to bottom):
//   JACOBI_MAX_SWEEPS
//   wg_jacobi_cols                  one-sided Jacobi in global memory (fallback for short sides > 256)
//   grp_sum, grp_from_next          all-reduce over / hand-over between the 16-lane groups of a wave (also the eigensolver's)
//   jacobi_lds128_body, wg_jacobi_lds128
//                                   the LDS Jacobi (register-resident stationary columns, DPP hand-over of the moving
//                                   block, MFMA all-reduce)
//   jacobi_blocked_body, wg_jacobi_blocked256, wg_jacobi_blocked128
//                                   its blocked drivers for short sides 129..256 (and TTN_LDS_COLS+1..128 in the 512-thread build)
// Needs: ttn_wg_prims.h.
// Used by: ttn_dense_kernels.h (wg_svd_cols), ttn_eig_kernels.h (grp_sum).
#pragma once
#include "ttn_wg_prims.h"

#define JACOBI_MAX_SWEEPS 40

// -------------------------------------------------------------------------------------------------
// One-sided (Hestenes) Jacobi on the columns of X (m x p, column-major, leading dimension ldx):
// X <- X*W with orthogonal columns; on exit column i = sigma_i * u_i.  Round-robin parallel
// ordering, one wave per column pair, lanes over rows.  Returns the number of sweeps used
// (negative if the sweep limit was hit).  X may live in LDS or in global memory.
// -------------------------------------------------------------------------------------------------
__device__ __noinline__ int wg_jacobi_cols(int m, int p, double* X, int ldx, int* flag /*LDS*/, double* red /*LDS*/, double* aneg_out /*LDS*/) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = TTN_WG >> 6;
    if (p < 2) { if (tid == 0) *aneg_out = 0.0; __syncthreads(); return 0; }
    const int pe = p + (p & 1);               // even number of slots; slot p (if odd) is a bye
    const int half = pe >> 1;
    const double tol = sqrt((double)m) * DBL_EPSILON;
    // columns whose norm is below eps*sqrt(m)*(largest column norm) carry singular values below what fp64
    // can resolve against sigma_max; they are left alone (rotating pure rounding noise never converges)
    double amax = 0.0;
    for (int c = wave; c < p; c += nwaves) {
        double a = 0.0;
        for (int r = lane; r < m; r += 64) { const double v = X[(long long)c * ldx + r]; a = fma(v, v, a); }
        amax = fmax(amax, wave_sum(a));
    }
    amax = wg_max(amax, red);
    const double aneg = (double)m * DBL_EPSILON * DBL_EPSILON * amax;
    if (tid == 0) *aneg_out = aneg;
    int sweep = 0;
    for (; sweep < JACOBI_MAX_SWEEPS; ++sweep) {
        if (tid == 0) *flag = 0;
        __syncthreads();
        int rotated = 0;
        for (int round = 0; round < pe - 1; ++round) {
            for (int kk = wave; kk < half; kk += nwaves) {
                int i, j;
                if (kk == 0) { i = round; j = pe - 1; }
                else { i = (round + kk) % (pe - 1); j = (round + pe - 1 - kk) % (pe - 1); }
                if (i > j) { const int t = i; i = j; j = t; }
                if (j >= p) continue;          // bye
                double* xi = X + (long long)i * ldx;
                double* xj = X + (long long)j * ldx;
                double a = 0.0, b = 0.0, g = 0.0;
                for (int r = lane; r < m; r += 64) {
                    const double u = xi[r], v = xj[r];
                    a = fma(u, u, a); b = fma(v, v, b); g = fma(u, v, g);
                }
                a = wave_sum(a); b = wave_sum(b); g = wave_sum(g);
                if (a <= aneg || b <= aneg) continue;
                if (fabs(g) <= tol * sqrt(a) * sqrt(b)) continue;
                // rotation annihilating g (Rutishauser formulas)
                const double zeta = (b - a) / (2.0 * g);
                const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
                const double cs = 1.0 / sqrt(fma(t, t, 1.0));
                const double sn = cs * t;
                for (int r = lane; r < m; r += 64) {
                    const double u = xi[r], v = xj[r];
                    xi[r] = cs * u - sn * v;
                    xj[r] = sn * u + cs * v;
                }
                rotated = 1;
            }
            __syncthreads();
        }
        if (rotated && lane == 0) atomicOr(flag, 1);
        __syncthreads();
        const int any = *flag;
        __syncthreads();
        if (!any) return sweep + 1;
    }
    return -sweep;
}


// -------------------------------------------------------------------------------------------------
// Fast path of the one-sided Jacobi for p <= 128 columns of length m <= 128, X resident in LDS with a
// FIXED leading dimension of 128 doubles (column c at X + 128*c).
//   * a wave works on 4 column pairs at once: 16 lanes per pair, lane `sub` owns rows sub + 16*t;
//     groups 1 and 3 walk t rotated by one so the two pairs of a 32-lane half hit disjoint LDS banks;
//   * the 64 pairs of a round-robin round are spread over the 16 waves (pair = 4*wave + group);
//   * squared column norms are cached in LDS (recomputed at the start of every sweep, updated by
//     a' = a - t*g, b' = b + t*g), so a rotation costs one dot product;
//   * reductions over the 16 lanes of a pair are 4 DPP steps (quad_perm, row_half_mirror, row_mirror);
//   * the rotation (t, c, s) uses v_rcp_f64 / v_rsq_f64 seeds: t only needs ~2^-40 relative accuracy
//     (it sets the speed of convergence), c = rsqrt(1+t^2) gets two Newton steps so that c^2+s^2 = 1
//     to rounding (that is what makes every applied rotation orthogonal, i.e. backward stable).
// -------------------------------------------------------------------------------------------------
typedef double lds_f64x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) lds_f64x2 lds_v2;

// All-reduce over the 16 lanes of a Jacobi lane group, result in every lane of the group.  MUST be called in
// wave-uniform control flow (the MFMA involves all 64 lanes).  The group of lane l is (l >> 2) & 3, i.e. the quad at
// position g of each of the four 16-lane rows.  Two v_mfma_f64_4x4x4 against a matrix of ones do the reduction in the
// matrix pipe: the instruction computes D_B[i][j] = sum_k A_B[i][k] with A_B[i][k] in lane B + 4i + 16k and D_B[i][j]
// in lane 16B + 4i + j (layout measured on gfx950, scratch/mfma444_test.hip), so the first sums over k, the second
// over B — together the 16 lanes with the same i.  Replaces 8 v_mov_dpp + 4 v_add_f64 + wait states on the VALU.
__device__ inline double grp_sum(double v) {
    const double s1 = __builtin_amdgcn_mfma_f64_4x4x4f64(v, 1.0, 0.0, 0, 0, 0);
    return __builtin_amdgcn_mfma_f64_4x4x4f64(s1, 1.0, 0.0, 0, 0, 0);
}
// Hand a value to the previous lane group: lane l receives from lane l + 4 of its 16-lane row (row_ror:12), i.e. member
// s of group g receives from member s of group (g + 1) mod 4.  Wave-uniform control flow only.
// (the same hand-over through the LDS crossbar, ds_bpermute_b32, measured 25 % slower per sweep: 279.5 vs 224.1 k clk)
__device__ inline double grp_from_next(double v) { return dpp_mov_f64<0x12C>(v); }

// One sweep-loop instance.  A column is owned by a group of 16 lanes; a lane holds NT2 16-byte pieces of it, so the
// instance reads 32*NT2 rows of every column (rows [m, 32*NT2) must be zero on entry).  A wave has 4 lane groups and
// works on blocks of 4 columns.  Group g = (lane >> 2) & 3, member s = (lane & 3) + 4*(lane >> 4) (see grp_sum); the
// member owns the row pairs {2s, 2s+1} + 32*t.
//
// What bounds the sweep (measured, profiles/README.md "Jacobi"): every rotation used to store its moving column to
// LDS (1 KiB) and ds_write_b128 moves 79 B/clk per CU — 2.5 M stores x 13 clk = 2/3 of the Jacobi time, which neither
// fewer VALU instructions (-20 %: no change), nor 8 lanes per column, nor 8 waves instead of 16 changed.  So:
//   * the stationary column of each lane group stays in REGISTERS for a whole level;
//   * the moving block is loaded from LDS once per block round and then handed from lane group to lane group in
//     registers (16 v_mov_dpp per hand-over, VALU) — one LDS store per column and block round instead of four;
//   * the 16-lane reductions run on the matrix pipe (grp_sum).
// Control flow: which waves work is wave-uniform (branches); which lane groups of a working wave hold real columns
// (only the last block of a p not divisible by 4 has phantom columns) is a MASK — phantom groups load whatever the
// LDS holds, their dot product is discarded and they never write — so that grp_sum / grp_from_next run converged.
// LD = leading dimension of the LDS image (128: up to 128 columns of <= 128 rows; 256: up to 64 columns of <= 256 rows, the
// blocked driver below).  max_sweeps / cross_only / aneg_fixed serve that driver: one sweep per visit, optionally only the
// TOP tournament level (= exactly the cross pairs between the first and the second half of the columns), and the
// negligible-column threshold of the WHOLE matrix instead of the one of the columns at hand (aneg_fixed < 0: compute it).
template <int NT2, int LD>
__device__ int jacobi_lds128_body(int m, int p, lds_f64* X, lds_f64* nrm2, int* flag, double* red,
                                  double* aneg_out, int max_sweeps = JACOBI_MAX_SWEEPS,
                                  bool cross_only = false, double aneg_fixed = -1.0) {
    constexpr int CMASK = TTN_LDS_IMG / LD - 1;         // columns the LDS image holds, minus one
    constexpr int G = 4;                                // lane groups per wave = columns per block
    constexpr int CH = 32;                              // doubles per 16-byte-per-lane piece of a column
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = TTN_WG >> 6;
    lds_i32* flagL = (lds_i32*)flag;                    // the convergence flag lives in LDS: ds ops, not FLAT ones through the generic pointer
    const int grp = (lane >> 2) & 3;
    const int sub = (lane & 3) | ((lane >> 4) << 2);
    const int roff = 2 * sub;                           // row offset inside a piece
#define JOFF(t) (roff + CH * (t))
    const double tol = sqrt((double)m) * DBL_EPSILON;
    const double tol2 = tol * tol;
    double aneg = 0.0;
    int sweep = 0;
    for (; sweep < max_sweeps; ++sweep) {
        // ---- refresh the cached squared norms ----
        double amax = 0.0;
        for (int cb = wave * G; cb < p; cb += nwaves * G) {
            const int c = (cb + grp) & CMASK;            // inside the LDS image even when >= p
            double a0 = 0.0, a1 = 0.0;
#pragma unroll
            for (int t = 0; t < NT2; ++t) {
                const lds_f64x2 v = *(lds_v2*)(X + c * LD + JOFF(t));
                a0 = fma(v.x, v.x, a0);
                a1 = fma(v.y, v.y, a1);
            }
            const double a = grp_sum(a0 + a1);
            if (c < p) {
                if (sub == 0) nrm2[c] = a;
                amax = fmax(amax, a);
            }
        }
        if (sweep == 0) {
            if (aneg_fixed >= 0.0) aneg = aneg_fixed;
            else {
                amax = wg_max(amax, red);
                aneg = (double)m * DBL_EPSILON * DBL_EPSILON * amax;
                if (tid == 0) *aneg_out = aneg;
            }
        }
        if (tid == 0) *flagL = 0;
        __syncthreads();
        int rotated = 0;
        // Block ordering.  The columns form nb blocks of 4 (nbp = nb rounded up to a power of two, phantom blocks idle).
        //  phase 0: the 6 pairs inside every block (round-robin, both columns through LDS);
        //  then log2(nbp) LEVELS of a recursive tournament: at a level the blocks are split into groups of gs, each
        //  group into a stationary half and a moving half; in round r wave (group, a) rotates its stationary block
        //  against moving block (a + r) mod h — 16 cross pairs in 4 inner rounds, the 4 lane groups of the wave taking
        //  the 4 disjoint pairs of an inner round.  nbp-1 block rounds per sweep, every pair exactly once.
        // Workgroup barriers: one per block round (the moving blocks change hands).
        const int nb = (p + G - 1) / G;
        int nbp = 1;
        while (nbp < nb) nbp <<= 1;
// t = tan(theta) of the Jacobi rotation from d = b - a, h = 2g:  t = sign(d) h / (|d| + sqrt(d^2 + h^2)); raw
// v_sqrt/v_rcp seeds are enough for t (it only sets the speed of convergence), c = rsqrt(1 + t^2) gets two Newton steps
// so that c^2 + s^2 = 1 to rounding (that is what makes every applied rotation orthogonal, i.e. backward stable).
#define JROT_MATH                                                                                             \
                const double dd_ = b - a, hh_ = g + g;                                                        \
                const double hyp_ = __builtin_amdgcn_sqrt(fma(dd_, dd_, hh_ * hh_));                          \
                const double t_ = copysign(hh_ * __builtin_amdgcn_rcp(fabs(dd_) + hyp_), hh_ * dd_ );         \
                const double w_ = fma(t_, t_, 1.0);                                                           \
                const double cs = fast_rsqrt2(w_);                                                            \
                const double sn = cs * t_;
        // ---- phase 0: pairs inside the blocks 2*slot and 2*slot+1 (circle method: local column 3 stays put) ----
        if (!cross_only)
        for (int slot0 = wave; 2 * slot0 < nb; slot0 += nwaves) {
            const int blk = 2 * slot0 + (grp >> 1), hq = grp & 1;
            const int c0 = G * blk;
#pragma unroll
            for (int rr = 0; rr < G - 1; ++rr) {
                const int li = (hq == 0) ? G - 1 : (rr + hq) % (G - 1);
                const int lj = (hq == 0) ? rr : (rr + G - 1 - hq) % (G - 1);
                const int i = (c0 + (li < lj ? li : lj)) & CMASK, j = (c0 + (li < lj ? lj : li)) & CMASK;
                const bool act = j < p && blk < nb;
                lds_f64* xi = X + i * LD;
                lds_f64* xj = X + j * LD;
                const double a = nrm2[i], b = nrm2[j];
                lds_f64x2 u[NT2], v[NT2];
                double g0 = 0.0, g1 = 0.0;
#pragma unroll
                for (int t = 0; t < NT2; ++t) {
                    u[t] = *(lds_v2*)(xi + JOFF(t));
                    v[t] = *(lds_v2*)(xj + JOFF(t));
                    g0 = fma(u[t].x, v[t].x, g0);
                    g1 = fma(u[t].y, v[t].y, g1);
                }
                const double g = grp_sum(g0 + g1);
                if (act && (a > aneg) && (b > aneg) && (g * g > tol2 * a * b)) {
                    JROT_MATH
#pragma unroll
                    for (int t = 0; t < NT2; ++t) {
                        lds_f64x2 nu, nv;
                        nu.x = fma(cs, u[t].x, -sn * v[t].x);
                        nu.y = fma(cs, u[t].y, -sn * v[t].y);
                        nv.x = fma(sn, u[t].x, cs * v[t].x);
                        nv.y = fma(sn, u[t].y, cs * v[t].y);
                        *(lds_v2*)(xi + JOFF(t)) = nu;
                        *(lds_v2*)(xj + JOFF(t)) = nv;
                    }
                    if (sub == 0) { nrm2[i] = fmax(a - t_ * g, 0.0); nrm2[j] = b + t_ * g; }
                    rotated = 1;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
        // ---- levels ----
        constexpr int PPW = ((CMASK + 1) / 8 + TTN_NWAVES - 1) / TTN_NWAVES;   // block pairs a wave owns per block round (image full)
        for (int gs = nbp; gs >= (cross_only ? nbp : 2); gs >>= 1) {
            const int h = gs >> 1;
            int gam[PPW], aa[PPW], ci[PPW];
            bool wact[PPW], iact[PPW];
            lds_f64x2 u[PPW][NT2];
            double an[PPW];
#pragma unroll
            for (int q = 0; q < PPW; ++q) {
                const int slot = wave + q * nwaves;
                wact[q] = slot < (nbp >> 1);                                // wave-uniform
                gam[q] = wact[q] ? slot / h : 0;
                aa[q] = wact[q] ? slot % h : 0;
                ci[q] = (G * (gam[q] * gs + aa[q]) + grp) & CMASK;            // stationary column of this lane group
                iact[q] = wact[q] && ci[q] < p;
                an[q] = nrm2[ci[q]];
#pragma unroll
                for (int t = 0; t < NT2; ++t) u[q][t] = *(lds_v2*)(X + ci[q] * LD + JOFF(t));
            }
            for (int r = 0; r < h; ++r) {
#pragma unroll
                for (int q = 0; q < PPW; ++q) {
                    if (wact[q]) {
                        int mrot = aa[q] + r; if (mrot >= h) mrot -= h;
                        const int cjb = G * (gam[q] * gs + h + mrot);
                        // the moving column this lane group starts with; it then takes the next group's column each inner round
                        const int cj0 = (cjb + grp) & CMASK;
                        lds_f64x2 v[NT2];
#pragma unroll
                        for (int t = 0; t < NT2; ++t) v[t] = *(lds_v2*)(X + cj0 * LD + JOFF(t));
                        double b = nrm2[cj0];
                        int dirty = 0;
#pragma unroll
                        for (int sft = 0; sft < G; ++sft) {
                            const int cj = (cjb + ((grp + sft) & (G - 1))) & CMASK;
                            const bool act = iact[q] && cj < p;
                            double g0 = 0.0, g1 = 0.0;
#pragma unroll
                            for (int t = 0; t < NT2; ++t) {
                                g0 = fma(u[q][t].x, v[t].x, g0);
                                g1 = fma(u[q][t].y, v[t].y, g1);
                            }
                            const double g = grp_sum(g0 + g1);
                            const double a = an[q];
                            if (act && (a > aneg) && (b > aneg) && (g * g > tol2 * a * b)) {
                                JROT_MATH
                                const double ic = w_ * cs;                 // 1/c
                                // u' = c (u - t v);  v' = t u' + v / c  — both in place (v_fmac / v_mul on their own registers)
#pragma unroll
                                for (int t = 0; t < NT2; ++t) {
                                    u[q][t].x = cs * fma(-t_, v[t].x, u[q][t].x);
                                    u[q][t].y = cs * fma(-t_, v[t].y, u[q][t].y);
                                    v[t].x = fma(t_, u[q][t].x, ic * v[t].x);
                                    v[t].y = fma(t_, u[q][t].y, ic * v[t].y);
                                }
                                b = b + t_ * g;
                                an[q] = fmax(a - t_ * g, 0.0);
                                dirty = 1;
                            }
                            if (sft < G - 1) {
#pragma unroll
                                for (int t = 0; t < NT2; ++t) { v[t].x = grp_from_next(v[t].x); v[t].y = grp_from_next(v[t].y); }
                                b = grp_from_next(b);
                                dirty = __builtin_amdgcn_update_dpp(0, dirty, 0x12C, 0xF, 0xF, true);
                            }
                        }
                        const int cjl = (cjb + ((grp + G - 1) & (G - 1))) & CMASK;     // the column this group ends up with
                        if (dirty && cjl < p) {
#pragma unroll
                            for (int t = 0; t < NT2; ++t) *(lds_v2*)(X + cjl * LD + JOFF(t)) = v[t];
                            if (sub == 0) nrm2[cjl] = b;
                            rotated = 1;
                        }
                    }
                }
                __syncthreads();                                           // the moving blocks change hands
            }
#pragma unroll
            for (int q = 0; q < PPW; ++q) {
                if (iact[q]) {
#pragma unroll
                    for (int t = 0; t < NT2; ++t) *(lds_v2*)(X + ci[q] * LD + JOFF(t)) = u[q][t];
                    if (sub == 0) nrm2[ci[q]] = an[q];
                }
            }
            __syncthreads();
        }
#undef JROT_MATH
#undef JOFF
        if (rotated) *flagL = 1;
        __syncthreads();
        const int any = *flagL;
        __syncthreads();
        if (!any) return sweep + 1;
    }
    return -sweep;
}

// Fast path of the one-sided Jacobi: p <= 128 columns of length m <= 128 in LDS, leading dimension 128; rows
// [m, 128) of every column must be ZERO (the caller pads).  See jacobi_lds128_body.
__device__ __noinline__ int wg_jacobi_lds128(int m, int p, double* Xg, double* nrm2g, int* flag, double* red,
                                             double* aneg_out /*LDS*/) {
    if (p < 2) { if (threadIdx.x == 0) *aneg_out = 0.0; __syncthreads(); return 0; }
    lds_f64* X = (lds_f64*)Xg;
    lds_f64* nrm2 = (lds_f64*)nrm2g;
    if (m <= 32) return jacobi_lds128_body<1, 128>(m, p, X, nrm2, flag, red, aneg_out);
    if (m <= 64) return jacobi_lds128_body<2, 128>(m, p, X, nrm2, flag, red, aneg_out);
    if (m <= 96) return jacobi_lds128_body<3, 128>(m, p, X, nrm2, flag, red, aneg_out);     // the 96-column ramp step
    return jacobi_lds128_body<4, 128>(m, p, X, nrm2, flag, red, aneg_out);
}

// -------------------------------------------------------------------------------------------------
// Blocked one-sided Jacobi for 128 < p <= 256 columns of length m <= 256 (ranks 65..128): the matrix (p x p doubles, up
// to 512 KB) lives in global memory (column-major, leading dimension ldx) and is processed in column blocks of 32 through
// the LDS image (leading dimension 256, 64 columns) by the same lane-group kernel as the p <= 128 fast path:
//   per sweep   (a) every block alone: one full sweep over its 496 pairs;
//               (b) every pair of blocks (I < J): I in columns 0..31, J in 32..63, only the top tournament level =
//                   exactly the 32 x 32 cross pairs —
//   i.e. every pair of columns once per sweep, like the cyclic orderings.  A block visit reads and writes its columns once
//   (coalesced); a visit that rotated nothing is not written back.  Converged when a whole sweep rotates nothing.
// Replaces the global-memory Jacobi (wg_jacobi_cols, 3-4x slower at these sizes), which remains the fallback for p > 256.
// -------------------------------------------------------------------------------------------------
// LD = leading dimension of the LDS image (>= m), JBW = columns per block: 2 * JBW * LD doubles of image.
template <int LD, int JBW>
__device__ inline void jb_load(lds_f64* X, int col0_lds, const double* Xg, int ldx, int c0, int ncols, int m) {
    // columns c0 .. c0+ncols-1 of Xg -> LDS columns col0_lds .., rows >= m and missing columns zero-filled (JBW columns always)
    for (int e = threadIdx.x; e < JBW * LD; e += TTN_WG) {
        const int r = e % LD, c = e / LD;
        X[(col0_lds + c) * LD + r] = (c < ncols && r < m) ? Xg[(long long)(c0 + c) * ldx + r] : 0.0;
    }
}
template <int LD, int JBW>
__device__ inline void jb_store(const lds_f64* X, int col0_lds, double* Xg, int ldx, int c0, int ncols, int m) {
    for (int e = threadIdx.x; e < JBW * LD; e += TTN_WG) {
        const int r = e % LD, c = e / LD;
        if (c < ncols && r < m) Xg[(long long)(c0 + c) * ldx + r] = X[(col0_lds + c) * LD + r];
    }
}

template <int LD, int JBW>
__device__ int jacobi_blocked_body(int m, int p, double* Xg, int ldx, double* Xlds, double* nrm2g, int* flag, double* red,
                                   double* aneg_out /*LDS*/) {
    static_assert(2 * JBW * LD <= TTN_LDS_IMG, "two column blocks must fit the LDS image");
    m = uni32(m); p = uni32(p); ldx = uni32(ldx);
    Xg = unip(Xg); Xlds = unip(Xlds); nrm2g = unip(nrm2g); flag = unip(flag); red = unip(red); aneg_out = unip(aneg_out);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = TTN_WG >> 6;
    lds_f64* X = (lds_f64*)Xlds;
    lds_f64* nrm2 = (lds_f64*)nrm2g;
    // negligible-column threshold of the whole matrix
    double amax = 0.0;
    for (int c = wave; c < p; c += nwaves) {
        double a = 0.0;
        for (int r = lane; r < m; r += 64) { const double v = Xg[(long long)c * ldx + r]; a = fma(v, v, a); }
        amax = fmax(amax, wave_sum(a));
    }
    amax = wg_max(amax, red);
    const double aneg = (double)m * DBL_EPSILON * DBL_EPSILON * amax;
    if (tid == 0) *aneg_out = aneg;
    __syncthreads();
    const int nbk = (p + JBW - 1) / JBW;
    for (int sweep = 0; sweep < JACOBI_MAX_SWEEPS; ++sweep) {
        int any = 0;
        for (int I = 0; I < nbk; ++I) {                                           // (a) inside every block
            const int nI = min(JBW, p - I * JBW);
            __syncthreads();
            jb_load<LD, JBW>(X, 0, Xg, ldx, I * JBW, nI, m);
            __syncthreads();
            const int r = jacobi_lds128_body<LD / 32, LD>(m, nI, X, nrm2, flag, red, aneg_out, 1, false, aneg);
            if (r < 0) { any = 1; jb_store<LD, JBW>(X, 0, Xg, ldx, I * JBW, nI, m); }
        }
        for (int I = 0; I + 1 < nbk; ++I)                                          // (b) between every two blocks
            for (int J = I + 1; J < nbk; ++J) {
                const int nJ = min(JBW, p - J * JBW);
                __syncthreads();
                jb_load<LD, JBW>(X, 0, Xg, ldx, I * JBW, JBW, m);
                jb_load<LD, JBW>(X, JBW, Xg, ldx, J * JBW, nJ, m);
                __syncthreads();
                const int r = jacobi_lds128_body<LD / 32, LD>(m, JBW + nJ, X, nrm2, flag, red, aneg_out, 1, true, aneg);
                if (r < 0) {
                    any = 1;
                    jb_store<LD, JBW>(X, 0, Xg, ldx, I * JBW, JBW, m);
                    jb_store<LD, JBW>(X, JBW, Xg, ldx, J * JBW, nJ, m);
                }
            }
        __syncthreads();
        if (!any) return sweep + 1;
    }
    return -JACOBI_MAX_SWEEPS;
}
// 128 < p <= 256 (ranks 65..128): image leading dimension 256, as many columns per block as two blocks fit the image
__device__ __noinline__ int wg_jacobi_blocked256(int m, int p, double* Xg, int ldx, double* Xlds, double* nrm2g, int* flag, double* red,
                                                 double* aneg_out /*LDS*/) {
    return jacobi_blocked_body<256, TTN_LDS_IMG / 512>(m, p, Xg, ldx, Xlds, nrm2g, flag, red, aneg_out);
}
#if TTN_LDS_COLS < 128
// TTN_LDS_COLS < p <= 128 in the small-image build: the same blocked scheme with leading dimension 128
__device__ __noinline__ int wg_jacobi_blocked128(int m, int p, double* Xg, int ldx, double* Xlds, double* nrm2g, int* flag, double* red,
                                                 double* aneg_out /*LDS*/) {
    return jacobi_blocked_body<128, TTN_LDS_IMG / 256>(m, p, Xg, ldx, Xlds, nrm2g, flag, red, aneg_out);
}
#endif
