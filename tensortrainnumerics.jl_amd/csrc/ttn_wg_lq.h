// ttn_wg_lq.h — Householder LQ by one workgroup, in three forms.
//
// Provides (top to bottom):
//   QR_NB                           Householder panel width
//   lq_lds_whole(_q)                the whole matrix in LDS (with _q: the orthogonal factor too) / the L blocks of TSQR column chunks
//   wg_block_reflector_apply        a compact-WY block reflector applied to rows in global memory
//   wg_lq_blocked                   blocked compact WY of any p x q matrix in global memory, trailing updates by wg_gemm
// Needs: ttn_wg_gemm.h (wg_gemm, GEMM_LDS_DOUBLES) and through it ttn_wg_prims.h.
// Used by: ttn_dense_kernels.h (route H of the bond step), ttn_ortho_kernels.h, ttn_hsvd_kernels.h; QR_NB sizes the LDS and
// scratch of every kernel that may call them.
#pragma once
#include "ttn_wg_gemm.h"

#define QR_NB 16                         // Householder panel width

// -------------------------------------------------------------------------------------------------
// Blocked Householder LQ (compact WY, panel QR_NB) of a row-major p x q matrix M2 (any p, q), in place.
// rr = min(p, q) row reflectors H_j = I - tau_j v_j v_j^T act from the right:  M2 * H_0 ... H_{rr-1} = [L 0].
// On exit M2[i][c], c <= i, c < rr holds L; M2[j][j+1:] holds the scaled v_j (v_j[j] = 1 implicit).
// If Qout != null it receives the rr x q matrix Q' = first rr rows of H_{rr-1} ... H_0 (orthonormal rows,
// M = L Q'), row-major with leading dimension q.  A column-major mm x nn matrix is the row-major nn x mm
// matrix of its transpose, so the same routine is the thin QR  T = Q R  with Q = Q'^T, R = L^T.
//
// Panel: the jb x len panel is factored in LDS (global memory if it does not fit) with ONE barrier per reflector:
// every wave recomputes the reflector of row r (no broadcast), wave w applies it to panel row r+1+w, and row r is
// left unscaled until the panel is done.  Trailing matrix: C <- C - ((C V^T) T) V by three GEMM calls.
// Scratch: Vb (QR_NB x q), Wb (max(p, rr) x QR_NB), Tst (ceil(rr/QR_NB) * QR_NB^2, only with Qout) in global memory;
// Ts, Ss (QR_NB^2 each), taus (QR_NB), red in LDS behind the GEMM region.
// -------------------------------------------------------------------------------------------------

// Householder LQ of a p x qc matrix (row-major, leading dimension lds_) entirely in LDS: p reflectors, one barrier each,
// wave w applies H_r to rows r+1+w, r+1+w+16, ...  Writes L (lower triangle, p x min(p,qc)) to dst (row-major, leading
// dimension ldd); with `full` also zeros above the diagonal up to column p-1 (the L blocks of a TSQR level are read whole).
// Ss: >= 128 doubles of LDS for the diagonal.  A: the LDS image (>= p*qc doubles).
__device__ inline void lq_lds_whole(int p, int qc, const double* src, int lds_, double* dst, int ldd, double* A_, double* Ss_, bool full) {
    // LDS address space pointers: through generic pointers every access would be a FLAT instruction
    lds_f64* A = (lds_f64*)A_;
    lds_f64* Ss = (lds_f64*)Ss_;
    const int tid = threadIdx.x;
    const int rr = min(p, qc);
    // One row per group of 16 lanes (64 rows per pass): the dot product <row_i, v> is a reduction over the 16 lanes of a DPP row
    // (row16_sum) instead of a whole-wave reduction per row, and the group that updates row r+1 also produces the NEXT reflector's
    // scalars (beta, tau, scale) as a by-product — nothing in a step is computed redundantly by all waves.
    const int grp = tid >> 4, l16 = tid & 15;
    lds_f64* par = Ss + 128;                            // [2][4]: beta, tau, scale of the current / next reflector
    __syncthreads();
    gmem_f64* srcg = (gmem_f64*)src;                              // M2 is global memory: global_load / global_store, not FLAT
    gmem_wf64* dstg = (gmem_wf64*)dst;
    wg_batched<8>((long long)p * qc, [&](long long e) { return srcg[(e / qc) * lds_ + (e % qc)]; }, [&](long long e, double v) { A[e] = v; });
    __syncthreads();
    if (grp == 0) {                                               // reflector 0
        double s = 0.0;
        for (int c = 1 + l16; c < qc; c += 16) { const double v = A[c]; s = fma(v, v, s); }
        const double xnorm2 = row16_sum(s), alpha = A[0];
        double tau = 0.0, scal = 0.0, beta = alpha;
        if (xnorm2 > 0.0) { beta = -copysign(sqrt(fma(alpha, alpha, xnorm2)), alpha); tau = (beta - alpha) / beta; scal = 1.0 / (alpha - beta); }
        if (l16 == 0) { par[0] = beta; par[1] = tau; par[2] = scal; }
    }
    __syncthreads();
    for (int r = 0; r < rr; ++r) {
        const lds_f64* pr = par + 4 * (r & 1);
        lds_f64* pn = par + 4 * ((r + 1) & 1);
        const double beta = pr[0], tau = pr[1], scal = pr[2];
        const lds_f64* row = A + r * qc;
        if (tid == 0) Ss[r] = beta;
        for (int i = r + 1 + grp; i < p; i += TTN_WG / 16) {
            lds_f64* ri = A + i * qc;
            // (LDS latency: four independent column groups per trip, so the loads of a trip are in flight together)
            if (tau != 0.0) {
                double w = 0.0;
                for (int c = r + 1 + l16; c < qc; c += 64) {
                    const bool k1 = c + 16 < qc, k2 = c + 32 < qc, k3 = c + 48 < qc;
                    const double a0 = ri[c], b0 = row[c];
                    const double a1 = k1 ? ri[c + 16] : 0.0, b1 = k1 ? row[c + 16] : 0.0;
                    const double a2 = k2 ? ri[c + 32] : 0.0, b2 = k2 ? row[c + 32] : 0.0;
                    const double a3 = k3 ? ri[c + 48] : 0.0, b3 = k3 ? row[c + 48] : 0.0;
                    w = fma(a0, b0, fma(a1, b1, fma(a2, b2, fma(a3, b3, w))));
                }
                w = fma(scal, row16_sum(w), ri[r]);
                const double tws = tau * w * scal;
                for (int c = r + 1 + l16; c < qc; c += 64) {
                    const bool k1 = c + 16 < qc, k2 = c + 32 < qc, k3 = c + 48 < qc;
                    const double a0 = ri[c], b0 = row[c];
                    const double a1 = k1 ? ri[c + 16] : 0.0, b1 = k1 ? row[c + 16] : 0.0;
                    const double a2 = k2 ? ri[c + 32] : 0.0, b2 = k2 ? row[c + 32] : 0.0;
                    const double a3 = k3 ? ri[c + 48] : 0.0, b3 = k3 ? row[c + 48] : 0.0;
                    ri[c] = fma(-tws, b0, a0);
                    if (k1) ri[c + 16] = fma(-tws, b1, a1);
                    if (k2) ri[c + 32] = fma(-tws, b2, a2);
                    if (k3) ri[c + 48] = fma(-tws, b3, a3);
                }
                if (l16 == 0) ri[r] -= tau * w;
            }
            if (i == r + 1 && r + 1 < rr) {                        // the next reflector from the freshly updated row r+1
                double s = 0.0;
                for (int c = r + 2 + l16; c < qc; c += 64) {
                    const double v0 = ri[c], v1 = (c + 16 < qc) ? ri[c + 16] : 0.0, v2 = (c + 32 < qc) ? ri[c + 32] : 0.0, v3 = (c + 48 < qc) ? ri[c + 48] : 0.0;
                    s = fma(v0, v0, fma(v1, v1, fma(v2, v2, fma(v3, v3, s))));
                }
                const double xnorm2 = row16_sum(s), alpha = ri[r + 1];
                double tau2 = 0.0, scal2 = 0.0, beta2 = alpha;
                if (xnorm2 > 0.0) { beta2 = -copysign(sqrt(fma(alpha, alpha, xnorm2)), alpha); tau2 = (beta2 - alpha) / beta2; scal2 = 1.0 / (alpha - beta2); }
                if (l16 == 0) { pn[0] = beta2; pn[1] = tau2; pn[2] = scal2; }
            }
        }
        __syncthreads();
    }
    const int ncol = full ? p : rr;
    for (int e = tid; e < p * ncol; e += TTN_WG) {
        const int r = e / ncol, c = e % ncol;
        if (c <= r && c < rr) dstg[(long long)r * ldd + c] = (c == r) ? Ss[r] : A[r * qc + c];
        else if (full) dstg[(long long)r * ldd + c] = 0.0;
    }
    __syncthreads();
}

// The same with the explicit thin Q' (p x q, orthonormal rows, M = L Q'): factor in LDS, then E = [I 0] times
// H_{p-1} ... H_0 in a second LDS image (2*p*q doubles in all: 64x128 cores of rank-64 trains fit).  In place: M2 receives L.
// Ts (>= 128 doubles): tau_r; Ss (>= 256 doubles): beta_r and the scale 1/(alpha - beta) of the stored reflectors.
__device__ inline void lq_lds_whole_q(int p, int q, double* M2, int ld, double* Qout, double* A_, double* Ss_, double* Ts_) {
    // same organisation as lq_lds_whole: LDS address-space pointers (no FLAT instructions), one row per group of 16 lanes with DPP
    // row sums, the next reflector's scalars as a by-product of the update of row r+1
    const int tid = threadIdx.x;
    const int grp = tid >> 4, l16 = tid & 15;
    lds_f64* A = (lds_f64*)A_;
    lds_f64* Ss = (lds_f64*)Ss_;
    lds_f64* Ts = (lds_f64*)Ts_;
    lds_f64* E = A + p * q;
    lds_f64* scl = Ss + 128;
    lds_f64* par = Ts + 128;                                      // [2][4]: beta, tau, scale of the current / next reflector
    gmem_wf64* M2g = (gmem_wf64*)M2;
    gmem_wf64* Qg = (gmem_wf64*)Qout;
    __syncthreads();
    for (int e = tid; e < p * q; e += TTN_WG) {
        const int r = e / q, c = e % q;
        A[e] = M2g[(long long)r * ld + c];
        E[e] = (r == c) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (grp == 0) {
        double s = 0.0;
        for (int c = 1 + l16; c < q; c += 16) { const double v = A[c]; s = fma(v, v, s); }
        const double xnorm2 = row16_sum(s), alpha = A[0];
        double tau = 0.0, scal = 0.0, beta = alpha;
        if (xnorm2 > 0.0) { beta = -copysign(sqrt(fma(alpha, alpha, xnorm2)), alpha); tau = (beta - alpha) / beta; scal = 1.0 / (alpha - beta); }
        if (l16 == 0) { par[0] = beta; par[1] = tau; par[2] = scal; }
    }
    __syncthreads();
    for (int r = 0; r < p; ++r) {
        const lds_f64* pr = par + 4 * (r & 1);
        lds_f64* pn = par + 4 * ((r + 1) & 1);
        const double beta = pr[0], tau = pr[1], scal = pr[2];
        const lds_f64* row = A + r * q;
        if (tid == 0) { Ss[r] = beta; scl[r] = scal; Ts[r] = tau; }
        for (int i = r + 1 + grp; i < p; i += TTN_WG / 16) {
            lds_f64* ri = A + i * q;
            if (tau != 0.0) {
                double w = 0.0;
                for (int c = r + 1 + l16; c < q; c += 64) {
                    const bool k1 = c + 16 < q, k2 = c + 32 < q, k3 = c + 48 < q;
                    const double a0 = ri[c], b0 = row[c];
                    const double a1 = k1 ? ri[c + 16] : 0.0, b1 = k1 ? row[c + 16] : 0.0;
                    const double a2 = k2 ? ri[c + 32] : 0.0, b2 = k2 ? row[c + 32] : 0.0;
                    const double a3 = k3 ? ri[c + 48] : 0.0, b3 = k3 ? row[c + 48] : 0.0;
                    w = fma(a0, b0, fma(a1, b1, fma(a2, b2, fma(a3, b3, w))));
                }
                w = fma(scal, row16_sum(w), ri[r]);
                const double tws = tau * w * scal;
                for (int c = r + 1 + l16; c < q; c += 16) ri[c] = fma(-tws, row[c], ri[c]);
                if (l16 == 0) ri[r] -= tau * w;
            }
            if (i == r + 1 && r + 1 < p) {
                double s = 0.0;
                for (int c = r + 2 + l16; c < q; c += 16) { const double v = ri[c]; s = fma(v, v, s); }
                const double xnorm2 = row16_sum(s), alpha = ri[r + 1];
                double tau2 = 0.0, scal2 = 0.0, beta2 = alpha;
                if (xnorm2 > 0.0) { beta2 = -copysign(sqrt(fma(alpha, alpha, xnorm2)), alpha); tau2 = (beta2 - alpha) / beta2; scal2 = 1.0 / (alpha - beta2); }
                if (l16 == 0) { pn[0] = beta2; pn[1] = tau2; pn[2] = scal2; }
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < p * p; e += TTN_WG) {                 // L into M2 (the caller reads c <= r only)
        const int r = e / p, c = e % p;
        if (c <= r) M2g[(long long)r * ld + c] = (c == r) ? Ss[r] : A[r * q + c];
    }
    // E <- E H_r for r = p-1 .. 0: rows i < r are still unit vectors orthogonal to v_r, so only rows i >= r change
    for (int r = p - 1; r >= 0; --r) {
        const lds_f64* row = A + r * q;                          // v_r = [0.., 1 at r, row[c] * scl[r] for c > r]
        const double tau = Ts[r], sc = scl[r];
        for (int i = r + grp; tau != 0.0 && i < p; i += TTN_WG / 16) {
            lds_f64* ei = E + i * q;
            double w = 0.0;
            for (int c = r + 1 + l16; c < q; c += 64) {
                const bool k1 = c + 16 < q, k2 = c + 32 < q, k3 = c + 48 < q;
                const double a0 = ei[c], b0 = row[c];
                const double a1 = k1 ? ei[c + 16] : 0.0, b1 = k1 ? row[c + 16] : 0.0;
                const double a2 = k2 ? ei[c + 32] : 0.0, b2 = k2 ? row[c + 32] : 0.0;
                const double a3 = k3 ? ei[c + 48] : 0.0, b3 = k3 ? row[c + 48] : 0.0;
                w = fma(a0, b0, fma(a1, b1, fma(a2, b2, fma(a3, b3, w))));
            }
            w = fma(sc, row16_sum(w), ei[r]);
            const double tws = tau * w * sc;
            for (int c = r + 1 + l16; c < q; c += 16) ei[c] = fma(-tws, row[c], ei[c]);
            if (l16 == 0) ei[r] -= tau * w;
        }
        __syncthreads();
    }
    for (int e = tid; e < p * q; e += TTN_WG) Qg[e] = E[e];
    __syncthreads();
}

// Block-reflector update with everything but C in LDS:  C (rows x len, row-major in GLOBAL memory, leading dimension ldc)
//     C <- C - ((C V^T) Top) V,   V (16 x len, LDS, leading dimension ldv), Top = T or T^T (16 x 16, LDS, row-major).
// One wave per tile of 16 rows of C, three fp64-MFMA passes (W = C V^T: len/4 MFMAs; W' = W Top: 4; C -= W' V: len/4), no
// workgroup barrier inside (a wave only needs its own W).  Replaces three generic GEMM calls per panel whose inner /
// outer dimension is 16 (prologue-dominated: ~150 k clk per panel against ~25 k here).  Rows of V beyond the panel height
// must be zero.  Wl: 256 doubles of LDS per wave.
__device__ inline int blkref_ldv(int len) { return ((len + 27) / 32) * 32 + 4; }     // >= len, == 4 mod 32: the 16 V rows a pass-1 read touches spread over the banks
__device__ inline void wg_block_reflector_apply(int rows, int len, double* Cg, int ldc, const double* Vl_, int ldv, const double* Tl_,
                                                bool transT, double* Wl_) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = TTN_WG >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const lds_f64* V = (const lds_f64*)Vl_;
    const lds_f64* T = (const lds_f64*)Tl_;
    lds_f64* W = (lds_f64*)Wl_ + wave * 256;
    const int ntile = (rows + 15) >> 4;
    for (int tile = wave; tile < ntile; tile += nwaves) {
        const int r0 = tile << 4;
        const bool rok = r0 + li < rows;
        const double* crow = Cg + (long long)(r0 + (rok ? li : 0)) * ldc;
        mfma_acc_t acc = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < len; k0 += 4) {                                   // W = C_tile V^T
            const int kk = k0 + lk;
            const double a = (rok && kk < len) ? crow[kk] : 0.0;
            const double b = (kk < len) ? V[li * ldv + kk] : 0.0;               // B[k][j] = V[j][k]
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) W[(lk + 4 * reg) * 16 + li] = acc[reg];
        __builtin_amdgcn_wave_barrier();
        mfma_acc_t acc2 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 4; ++t) {                                           // W' = W Top
            const int kk = 4 * t + lk;
            const double a = W[li * 16 + kk];
            const double b = transT ? T[li * 16 + kk] : T[kk * 16 + li];        // B[k][j] = Top[k][j]
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc2, 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) W[(lk + 4 * reg) * 16 + li] = acc2[reg];
        __builtin_amdgcn_wave_barrier();
        double at[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) at[t] = W[li * 16 + 4 * t + lk];
        for (int c0 = 0; c0 < len; c0 += 16) {                                  // C_tile -= W' V
            const bool cok = c0 + li < len;
            mfma_acc_t acc3 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double b = cok ? V[(4 * t + lk) * ldv + c0 + li] : 0.0;
                acc3 = __builtin_amdgcn_mfma_f64_16x16x4f64(at[t], b, acc3, 0, 0, 0);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = r0 + lk + 4 * reg;
                if (row < rows && cok) Cg[(long long)row * ldc + c0 + li] -= acc3[reg];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__device__ __noinline__ void wg_lq_blocked(int p, int q, double* M2, int ld, double* Vb, double* Wb, double* Tst, double* Qout,
                                           double* lds_gemm, double* Ts, double* Ss, double* taus, double* red) {
    // arguments of an out-of-line function arrive in VGPRs: pin the workgroup-uniform ones to SGPRs
    p = uni32(p); q = uni32(q); ld = uni32(ld);
    M2 = unip(M2); Vb = unip(Vb); Wb = unip(Wb); Tst = unip(Tst); Qout = unip(Qout);
    lds_gemm = unip(lds_gemm); Ts = unip(Ts); Ss = unip(Ss); taus = unip(taus); red = unip(red);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = TTN_WG >> 6;
    const int rr = min(p, q);
    if (Qout && rr == p && p <= 128 && 2LL * p * q <= GEMM_LDS_DOUBLES) {       // small cores: factor AND explicit Q' in LDS
        lq_lds_whole_q(p, q, M2, ld, Qout, lds_gemm, Ss, Ts);
        return;
    }
    // ---- matrices that fit the LDS whole (the small H-route steps of a sweep: 96x128, 64x128, ...): ONE "panel", no
    //      trailing GEMMs at all.  Wider ones with p <= 88 rows go through the LDS in column chunks of width w >= 2p
    //      (TSQR): L_i of every chunk is written back side by side, [L_1 L_2 ...] is factored again until one chunk is left
    //      — M M^T = sum L_i L_i^T, so the final L is an L factor of M (the callers use L only, never Q) ----
    if (!Qout && rr == p && p <= 128) {
        const int w = GEMM_LDS_DOUBLES / p;                // columns of a chunk
        if (q <= w || w >= 2 * p) {
            int qc = q;                                     // current width of the matrix held in M2[:, 0:qc]
            for (;;) {
                const int nchunk = (qc + w - 1) / w;
                for (int ci = 0; ci < nchunk; ++ci) {
                    const int c0 = ci * w, cw = min(w, qc - c0);
                    lq_lds_whole(p, cw, M2 + c0, ld, M2 + (long long)ci * p, ld, lds_gemm, Ss, nchunk > 1);
                }
                if (nchunk == 1) break;
                qc = nchunk * p;
            }
            return;
        }
    }
    double* betas = Ss;                                  // QR_NB (Ss is free while a panel is being factored)
    double* scl = Ss + QR_NB;                            // QR_NB
    for (int j0 = 0; j0 < rr; j0 += QR_NB) {
        const int jb = min(QR_NB, rr - j0);
        const int len = q - j0;
        const bool in_lds = (long long)jb * len <= GEMM_LDS_DOUBLES;
        // fast trailing update (wg_block_reflector_apply): the panel is factored in LDS with the padded leading dimension
        // ldv and then turned into the explicit V in place; 16 rows of V + 256 doubles of W per wave must fit the region
        const int ldv = blkref_ldv(len);
        const bool fastp = (long long)QR_NB * ldv + 256 * (TTN_WG / 64) <= GEMM_LDS_DOUBLES;
        double* Pn = in_lds ? lds_gemm : (M2 + (long long)j0 * ld + j0);
        const int ldp = fastp ? ldv : (in_lds ? len : ld);
        __syncthreads();
        if (in_lds) {
            for (int e = tid; e < jb * len; e += TTN_WG) { const int r = e / len, c = e - r * len; Pn[(long long)r * ldp + c] = M2[(long long)(j0 + r) * ld + j0 + c]; }
            __syncthreads();
        }
        // ---- panel factorisation ----
        for (int r = 0; r < jb; ++r) {
            const double* row = Pn + (long long)r * ldp;
            double s = 0.0;
            for (int c = r + 1 + lane; c < len; c += 64) { const double v = row[c]; s = fma(v, v, s); }
            const double xnorm2 = wave64_sum_fast(s);
            const double alpha = row[r];
            double tau = 0.0, scal = 0.0, beta = alpha;
            if (xnorm2 > 0.0) {
                beta = -copysign(sqrt(fma(alpha, alpha, xnorm2)), alpha);
                tau = (beta - alpha) / beta;
                scal = 1.0 / (alpha - beta);
            }
            if (tid == 0) { taus[r] = tau; scl[r] = scal; betas[r] = beta; }
            for (int i = r + 1 + wave; tau != 0.0 && i < jb; i += nwaves) {   // wave w applies H_r to panel rows r+1+w, ...
                double* ri = Pn + (long long)i * ldp;
                double w = 0.0;
                for (int c = r + 1 + lane; c < len; c += 64) w = fma(ri[c], row[c], w);
                w = fma(scal, wave64_sum_fast(w), ri[r]);
                const double tws = tau * w * scal;
                for (int c = r + 1 + lane; c < len; c += 64) ri[c] = fma(-tws, row[c], ri[c]);
                if (lane == 0) ri[r] -= tau * w;
            }
            __syncthreads();
        }
        // ---- write the panel back (L entries, beta on the diagonal, scaled v to the right) and the explicit V ----
        for (int e = tid; e < QR_NB * len; e += TTN_WG) {
            const int r = e / len, c = e - r * len;
            if (r < jb) {
                const double x = Pn[(long long)r * ldp + c];
                const double out = (c < r) ? x : ((c == r) ? betas[r] : x * scl[r]);
                const double vv = (c < r) ? 0.0 : ((c == r) ? 1.0 : out);
                if (fastp) Pn[(long long)r * ldp + c] = vv;               // the LDS panel becomes V (same element, same thread)
                else Vb[(long long)r * len + c] = vv;
                M2[(long long)(j0 + r) * ld + j0 + c] = out;
            } else if (fastp) Pn[(long long)r * ldp + c] = 0.0;            // rows of V beyond a short last panel
        }
        __syncthreads();
        if (fastp) {                                                      // betas / scl (which live in Ss) have been consumed
            for (int e = tid; e < QR_NB * QR_NB; e += TTN_WG) Ss[e] = 0.0;
            __syncthreads();
        }
        const int rows_t = p - (j0 + jb);
        if (rows_t <= 0 && !Qout) break;
        View Vv = mkview(Vb, plain(len), plain(1));                       // jb x len
        // S = V V^T, then T (upper triangular): T[j][j] = tau_j ; T[i][j] = -tau_j * sum_{l=i}^{j-1} T[i][l] S[l][j]
        if (fastp) {
            // split-K MFMA: wave w sums its slice of k, the 16 partial tiles meet in Ss by LDS atomic adds
            const int li = lane & 15, lk = lane >> 4;
            const int kc = (((len + nwaves - 1) / nwaves) + 3) & ~3;
            const lds_f64* V = (const lds_f64*)Pn;
            mfma_acc_t acc = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
            for (int k0 = wave * kc; k0 < min(len, (wave + 1) * kc); k0 += 4) {
                const int kk = k0 + lk;
                const double a = (kk < len) ? V[li * ldp + kk] : 0.0;      // A[i][k] = V[i][k], B[k][j] = V[j][k]: the same register
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) atomicAdd(&Ss[(lk + 4 * reg) * QR_NB + li], acc[reg]);
            __syncthreads();
        } else {
            // panel too long for the LDS form (V is in global memory): 256 dot products, one wave each.  NOT a wg_gemm call: Ss is
            // LDS and the GEMM stores through global-address-space pointers (that call faulted on the first matrix long enough to
            // get here: q > 412 in the 512-thread build, q > 796 in the 1024-thread one)
            for (int e = wave; e < jb * jb; e += nwaves) {
                const int i = e / jb, j = e - i * jb;
                double a = 0.0;
                for (int c = lane; c < len; c += 64) a = fma(Vb[(long long)i * len + c], Vb[(long long)j * len + c], a);
                a = wave_sum(a);
                if (lane == 0) Ss[i * QR_NB + j] = a;
            }
            __syncthreads();
        }
        if (tid < QR_NB) {                                // lane i builds row i of T: it only needs its own row
            const int i = tid;
            for (int j = 0; j < QR_NB; ++j) Ts[i * QR_NB + j] = 0.0;
            if (i < jb) {
                Ts[i * QR_NB + i] = taus[i];
                for (int j = i + 1; j < jb; ++j) {
                    double acc = 0.0;
                    for (int l = i; l < j; ++l) acc = fma(Ts[i * QR_NB + l], Ss[l * QR_NB + j], acc);
                    Ts[i * QR_NB + j] = -taus[j] * acc;
                }
            }
        }
        __syncthreads();
        if (Qout) for (int e = tid; e < QR_NB * QR_NB; e += TTN_WG) Tst[(long long)(j0 / QR_NB) * QR_NB * QR_NB + e] = Ts[e];
        if (rows_t > 0 && fastp) {
            wg_block_reflector_apply(rows_t, len, M2 + (long long)(j0 + jb) * ld + j0, ld, Pn, ldp, Ts, false, Pn + (long long)QR_NB * ldp);
        } else if (rows_t > 0) {
            // W = C V^T (rows_t x jb), C = M2[j0+jb:, j0:] ; W <- W T ; C <- C - W V
            View Cv = mkview(M2 + (long long)(j0 + jb) * ld + j0, plain(ld), plain(1));
            View Wv = mkview(Wb, plain(QR_NB), plain(1));
            wg_gemm(rows_t, jb, len, Cv, tview(Vv), Wv, 1.0, 0.0, lds_gemm);
            for (int i = tid; i < rows_t; i += TTN_WG) {
                double w[QR_NB], o[QR_NB];
                for (int l = 0; l < jb; ++l) w[l] = Wb[(long long)i * QR_NB + l];
                for (int c = 0; c < jb; ++c) {
                    double acc = 0.0;
                    for (int l = 0; l <= c; ++l) acc = fma(w[l], Ts[l * QR_NB + c], acc);
                    o[c] = acc;
                }
                for (int c = 0; c < jb; ++c) Wb[(long long)i * QR_NB + c] = o[c];
            }
            __syncthreads();
            wg_gemm(rows_t, len, jb, Wv, Vv, Cv, -1.0, 1.0, lds_gemm);
        }
    }
    __syncthreads();
    if (!Qout) return;
    // ---- Q' = [I 0] H_{rr-1} ... H_0, panels in reverse: Qs <- Qs - ((Qs V^T) T^T) V on Qs = Q'[j0:, j0:] ----
    for (long long e = tid; e < (long long)rr * q; e += TTN_WG) { const int i = (int)(e / q), c = (int)(e - (long long)i * q); Qout[e] = (i == c) ? 1.0 : 0.0; }
    __syncthreads();
    for (int j0 = ((rr - 1) / QR_NB) * QR_NB; j0 >= 0; j0 -= QR_NB) {
        const int jb = min(QR_NB, rr - j0);
        const int len = q - j0;
        const int ldv = blkref_ldv(len);
        const bool fastp = (long long)QR_NB * ldv + 256 * (TTN_WG / 64) <= GEMM_LDS_DOUBLES;
        __syncthreads();
        if (fastp) {
            for (int e = tid; e < QR_NB * len; e += TTN_WG) {
                const int r = e / len, c = e - r * len;
                lds_gemm[(long long)r * ldv + c] = (r >= jb || c < r) ? 0.0 : ((c == r) ? 1.0 : M2[(long long)(j0 + r) * ld + j0 + c]);
            }
        } else
        for (int e = tid; e < jb * len; e += TTN_WG) {
            const int r = e / len, c = e - r * len;
            Vb[e] = (c < r) ? 0.0 : ((c == r) ? 1.0 : M2[(long long)(j0 + r) * ld + j0 + c]);
        }
        for (int e = tid; e < QR_NB * QR_NB; e += TTN_WG) Ts[e] = Tst[(long long)(j0 / QR_NB) * QR_NB * QR_NB + e];
        __syncthreads();
        const int rows_q = rr - j0;
        if (fastp) {
            wg_block_reflector_apply(rows_q, len, Qout + (long long)j0 * q + j0, q, lds_gemm, ldv, Ts, true, lds_gemm + (long long)QR_NB * ldv);
            continue;
        }
        View Vv = mkview(Vb, plain(len), plain(1));
        View Qs = mkview(Qout + (long long)j0 * q + j0, plain(q), plain(1));
        View Wv = mkview(Wb, plain(QR_NB), plain(1));
        wg_gemm(rows_q, jb, len, Qs, tview(Vv), Wv, 1.0, 0.0, lds_gemm);
        for (int i = tid; i < rows_q; i += TTN_WG) {       // W <- W T^T : o[c] = sum_{l >= c} w[l] T[c][l]
            double w[QR_NB], o[QR_NB];
            for (int l = 0; l < jb; ++l) w[l] = Wb[(long long)i * QR_NB + l];
            for (int c = 0; c < jb; ++c) {
                double acc = 0.0;
                for (int l = c; l < jb; ++l) acc = fma(w[l], Ts[c * QR_NB + l], acc);
                o[c] = acc;
            }
            for (int c = 0; c < jb; ++c) Wb[(long long)i * QR_NB + c] = o[c];
        }
        __syncthreads();
        wg_gemm(rows_q, len, jb, Wv, Vv, Qs, -1.0, 1.0, lds_gemm);
    }
    __syncthreads();
}
