// ttn_als_eig_kernels.h — the one-site eigensolvers als_eigsolve (src/solvers/als.jl:251-326, local problem K_eigmin :72-91) and
// als_gen_eigsolv (src/solvers/als.jl:344-426, local problem K_eiggenmin :93-105) for a batch of start trains and one operator (and one
// metric S): one workgroup owns one train for one stage of the schedule, at the stage's fixed ranks, like k_als_linsolve, whose
// environment updates and QR core moves it shares.  The host walks the stages: k_als_eig, then k_increase_ranks and ttn_orthogonalize.
//
// Local problem at site i: the unknown V (n_i, r_{i-1}, r_i) viewed as the na x nb matrix (na = n_i r_{i-1}, nb = r_i), and
//   K[(ab, c), (de, f)] = sum_z G_i[ab, de, z] H_i[z, c, f]    (the Kronecker sum wg_two_site_apply applies: G_i (na, na, R_i), H_i (R_i, nb, nb))
// symmetrised, K_s = 1/2 (K + K^T), as the two-site eigensolvers do.
//   standard     the smallest eigenpair of K_s.  Dense (wg_sym_eig_smallest) unless N > 2048 or (it_solver and N > itslv_thresh) — the
//                reference goes iterative only when both hold (als.jl:74) — then thick-restart Lanczos from the current core.
//   generalized  the smallest eigenpair of the pencil (K_s, S_s), S_s from a second set of environments of S.  Dense when !it_solver and
//                N <= min(itslv_thresh, 2048): S_s = L L^T (blocked workgroup Cholesky), C = L^-1 K_s L^-T, the smallest pair (mu, y) of C,
//                x = L^-T y.  Otherwise LOBPCG with block size 1 and no preconditioner (the reference's lobpcg(K, S, false, x0, 1;
//                maxiter = 500, tol = 1e-8), als.jl:96).  A Cholesky pivot <= 0 (S_s not positive definite) stops the train with
//                TTN_ST_SINGULAR.  The local vector leaves S-normalised (x^T S_s x = 1).
// Every local eigenvector leaves with a deterministic sign (wg_fix_sign), so a batch reproduces single calls bit for bit.
#pragma once
#include "ttn_eigsolve_kernels.h"

#define TTN_CHOL_NB 32
#define TTN_LOBPCG_MAXITER 500
#define TTN_LOBPCG_TOL 1.0e-8

// S = L L^T in place (N x N column-major, leading dimension N; the lower triangle receives L, the strict upper triangle is left
// with trailing-update garbage).  Panels of TTN_CHOL_NB columns are factored column by column; the trailing block gets
// A22 -= L21 L21^T as one MFMA GEMM (wg_gemm), as wg_lu_solve does.  Returns 1 if a pivot is <= 0 (or not finite): S is not
// positive definite.
__device__ __noinline__ int wg_chol_lower(int N, double* A, double* red, double* lds) {
    N = uni32(N); A = unip(A); red = unip(red); lds = unip(lds);
    const int tid = threadIdx.x;
    for (int k0 = 0; k0 < N; k0 += TTN_CHOL_NB) {
        const int w = min(TTN_CHOL_NB, N - k0);
        for (int j = k0; j < k0 + w; ++j) {
            double* colj = A + (long long)j * N;
            const double pivot = unif64(colj[j]);
            if (!(pivot > 0.0) || !(pivot <= 1.7976931348623157e308)) return 1;
            const double ljj = sqrt(pivot);
            __syncthreads();                                           // everybody has the pivot before it is overwritten
            for (int i = j + tid; i < N; i += TTN_WG) colj[i] = (i == j) ? ljj : colj[i] / ljj;
            __syncthreads();
            const int m = N - j - 1, nc = k0 + w - j - 1;             // the rest of the panel: A[i, c] -= L[i, j] L[c, j], i >= c
            for (long long e = tid; e < (long long)m * nc; e += TTN_WG) {
                const int i = j + 1 + (int)(e % m), c = j + 1 + (int)(e / m);
                if (i >= c) A[(long long)c * N + i] = fma(-colj[i], colj[c], A[(long long)c * N + i]);
            }
            __syncthreads();
        }
        const int m = N - k0 - w;
        if (m > 0) {
            const View L21 = mkview(A + (long long)k0 * N + (k0 + w), plain(1), plain(N));                 // m x w
            const View A22 = mkview(A + (long long)(k0 + w) * N + (k0 + w), plain(1), plain(N));           // m x m
            wg_gemm(m, m, w, L21, tview(L21), A22, -1.0, 1.0, lds);
        }
        __syncthreads();
    }
    return 0;
}

// B <- L^-1 B for the lower triangle L of wg_chol_lower (N x N, ld N) and B (N x nc, ld N), in place: block rows of TTN_CHOL_NB,
// each first takes the contribution of the rows above it (one MFMA GEMM), then is solved with its diagonal block staged in LDS,
// one thread per column.
__device__ __noinline__ void wg_trsm_lower(int N, int nc, const double* L, double* B, double* lds) {
    N = uni32(N); nc = uni32(nc); L = unip(L); B = unip(B); lds = unip(lds);
    const int tid = threadIdx.x;
    for (int k0 = 0; k0 < N; k0 += TTN_CHOL_NB) {
        const int w = min(TTN_CHOL_NB, N - k0);
        if (k0 > 0)
            wg_gemm(w, nc, k0, mkview(const_cast<double*>(L) + k0, plain(1), plain(N)), mkview(B, plain(1), plain(N)),
                    mkview(B + k0, plain(1), plain(N)), -1.0, 1.0, lds);
        __syncthreads();
        double* Lk = lds;                                               // [jj * NB + ii], ii >= jj
        for (int e = tid; e < TTN_CHOL_NB * TTN_CHOL_NB; e += TTN_WG) {
            const int ii = e % TTN_CHOL_NB, jj = e / TTN_CHOL_NB;
            Lk[e] = (ii < w && jj < w && ii >= jj) ? L[(long long)(k0 + jj) * N + k0 + ii] : (ii == jj ? 1.0 : 0.0);
        }
        __syncthreads();
        for (int c = tid; c < nc; c += TTN_WG) {
            double* col = B + (long long)c * N + k0;
            double u[TTN_CHOL_NB];
#pragma unroll
            for (int ii = 0; ii < TTN_CHOL_NB; ++ii) u[ii] = (ii < w) ? col[ii] : 0.0;
#pragma unroll
            for (int jj = 0; jj < TTN_CHOL_NB; ++jj) {
                u[jj] = u[jj] / Lk[jj * TTN_CHOL_NB + jj];
#pragma unroll
                for (int ii = jj + 1; ii < TTN_CHOL_NB; ++ii) u[ii] = fma(-Lk[jj * TTN_CHOL_NB + ii], u[jj], u[ii]);
            }
#pragma unroll
            for (int ii = 0; ii < TTN_CHOL_NB; ++ii) if (ii < w) col[ii] = u[ii];
        }
        __syncthreads();
    }
}

// y <- L^-T y (one vector, in place), by blocks of TTN_CHOL_NB from the bottom: the rows below a block contribute through one wave per
// column, the block's own upper triangle is solved by one thread.
__device__ __noinline__ void wg_trsv_lower_t(int N, const double* L, double* y) {
    N = uni32(N); L = unip(L); y = unip(y);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int kb = ((N - 1) / TTN_CHOL_NB) * TTN_CHOL_NB; kb >= 0; kb -= TTN_CHOL_NB) {
        const int w = min(TTN_CHOL_NB, N - kb), r0 = kb + w;
        for (int c = wave; c < w; c += TTN_NWAVES) {
            const double* col = L + (long long)(kb + c) * N;
            double a = 0.0;
            for (int i = r0 + lane; i < N; i += 64) a = fma(col[i], y[i], a);
            a = wave_sum(a);
            if (lane == 0) y[kb + c] -= a;
        }
        __syncthreads();
        if (tid == 0) {
            for (int c = w - 1; c >= 0; --c) {
                const double* col = L + (long long)(kb + c) * N;
                double a = y[kb + c];
                for (int q = c + 1; q < w; ++q) a = fma(-col[kb + q], y[kb + q], a);
                y[kb + c] = a / col[kb + c];
            }
        }
        __syncthreads();
    }
}

// The smallest eigenpair of the m x m pencil (Gk, Gs) (m <= 3, both symmetric, column-major with ld 3) by ONE thread: Gs = L L^T,
// C = L^-1 Gk L^-T, cyclic Jacobi on C, c = L^-T y.  Returns false if a pivot of Gs is below `piv_tol` times its diagonal entry
// (the basis is numerically dependent): the caller drops its last vector.
__device__ inline bool small_gen_eig(int m, const double* Gk, const double* Gs, double piv_tol, double* lam, double* c) {
    double L[9] = {0.0}, C[9], V[9];
    for (int j = 0; j < m; ++j) {
        double a = Gs[j + 3 * j];
        for (int q = 0; q < j; ++q) a -= L[j + 3 * q] * L[j + 3 * q];
        if (!(a > piv_tol * fabs(Gs[j + 3 * j])) || !(a > 0.0)) return false;
        L[j + 3 * j] = sqrt(a);
        for (int i = j + 1; i < m; ++i) {
            double b = Gs[i + 3 * j];
            for (int q = 0; q < j; ++q) b -= L[i + 3 * q] * L[j + 3 * q];
            L[i + 3 * j] = b / L[j + 3 * j];
        }
    }
    // C = L^-1 Gk L^-T: Y = L^-1 Gk (columns), then C = L^-1 Y^T
    double Y[9];
    for (int col = 0; col < m; ++col)
        for (int i = 0; i < m; ++i) {
            double a = Gk[i + 3 * col];
            for (int q = 0; q < i; ++q) a -= L[i + 3 * q] * Y[q + 3 * col];
            Y[i + 3 * col] = a / L[i + 3 * i];
        }
    for (int col = 0; col < m; ++col)
        for (int i = 0; i < m; ++i) {
            double a = Y[col + 3 * i];
            for (int q = 0; q < i; ++q) a -= L[i + 3 * q] * C[q + 3 * col];
            C[i + 3 * col] = a / L[i + 3 * i];
        }
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) { V[i + 3 * j] = (i == j) ? 1.0 : 0.0; if (i < j) { const double s = 0.5 * (C[i + 3 * j] + C[j + 3 * i]); C[i + 3 * j] = s; C[j + 3 * i] = s; } }
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < m; ++p) for (int q = p + 1; q < m; ++q) off += C[p + 3 * q] * C[p + 3 * q];
        if (!(off > 1.0e-300)) break;
        for (int p = 0; p < m; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = C[p + 3 * q];
                if (apq == 0.0) continue;
                const double th = (C[q + 3 * q] - C[p + 3 * p]) / (2.0 * apq);
                const double t = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < m; ++k) {                              // columns p, q
                    const double ckp = C[k + 3 * p], ckq = C[k + 3 * q];
                    C[k + 3 * p] = cs * ckp - sn * ckq; C[k + 3 * q] = sn * ckp + cs * ckq;
                }
                for (int k = 0; k < m; ++k) {                              // rows p, q
                    const double cpk = C[p + 3 * k], cqk = C[q + 3 * k];
                    C[p + 3 * k] = cs * cpk - sn * cqk; C[q + 3 * k] = sn * cpk + cs * cqk;
                }
                for (int k = 0; k < m; ++k) {
                    const double vkp = V[k + 3 * p], vkq = V[k + 3 * q];
                    V[k + 3 * p] = cs * vkp - sn * vkq; V[k + 3 * q] = sn * vkp + cs * vkq;
                }
            }
    }
    int jm = 0;
    for (int j = 1; j < m; ++j) if (C[j + 3 * j] < C[jm + 3 * jm]) jm = j;
    *lam = C[jm + 3 * jm];
    for (int i = m - 1; i >= 0; --i) {                                   // c = L^-T y
        double a = V[i + 3 * jm];
        for (int q = i + 1; q < m; ++q) a -= L[q + 3 * i] * c[q];
        c[i] = a / L[i + 3 * i];
    }
    for (int i = m; i < 3; ++i) c[i] = 0.0;
    return true;
}

// ---- LOBPCG, block size 1, no preconditioner, for the smallest eigenpair of the pencil (K_s, S_s) ----
// Both operators are applied matrix-free by wg_two_site_apply (A: GA, HA with RzA terms; S: GS, HS with RzS).  x: in = start vector,
// out = the S-normalised Ritz vector.  wv: 9 N doubles (x K x, S x, r, K r, S r, p, K p, S p), W: max(RzA, RzS) N (slab of the apply),
// sm: 64 doubles.  Each iteration applies K_s and S_s once (to the residual) and solves the Rayleigh-Ritz problem on [x, r, p]; p, then r,
// is dropped when the S-Gram matrix of the basis is numerically singular.  Stops at ||K_s x - lam S_s x|| <= tol or after maxiter
// iterations.  Returns the number of operator applications (K_s and S_s each count); -1 if x^T S_s x <= 0 (S_s not positive definite).
__device__ __noinline__ int wg_lobpcg_gen(int na, int nb, int RzA, double* GA, double* HA, int RzS, double* GS, double* HS, double* x, double* wv,
                                          double* W, double* sm, double tol, int maxiter, double* lam_out, double* res_out, double* red, double* lds) {
    na = uni32(na); nb = uni32(nb); RzA = uni32(RzA); RzS = uni32(RzS); maxiter = uni32(maxiter);
    GA = unip(GA); HA = unip(HA); GS = unip(GS); HS = unip(HS); x = unip(x); wv = unip(wv); W = unip(W); sm = unip(sm); red = unip(red); lds = unip(lds);
    const int tid = threadIdx.x;
    const long long N = (long long)na * nb;
    double *Kx = wv, *Sx = wv + N, *r = wv + 2 * N, *Kr = wv + 3 * N, *Sr = wv + 4 * N, *p = wv + 5 * N, *Kp = wv + 6 * N, *Sp = wv + 7 * N;
    int napply = 0;
    auto applyK = [&](double* v, double* out) { wg_two_site_apply(na, nb, RzA, GA, HA, v, out, W, lds); ++napply; };
    auto applyS = [&](double* v, double* out) { wg_two_site_apply(na, nb, RzS, GS, HS, v, out, W, lds); ++napply; };
    auto dot = [&](const double* u, const double* v) {
        double a = 0.0;
        for (long long i = tid; i < N; i += TTN_WG) a = fma(u[i], v[i], a);
        return unif64(wg_sum(a, red));
    };
    auto scale3 = [&](double s, double* u, double* ku, double* su) {
        for (long long i = tid; i < N; i += TTN_WG) { u[i] *= s; ku[i] *= s; su[i] *= s; }
        __syncthreads();
    };
    {
        double nx = dot(x, x);
        if (!(nx > 0.0)) {                                          // a vanishing start: the all-ones vector
            for (long long i = tid; i < N; i += TTN_WG) x[i] = 1.0;
            __syncthreads();
        }
    }
    applyK(x, Kx);
    applyS(x, Sx);
    const double xsx = dot(x, Sx);
    if (!(xsx > 0.0)) { *lam_out = 0.0; *res_out = 0.0; return -1; }
    scale3(1.0 / sqrt(xsx), x, Kx, Sx);
    double lam = dot(x, Kx), res = 0.0;
    bool have_p = false;
    for (int it = 0;; ++it) {
        for (long long i = tid; i < N; i += TTN_WG) r[i] = fma(-lam, Sx[i], Kx[i]);
        __syncthreads();
        res = sqrt(dot(r, r));
        if (res <= tol || it >= maxiter || N == 1) break;
        applyK(r, Kr);
        applyS(r, Sr);
        const double rsr = dot(r, Sr);
        if (!(rsr > 0.0)) break;                                    // r is S-null: no direction to add
        scale3(1.0 / sqrt(rsr), r, Kr, Sr);
        // the Gram matrices of [x, r, p]: one fused pass, 10 products
        double acc[10] = {0.0};
        for (long long i = tid; i < N; i += TTN_WG) {
            const double xi = x[i], ri = r[i];
            acc[0] = fma(xi, Kr[i], acc[0]); acc[1] = fma(ri, Kr[i], acc[1]); acc[2] = fma(xi, Sr[i], acc[2]);
            if (have_p) {
                const double pi = p[i];
                acc[3] = fma(pi, Kr[i], acc[3]); acc[4] = fma(pi, Sr[i], acc[4]);
                acc[5] = fma(xi, Kp[i], acc[5]); acc[6] = fma(xi, Sp[i], acc[6]);
                acc[7] = fma(pi, Kp[i], acc[7]); acc[8] = fma(pi, Sp[i], acc[8]);
                acc[9] = fma(ri, Kp[i], acc[9]);
            }
        }
        for (int q = 0; q < (have_p ? 10 : 3); ++q) acc[q] = unif64(wg_sum(acc[q], red));
        int m = (have_p && N >= 3) ? 3 : 2;
        if (tid == 0) {
            double Gk[9], Gs[9];
            Gk[0] = lam; Gs[0] = 1.0;
            Gk[1] = Gk[3] = acc[0]; Gs[1] = Gs[3] = acc[2];
            Gk[4] = acc[1]; Gs[4] = 1.0;
            Gk[2] = Gk[6] = have_p ? acc[5] : 0.0; Gs[2] = Gs[6] = have_p ? acc[6] : 0.0;
            Gk[5] = Gk[7] = have_p ? 0.5 * (acc[3] + acc[9]) : 0.0; Gs[5] = Gs[7] = have_p ? acc[4] : 0.0;
            Gk[8] = have_p ? acc[7] : 0.0; Gs[8] = have_p ? acc[8] : 1.0;
            double mu = lam, c[3] = {1.0, 0.0, 0.0};
            int mm = m;
            while (mm > 1 && !small_gen_eig(mm, Gk, Gs, 1.0e-12, &mu, c)) --mm;
            if (mm == 1) { mu = lam; c[0] = 1.0; c[1] = c[2] = 0.0; }
            // S-norm^2 of the new search direction c1 r + c2 p
            double ps = c[1] * c[1] * Gs[4] + c[2] * c[2] * Gs[8] + 2.0 * c[1] * c[2] * Gs[5];
            sm[0] = c[0]; sm[1] = c[1]; sm[2] = c[2]; sm[3] = mu; sm[4] = (double)mm; sm[5] = ps;
        }
        __syncthreads();
        const double c0 = unif64(sm[0]), c1 = unif64(sm[1]), c2 = unif64(sm[2]), ps = unif64(sm[5]);
        const int mm = (int)unif64(sm[4]);
        __syncthreads();
        if (mm == 1) break;                                         // no independent direction left: x is as good as it gets
        const double pn = ps > 0.0 ? 1.0 / sqrt(ps) : 0.0;
        for (long long i = tid; i < N; i += TTN_WG) {
            const double np = c1 * r[i] + (mm == 3 ? c2 * p[i] : 0.0);
            const double nkp = c1 * Kr[i] + (mm == 3 ? c2 * Kp[i] : 0.0);
            const double nsp = c1 * Sr[i] + (mm == 3 ? c2 * Sp[i] : 0.0);
            x[i] = fma(c0, x[i], np); Kx[i] = fma(c0, Kx[i], nkp); Sx[i] = fma(c0, Sx[i], nsp);
            p[i] = np * pn; Kp[i] = nkp * pn; Sp[i] = nsp * pn;
        }
        __syncthreads();
        have_p = pn > 0.0;
        const double s2 = dot(x, Sx);
        if (!(s2 > 0.0)) { *lam_out = lam; *res_out = res; return -1; }
        scale3(1.0 / sqrt(s2), x, Kx, Sx);
        lam = dot(x, Kx);
    }
    *lam_out = lam;
    *res_out = res;
    return napply;
}

// ---- the sweep kernel: one stage of the schedule at fixed ranks ----
struct AlsEigArgs {
    TTODev A, S;                 // S: the metric of the generalized problem (gen = 1)
    TTDev x;
    int gen, nsweeps;
    double* scratch;
    long long scratch_stride;
    const long long* off;        // device [4][d]: offsets of G_i, GS_i, H_i, HS_i in the per-train scratch
    long long offK, offK2, offEig, offPb, offT1, offT2, offTm, offQb, offRb, offVb, offWb, offTst, offIt;
    long long it_nmax;           // iterative area: Lanczos V (m+1) N, tmp KEEP N, W Rz N, small workspace; LOBPCG 9 N, W Rz N, 64
    int it_above;                // local problems with more unknowns go to the matrix-free branch
    int lz_maxrestart;
    double lz_tol;
    int* status;                 // [batch]
    double* hist_E;              // [batch][hist_len], this stage from hist_off on
    int hist_len, hist_off;
    int* it_count;               // [batch] operator applications of the matrix-free solves (accumulated over stages)
    double* it_res;              // [batch] largest final residual of the matrix-free solves
};

#define XC(i) (E.x.data + (long long)E.tb * E.x.stride + E.x.off[i])
#define WG_FOR(total) for (long long e_ = threadIdx.x; e_ < (long long)(total); e_ += TTN_WG)

__global__ void __launch_bounds__(TTN_WG) k_als_eig(AlsEigArgs R) {
    extern __shared__ double lds[];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int d = R.x.d;
    {
        const int st = R.status[b];                  // an earlier stage stopped this train
        if (st == TTN_ST_SINGULAR || st == TTN_ST_NONFINITE) return;
    }
    double* scr = R.scratch + (long long)b * R.scratch_stride;
    double* red = lds + GEMM_LDS_TOTAL;
    int* iflag = reinterpret_cast<int*>(red + 32 + 2 * QR_NB * QR_NB + QR_NB + 8);
    long long* xr = R.x.rks + (long long)b * (d + 1);
    AlsEnv E;
    E.A = R.A; E.b = R.x; E.x = R.x; E.tb = b; E.scr = scr; E.off = R.off; E.xr = xr; E.br = xr;
    E.T1 = scr + R.offT1; E.T2 = scr + R.offT2; E.d = d;
    AlsEnv ES = E;                                   // the metric's environments: GS_i, HS_i in the slots off[d + i], off[3d + i]
    ES.A = R.S; ES.off = R.off + d;
    AlsMove Mv;
    Mv.W.Vb = scr + R.offVb; Mv.W.Wb = scr + R.offWb; Mv.W.Tst = scr + R.offTst;
    Mv.W.red = red; Mv.W.Ts = red + 32; Mv.W.Ss = Mv.W.Ts + QR_NB * QR_NB; Mv.W.taus = Mv.W.Ss + QR_NB * QR_NB;
    Mv.Tm = scr + R.offTm; Mv.Qb = scr + R.offQb; Mv.Rb = scr + R.offRb;
    double* K = scr + R.offK;
    double* K2 = scr + R.offK2;
    double* Pb = scr + R.offPb;
    const bool gen = R.gen != 0;

    // ---- initial environments (als.jl:268-276, :360-368): G_1 = A_1, H from the right ----
    auto init_env = [&](const AlsEnv& En) {
        const int n0 = uni32(R.x.dims[0]), R1 = uni32((int)En.A.rks[1]);
        double* g0 = En.scr + En.off[0];
        const double* a0 = En.A.data + En.A.off[0];
        WG_FOR((long long)n0 * n0 * R1) g0[e_] = a0[e_];
        if (tid == 0) (En.scr + En.off[2 * d + d - 1])[0] = 1.0;
        __syncthreads();
        for (int i = d - 1; i >= 1; --i) als_update_H_op(En, i);
    };
    init_env(E);
    if (gen) init_env(ES);

    int it_count = 0;
    double it_res = 0.0;
    bool it_fail = false;
    int status = 0;
    // local eigenproblem of site i: the eigenvector into Pb as (n, r_{i-1}, r_i) column-major; returns lambda
    auto local = [&](int i) -> double {
        const int n = uni32(R.x.dims[i]), rl = uni32((int)xr[i]), rr = uni32((int)xr[i + 1]);
        const int na = n * rl, nb = rr, N = na * nb;
        const int Rz = uni32((int)R.A.rks[i + 1]), RzS = gen ? uni32((int)R.S.rks[i + 1]) : 1;
        double* Gi = scr + R.off[i];
        double* Hi = scr + R.off[2 * d + i];
        double* GSi = scr + R.off[d + i];
        double* HSi = scr + R.off[3 * d + i];
        double lam = 0.0;
        if (N > R.it_above) {
            double* xi = XC(i);
            WG_FOR(N) Pb[e_] = xi[e_];                                   // start from the current core (als.jl:78, :96)
            __syncthreads();
            double* it = scr + R.offIt;
            double res = 0.0;
            if (!gen) {
                double* V = it;
                double* tmp = V + (long long)(TTN_LZ_M + 1) * R.it_nmax;
                double* W = tmp + (long long)TTN_LZ_KEEP * R.it_nmax;
                double* sm = W + (long long)Rz * R.it_nmax;
                it_count += wg_lanczos_smallest(na, nb, Rz, Gi, Hi, Pb, V, tmp, W, sm, R.lz_tol, R.lz_maxrestart, &lam, &res, red, lds);
                if (!(res <= 1.0e3 * R.lz_tol)) it_fail = true;
            } else {
                double* wv = it;
                double* W = wv + 9 * R.it_nmax;
                double* sm = W + (long long)max(Rz, RzS) * R.it_nmax;
                const int na_ = wg_lobpcg_gen(na, nb, Rz, Gi, Hi, RzS, GSi, HSi, Pb, wv, W, sm, TTN_LOBPCG_TOL, TTN_LOBPCG_MAXITER, &lam, &res, red, lds);
                if (na_ < 0) { status = TTN_ST_SINGULAR; return 0.0; }
                it_count += na_;
                if (!(res <= 1.0e3 * TTN_LOBPCG_TOL)) it_fail = true;
            }
            it_res = fmax(it_res, res);
        } else {
            auto assemble = [&](double* M, const double* G, const double* H, int Rq) {
                WG_FOR((long long)N * N) {
                    const int row = (int)(e_ % N), col = (int)(e_ / N);
                    const int ab = row % na, c = row / na, de = col % na, f = col / na;
                    double a = 0.0;
                    for (int z = 0; z < Rq; ++z) a = fma(G[ab + (long long)na * (de + (long long)na * z)], H[z + Rq * (c + (long long)nb * f)], a);
                    M[e_] = a;
                }
                __syncthreads();
                WG_FOR((long long)N * N) {                                  // 1/2 (M + M^T)
                    const int row = (int)(e_ % N), col = (int)(e_ / N);
                    if (row < col) {
                        const double s = 0.5 * (M[e_] + M[col + (long long)N * row]);
                        M[e_] = s; M[col + (long long)N * row] = s;
                    }
                }
                __syncthreads();
            };
            assemble(K, Gi, Hi, Rz);
            double* ew = scr + R.offEig;
            if (gen) {
                assemble(K2, GSi, HSi, RzS);
                if (wg_chol_lower(N, K2, red, lds)) { status = TTN_ST_SINGULAR; return 0.0; }
                wg_trsm_lower(N, N, K2, K, lds);                            // Y = L^-1 K_s
                WG_FOR((long long)N * N) {                                  // Y^T = K_s L^-T
                    const int row = (int)(e_ % N), col = (int)(e_ / N);
                    if (row < col) { const double t = K[e_]; K[e_] = K[col + (long long)N * row]; K[col + (long long)N * row] = t; }
                }
                __syncthreads();
                wg_trsm_lower(N, N, K2, K, lds);                            // C = L^-1 K_s L^-T
                WG_FOR((long long)N * N) {
                    const int row = (int)(e_ % N), col = (int)(e_ / N);
                    if (row < col) {
                        const double s = 0.5 * (K[e_] + K[col + (long long)N * row]);
                        K[e_] = s; K[col + (long long)N * row] = s;
                    }
                }
                __syncthreads();
            }
            wg_sym_eig_smallest(N, K, N, 1, ew, Pb, N, ew + 8, red);
            lam = unif64(ew[0]);
            if (gen) wg_trsv_lower_t(N, K2, Pb);                            // x = L^-T y: x^T S_s x = y^T y = 1
        }
        if (!wg_fix_sign(N, Pb, red, iflag) || !(fabs(lam) <= 1.7976931348623157e308)) status = TTN_ST_NONFINITE;
        return lam;
    };

    double* hE = R.hist_E + (long long)b * R.hist_len + R.hist_off;
    int t = 0;
    for (int sw = 0; sw < R.nsweeps && !status; ++sw) {
        for (int i = 0; i < d - 1; ++i) {                                   // first half sweep (als.jl:302-309)
            const double lam = local(i);
            if (status) break;
            if (tid == 0) hE[t] = lam;
            ++t;
            als_right_core_move(E, Mv, Pb, i, lds);
            als_update_G_op(E, i);
            if (gen) als_update_G_op(ES, i);
        }
        if (status) break;
        for (int i = d - 1; i >= 1; --i) {                                  // second half sweep (als.jl:312-318)
            const double lam = local(i);
            if (status) break;
            if (tid == 0) hE[t] = lam;
            ++t;
            als_left_core_move(E, Mv, Pb, i, lds);
            als_update_H_op(E, i);
            if (gen) als_update_H_op(ES, i);
        }
    }
    if (it_fail && !status) status = TTN_ST_LANCZOS;
    if (tid == 0) {
        if (status) ttn_set_status(&R.status[b], status);
        R.it_count[b] += it_count;
        R.it_res[b] = fmax(R.it_res[b], it_res);
    }
}

// ---- stage transition: increase_ranks (src/tt_tools.jl:443-489) into a second handle ----
// Core i of y = core i of x zero-padded to (n_i, rn_i, rn_{i+1}); with noise != 0 the new blocks get noise * Q as increase_ranks_noise places
// them (only r_i grows: the new right columns; only r_{i-1}: the new left rows; both: the corner block), Q orthonormal like rand_orthogonal.
// Q comes from a splitmix64 stream keyed by (seed, site, entry) — not by the train — and a Householder QR, so the batch gives the trains
// of single calls.  Scratch per train: Tm, Qb (mm x rr doubles each), Rb, Vb, Wb, Tst as for the core moves.
struct IncArgs {
    TTDev x, y;
    const long long* rn;         // device [d+1]: the new ranks
    double noise;
    unsigned long long seed;
    double* scratch;
    long long scratch_stride, offTm, offQb, offRb, offVb, offWb, offTst;
};

__device__ inline double inc_noise_entry(unsigned long long seed, int site, long long entry) {
    unsigned long long z = seed * 0xD1B54A32D192ED03ull + ((unsigned long long)(site + 1) << 40) + (unsigned long long)entry + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-52 - 1.0;
}

__global__ void __launch_bounds__(TTN_WG) k_increase_ranks(IncArgs P) {
    extern __shared__ double lds[];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int d = P.x.d;
    double* scr = P.scratch + (long long)b * P.scratch_stride;
    double* red = lds + GEMM_LDS_TOTAL;
    OrthoWork W;
    W.Vb = scr + P.offVb; W.Wb = scr + P.offWb; W.Tst = scr + P.offTst;
    W.red = red; W.Ts = red + 32; W.Ss = W.Ts + QR_NB * QR_NB; W.taus = W.Ss + QR_NB * QR_NB;
    double* Tm = scr + P.offTm; double* Qb = scr + P.offQb; double* Rb = scr + P.offRb;
    const long long* xr = P.x.rks + (long long)b * (d + 1);
    long long* yr = P.y.rks + (long long)b * (d + 1);
    for (int i = 0; i < d; ++i) {
        const int n = uni32(P.x.dims[i]);
        const int rl0 = uni32((int)xr[i]), rr0 = uni32((int)xr[i + 1]);
        const int rl = uni32((int)P.rn[i]), rr = uni32((int)P.rn[i + 1]);
        const double* xc = P.x.data + (long long)b * P.x.stride + P.x.off[i];
        double* yc = P.y.data + (long long)b * P.y.stride + P.y.off[i];
        WG_FOR((long long)n * rl * rr) {
            long long t = e_; const int a = t % n; t /= n; const int bq = t % rl; const int c = (int)(t / rl);
            yc[e_] = (bq < rl0 && c < rr0) ? xc[a + (long long)n * (bq + (long long)rl0 * c)] : 0.0;
        }
        __syncthreads();
        if (P.noise == 0.0) continue;
        // the new block: mq x nq orthonormal (columns if mq >= nq, else rows), as a linear array reshaped to (n, bl, bc) column-major,
        // placed at rows rlo.., columns rco.. of the core
        int mq, nq, bl, bc, rlo, rco;
        if (rl == rl0 && rr > rr0) { mq = n * rl; nq = rr - rr0; bl = rl; bc = rr - rr0; rlo = 0; rco = rr0; }
        else if (rr == rr0 && rl > rl0) { mq = rl - rl0; nq = n * rr; bl = rl - rl0; bc = rr; rlo = rl0; rco = 0; }
        else if (rl > rl0 && rr > rr0) { mq = (rl - rl0) * n; nq = rr - rr0; bl = rl - rl0; bc = rr - rr0; rlo = rl0; rco = rr0; }
        else continue;
        const bool tr = mq < nq;                                    // orthonormal rows: QR of the transpose
        const int tm = tr ? nq : mq, tn = tr ? mq : nq;
        WG_FOR((long long)tm * tn) Tm[e_] = inc_noise_entry(P.seed, i, e_);
        __syncthreads();
        wg_qr_explicit(tm, tn, Tm, Qb, Rb, W, lds);
        WG_FOR((long long)mq * nq) {
            const int row = (int)(e_ % mq), col = (int)(e_ / mq);
            const double q = tr ? Qb[col + (long long)tm * row] : Qb[e_];
            long long t = e_; const int a = t % n; t /= n; const int bq = t % bl; const int c = (int)(t / bl);
            (void)bc;
            yc[a + (long long)n * ((rlo + bq) + (long long)rl * (rco + c))] = P.noise * q;
        }
        __syncthreads();
    }
    if (tid <= d) yr[tid] = P.rn[tid];
}
#undef XC
#undef WG_FOR
