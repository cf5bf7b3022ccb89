// ttn_eigsolve_kernels.h — the two-site eigensolvers dmrg_eigsolve (src/solvers/dmrg.jl:501-578, local problem K_eigmin :235-259) and
// mals_eigsolve (src/solvers/mals.jl:335-425, local problem K_eigmin_mals :171-217) for a batch of start trains and one operator: one
// workgroup owns one train for the whole solve, like k_mals_linsolve, whose window walk, rank rules and SVD core moves it shares.
//
// Local problem: the smallest eigenpair of the symmetrised two-site operator K_s = 1/2 (K + K^T), K[(ab,cd),(ef,gh)] = sum_z G_z[ab,ef] H_z[cd,gh]
// on the na x nb unknown (na = n_i r_i, nb = n_{i+1} r_{i+2}).  Two branches, chosen per local problem like the reference:
//   dense        (N <= threshold, N <= TTN_DENSE_LOCAL_MAX): K assembled and symmetrised, Householder tridiagonalisation by the workgroup,
//                the eigenvalue by multisection on Sturm counts, its vector by inverse iteration on the tridiagonal, back-transformed by the
//                stored reflectors (wg_sym_eig_smallest).  The reference calls LAPACK (eigen(Hermitian(K), 1:1)).
//   matrix-free  thick-restart Lanczos (wg_lanczos_smallest) on wg_two_site_apply, Krylov dimension TTN_LZ_M (KrylovKit's default 30),
//                full reorthogonalisation against the basis, at most `maxiter` restarts, stopped when the residual norm of the
//                normalised Ritz vector is <= tol.  The reference uses KrylovKit eigsolve (DMRG) and IterativeSolvers lobpcg (MALS): all
//                three converge to the same eigenpair to `tol`, not to the same rounding.
// Every local eigenvector leaves with a deterministic sign: its entry of largest modulus (the first such) is positive.
#pragma once
#include "ttn_als_kernels.h"

#define TTN_LZ_M 30                  // Krylov dimension of the matrix-free branch (KrylovKit.KrylovDefaults.krylovdim)
#define TTN_LZ_KEEP 10               // Ritz vectors kept by a thick restart
#define TTN_LZ_LD 32                 // leading dimension of the projected matrices

// Workgroup maximum of values of any sign (wg_max pads the missing waves with 0.0, which is right for the moduli it is used on).
__device__ inline double wg_max_signed(double v, double* red) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    double t = (l < nw) ? red[l] : -1.7976931348623157e308;
    __syncthreads();
    return wave_max(t);
}

// ---- Householder tridiagonalisation of a symmetric N x N matrix (column-major, leading dimension ld, both triangles stored) ----
// T = Q^T A Q with Q = H_0 H_1 ... H_{N-3}, H_k = I - tau_k v_k v_k^T, v_k = (0..0, 1, A[k+2:N, k]) (the unit entry at k+1 implicit).
// dg[0..N), e[0..N-1): the tridiagonal.  vw: 2N doubles of global scratch.  The trailing block is updated in full (both triangles).
__device__ __noinline__ void wg_sym_tridiag(int N, double* A, int ld, double* dg, double* e, double* tau, double* vw, double* red) {
    N = uni32(N); ld = uni32(ld); A = unip(A); dg = unip(dg); e = unip(e); tau = unip(tau); vw = unip(vw); red = unip(red);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* v = vw;
    double* p = vw + N;
    for (int k = 0; k + 2 < N; ++k) {
        const int m = N - k - 1;                                 // length of the reflector (rows k+1 .. N-1)
        double* x = A + (long long)k * ld + k + 1;
        double s2 = 0.0;
        for (int i = 1 + tid; i < m; i += TTN_WG) s2 = fma(x[i], x[i], s2);
        s2 = unif64(wg_sum(s2, red));
        const double alpha = unif64(x[0]);
        double tk = 0.0, beta = alpha, scale = 0.0;
        if (s2 > 0.0) {
            beta = -copysign(sqrt(fma(alpha, alpha, s2)), alpha);
            tk = (beta - alpha) / beta;
            scale = 1.0 / (alpha - beta);
        }
        for (int i = tid; i < m; i += TTN_WG) v[i] = (i == 0) ? 1.0 : x[i] * scale;
        if (tid == 0) { tau[k] = tk; e[k] = beta; dg[k] = A[(long long)k * ld + k]; }
        __syncthreads();
        if (tk != 0.0) {
            // p = tau A22 v: one wave per column of A22 (columns are rows by symmetry)
            double* A22 = A + (long long)(k + 1) * ld + k + 1;
            for (int c = wave; c < m; c += TTN_NWAVES) {
                const double* col = A22 + (long long)c * ld;
                double a = 0.0;
                for (int i = lane; i < m; i += 64) a = fma(col[i], v[i], a);
                a = wave_sum(a);
                if (lane == 0) p[c] = tk * a;
            }
            __syncthreads();
            double pv = 0.0;
            for (int i = tid; i < m; i += TTN_WG) pv = fma(p[i], v[i], pv);
            pv = unif64(wg_sum(pv, red));
            const double h = 0.5 * tk * pv;
            for (int i = tid; i < m; i += TTN_WG) p[i] = fma(-h, v[i], p[i]);      // w = p - (tau/2)(p^T v) v
            __syncthreads();
            for (long long t = tid; t < (long long)m * m; t += TTN_WG) {            // A22 -= v w^T + w v^T
                const int i = (int)(t % m), c = (int)(t / m);
                double* a = A22 + (long long)c * ld + i;
                *a = fma(-v[i], p[c], fma(-p[i], v[c], *a));
            }
        }
        for (int i = 1 + tid; i < m; i += TTN_WG) x[i] = v[i];                     // the reflector below the subdiagonal
        __syncthreads();
    }
    if (tid == 0) {
        if (N >= 2) {
            dg[N - 2] = A[(long long)(N - 2) * ld + N - 2];
            e[N - 2] = A[(long long)(N - 2) * ld + N - 1];
            tau[N - 2] = 0.0;
        }
        dg[N - 1] = A[(long long)(N - 1) * ld + N - 1];
    }
    __syncthreads();
}

// Number of eigenvalues of the tridiagonal (dg, e) below x (Sturm count of the LDL^T pivots; a vanishing pivot is replaced by -pivmin).
__device__ inline int tri_sturm_count(int N, const double* dg, const double* e, double x, double pivmin) {
    int c = 0;
    double q = dg[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    c += q < 0.0;
    for (int i = 1; i < N; ++i) {
        q = (dg[i] - x) - e[i - 1] * (e[i - 1] / q);
        if (fabs(q) < pivmin) q = -pivmin;
        c += q < 0.0;
    }
    return c;
}

// Eigenvalue j (0-based, ascending) of the tridiagonal by multisection: every thread counts at its own point of the bracket, the bracket
// shrinks by a factor TTN_WG + 1 per round.  Uniform result.
__device__ __noinline__ double wg_tri_eigval(int N, const double* dg, const double* e, int j, double* red) {
    N = uni32(N); j = uni32(j); dg = unip(dg); e = unip(e); red = unip(red);
    double lo = 1.0e300, hi = -1.0e300, tn = 0.0;
    for (int i = 0; i < N; ++i) {                               // Gershgorin bracket
        const double r = (i > 0 ? fabs(e[i - 1]) : 0.0) + (i + 1 < N ? fabs(e[i]) : 0.0);
        lo = fmin(lo, dg[i] - r); hi = fmax(hi, dg[i] + r);
        tn = fmax(tn, fabs(dg[i]) + r);
    }
    const double eps = 2.220446049250313e-16;
    const double pivmin = fmax(tn * 1.0e-300, 2.2250738585072014e-308) + 0.0;
    lo -= 2.0 * eps * tn + pivmin; hi += 2.0 * eps * tn + pivmin;
    for (int round = 0; round < 12; ++round) {
        if (hi - lo <= 2.0 * eps * fmax(fabs(lo), fabs(hi)) + pivmin) break;
        const double step = (hi - lo) / (TTN_WG + 1);
        const double x = lo + (threadIdx.x + 1) * step;
        const bool above = tri_sturm_count(N, dg, e, x, pivmin) > j;
        const double nlo = unif64(wg_max_signed(above ? -1.0e300 : x, red));
        const double nhi = -unif64(wg_max_signed(above ? -x : -1.0e300, red));
        if (nlo > lo) lo = nlo;
        if (nhi < hi) hi = nhi;
    }
    return 0.5 * (lo + hi);
}

// Inverse iteration for the eigenvector of the tridiagonal (dg, e) at the eigenvalue lam, by ONE thread: Gaussian elimination with
// partial pivoting of T - lam I (pivots below eps ||T|| replaced by eps ||T||), three solves from a fixed start vector, unit 2-norm.
// y: N doubles; w: 5N doubles of scratch.
__device__ void tri_inverse_iteration(int N, const double* dg, const double* e, double lam, double* y, double* w) {
    double* u0 = w; double* u1 = w + N; double* u2 = w + 2 * N; double* l = w + 3 * N; double* sw = w + 4 * N;
    double tn = 0.0;
    for (int i = 0; i < N; ++i) tn = fmax(tn, fabs(dg[i]) + (i > 0 ? fabs(e[i - 1]) : 0.0) + (i + 1 < N ? fabs(e[i]) : 0.0));
    const double tiny = fmax(tn * 2.220446049250313e-16, 1.0e-300);
    double dc = dg[0] - lam, fc = N > 1 ? e[0] : 0.0;
    for (int i = 0; i + 1 < N; ++i) {
        const double sub = e[i], an = dg[i + 1] - lam, ns = (i + 2 < N) ? e[i + 1] : 0.0;
        if (fabs(dc) >= fabs(sub)) {
            const double piv = fabs(dc) < tiny ? copysign(tiny, dc) : dc;
            const double m = sub / piv;
            u0[i] = piv; u1[i] = fc; u2[i] = 0.0; l[i] = m; sw[i] = 0.0;
            dc = an - m * fc; fc = ns;
        } else {
            const double m = dc / sub;
            u0[i] = sub; u1[i] = an; u2[i] = ns; l[i] = m; sw[i] = 1.0;
            dc = fc - m * an; fc = -m * ns;
        }
    }
    u0[N - 1] = fabs(dc) < tiny ? copysign(tiny, dc) : dc;
    for (int i = 0; i < N; ++i) y[i] = 1.0 + 0.5 * sin(1.0 + 0.7 * i);            // fixed start, no symmetry to be orthogonal to
    for (int it = 0; it < 3; ++it) {
        for (int i = 0; i + 1 < N; ++i) {                                           // L^-1 (with the row interchanges)
            if (sw[i] != 0.0) { const double t = y[i]; y[i] = y[i + 1]; y[i + 1] = t; }
            y[i + 1] -= l[i] * y[i];
        }
        for (int i = N - 1; i >= 0; --i) {                                          // U^-1
            double a = y[i];
            if (i + 1 < N) a -= u1[i] * y[i + 1];
            if (i + 2 < N) a -= u2[i] * y[i + 2];
            y[i] = a / u0[i];
        }
        double mx = 0.0;
        for (int i = 0; i < N; ++i) mx = fmax(mx, fabs(y[i]));
        double s = 0.0;
        for (int i = 0; i < N; ++i) { y[i] /= mx; s = fma(y[i], y[i], s); }
        s = 1.0 / sqrt(s);
        for (int i = 0; i < N; ++i) y[i] *= s;
    }
}

// Entry i of the fixed pseudo-random start vector of a recomputed vector j: uniform in [-1, 1) (splitmix64 of (j, i)), the same on every run.
__device__ inline double tri_restart_entry(int i, int j) {
    unsigned long long z = ((unsigned long long)(j + 1) << 32) + (unsigned long long)i + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-52 - 1.0;
}

// y_j -= sum_q (y_q^T y_j) y_q over the columns q < j of Y (modified Gram-Schmidt, one pass), by ONE thread.
__device__ inline void tri_mgs(int N, const double* Y, int ldy, int j, double* yj) {
    for (int q = 0; q < j; ++q) {
        const double* yq = Y + (long long)q * ldy;
        double s = 0.0;
        for (int i = 0; i < N; ++i) s = fma(yq[i], yj[i], s);
        for (int i = 0; i < N; ++i) yj[i] = fma(-s, yq[i], yj[i]);
    }
}

// Vector j again, when the one from the common start collapsed under Gram-Schmidt (its eigenvalue repeats an earlier one to working
// precision, so inverse iteration found an earlier vector's direction): three solves with the factors tri_inverse_iteration left in w
// (T - lam_j I), from the pseudo-random start of j, each iterate orthogonalised (twice) against the columns q < j of Y before the solve
// and once more at the end (LAPACK dstein's reorthogonalisation inside a cluster).  By ONE thread; y_j = Y column j, not normalised.
__device__ void tri_inverse_iteration_restart(int N, const double* w, double* Y, int ldy, int j) {
    const double* u0 = w; const double* u1 = w + N; const double* u2 = w + 2 * N; const double* l = w + 3 * N; const double* sw = w + 4 * N;
    double* y = Y + (long long)j * ldy;
    for (int i = 0; i < N; ++i) y[i] = tri_restart_entry(i, j);
    for (int it = 0; it < 3; ++it) {
        tri_mgs(N, Y, ldy, j, y);
        tri_mgs(N, Y, ldy, j, y);
        for (int i = 0; i + 1 < N; ++i) {
            if (sw[i] != 0.0) { const double t = y[i]; y[i] = y[i + 1]; y[i + 1] = t; }
            y[i + 1] -= l[i] * y[i];
        }
        for (int i = N - 1; i >= 0; --i) {
            double a = y[i];
            if (i + 1 < N) a -= u1[i] * y[i + 1];
            if (i + 2 < N) a -= u2[i] * y[i + 2];
            y[i] = a / u0[i];
        }
        double mx = 0.0;
        for (int i = 0; i < N; ++i) mx = fmax(mx, fabs(y[i]));
        double s = 0.0;
        for (int i = 0; i < N; ++i) { y[i] /= mx; s = fma(y[i], y[i], s); }
        s = 1.0 / sqrt(s);
        for (int i = 0; i < N; ++i) y[i] *= s;
    }
    tri_mgs(N, Y, ldy, j, y);
    tri_mgs(N, Y, ldy, j, y);
}

// y <- Q y for the reflectors wg_sym_tridiag left in A (H_{N-3} first), by ONE wave (the caller picks it).
__device__ void wave_tri_backtransform(int N, const double* A, int ld, const double* tau, double* y) {
    const int lane = threadIdx.x & 63;
    for (int k = N - 3; k >= 0; --k) {
        const double tk = tau[k];
        if (tk == 0.0) continue;
        const double* v = A + (long long)k * ld + k + 1;
        const int m = N - k - 1;
        double a = 0.0;
        for (int i = lane; i < m; i += 64) a = fma(i == 0 ? 1.0 : v[i], y[k + 1 + i], a);
        a = tk * wave_sum(a);
        for (int i = lane; i < m; i += 64) y[k + 1 + i] = fma(-a, i == 0 ? 1.0 : v[i], y[k + 1 + i]);
    }
}

// Flip the sign of v (length N) so that its first entry of largest modulus is positive.  iflag: one LDS int.  Returns false, and leaves v
// as it is, if an entry is NaN or infinite (they enter the maximum as +inf: fmax alone would drop a NaN, and an all-NaN v would find no
// entry equal to the maximum and index v[0x7fffffff]).
__device__ bool wg_fix_sign(long long N, double* v, double* red, int* iflag) {
    double vm = 0.0;
    for (long long i = threadIdx.x; i < N; i += TTN_WG) {
        const double a = fabs(v[i]);
        vm = fmax(vm, a <= 1.7976931348623157e308 ? a : __builtin_inf());
    }
    if (threadIdx.x == 0) *iflag = 0x7fffffff;
    vm = unif64(wg_max(vm, red));
    if (!(vm <= 1.7976931348623157e308)) return false;      // uniform: no barrier is skipped by part of the workgroup
    for (long long i = threadIdx.x; i < N; i += TTN_WG) if (fabs(v[i]) == vm) atomicMin(iflag, (int)i);
    __syncthreads();
    const int im = uni32(*iflag);
    const bool neg = im < N && v[im] < 0.0;
    __syncthreads();
    if (neg) for (long long i = threadIdx.x; i < N; i += TTN_WG) v[i] = -v[i];
    __syncthreads();
    return true;
}

// The k smallest eigenpairs of the symmetric N x N matrix A (ld, destroyed): lam[0..k), the orthonormal vectors as the columns of Y
// (N x k, leading dimension ldy).  work: 3N + 5N k doubles.  k <= TTN_NWAVES (one wave back-transforms one vector).
__device__ __noinline__ void wg_sym_eig_smallest(int N, double* A, int ld, int k, double* lam, double* Y, int ldy, double* work, double* red) {
    N = uni32(N); k = uni32(k); ld = uni32(ld); ldy = uni32(ldy); A = unip(A); lam = unip(lam); Y = unip(Y); work = unip(work); red = unip(red);
    double* dg = work; double* e = work + N; double* tau = work + 2 * N; double* vw = work + 3 * N;
    if (N == 1) {
        if (threadIdx.x == 0) { lam[0] = A[0]; Y[0] = 1.0; }
        __syncthreads();
        return;
    }
    wg_sym_tridiag(N, A, ld, dg, e, tau, vw, red);
    for (int j = 0; j < k; ++j) {
        const double l = wg_tri_eigval(N, dg, e, j, red);
        if (threadIdx.x == 0) lam[j] = l;
    }
    __syncthreads();
    // the vectors of the tridiagonal: thread j runs the inverse iteration of pair j (scratch behind the k columns: work + 3N onward)
    double* w = work + 3 * N;                                    // 5N doubles per thread are needed: the callers size `work` for it
    if ((int)threadIdx.x < k) tri_inverse_iteration(N, dg, e, lam[threadIdx.x], Y + (long long)threadIdx.x * ldy, w + (long long)threadIdx.x * 5 * N);
    __syncthreads();
    // modified Gram-Schmidt over the k vectors (close eigenvalues give close inverse-iteration vectors), by thread 0.  A unit vector whose
    // remainder falls below 1/2 lay mostly in the span of the earlier ones: it is recomputed from another start (a repeated eigenvalue of a
    // split tridiagonal gives the same vector twice, and the remainder is rounding, or exactly zero).  Above 1/2 the remainder keeps its
    // accuracy, and the vectors are the plain inverse-iteration ones (k = 1 never gets here).
    if (threadIdx.x == 0) {
        for (int j = 1; j < k; ++j) {
            double* yj = Y + (long long)j * ldy;
            tri_mgs(N, Y, ldy, j, yj);
            double s = 0.0;
            for (int i = 0; i < N; ++i) s = fma(yj[i], yj[i], s);
            if (!(s >= 0.25)) {
                tri_inverse_iteration_restart(N, w + (long long)j * 5 * N, Y, ldy, j);
                s = 0.0;
                for (int i = 0; i < N; ++i) s = fma(yj[i], yj[i], s);
            }
            s = 1.0 / sqrt(s);
            for (int i = 0; i < N; ++i) yj[i] *= s;
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    if (wave < k) wave_tri_backtransform(N, A, ld, tau, Y + (long long)wave * ldy);
    __syncthreads();
}

// Unit-test hook (ttn_selftest_sym_eig): one workgroup runs wg_sym_eig_smallest exactly as the solver does (ld = ldy = N; work: 3N + 5N k).
__global__ void __launch_bounds__(TTN_WG) k_selftest_sym_eig(int N, int k, double* A, double* lam, double* Y, double* work) {
    __shared__ double red[64];
    wg_sym_eig_smallest(N, A, N, k, lam, Y, N, work, red);
}

// ---- thick-restart Lanczos for the smallest eigenpair of K_s (wg_two_site_apply) ----
// x: in = start vector, out = the normalised Ritz vector.  V: (m+1) N doubles (basis), tmp: TTN_LZ_KEEP N (restart), W: Rz N (slab of the
// apply), sm: small workspace (TTN_LZ_LD * (2 TTN_LZ_LD + 2) + 6 * TTN_LZ_LD * (TTN_LZ_KEEP + 1) doubles).  Returns the number of operator
// applications; *lam_out, *res_out: the Ritz value and its residual norm ||K_s x - lam x|| (from the Lanczos relation).
__device__ __noinline__ int wg_lanczos_smallest(int na, int nb, int Rz, double* G, double* H, double* x, double* V, double* tmp, double* W,
                                                double* sm, double tol, int maxrestart, double* lam_out, double* res_out, double* red, double* lds) {
    na = uni32(na); nb = uni32(nb); Rz = uni32(Rz); maxrestart = uni32(maxrestart);
    G = unip(G); H = unip(H); x = unip(x); V = unip(V); tmp = unip(tmp); W = unip(W); sm = unip(sm); red = unip(red); lds = unip(lds);
    const int tid = threadIdx.x;
    const long long N = (long long)na * nb;
    const int m = (int)(N < TTN_LZ_M ? N : TTN_LZ_M);
    const int keep = m - 1 < TTN_LZ_KEEP ? m - 1 : TTN_LZ_KEEP;
    double* Hm = sm;                                             // projected matrix, TTN_LZ_LD x TTN_LZ_LD
    double* Hc = Hm + TTN_LZ_LD * TTN_LZ_LD;                     // its copy (destroyed by the eigensolver)
    double* hcol = Hc + TTN_LZ_LD * TTN_LZ_LD;                   // 2 * TTN_LZ_LD: one Gram-Schmidt column and its second pass
    double* th = hcol + 2 * TTN_LZ_LD;                           // Ritz values
    double* Y = th + TTN_LZ_LD;                                  // Ritz vectors of Hm, TTN_LZ_LD x (keep + 1)
    double* ework = Y + TTN_LZ_LD * (TTN_LZ_KEEP + 1);           // wg_sym_eig_smallest scratch: 3 LD + 5 LD (keep + 1)
    auto nrm = [&](const double* u) {
        double a = 0.0;
        for (long long i = tid; i < N; i += TTN_WG) a = fma(u[i], u[i], a);
        return sqrt(unif64(wg_sum(a, red)));
    };
    // one Gram-Schmidt pass against the first ncol basis vectors: h = V^T w (one wave per column), then w -= V h (one thread per row).
    // Matrix-vector products, memory bound: plain loops rather than the MFMA GEMM.
    const int lane = tid & 63, wave = tid >> 6;
    auto gs_pass = [&](int ncol, double* w, double* h) {
        for (int c = wave; c < ncol; c += TTN_NWAVES) {
            const double* vc = V + N * c;
            double a = 0.0;
            for (long long i = lane; i < N; i += 64) a = fma(vc[i], w[i], a);
            a = wave_sum(a);
            if (lane == 0) h[c] = a;
        }
        __syncthreads();
        for (long long i = tid; i < N; i += TTN_WG) {
            double a = w[i];
            for (int c = 0; c < ncol; ++c) a = fma(-V[i + N * c], h[c], a);
            w[i] = a;
        }
        __syncthreads();
    };
    // out[:, c] = V[:, :msize] Y[:, c] for c < ncol (out does not overlap V's first msize columns)
    auto combine = [&](int msize, int ncol, double* out) {
        for (long long t = tid; t < N * ncol; t += TTN_WG) {
            const long long i = t % N; const int c = (int)(t / N);
            double a = 0.0;
            for (int q = 0; q < msize; ++q) a = fma(V[i + N * q], Y[q + TTN_LZ_LD * c], a);
            out[t] = a;
        }
        __syncthreads();
    };
    for (int e_ = tid; e_ < TTN_LZ_LD * TTN_LZ_LD; e_ += TTN_WG) Hm[e_] = 0.0;
    double nx = nrm(x);
    if (!(nx > 0.0)) {                                           // a vanishing start: the all-ones vector
        for (long long i = tid; i < N; i += TTN_WG) x[i] = 1.0;
        __syncthreads();
        nx = sqrt((double)N);
    }
    for (long long i = tid; i < N; i += TTN_WG) V[i] = x[i] / nx;
    __syncthreads();
    int j0 = 0, restarts = 0, napply = 0;
    double hnorm = 0.0;
    for (;;) {
        int msize = m;
        double beta = 0.0;
        bool breakdown = false;
        for (int j = j0; j < m; ++j) {
            double* vj = V + N * j;
            double* w = V + N * (j + 1);
            wg_two_site_apply(na, nb, Rz, G, H, vj, w, W, lds);
            ++napply;
            // full reorthogonalisation, twice (classical Gram-Schmidt with one refinement): h = V^T w, w -= V h
            gs_pass(j + 1, w, hcol);
            gs_pass(j + 1, w, hcol + TTN_LZ_LD);
            beta = nrm(w);
            if (tid <= j) {
                const double h = hcol[tid] + hcol[TTN_LZ_LD + tid];
                Hm[tid + TTN_LZ_LD * j] = h;
                Hm[j + TTN_LZ_LD * tid] = h;
            }
            if (tid == 0 && j + 1 < TTN_LZ_LD) { Hm[(j + 1) + TTN_LZ_LD * j] = beta; Hm[j + TTN_LZ_LD * (j + 1)] = beta; }
            __syncthreads();
            double hc = 0.0;
            for (int i = 0; i <= j; ++i) hc += fabs(Hm[i + TTN_LZ_LD * j]);
            hnorm = fmax(hnorm, hc + beta);
            if (beta <= 1.0e-14 * hnorm || j + 1 == N) {            // invariant subspace: the projected problem is exact
                msize = j + 1; breakdown = true;
                break;
            }
            const double ib = 1.0 / beta;
            for (long long i = tid; i < N; i += TTN_WG) w[i] *= ib;
            __syncthreads();
        }
        // Ritz pairs of the projected matrix
        int kk = keep < msize - 1 ? keep : msize - 1;
        if (kk < 1) kk = 1;
        for (int e_ = tid; e_ < TTN_LZ_LD * TTN_LZ_LD; e_ += TTN_WG) Hc[e_] = Hm[e_];
        __syncthreads();
        wg_sym_eig_smallest(msize, Hc, TTN_LZ_LD, kk, th, Y, TTN_LZ_LD, ework, red);
        const double res = (msize == N) ? 0.0 : fabs(beta * Y[msize - 1]);   // ||K_s x - theta x|| = beta |e_m^T y|
        const bool done = res <= tol || breakdown || restarts >= maxrestart;
        if (done) {
            combine(msize, 1, x);                                        // x = V Y[:, 0]
            const double nxx = nrm(x);
            for (long long i = tid; i < N; i += TTN_WG) x[i] /= nxx;
            __syncthreads();
            *lam_out = unif64(th[0]);
            *res_out = res;
            return napply;
        }
        ++restarts;
        // thick restart: V[:, :kk] = V Y[:, :kk], V[:, kk] = the last Lanczos vector, Hm = diag(theta) bordered by beta Y[m-1, :kk]
        combine(msize, kk, tmp);
        for (long long i = tid; i < N * kk; i += TTN_WG) V[i] = tmp[i];
        for (long long i = tid; i < N; i += TTN_WG) V[N * kk + i] = V[N * msize + i];
        for (int e_ = tid; e_ < TTN_LZ_LD * TTN_LZ_LD; e_ += TTN_WG) {
            const int r = e_ % TTN_LZ_LD, c = e_ / TTN_LZ_LD;
            double h = 0.0;
            if (r == c && r < kk) h = th[r];
            else if (c == kk && r < kk) h = beta * Y[msize - 1 + TTN_LZ_LD * r];
            else if (r == kk && c < kk) h = beta * Y[msize - 1 + TTN_LZ_LD * c];
            Hm[e_] = h;
        }
        __syncthreads();
        j0 = kk;
    }
}

// ---- the sweep kernel ----
struct EigArgs {
    MalsArgs M;                  // operator, x, scratch offsets, SVD knobs, mode / sweep plan (M.L.b unused: no right-hand side)
    double* hist_E;              // [batch][hist_len] eigenvalue of every micro-step
    long long* hist_r;           // [batch][hist_len] max rank after the micro-step's core move (the closing DMRG solve: before it)
    int hist_len;
    int lz_all, lz_above, lz_maxrestart;     // matrix-free if lz_all or N > lz_above
    double lz_tol;
    long long offLz, offEig, lz_nmax;        // Lanczos area: V (m+1) N, tmp KEEP N, W Rz N, then the small workspace; dense eigen work
    int* lz_iters;               // [batch] operator applications of the Lanczos solves
    double* lz_res;              // [batch] largest final Lanczos residual
};

#define XC(i) (E.x.data + (long long)E.tb * E.x.stride + E.x.off[i])
#define AC(i) (E.A.data + (long long)E.tb * E.A.stride + E.A.off[i])      // (stride 0: one operator for every train)
#define GP(i) (E.scr + E.off[i])
#define HP(i) (E.scr + E.off[2 * E.d + (i)])
#define WG_FOR(total) for (long long e_ = threadIdx.x; e_ < (long long)(total); e_ += TTN_WG)

__global__ void __launch_bounds__(TTN_WG) k_two_site_eig(EigArgs R) {
    extern __shared__ double lds[];
    const MalsArgs& Q = R.M;
    const AlsArgs& P = Q.L;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int d = P.x.d;
    double* scr = P.scratch + (long long)b * P.scratch_stride;
    double* red = lds + GEMM_LDS_TOTAL;
    BondCtx S;
    S.ldsX = lds;
    S.red = red;
    S.Ts = S.red + 32;
    S.Ss = S.Ts + QR_NB * QR_NB;
    S.taus = S.Ss + QR_NB * QR_NB;
    S.scal = S.taus + QR_NB;
    S.iflag = reinterpret_cast<int*>(S.scal + 8);
    S.nrm2 = S.scal + 16;
    S.M = nullptr; S.M2 = nullptr;
    S.Vb = scr + P.offVb; S.Wb = scr + P.offWb;
    S.Us = scr + Q.offUs; S.Xg = scr + Q.offXg;
    S.sig = scr + Q.offSig; S.sigs = S.sig + Q.pmax; S.perm = reinterpret_cast<int*>(S.sigs + Q.pmax);
    S.Ga = S.Gb = S.Cc = S.T1 = S.T2 = S.T3 = nullptr;
    double* K = scr + P.offK;
    double* Pb = scr + P.offPb;
    double* M2 = scr + Q.offM2;
    if (tid == 0) Q.C.sweep_stats[b] = 0;
    long long* xr = P.x.rks + (long long)b * (d + 1);
    AlsEnv E;
    E.A = P.A; E.b = P.x; E.x = P.x; E.tb = b; E.scr = scr; E.off = P.off; E.xr = xr; E.br = xr;
    E.T1 = scr + P.offT1; E.T2 = scr + P.offT2; E.d = d;
    __syncthreads();

    // local eigenproblem of window i: the eigenvector into Pb as (n1, r_i, n2, r_{i+2}) column-major; returns lambda
    int lz_iters = 0;
    double lz_res = 0.0;
    bool lz_fail = false;
    bool nonfinite = false;                      // uniform: set from workgroup-wide values
    auto eigsolve = [&](int i, int& a_out, int& b_out, bool v0_swapped) -> double {
        const int n1 = uni32(P.x.dims[i]), n2 = uni32(P.x.dims[i + 1]);
        const int rl = uni32((int)xr[i]), rr = uni32((int)xr[i + 2]);
        const int Rz = uni32((int)P.A.rks[i + 1]);
        double *Gi = GP(i), *Hi = HP(i);
        const int na = n1 * rl, nb = n2 * rr, N = na * nb;
        a_out = na; b_out = nb;
        double lam;
        if (R.lz_all || N > R.lz_above) {
            double* lz = scr + R.offLz;
            double* V = lz;
            double* tmp = V + (long long)(TTN_LZ_M + 1) * R.lz_nmax;
            double* W = tmp + (long long)TTN_LZ_KEEP * R.lz_nmax;
            double* sm = W + (long long)Rz * R.lz_nmax;
            const int rm = uni32((int)xr[i + 1]);
            // start vector: the current two-site block, as k_mals_linsolve's matrix-free branch builds it (swapped physical indices after
            // a left move in the DMRG mode, dmrg.jl:331-334)
            if (v0_swapped && n1 == n2) {
                for (int j = 0; j < n1; ++j)
                    for (int k = 0; k < n2; ++k)
                        wg_gemm(rl, rr, rm, mkview(XC(i) + k, plain(n1), plain((long long)n1 * rl)), mkview(XC(i + 1) + j, plain(n2), plain((long long)n2 * rm)),
                                mkview(Pb + j + (long long)na * k, plain(n1), plain((long long)na * n2)), 1.0, 0.0, lds);
            } else {
                wg_gemm(na, nb, rm, mkview(XC(i), plain(1), plain(na)), mkview(XC(i + 1), plain(n2), Idx{n2, 1, (long long)n2 * rm}),
                        mkview(Pb, plain(1), plain(na)), 1.0, 0.0, lds);
            }
            __syncthreads();
            double res;
            lz_iters += wg_lanczos_smallest(na, nb, Rz, Gi, Hi, Pb, V, tmp, W, sm, R.lz_tol, R.lz_maxrestart, &lam, &res, red, lds);
            lz_res = fmax(lz_res, res);
            if (!(res <= 1.0e3 * R.lz_tol)) lz_fail = true;
        } else {
            WG_FOR((long long)N * N) {
                const int row = (int)(e_ % N), col = (int)(e_ / N);
                const int ab = row % na, cd = row / na, ef = col % na, gh = col / na;
                double a = 0.0;
                for (int z = 0; z < Rz; ++z) a = fma(Gi[ab + (long long)na * (ef + (long long)na * z)], Hi[z + Rz * (cd + (long long)nb * gh)], a);
                K[e_] = a;
            }
            __syncthreads();
            WG_FOR((long long)N * N) {                                 // K_s = 1/2 (K + K^T)
                const int row = (int)(e_ % N), col = (int)(e_ / N);
                if (row < col) {
                    const double s = 0.5 * (K[e_] + K[col + (long long)N * row]);
                    K[e_] = s; K[col + (long long)N * row] = s;
                }
            }
            __syncthreads();
            double* ew = scr + R.offEig;
            wg_sym_eig_smallest(N, K, N, 1, ew, Pb, N, ew + 8, red);
            lam = unif64(ew[0]);
        }
        if (!wg_fix_sign(N, Pb, red, S.iflag) || !(fabs(lam) <= 1.7976931348623157e308)) nonfinite = true;
        return lam;
    };

    // The orthonormal factor of a core move, re-orthonormalised by a Householder QR whose R goes into the neighbour (the product is
    // unchanged).  The SVD step's orthonormal factor loses orthogonality in directions of singular values near the rounding level
    // (kept by a small tol), and a projected eigenproblem on a non-orthonormal basis can fall below the true ground state.
    OrthoWork W;
    W.Vb = S.Vb; W.Wb = S.Wb; W.Tst = scr + P.offTst; W.red = red; W.Ts = S.Ts; W.Ss = S.Ss; W.taus = S.taus;
    double* Tm = scr + P.offTm;
    double* Qb = scr + P.offQb;
    double* Rb = scr + P.offRb;
    double* T1 = E.T1;
    auto reortho = [&](int i, int r, int dir) {
        const int n1 = uni32(P.x.dims[i]), n2 = uni32(P.x.dims[i + 1]);
        const int rl = uni32((int)xr[i]), rr = uni32((int)xr[i + 2]);
        double* xi = XC(i);
        double* xn = XC(i + 1);
        if (dir == 0) {                                   // x_i (n1 rl x r) = Q R, x_{i+1}[a, b, c] <- sum_z R[b, z] x_{i+1}[a, z, c]
            const int mm = n1 * rl;
            WG_FOR((long long)mm * r) Tm[e_] = xi[e_];
            __syncthreads();
            wg_qr_explicit(mm, r, Tm, Qb, Rb, W, lds);
            WG_FOR((long long)mm * r) xi[e_] = Qb[e_];
            WG_FOR((long long)n2 * r * rr) {
                long long t_ = e_; const int a_ = t_ % n2; t_ /= n2; const int bq = t_ % r; const int c = (int)(t_ / r);
                double a = 0.0;
                for (int z = 0; z < r; ++z) a = fma(Rb[bq + (long long)r * z], xn[a_ + n2 * (z + (long long)r * c)], a);
                T1[e_] = a;
            }
            __syncthreads();
            WG_FOR((long long)n2 * r * rr) xn[e_] = T1[e_];
        } else {                                          // M[(x + n2 a2), a1] = x_{i+1}[x, a1, a2] = Q R, x_i[a, b, c] <- sum_z x_i[a, b, z] R[c, z]
            const int mm = n2 * rr;
            WG_FOR((long long)mm * r) {
                const int row = (int)(e_ % mm), a1 = (int)(e_ / mm);
                Tm[e_] = xn[row % n2 + n2 * (a1 + (long long)r * (row / n2))];
            }
            __syncthreads();
            wg_qr_explicit(mm, r, Tm, Qb, Rb, W, lds);
            WG_FOR((long long)mm * r) {
                const int row = (int)(e_ % mm), a1 = (int)(e_ / mm);
                xn[row % n2 + n2 * (a1 + (long long)r * (row / n2))] = Qb[e_];
            }
            const long long nr = (long long)n1 * rl;
            WG_FOR(nr * r) {
                const long long ab = e_ % nr; const int c = (int)(e_ / nr);
                double a = 0.0;
                for (int z = 0; z < r; ++z) a = fma(xi[ab + nr * z], Rb[c + (long long)r * z], a);
                T1[e_] = a;
            }
            __syncthreads();
            WG_FOR(nr * r) xi[e_] = T1[e_];
        }
        __syncthreads();
    };

    // ---- initial environments: G_0 = A_1, H_{d-2} = A_d (mals.jl:255-265 without the right-hand side) ----
    {
        const int n0 = uni32(P.x.dims[0]), R1 = uni32((int)P.A.rks[1]);
        WG_FOR((long long)n0 * n0 * R1) GP(0)[e_] = AC(0)[e_];
        const int n = uni32(P.x.dims[d - 1]), Rz = uni32((int)P.A.rks[d - 1]);
        WG_FOR((long long)Rz * n * n) {
            long long t = e_; const int z = t % Rz; t /= Rz; const int j = t % n; const int k = (int)(t / n);
            HP(d - 2)[e_] = AC(d - 1)[j + n * (k + (long long)n * z)];
        }
        __syncthreads();
    }
    for (int i = d - 2; i >= 1; --i) mals_update_H_op(E, i);
    int status = 0;
    const int mode = uni32(Q.mode);
    const int per = mode == 0 ? 2 * (d - 1) : 2 * (d - 2);                 // windows visited by one sweep
    const int total = mode == 0 ? uni32(Q.nsweeps) * per : uni32(Q.nsweeps) * per + 1;
    const int rule = mode == 0 ? 1 : 2;
    int prev_dir = 0;
    double* hE = R.hist_E + (long long)b * R.hist_len;
    long long* hR = R.hist_r + (long long)b * R.hist_len;
    auto max_rank = [&]() { long long m_ = 0; for (int k = 0; k <= d; ++k) m_ = xr[k] > m_ ? xr[k] : m_; return m_; };
    for (int t = 0; t < total && !status; ++t) {
        int i, dir, rmax;
        if (t == total - 1 && mode == 1) { i = 0; dir = 1; rmax = Q.rmax_final; }
        else { const int u = t % per; const int h = mode == 0 ? d - 1 : d - 2; dir = u >= h; i = dir ? (mode == 0 ? 2 * (d - 1) - 1 - u : 2 * (d - 2) - u) : u; rmax = Q.rmax_sweep[t / per]; }
        i = uni32(i); dir = uni32(dir); rmax = uni32(rmax);
        int na, nb;
        const double lam = eigsolve(i, na, nb, mode == 1 && prev_dir == 1);
        prev_dir = dir;
        const bool closing = mode == 1 && t == total - 1;
        if (tid == 0) { hE[t] = lam; if (closing) hR[t] = max_rank(); }  // dmrg.jl:539-540: the closing entries come before the left move
        if (nonfinite) { status = TTN_ST_NONFINITE; break; }      // no core move of a NaN block
        const int n2 = uni32(P.x.dims[i + 1]);
        double* xi = XC(i);
        double* xn = XC(i + 1);
        int r;
        if (dir == 0)
            r = wg_hsvd_step(Q.C, b, S, mkview(Pb, plain(1), plain(na)), na, nb, M2, 2, n2, 0, xi, xn, Q.tol, (int)P.x.cap[i + 1], lds, rule, rmax);
        else
            r = wg_hsvd_step(Q.C, b, S, mkview(Pb, plain(na), plain(1)), nb, na, M2, 1, n2, 0, xn, xi, Q.tol, (int)P.x.cap[i + 1], lds, rule, rmax);
        if (r < 0) { status = TTN_ST_RANK_OVERFLOW; break; }
        if (tid == 0) xr[i + 1] = r;
        __syncthreads();
        reortho(i, r, dir);
        if (tid == 0 && !closing) hR[t] = max_rank();
        __syncthreads();
        if (dir == 0) als_update_G_op(E, i);
        else if (i > 0) mals_update_H_op(E, i);
    }
    if (lz_fail && !status) status = TTN_ST_LANCZOS;
    if (tid == 0) {
        if (status) ttn_set_status(&P.status[b], status);
        if (R.lz_iters) R.lz_iters[b] = lz_iters;
        if (R.lz_res) R.lz_res[b] = lz_res;
    }
}
#undef XC
#undef AC
#undef GP
#undef HP
#undef WG_FOR
