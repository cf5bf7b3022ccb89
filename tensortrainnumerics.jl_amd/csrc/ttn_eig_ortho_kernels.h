// ttn_eig_ortho_kernels.h — excited states with the two-site eigensolvers: the walk of k_two_site_eig (ttn_eigsolve_kernels.h) with a
// penalty against m given trains phi_1 .. phi_m.  The local problem of window i becomes
//     K_eff = 1/2 (K + K^T) + sum_j w_j p_j p_j^T,     p_j = the projection of phi_j / ||phi_j|| onto the two-site basis of x,
// whose smallest eigenpair is the lowest state of A + sum_j w_j |phi_j><phi_j| / <phi_j, phi_j> in that basis: with the weights above
// the gap to the wanted level, the next state orthogonal to the phi_j.  The rank-m term is never formed as a TT operator.
//
// Per phi_j the workgroup keeps two chains of overlap environments, the right-hand-side halves of k_mals_linsolve's environments
// with phi_j in the place of b (r = ranks of x, p = ranks of phi_j, both current):
//     L_j[k]  (r_k x p_k)   = the cores 0 .. k-1 of x and phi_j contracted over their physical indices,    L_j[0] = 1
//     R_j[k]  (r_k x p_k)   = the cores k .. d-1,                                                          R_j[d] = 1
// All R_j[k], k >= 2, are built once after the H environments; after a right move of window i the left chain advances to
// L_j[i+1] from the new core i, after a left move the right chain to R_j[i+1] from the new core i+1 (the cores the QR
// re-orthonormalisation has fixed).  Each advance is two MFMA products (wg_gemm), the projection
//     p_j[s, a, t, c] = sum L_j[i][a, al] phi_j,i[s, al, be] phi_j,i+1[t, be, ga] R_j[i+2][c, ga] / ||phi_j||
// three, into Pb's layout (n_i, r_i, n_{i+1}, r_{i+2}) column-major.  The m vectors stay in scratch for the local solve:
//     dense        K[row, col] += sum_j w_j p_j[row] p_j[col] on the symmetrised matrix, both triangles, then wg_sym_eig_smallest;
//     matrix-free  wg_lanczos_penalised: wg_lanczos_smallest with out += sum_j w_j p_j (p_j^T v) behind wg_two_site_apply, the m dot
//                  products first (wave j takes p_j), then one pass of AXPYs.
// The plain kernel and its Lanczos routine are not touched: this header carries its own copy of both (see there).
// The eigenvalue written to the history is that of K_eff: <H> + sum_j w_j <phi_j, x>^2 / <phi_j, phi_j> in the local basis, not the
// energy (the caller takes that with a Rayleigh quotient).  After the walk the right chain is advanced over cores 1 and 0:
// R_j[0] is the 1 x 1 overlap <phi_j, x>, returned divided by ||phi_j||.
#pragma once
#include "ttn_eigsolve_kernels.h"

#ifndef TTN_EIG_ORTHO_MAX            // (include/ttn_eig_ortho.h states the same bound to callers)
#define TTN_EIG_ORTHO_MAX 8          // penalty trains of one call (one wave per dot product of the matrix-free operator)
#endif
static_assert(TTN_EIG_ORTHO_MAX <= TTN_NWAVES, "one wave per penalty train");

struct EigOrthoArgs {
    int m;                                   // penalty trains
    TTDev phi[TTN_EIG_ORTHO_MAX];            // batch 1: every train of x is penalised by train 0
    const double* weight;                    // device [batch][m]
    const double* inv_norm;                  // device [batch][m]: 1 / ||phi_j|| of the train that penalises train b
    double* ovl;                             // device [batch][m]: <phi_j, x> / ||phi_j|| of the final state
    // per-train scratch, in doubles from the train's base: the chains of phi_j start at offChain + chain0[j], slot k of the left chain
    // at k * slot[j], of the right chain at (d + 1 + k) * slot[j] (slot[j] = max capacity of x times max rank bound of phi_j);
    // offP: m projected vectors of nmax doubles; offU, offW: the two intermediates of a projection / chain advance; offC: m doubles
    long long offChain, offP, offU, offW, offC, nmax;
    long long chain0[TTN_EIG_ORTHO_MAX], slot[TTN_EIG_ORTHO_MAX];
};

// out += sum_j w_j p_j (p_j^T v): the rank-m term of the matrix-free operator
struct LzPenalty {
    int m;
    const double* P;             // m vectors, stride nmax
    long long nmax;
    const double* w;             // m weights of this train
    double* c;                   // m doubles of scratch
    __device__ __forceinline__ void operator()(const double* v, double* out, long long N) const {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        if (wave < m) {
            const double* pj = P + nmax * wave;
            double a = 0.0;
            for (long long i = lane; i < N; i += 64) a = fma(pj[i], v[i], a);
            a = wave_sum(a);
            if (lane == 0) c[wave] = w[wave] * a;
        }
        __syncthreads();
        for (long long i = tid; i < N; i += TTN_WG) {
            double a = out[i];
            for (int j = 0; j < m; ++j) a = fma(c[j], P[nmax * j + i], a);
            out[i] = a;
        }
        __syncthreads();
    }
};

// wg_lanczos_smallest (ttn_eigsolve_kernels.h) with extra(v, out, N) behind every operator application: the same statements otherwise,
// as a second routine so that the plain one keeps the machine code it has (a change to one belongs in the other).
__device__ __noinline__ int wg_lanczos_penalised(int na, int nb, int Rz, double* G, double* H, double* x, double* V, double* tmp, double* W,
                                                  double* sm, double tol, int maxrestart, double* lam_out, double* res_out, double* red, double* lds,
                                                  LzPenalty extra) {
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
            extra(vj, w, N);
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


// What the walk hands to the penalty.
struct EigWalk {
    TTDev x;                     // the train being solved for
    const long long* xr;         // its current ranks
    int b, d;                    // train, sites
    double *scr, *lds, *red;     // per-train scratch, the workgroup's LDS, its reduction words
};

struct EigOrthoPenalty {
    const EigOrthoArgs& O;
    EigWalk Wk;
    int na, nb;                  // the local problem of the last project()
    __device__ explicit EigOrthoPenalty(const EigOrthoArgs& O_) : O(O_), Wk(), na(0), nb(0) {}

    __device__ __forceinline__ int ptrain(int j) const { return O.phi[j].batch == 1 ? 0 : Wk.b; }
    __device__ __forceinline__ double* pcore(int j, int k) const { return O.phi[j].data + (long long)ptrain(j) * O.phi[j].stride + O.phi[j].off[k]; }
    __device__ __forceinline__ int prank(int j, int k) const { return uni32((int)O.phi[j].rks[(long long)ptrain(j) * (Wk.d + 1) + k]); }
    __device__ __forceinline__ double* xcore(int k) const { return Wk.x.data + (long long)Wk.b * Wk.x.stride + Wk.x.off[k]; }
    __device__ __forceinline__ int xrank(int k) const { return uni32((int)Wk.xr[k]); }
    __device__ __forceinline__ double* Lc(int j, int k) const { return Wk.scr + O.offChain + O.chain0[j] + (long long)k * O.slot[j]; }
    __device__ __forceinline__ double* Rc(int j, int k) const { return Wk.scr + O.offChain + O.chain0[j] + (long long)(Wk.d + 1 + k) * O.slot[j]; }
    __device__ __forceinline__ double* pvec(int j) const { return Wk.scr + O.offP + O.nmax * j; }

    // L_j[k+1][be, be'] = sum_{s, al, al'} x_k[s, al, be] L_j[k][al, al'] phi_k[s, al', be']
    __device__ void advance_left(int j, int k) {
        const int n = uni32(Wk.x.dims[k]), rl = xrank(k), r = xrank(k + 1), pl = prank(j, k), pr = prank(j, k + 1);
        double* T = Wk.scr + O.offU;
        // T[al', s + n be] = sum_al L[al, al'] x_k[s, al, be]
        wg_gemm(pl, n * r, rl, mkview(Lc(j, k), plain(rl), plain(1)), mkview(xcore(k), plain(n), Idx{n, 1, (long long)n * rl}),
                mkview(T, plain(1), plain(pl)), 1.0, 0.0, Wk.lds);
        // L[k+1][be, be'] = sum_{s, al'} T[al', s, be] phi_k[s, al', be']
        wg_gemm(r, pr, n * pl, mkview(T, plain((long long)pl * n), Idx{n, pl, 1}), mkview(pcore(j, k), plain(1), plain((long long)n * pl)),
                mkview(Lc(j, k + 1), plain(1), plain(r)), 1.0, 0.0, Wk.lds);
        __syncthreads();
    }
    // R_j[k][be, be'] = sum_{t, ga, ga'} x_k[t, be, ga] R_j[k+1][ga, ga'] phi_k[t, be', ga']
    __device__ void advance_right(int j, int k) {
        const int n = uni32(Wk.x.dims[k]), r = xrank(k), rr = xrank(k + 1), pl = prank(j, k), pr = prank(j, k + 1);
        double* T = Wk.scr + O.offU;
        // T[(t, be), ga'] = sum_ga x_k[(t, be), ga] R[k+1][ga, ga']
        wg_gemm(n * r, pr, rr, mkview(xcore(k), plain(1), plain((long long)n * r)), mkview(Rc(j, k + 1), plain(1), plain(rr)),
                mkview(T, plain(1), plain((long long)n * r)), 1.0, 0.0, Wk.lds);
        // R[k][be, be'] = sum_{t, ga'} T[t, be, ga'] phi_k[t, be', ga']
        wg_gemm(r, pl, n * pr, mkview(T, plain(n), Idx{n, 1, (long long)n * r}), mkview(pcore(j, k), Idx{n, 1, (long long)n * pl}, plain(n)),
                mkview(Rc(j, k), plain(1), plain(r)), 1.0, 0.0, Wk.lds);
        __syncthreads();
    }

    __device__ void begin(const EigWalk& W_) {
        Wk = W_;
        const int d = Wk.d;
        if (threadIdx.x < O.m) { Lc(threadIdx.x, 0)[0] = 1.0; Rc(threadIdx.x, d)[0] = 1.0; }
        __syncthreads();
        for (int j = 0; j < O.m; ++j)
            for (int k = d - 1; k >= 2; --k) advance_right(j, k);
    }

    __device__ void project(int i) {
        const int n1 = uni32(Wk.x.dims[i]), n2 = uni32(Wk.x.dims[i + 1]);
        const int rl = xrank(i), rr = xrank(i + 2);
        na = n1 * rl; nb = n2 * rr;
        double* U = Wk.scr + O.offU;
        double* Wt = Wk.scr + O.offW;
        for (int j = 0; j < O.m; ++j) {
            const int pl = prank(j, i), pm = prank(j, i + 1), pr = prank(j, i + 2);
            // U[(s, a), be] = sum_al L[a, al] phi_i[s, al, be]
            wg_gemm(rl, n1 * pm, pl, mkview(Lc(j, i), plain(1), plain(rl)), mkview(pcore(j, i), plain(n1), Idx{n1, 1, (long long)n1 * pl}),
                    mkview(U, plain(n1), Idx{n1, 1, (long long)na}), 1.0, 0.0, Wk.lds);
            // Wt[be, (t, c)] = sum_ga phi_{i+1}[(t, be), ga] R[c, ga]
            wg_gemm(n2 * pm, rr, pr, mkview(pcore(j, i + 1), plain(1), plain((long long)n2 * pm)), mkview(Rc(j, i + 2), plain(rr), plain(1)),
                    mkview(Wt, Idx{n2, pm, 1}, plain((long long)pm * n2)), 1.0, 0.0, Wk.lds);
            // p_j = U Wt / ||phi_j||
            wg_gemm(na, nb, pm, mkview(U, plain(1), plain(na)), mkview(Wt, plain(1), plain(pm)), mkview(pvec(j), plain(1), plain(na)),
                    O.inv_norm[(long long)Wk.b * O.m + j], 0.0, Wk.lds);
        }
        __syncthreads();
    }

    __device__ void dense(double* K, int N) {
        const double* w = O.weight + (long long)Wk.b * O.m;
        const double* P = pvec(0);
        for (long long e = threadIdx.x; e < (long long)N * N; e += TTN_WG) {
            const int row = (int)(e % N), col = (int)(e / N);
            double a = K[e];
            for (int j = 0; j < O.m; ++j) a = fma(w[j] * P[O.nmax * j + row], P[O.nmax * j + col], a);
            K[e] = a;
        }
        __syncthreads();
    }

    __device__ __forceinline__ LzPenalty lanczos() const {
        return LzPenalty{O.m, pvec(0), O.nmax, O.weight + (long long)Wk.b * O.m, Wk.scr + O.offC};
    }

    __device__ void moved(int i, int dir) {
        for (int j = 0; j < O.m; ++j) {
            if (dir == 0) advance_left(j, i);
            else advance_right(j, i + 1);
        }
    }

    // both modes end with a left move of window 0: R_j[1] is current
    __device__ void finish() {
        for (int j = 0; j < O.m; ++j) {
            advance_right(j, 0);
            if (threadIdx.x == 0) O.ovl[(long long)Wk.b * O.m + j] = Rc(j, 0)[0] * O.inv_norm[(long long)Wk.b * O.m + j];
        }
    }
};

// ---- the sweep ----
// k_two_site_eig's walk, statement for statement, with six calls into the penalty: begin (after the initial H environments), project
// (before a local problem), dense (on the symmetrised K), lanczos (the extra term of the matrix-free operator), moved (after a core
// move and its environment update) and finish.  A second copy, not a template over both: the plain kernel and the entry points that
// launch it keep their machine code and their timing that way; a change to one walk belongs in the other.
#define XC(i) (E.x.data + (long long)E.tb * E.x.stride + E.x.off[i])
#define AC(i) (E.A.data + (long long)E.tb * E.A.stride + E.A.off[i])      // (stride 0: one operator for every train)
#define GP(i) (E.scr + E.off[i])
#define HP(i) (E.scr + E.off[2 * E.d + (i)])
#define WG_FOR(total) for (long long e_ = threadIdx.x; e_ < (long long)(total); e_ += TTN_WG)
__device__ __forceinline__ void two_site_eig_ortho_walk(const EigArgs& R, EigOrthoPenalty pen, double* lds) {
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
            lz_iters += wg_lanczos_penalised(na, nb, Rz, Gi, Hi, Pb, V, tmp, W, sm, R.lz_tol, R.lz_maxrestart, &lam, &res, red, lds, pen.lanczos());
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
            pen.dense(K, N);
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
    pen.begin(EigWalk{P.x, xr, b, d, scr, lds, red});
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
        pen.project(i);
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
        pen.moved(i, dir);
    }
    if (!status) pen.finish();
    if (lz_fail && !status) status = TTN_ST_LANCZOS;
    if (tid == 0) {
        if (status) ttn_set_status(&P.status[b], status);
        if (R.lz_iters) R.lz_iters[b] = lz_iters;
        if (R.lz_res) R.lz_res[b] = lz_res;
    }
}

__global__ void __launch_bounds__(TTN_WG) k_two_site_eig_ortho(EigArgs R, EigOrthoArgs O) {
    extern __shared__ double lds[];
    two_site_eig_ortho_walk(R, EigOrthoPenalty(O), lds);
}
#undef XC
#undef AC
#undef GP
#undef HP
#undef WG_FOR
