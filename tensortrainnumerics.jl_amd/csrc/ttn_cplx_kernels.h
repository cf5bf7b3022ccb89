// ttn_cplx_kernels.h — ComplexF64 trains: apply, hadamard, scalar *, dot and the tt_compress! bond step.
//
// A complex core is Julia's Array{ComplexF64,3} as it lies: column-major (n, r_l, r_r), interleaved (re, im).  Byte for byte that is
// the real core (2n, r_l, r_r), and a complex handle keeps 2n in its DEVICE dims table: the rank kernels, k_add, k_replicate and the
// copy form of k_scale run on it unchanged.  The kernels below halve that number again (dims[k] >> 1).  A complex operator core
// (n, n, R_l, R_r) keeps n in its table; only its slots are twice as long.
#pragma once
#include "ttn_common.h"
#include "ttn_stream_kernels.h"
#include "ttn_dense_kernels.h"
#include "ttn_densefact_kernels.h"

#ifndef TTN_ZAPPLY_K
#define TTN_ZAPPLY_K 2                    // output columns per thread in k_zapply (32-byte fibres at n = 2); the sweep: DESIGN §4.17, tools/diag_complex.py
#endif
#define TTN_ZHAD_K 2
#define TTN_ZC_WG 1024                    // threads of k_zcompress / k_zdot: one workgroup per train
#define TTN_ZC_LDS_N 96                   // largest short side whose square factor (n x n complex) sits in LDS: 96^2 * 16 B = 144 KiB
#define TTN_ZC_LDS_BYTES (sizeof(double) * 2 * TTN_ZC_LDS_N * TTN_ZC_LDS_N)
#define TTN_ZC_MAX_SWEEPS 60
#define TTN_ZDOT_LDS_DOUBLES 7680         // W and T of k_zdot in LDS when 2 (ra rb + n ra rb') doubles fit (60 KiB)

typedef dfnum<true> zc;
typedef dfc zt;
typedef double zd2v_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ zt zload(const double* p, long long i) { const zd2v_t v = *reinterpret_cast<const zd2v_t*>(p + 2 * i); return zt{v.x, v.y}; }
__device__ __forceinline__ void zstore(double* p, long long i, zt v) { zd2v_t o; o.x = v.x; o.y = v.y; *reinterpret_cast<zd2v_t*>(p + 2 * i) = o; }
__device__ __forceinline__ void zstore_nt(double* p, long long i, zt v) { zd2v_t o; o.x = v.x; o.y = v.y; __builtin_nontemporal_store(o, reinterpret_cast<zd2v_t*>(p + 2 * i)); }
__device__ __forceinline__ zt zfma(zt a, zt b, zt c) {          // c + a b
    return zt{fma(a.x, b.x, fma(-a.y, b.y, c.x)), fma(a.x, b.y, fma(a.y, b.x, c.y))};
}
template <bool C> __device__ __forceinline__ zt zload_as(const double* p, long long i) { return C ? zload(p, i) : zt{p[i], 0.0}; }

// ---------------------------------------------------------------------------------------------
// apply:  Y_k[i, a' + Rl v', a + Rr v] = sum_j A_k[i,j,a',a] X_k[j,v',v], Y complex; the operator (CA) and / or the train (CX) complex.
// k_apply's mapping (§4.1): one thread = one output row p = a' + Rl v' and TTN_ZAPPLY_K consecutive columns c = a + Rr v, the lanes of a
// wave on consecutive rows, 16-byte non-temporal stores.  The operator core is read through the caches (the QFT core is 43 KB at
// K = 25, 166 KB at K = 50: beyond k_apply's LDS staging rule); consecutive lanes read consecutive a', i.e. consecutive n^2-blocks.
// ---------------------------------------------------------------------------------------------
template <bool CA, bool CX>
__global__ void __launch_bounds__(TTN_STREAM_TB) k_zapply(TTODev A, TTDev x, TTDev y) {
    const int k = blockIdx.y, b = blockIdx.z;
    const int n = y.dims[k] >> 1;
    const int Rl = (int)A.rks[k], Rr = (int)A.rks[k + 1];
    const long long* xr = x.rks + (long long)b * (x.d + 1);
    const int rl = (int)xr[k], rr = (int)xr[k + 1];
    const double* Ak = A.data + A.off[k];
    const double* Xk = x.data + (long long)b * x.stride + x.off[k];
    double* Yk = y.data + (long long)b * y.stride + y.off[k];
    const unsigned int uP = (unsigned int)Rl * (unsigned int)rl, uQ = (unsigned int)Rr * (unsigned int)rr;
    const unsigned int cgroups = (uQ + TTN_ZAPPLY_K - 1) / TTN_ZAPPLY_K, items = uP * cgroups;
    for (unsigned int it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const unsigned int p = it % uP, c0 = (it / uP) * TTN_ZAPPLY_K;
        const unsigned int al = p % (unsigned int)Rl, vl = p / (unsigned int)Rl;
        unsigned int ar = c0 % (unsigned int)Rr, vr = c0 / (unsigned int)Rr;
        if (n == 2) {
            zt o[TTN_ZAPPLY_K][2];
#pragma unroll
            for (int j = 0; j < TTN_ZAPPLY_K; ++j) {
                o[j][0] = o[j][1] = zt{0.0, 0.0};
                if (c0 + j < uQ) {
                    const long long xb = 2 * ((long long)vl + (long long)rl * vr), ab = 4 * ((long long)al + (long long)Rl * ar);
                    const zt x0 = zload_as<CX>(Xk, xb), x1 = zload_as<CX>(Xk, xb + 1);
                    o[j][0] = zfma(zload_as<CA>(Ak, ab + 2), x1, zc::mul(zload_as<CA>(Ak, ab), x0));
                    o[j][1] = zfma(zload_as<CA>(Ak, ab + 3), x1, zc::mul(zload_as<CA>(Ak, ab + 1), x0));
                }
                if (++ar == (unsigned int)Rr) { ar = 0; ++vr; }
            }
#pragma unroll
            for (int j = 0; j < TTN_ZAPPLY_K; ++j)
                if (c0 + j < uQ) {
                    const long long yb = 2 * ((long long)p + (long long)uP * (c0 + j));
                    zstore_nt(Yk, yb, o[j][0]);
                    zstore_nt(Yk, yb + 1, o[j][1]);
                }
        } else {
            for (int j = 0; j < TTN_ZAPPLY_K && c0 + j < uQ; ++j) {
                const long long xb = (long long)n * ((long long)vl + (long long)rl * vr), ab = (long long)n * n * ((long long)al + (long long)Rl * ar);
                const long long yb = (long long)n * ((long long)p + (long long)uP * (c0 + j));
                for (int i = 0; i < n; ++i) {
                    zt acc = zt{0.0, 0.0};
                    for (int jj = 0; jj < n; ++jj) acc = zfma(zload_as<CA>(Ak, ab + i + (long long)n * jj), zload_as<CX>(Xk, xb + jj), acc);
                    zstore_nt(Yk, yb + i, acc);
                }
                if (++ar == (unsigned int)Rr) { ar = 0; ++vr; }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// hadamard: Z_k[s, ay + ryl ax, by + ryr bx] = X_k[s,ax,bx] Y_k[s,ay,by], no conjugation (src/tt_operations.jl:343-361); k_hadamard's
// mapping: one thread = one left index p and TTN_ZHAD_K consecutive right indices q.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TTN_STREAM_TB) k_zhadamard(TTDev x, TTDev y, TTDev z) {
    const int k = blockIdx.y, b = blockIdx.z;
    const int n = x.dims[k] >> 1;
    const long long* xr = x.rks + (long long)b * (x.d + 1);
    const long long* yr = y.rks + (long long)b * (y.d + 1);
    const int rxl = (int)xr[k], rxr = (int)xr[k + 1], ryl = (int)yr[k], ryr = (int)yr[k + 1];
    const unsigned int uP = (unsigned int)(rxl * ryl), uQ = (unsigned int)(rxr * ryr);
    const double* Xk = x.data + (long long)b * x.stride + x.off[k];
    const double* Yk = y.data + (long long)b * y.stride + y.off[k];
    double* Zk = z.data + (long long)b * z.stride + z.off[k];
    const unsigned int qgroups = (uQ + TTN_ZHAD_K - 1) / TTN_ZHAD_K, items = uP * qgroups;
    for (unsigned int it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
        const unsigned int p = it % uP, q0 = (it / uP) * TTN_ZHAD_K;
        const unsigned int ay = p % (unsigned int)ryl, ax = p / (unsigned int)ryl;
        unsigned int by = q0 % (unsigned int)ryr, bx = q0 / (unsigned int)ryr;
        for (int j = 0; j < TTN_ZHAD_K && q0 + j < uQ; ++j) {
            const long long xb = (long long)n * (ax + (long long)rxl * bx), yb = (long long)n * (ay + (long long)ryl * by);
            const long long zb = (long long)n * ((long long)p + (long long)uP * (q0 + j));
            for (int s = 0; s < n; ++s) zstore_nt(Zk, zb + s, zc::mul(zload(Xk, xb + s), zload(Yk, yb + s)));
            if (++by == (unsigned int)ryr) { by = 0; ++bx; }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// scalar *: copy every core, multiply core `which` by a = (ar, ai) (src/tt_operations.jl:256-266); zero -> the all-zero train.  ab (device,
// per train, interleaved) overrides (ar, ai): a train whose factor is 0 becomes the zero train.  k_scale's mapping, one complex per trip.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TTN_STREAM_TB) k_zscale(TTDev x, TTDev y, double ar, double ai, int which, int zero, const int* which_b, const double* ab) {
    const int k = blockIdx.y, b = blockIdx.z;
    if (which_b) which = which_b[b];
    if (ab) { ar = ab[2 * b]; ai = ab[2 * b + 1]; zero = (ar == 0.0 && ai == 0.0) ? 1 : 0; }
    const long long* xr = x.rks + (long long)b * (x.d + 1);
    const long long total = (long long)(x.dims[k] >> 1) * xr[k] * xr[k + 1];
    const double* Xk = x.data + (long long)b * x.stride + x.off[k];
    double* Yk = y.data + (long long)b * y.stride + y.off[k];
    const zt a = zt{ar, ai};
    const bool mul = (k == which);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        zt v = zero ? zt{0.0, 0.0} : zload(Xk, e);
        if (mul && !zero) v = zc::mul(a, v);
        zstore_nt(Yk, e, v);
    }
}

// ---------------------------------------------------------------------------------------------
// dot(a, b) with the FIRST argument conjugated (src/tt_operations.jl:243-248), one workgroup per train:
//   T[i, p, b'] = sum_q W[p, q] B_k[i, q, b'],   W'[a', b'] = sum_{i, p} conj(A_k[i, p, a']) T[i, p, b'],   W = 1 at the start.
// W and T stay in LDS across the sites when they fit (ranks up to 32 x 32 at n = 2), in the train's global scratch otherwise.  Plain
// complex FMAs, no MFMA: the contraction is small against the apply and the rounding it feeds.
// ---------------------------------------------------------------------------------------------
struct ZDotArgs {
    TTDev a, b;
    double* scratch;
    long long scratch_stride;     // doubles per train: 2 (wmax + tmax)
    long long wmax, tmax;         // complex numbers in W / T
    int in_lds;
    double* out;                  // [batch] interleaved
};
__global__ void __launch_bounds__(TTN_ZC_WG) k_zdot(ZDotArgs P) {
    extern __shared__ double zdot_smem[];
    const int b = blockIdx.x, tid = threadIdx.x, d = P.a.d;
    double* W = P.in_lds ? zdot_smem : P.scratch + (long long)b * P.scratch_stride;
    double* T = W + 2 * P.wmax;
    const long long* ar = P.a.rks + (long long)b * (d + 1);
    const long long* br = P.b.rks + (long long)b * (d + 1);
    for (long long e = tid; e < ar[0] * br[0]; e += TTN_ZC_WG) zstore(W, e, (e % ar[0] == e / ar[0]) ? zt{1.0, 0.0} : zt{0.0, 0.0});
    __syncthreads();
    for (int k = 0; k < d; ++k) {
        const int n = P.a.dims[k] >> 1;
        const int ra = (int)ar[k], ra2 = (int)ar[k + 1], rb = (int)br[k], rb2 = (int)br[k + 1];
        const double* Ak = P.a.data + (long long)b * P.a.stride + P.a.off[k];
        const double* Bk = P.b.data + (long long)b * P.b.stride + P.b.off[k];
        const long long nt = (long long)n * ra * rb2;
        for (long long e = tid; e < nt; e += TTN_ZC_WG) {
            const int i = (int)(e % n), p = (int)((e / n) % ra), c = (int)(e / ((long long)n * ra));
            zt acc = zt{0.0, 0.0};
            for (int q = 0; q < rb; ++q) acc = zfma(zload(W, p + (long long)ra * q), zload(Bk, i + (long long)n * (q + (long long)rb * c)), acc);
            zstore(T, e, acc);
        }
        __syncthreads();
        const long long nw = (long long)ra2 * rb2;
        for (long long e = tid; e < nw; e += TTN_ZC_WG) {
            const int a2 = (int)(e % ra2), c = (int)(e / ra2);
            zt acc = zt{0.0, 0.0};
            const long long abase = (long long)n * ra * a2, tbase = (long long)n * ra * c;
            for (long long ip = 0; ip < (long long)n * ra; ++ip) acc = zfma(zc::conj(zload(Ak, abase + ip)), zload(T, tbase + ip), acc);
            zstore(W, e, acc);
        }
        __syncthreads();
    }
    if (tid == 0) { const zt v = zload(W, 0); P.out[2 * b] = v.x; P.out[2 * b + 1] = v.y; }
}

// ---------------------------------------------------------------------------------------------
// k_zcompress: tt_compress! / _tt_bond_truncate! / one-directional sweeps on complex trains (src/tt_tools.jl:743-789), one workgroup
// per train for the whole call, ranks device-resident — the contract of k_compress.  One bond step:
//   1. G (m x n, m >= n) = the merged matrix M[(alpha + Dl s1), (s2 + n2 beta)] or its conjugate transpose, whichever is tall;
//   2. Householder QR of G in place (zlarfg's real beta, as k_dense_qr): G = Q R, reflectors kept below the diagonal;
//   3. one-sided complex Jacobi on the n x n factor R (k_dense_svd<true>'s numerics: rotate above 2 eps sqrt(n), stop below
//      8 eps sqrt(n), hypot in the angle), R in LDS when n <= TTN_ZC_LDS_N, V accumulated in global memory:  R V = W = U_R S;
//   4. the rank rule of the effective _svdtrunc (relative tail norm when truncerr > 0, min(len, max_bond) otherwise);
//   5. Z = Q [W_j / sqrt(s_j); 0] (m x r) by the reflectors, Vs = V_j sqrt(s_j) (n x r); tall: core k <- Z, core k+1 <- Vs^H; wide: core
//      k <- Vs, core k+1 <- Z^H, the (l, s, r) <-> (s, l, r) permutes folded into the indexing.  sqrt(s) on both sides, no gauge step.
// A column with s_j = 0 contributes zeros on both sides, as U sqrt(S) and sqrt(S) V^H do whatever null vector LAPACK picks.
// ---------------------------------------------------------------------------------------------
struct ZCompressArgs {
    TTDev tt;
    long long max_bond;
    double truncerr;
    int sweeps, k_single, k_first, k_last;      // as CompressArgs
    double* scratch;
    long long scratch_stride;
    int pmax, qmax;
    int* status;
    int* sweep_stats;
};
// doubles of scratch per train
__host__ __device__ inline long long zcompress_scratch(long long pmax, long long qmax) { return 4 * pmax * qmax + 4 * pmax * pmax + 4 * pmax + 64; }

__device__ void zc_bond_step(const ZCompressArgs& P, int b, int k, double* Rl_, double* red, double* sh, int* ish) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = TTN_ZC_WG / 64;
    const TTDev& t = P.tt;
    long long* rks = t.rks + (long long)b * (t.d + 1);
    const int n1 = t.dims[k] >> 1, n2 = t.dims[k + 1] >> 1;
    const int Dl = (int)rks[k], Dm = (int)rks[k + 1], Dr = (int)rks[k + 2];
    const int Mr = n1 * Dl, Mc = n2 * Dr;
    const bool tall = Mr >= Mc;
    const int m = tall ? Mr : Mc, n = tall ? Mc : Mr;
    double* C1 = t.data + (long long)b * t.stride + t.off[k];
    double* C2 = t.data + (long long)b * t.stride + t.off[k + 1];
    double* S = P.scratch + (long long)b * P.scratch_stride;
    const long long pq = (long long)P.pmax * P.qmax, pp = (long long)P.pmax * P.pmax;
    double* G = S;                          // m x n complex
    double* Z = G + 2 * pq;                 // m x r complex
    double* V = Z + 2 * pq;                 // n x n complex
    double* Rg = V + 2 * pp;                // n x n complex when it does not fit the LDS
    double* taus = Rg + 2 * pp;             // n complex
    double* dw = taus + 2 * P.pmax;         // n column norms
    int* perm = reinterpret_cast<int*>(dw + P.pmax);      // n ints (pmax doubles reserved)
    double* Rp = (n <= TTN_ZC_LDS_N) ? Rl_ : Rg;

    // ---- 1. merge ----
    double amx = 0.0;
    for (long long e = tid; e < (long long)Mr * Mc; e += TTN_ZC_WG) {
        const int R = (int)(e % Mr), Cc = (int)(e / Mr);
        const int al = R % Dl, s1 = R / Dl, s2 = Cc % n2, be = Cc / n2;
        zt acc = zt{0.0, 0.0};
        for (int g = 0; g < Dm; ++g)
            acc = zfma(zload(C1, s1 + (long long)n1 * (al + (long long)Dl * g)), zload(C2, s2 + (long long)n2 * (g + (long long)Dm * be)), acc);
        if (tall) zstore(G, R + (long long)m * Cc, acc);
        else zstore(G, Cc + (long long)m * R, zc::conj(acc));
        amx = fmax(amx, fmax(fabs(acc.x), fabs(acc.y)));
    }
    // The step below is UNSCALED (reflector norms, column norms and the rank rule sum squares; the rotation test has an absolute floor):
    // a merged matrix whose size is outside SCALE_SAFE (ttn_common.h) is divided by an exact, even power of two here, and each of the
    // two cores gets the root of it back at the end.
    const int kexp = scale_rescue_exponent(wg_max(amx, red), true);
    __syncthreads();
    if (kexp != 0) {
        const double f = ldexp(1.0, -kexp);
        for (long long e = tid; e < (long long)m * n; e += TTN_ZC_WG) zstore(G, e, zc::scale(zload(G, e), f));
        __syncthreads();
    }
    // ---- 2. Householder QR of G ----
    for (int kk = 0; kk < n; ++kk) {
        double part = 0.0;
        for (int i = kk + 1 + tid; i < m; i += TTN_ZC_WG) part += zc::abs2(zload(G, i + (long long)m * kk));
        const double xnorm2 = wg_sum(part, red);
        if (tid == 0) {
            const zt alpha = zload(G, kk + (long long)m * kk);
            zt tau = zt{0.0, 0.0}, scal = zt{0.0, 0.0};
            double beta = alpha.x;
            if (xnorm2 != 0.0 || alpha.y != 0.0) {
                beta = -copysign(sqrt(zc::abs2(alpha) + xnorm2), alpha.x);
                tau = zt{(beta - alpha.x) / beta, -alpha.y / beta};
                const zt den = zt{alpha.x - beta, alpha.y};
                const double d2 = zc::abs2(den);
                scal = zt{den.x / d2, -den.y / d2};
            }
            zstore(taus, kk, tau);
            sh[0] = scal.x; sh[1] = scal.y; sh[2] = beta; sh[3] = tau.x; sh[4] = tau.y;
        }
        __syncthreads();
        const zt scal = zt{sh[0], sh[1]}, tau = zt{sh[3], sh[4]};
        const double beta = sh[2];
        const bool trivial = (tau.x == 0.0 && tau.y == 0.0);
        if (!trivial)
            for (int i = kk + 1 + tid; i < m; i += TTN_ZC_WG) zstore(G, i + (long long)m * kk, zc::mul(zload(G, i + (long long)m * kk), scal));
        __syncthreads();
        if (!trivial) {
            const zt ctau = zc::conj(tau);
            for (int j = kk + 1 + wave; j < n; j += nwaves) {          // H^H = I - conj(tau) v v^H on column j: one wave, lanes over the rows
                zt w = zt{0.0, 0.0};
                for (int i = kk + 1 + lane; i < m; i += 64) w = zfma(zc::conj(zload(G, i + (long long)m * kk)), zload(G, i + (long long)m * j), w);
                w = zc::wsum(w);
                w = zc::add(w, zload(G, kk + (long long)m * j));
                const zt tw = zc::mul(ctau, w);
                for (int i = kk + 1 + lane; i < m; i += 64)
                    zstore(G, i + (long long)m * j, zc::sub(zload(G, i + (long long)m * j), zc::mul(tw, zload(G, i + (long long)m * kk))));
                if (lane == 0) zstore(G, kk + (long long)m * j, zc::sub(zload(G, kk + (long long)m * j), tw));
            }
        }
        if (tid == 0) zstore(G, kk + (long long)m * kk, zt{beta, 0.0});
        __syncthreads();
    }
    // ---- 3. Jacobi on R ----
    for (long long e = tid; e < (long long)n * n; e += TTN_ZC_WG) {
        const int i = (int)(e % n), j = (int)(e / n);
        zstore(Rp, e, (i <= j) ? zload(G, i + (long long)m * j) : zt{0.0, 0.0});
        zstore(V, e, (i == j) ? zt{1.0, 0.0} : zt{0.0, 0.0});
    }
    __syncthreads();
    const int np = n + (n & 1);
    const double tol_rot = 2.0 * DBL_EPSILON * sqrt((double)n), tol_conv = 8.0 * DBL_EPSILON * sqrt((double)n);
    int sweep = 0;
    for (; sweep < TTN_ZC_MAX_SWEEPS && n > 1; ++sweep) {
        if (tid == 0) ish[0] = 0;
        __syncthreads();
        for (int round = 0; round < np - 1; ++round) {
            for (int pr = wave; pr < np / 2; pr += nwaves) {
                const int a = (pr == 0) ? np - 1 : (round + pr) % (np - 1);
                const int c_ = (round + np - 1 - pr) % (np - 1);
                const int p = a < c_ ? a : c_, q = a < c_ ? c_ : a;
                if (q >= n) continue;
                double al = 0.0, be = 0.0;
                zt ga = zt{0.0, 0.0};
                for (int i = lane; i < n; i += 64) {
                    const zt gp = zload(Rp, i + (long long)n * p), gq = zload(Rp, i + (long long)n * q);
                    al += zc::abs2(gp); be += zc::abs2(gq);
                    ga = zfma(zc::conj(gp), gq, ga);
                }
                al = wave_sum(al); be = wave_sum(be); ga = zc::wsum(ga);
                const double ag = zc::absv(ga), nn = sqrt(al * be);
                if (ag > tol_rot * nn && ag > 1.0e-154) {
                    if (lane == 0 && ag > tol_conv * nn) ish[0] = 1;
                    const zt ph = zc::scale(ga, 1.0 / ag);
                    const double zeta = (be - al) / (2.0 * ag);
                    const double tt_ = copysign(1.0, zeta) / (fabs(zeta) + hypot(1.0, zeta));
                    const double c = 1.0 / sqrt(1.0 + tt_ * tt_), s_ = c * tt_;
                    const zt sph = zc::scale(ph, s_), sphc = zc::conj(sph);
                    for (int i = lane; i < n; i += 64) {
                        const zt gp = zload(Rp, i + (long long)n * p), gq = zload(Rp, i + (long long)n * q);
                        zstore(Rp, i + (long long)n * p, zc::sub(zc::scale(gp, c), zc::mul(sphc, gq)));
                        zstore(Rp, i + (long long)n * q, zc::add(zc::mul(sph, gp), zc::scale(gq, c)));
                        const zt vp = zload(V, i + (long long)n * p), vq = zload(V, i + (long long)n * q);
                        zstore(V, i + (long long)n * p, zc::sub(zc::scale(vp, c), zc::mul(sphc, vq)));
                        zstore(V, i + (long long)n * q, zc::add(zc::mul(sph, vp), zc::scale(vq, c)));
                    }
                }
            }
            __syncthreads();
        }
        const int again = ish[0];
        __syncthreads();
        if (!again) break;
    }
    if (tid == 0) {
        if (sweep >= TTN_ZC_MAX_SWEEPS) ttn_set_status(P.status + b, TTN_ST_JACOBI);
        P.sweep_stats[b] += sweep + (sweep < TTN_ZC_MAX_SWEEPS && n > 1 ? 1 : 0);
    }
    // ---- singular values = column norms of W, sorted descending by counting ----
    for (int j = wave; j < n; j += nwaves) {
        double a = 0.0;
        for (int i = lane; i < n; i += 64) a += zc::abs2(zload(Rp, i + (long long)n * j));
        a = wave_sum(a);
        if (lane == 0) dw[j] = sqrt(a);
    }
    __syncthreads();
    for (int j = tid; j < n; j += TTN_ZC_WG) {
        int rank = 0;
        const double v = dw[j];
        for (int q = 0; q < n; ++q) { const double w = dw[q]; rank += (w > v || (w == v && q < j)) ? 1 : 0; }
        perm[rank] = j;
    }
    __syncthreads();
    // ---- 4. the rank ----
    if (tid == 0) {
        int r = n;
        if (P.truncerr > 0.0) {
            double nrm2 = 0.0;
            for (int i = n - 1; i >= 0; --i) { const double s_ = dw[perm[i]]; nrm2 += s_ * s_; }
            const double nrm = sqrt(nrm2);
            double cum = 0.0;
            for (int i = n; i >= 1; --i) {
                const double s_ = dw[perm[i - 1]];
                cum += s_ * s_;
                if (sqrt(cum) > P.truncerr * nrm) { r = i; break; }
            }
        }
        if ((long long)r > P.max_bond) r = (int)P.max_bond;
        if ((long long)r > t.cap[k + 1]) { r = (int)t.cap[k + 1]; ttn_set_status(P.status + b, TTN_ST_RANK_OVERFLOW); }
        ish[1] = r;
    }
    __syncthreads();
    const int r = ish[1];
    // ---- 5. Z = Q [W_j / sqrt(s_j); 0] ----
    for (long long e = tid; e < (long long)m * r; e += TTN_ZC_WG) {
        const int i = (int)(e % m), j = (int)(e / m);
        const double s_ = dw[perm[j]];
        zstore(Z, e, (i < n && s_ > 0.0) ? zc::scale(zload(Rp, i + (long long)n * perm[j]), 1.0 / sqrt(s_)) : zt{0.0, 0.0});
    }
    __syncthreads();
    for (int kk = n - 1; kk >= 0; --kk) {
        const zt tau = zload(taus, kk);
        if (tau.x != 0.0 || tau.y != 0.0) {
            for (int j = wave; j < r; j += nwaves) {
                zt w = zt{0.0, 0.0};
                for (int i = kk + 1 + lane; i < m; i += 64) w = zfma(zc::conj(zload(G, i + (long long)m * kk)), zload(Z, i + (long long)m * j), w);
                w = zc::wsum(w);
                w = zc::add(w, zload(Z, kk + (long long)m * j));
                const zt tw = zc::mul(tau, w);
                for (int i = kk + 1 + lane; i < m; i += 64)
                    zstore(Z, i + (long long)m * j, zc::sub(zload(Z, i + (long long)m * j), zc::mul(tw, zload(G, i + (long long)m * kk))));
                if (lane == 0) zstore(Z, kk + (long long)m * j, zc::sub(zload(Z, kk + (long long)m * j), tw));
            }
            __syncthreads();
        }
    }
    __syncthreads();
    // ---- the two cores (the merged matrix is gone: both slots are free) ----
    for (long long e = tid; e < (long long)Mr * r; e += TTN_ZC_WG) {          // core k [s1, alpha, j] <- U sqrt(S) [alpha + Dl s1, j]
        const int R = (int)(e % Mr), j = (int)(e / Mr);
        const int al = R % Dl, s1 = R / Dl;
        const zt v = tall ? zload(Z, R + (long long)m * j) : zc::scale(zload(V, R + (long long)n * perm[j]), sqrt(dw[perm[j]]));
        zstore(C1, s1 + (long long)n1 * (al + (long long)Dl * j), v);
    }
    for (long long e = tid; e < (long long)Mc * r; e += TTN_ZC_WG) {          // core k+1 [s2, j, beta] <- sqrt(S) V^H [j, s2 + n2 beta]
        const int Cc = (int)(e % Mc), j = (int)(e / Mc);
        const int s2 = Cc % n2, be = Cc / n2;
        const zt v = tall ? zc::scale(zload(V, Cc + (long long)n * perm[j]), sqrt(dw[perm[j]])) : zload(Z, Cc + (long long)m * j);
        zstore(C2, s2 + (long long)n2 * (j + (long long)r * be), zc::conj(v));
    }
    if (kexp != 0) {
        const double f = ldexp(1.0, kexp / 2);
        __syncthreads();
        for (long long e = tid; e < (long long)Mr * r; e += TTN_ZC_WG) zstore(C1, e, zc::scale(zload(C1, e), f));
        for (long long e = tid; e < (long long)Mc * r; e += TTN_ZC_WG) zstore(C2, e, zc::scale(zload(C2, e), f));
    }
    if (tid == 0) rks[k + 1] = r;
    __syncthreads();
}

__global__ void __launch_bounds__(TTN_ZC_WG) k_zcompress(ZCompressArgs P) {
    extern __shared__ double zc_smem[];
    __shared__ double red[40];
    __shared__ double sh[8];
    __shared__ int ish[4];
    const int b = blockIdx.x, d = P.tt.d;
    if (threadIdx.x == 0) P.sweep_stats[b] = 0;
    __syncthreads();
    if (P.k_single > 0) { zc_bond_step(P, b, P.k_single - 1, zc_smem, red, sh, ish); return; }
    if (P.k_single < 0) {
        if (P.k_first <= P.k_last) for (int k = P.k_first; k <= P.k_last; ++k) zc_bond_step(P, b, k, zc_smem, red, sh, ish);
        else for (int k = P.k_first; k >= P.k_last; --k) zc_bond_step(P, b, k, zc_smem, red, sh, ish);
        return;
    }
    for (int sw = 0; sw < P.sweeps; ++sw) {
        for (int k = 0; k + 1 < d; ++k) zc_bond_step(P, b, k, zc_smem, red, sh, ish);
        for (int k = d - 2; k >= 0; --k) zc_bond_step(P, b, k, zc_smem, red, sh, ish);
    }
}
