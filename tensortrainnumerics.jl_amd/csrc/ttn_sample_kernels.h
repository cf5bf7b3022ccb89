// ttn_sample_kernels.h — sampling of resident trains (include/ttn_sample.h): configurations z drawn from
//       p(z) = x(z)^2 / <x, x>        (TTN_SAMPLE_BORN)        or        p(z) = x(z) / sum_z x(z)        (TTN_SAMPLE_DENSITY)
// by the conditional sweep over the sites.  Float64 only.
//
//   phase 0   the right environments, once per call: Born mode takes the G chain of k_grad_chain (ttn_grad_kernels.h) on (x, x),
//             G_{d+1} = [1], G_k = sum_z A_k[z] G_{k+1} A_k[z]^T; density mode walks the vectors g_{d+1} = [1], g_k = sum_z A_k[z] g_{k+1}
//             in k_sample_genv (one workgroup per train).
//   phase 1   k_sample_sweep, grid (sample tiles, trains): a workgroup carries SAMPLE_TILE = 64 samples through all d sites.  The running
//             left vectors are the rows of V (64 x r_{k-1}); a site forms the candidates W_z = V A_k[z] for every z, the weights
//             p_z[s] = W_z[s, :] G_{k+1} W_z[s, :]^T (Born) or W_z[s, :] g_{k+1} (density), and then ONE THREAD PER SAMPLE picks z from the
//             cumulative sums, adds log(p_z / tot) and the 16 waves copy the chosen row, scaled by a power of two, into V.  The products
//             never diverge: only the pick is per sample.
//
// Routes, one per SITE as in k_grad_chain:
//   * on chip (n = 2, both ranks <= 64): V, W_0 and W_1 are three LDS images of the k_dot_fused layout, stored TRANSPOSED (entry (s, a) at
//     DOT_AT(a, s)): wave (ta, ts) owns the 16 x 16 tile (a-block ta, sample block ts) of W_0^T and W_1^T = A_k[z]^T V^T — the core
//     fragment of both z arrives in one 16-byte load, V^T is the B operand read from LDS — and, in Born mode, the tile (b-block, sample
//     block) of T_z^T = G W_z^T with G read from global memory (it is shared by every tile of the train and stays in L2).  All on
//     v_mfma_f64_16x16x4_f64.  p_z is summed from 16 partial sums per sample in a fixed order.
//   * general (any other n or rank): the same products by wg_gemm on per-workgroup workspace, W[s, (z, a)] = V A_k as ONE 64 x n r' x r
//     product and T = W G as one 64 n x r' x r' product.
// V moves between LDS and workspace when consecutive sites differ in route.
//
// Every reduction of this file has a fixed order.  The Born environments come from k_grad_chain, whose on-chip sites add with LDS
// atomics: a call is reproducible to rounding, and two calls can differ only in a sample whose t = u tot lies within rounding of a
// cumulative sum.
#pragma once
#include "ttn_common.h"
#include "ttn_wg_gemm.h"
#include "ttn_dot_kernels.h"

#define SAMPLE_TILE 64                                                   // samples per workgroup: one lane of wave 0 per sample, four 16-row MFMA blocks
#define SAMPLE_MAX_D DOT_MAX_D
#define SAMPLE_DRAW_KIND 6                                               // cross.DRAW_SAMPLE: the draw kind of the sub-seed
// LDS: three images, then 2 x 16 x 64 partial sums and 64 picks.  These lie inside the region the workgroup GEMMs own (their staging tail
// and descriptor), which is free whenever no GEMM runs: no byte beyond what k_dot_fused already asks for.
#define SAMPLE_PART_AT (3 * DOT_MS_DOUBLES)
#define SAMPLE_PART_DOUBLES (2 * TTN_NWAVES * SAMPLE_TILE)
#define SAMPLE_ZSEL_AT (SAMPLE_PART_AT + SAMPLE_PART_DOUBLES)
#define SAMPLE_LDS_BYTES (sizeof(double) * DOT_LDS_DOUBLES)
static_assert(TTN_NWAVES == 16, "k_sample_sweep: 16 waves form the 4 x 4 tile grid of a 64 x 64 image");
static_assert(SAMPLE_ZSEL_AT + SAMPLE_TILE / 2 <= DOT_LDS_DOUBLES, "k_sample_sweep: the partial sums do not fit behind the images");

struct SampleArgs {
    TTDev x;                 // the trains of this launch (a chunk of the handle's batch: data and rks advanced by the host)
    const double* genv;      // right environments: train b, bond m (0 .. d) at genv + b gbs + m gss; bond m is r_m x r_m column-major (Born)
    long long gbs, gss;      //                     or r_m entries (density)
    int born;
    long long S;             // samples per train of the whole call (the stride of the outputs)
    long long s0, s1;        // this launch draws the samples s0 <= s < s1: gridDim.x = ceil((s1 - s0) / SAMPLE_TILE)
    unsigned long long seed;
    long long b0;            // index of the launch's first train in the batch (the sub-seed depends on it; the pointers below are advanced)
    const double* u;         // [k + d (s + S b)], or null: the uniforms are generated
    long long* idx;          // [k + d (s + S b)], 1-based
    double* logp;            // [s + S b]
    unsigned long long* info;   // [2 b]: clamps, [2 b + 1]: dead samples (zeroed by the host); or null
    double* work;            // general route: wstride doubles per workgroup — V [0, vsz), W [vsz, vsz + wsz), T behind it, then 64 nmax weights
    long long wstride, vsz, wsz;
};

struct SampleEnvArgs {
    TTDev x;
    double* g;               // [batch][d + 1][gss]
    long long gbs, gss;
};

// word j (1-based) of the splitmix64 stream of `sub` (constructors._splitmix64), as the 53-bit uniform (word >> 11) 2^-53
__device__ __forceinline__ double sample_uniform(unsigned long long sub, unsigned long long j) {
    unsigned long long z = sub + j * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// cross._subseed(seed, kind, a, 0) in 64-bit wrap-around arithmetic
__device__ __forceinline__ unsigned long long sample_subseed(unsigned long long seed, unsigned long long kind, unsigned long long a) {
    const unsigned long long p = 1000003ULL;
    return ((seed * p + kind) * p + a) * p;
}

__device__ __forceinline__ double sample_wave_sum(double p) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) p += __shfl_down(p, s, 64);
    return p;
}

struct SampleState {
    double lp;
    int clamps;
    bool dead;
};

// Steps 3 - 6 and 8 of include/ttn_sample.h for one sample: pz(z) is its weight p_z.  Returns the drawn z (0-based), or -1 for a dead sample.
template <class PF>
__device__ __forceinline__ int sample_pick(int n, PF pz, double u, SampleState& st) {
    if (st.dead) return -1;
    double tot = 0.0;
    for (int z = 0; z < n; ++z) {
        double p = pz(z);
        if (p < 0.0) { p = 0.0; ++st.clamps; }
        tot += p;
    }
    if (!(tot > 0.0) || !(tot < __builtin_inf())) {                       // 0, NaN or infinite
        st.dead = true;
        st.lp = -__builtin_inf();
        return -1;
    }
    const double t = u * tot;
    double c = 0.0, pc = 0.0;
    int zc = n - 1;
    for (int z = 0; z < n; ++z) {
        double p = pz(z);
        if (p < 0.0) p = 0.0;
        c += p;
        pc = p;
        if (t < c) { zc = z; break; }
    }
    st.lp += log(pc / tot);
    return zc;
}

// ---------------------------------------------------------------------------------------------
// density mode: g_{d+1} = [1], g_k[al] = sum_{z, a} A_k[z, al, a] g_{k+1}[a] — wave w owns the rows al = w, w + 16, ...; a lane sums the
// pairs (z, a) = lane, lane + 64, ... and the 64 lane sums are added by shuffles: a fixed order
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TTN_WG) k_sample_genv(SampleEnvArgs P) {
    const int d = P.x.d, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const long long* rk = P.x.rks + (long long)b * (d + 1);
    double* gb = P.g + (long long)b * P.gbs;
    const double* Xb = P.x.data + (long long)b * P.x.stride;
    {
        const int rd = uni32((int)rk[d]);
        for (int e = tid; e < rd; e += TTN_WG) gb[(long long)d * P.gss + e] = (e == 0) ? 1.0 : 0.0;
        __syncthreads();
    }
    for (int k = d - 1; k >= 0; --k) {
        const int r = uni32((int)rk[k]), r2 = uni32((int)rk[k + 1]), n = uni32(P.x.dims[k]);
        const double* Xk = Xb + P.x.off[k];
        const double* gin = gb + (long long)(k + 1) * P.gss;
        double* gout = gb + (long long)k * P.gss;
        const long long cols = (long long)n * r2;
        for (int al = wave; al < r; al += TTN_NWAVES) {
            double acc = 0.0;
            for (long long j = lane; j < cols; j += 64) {
                const int z = (int)(j % n), a = (int)(j / n);
                acc = fma(Xk[z + (long long)n * (al + (long long)r * a)], gin[a], acc);
            }
            acc = sample_wave_sum(acc);
            if (lane == 0) gout[al] = acc;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// one site of the on-chip class.  V, W0, W1: images, entry (sample s, rank index a) at DOT_AT(a, s).  On return (after a barrier) the 16
// partial sums of p_z[s] stand at part[(16 z + g) 64 + s].
// ---------------------------------------------------------------------------------------------
__device__ __noinline__ void sample_site_chip(const double* Xk, const double* G, int born, int r, int r2, const lds_f64* V, lds_f64* W0, lds_f64* W1,
                                              lds_f64* part) {
    Xk = unip(Xk); G = unip(G); born = uni32(born); r = uni32(r); r2 = uni32(r2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int ta = wave & 3, ts = wave >> 2;
    const int sq = 16 * ts + li;
    // ---- W_z^T[a, s] = sum_al A_k[z, al, a] V[s, al]: rows a = 16 ta + ., columns s = 16 ts + . ----
    if (16 * ta < r2) {                                                   // wave-uniform
        mfma_acc_t w0 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}, w1 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
        const int aq = 16 * ta + li;
        const int nt = (r + 3) >> 2;                                      // k-steps of four al
        for (int t = 0; t < nt; ++t) {
            const dot_f64x2 av = dot_load2(Xk, 4 * t + lk, aq, r, r2, r);                 // A_k[., al = 4 t + lk, a = aq]
            const double bv = V[DOT_AT(4 * t + lk, sq)];
            w0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv, w0, 0, 0, 0);
            w1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv, w1, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {                              // rows a >= r2 of the block are exact zeros
            W0[DOT_AT(16 * ta + lk + 4 * reg, sq)] = w0[reg];
            W1[DOT_AT(16 * ta + lk + 4 * reg, sq)] = w1[reg];
        }
    }
    __syncthreads();
    double pp0 = 0.0, pp1 = 0.0;
    if (born) {
        // ---- T_z^T[b, s] = sum_a G[b, a] W_z^T[a, s]: rows b = 16 ta + ., and this lane's share of sum_b W_z^T[b, s] T_z^T[b, s] ----
        if (16 * ta < r2) {                                               // wave-uniform
            mfma_acc_t t0 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}, t1 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
            const int bq = 16 * ta + li;
            const int nt = (r2 + 3) >> 2;                                 // k-steps of four a
            for (int t = 0; t < nt; ++t) {
                const int a = 4 * t + lk;
                const bool ok = (bq < r2) && (a < r2);
                double ga = G[ok ? bq + r2 * a : 0];
                if (!ok) ga = 0.0;
                t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ga, W0[DOT_AT(a, sq)], t0, 0, 0, 0);
                t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ga, W1[DOT_AT(a, sq)], t1, 0, 0, 0);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                pp0 = fma(t0[reg], W0[DOT_AT(16 * ta + lk + 4 * reg, sq)], pp0);
                pp1 = fma(t1[reg], W1[DOT_AT(16 * ta + lk + 4 * reg, sq)], pp1);
            }
        }
        part[(4 * ta + lk) * SAMPLE_TILE + sq] = pp0;
        part[(TTN_NWAVES + 4 * ta + lk) * SAMPLE_TILE + sq] = pp1;
    } else {
        // ---- wave w: the rows a = w, w + 16, ... of sum_a W_z^T[a, s] g[a], lane = sample ----
        for (int a = wave; a < r2; a += TTN_NWAVES) {
            const double ga = G[a];
            pp0 = fma(W0[DOT_AT(a, lane)], ga, pp0);
            pp1 = fma(W1[DOT_AT(a, lane)], ga, pp1);
        }
        part[wave * SAMPLE_TILE + lane] = pp0;
        part[(TTN_NWAVES + wave) * SAMPLE_TILE + lane] = pp1;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// block (tile, b): the samples s0 + 64 tile .. of train b through all sites
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TTN_WG) k_sample_sweep(SampleArgs P) {
    extern __shared__ double lds[];
    const int d = P.x.d, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const long long s = P.s0 + (long long)blockIdx.x * SAMPLE_TILE + lane;               // the sample of this lane (every wave sees all 64)
    const bool valid = s < P.s1;
    lds_f64* img = (lds_f64*)lds;
    lds_f64* Vi = img;
    lds_f64* W0 = img + DOT_MS_DOUBLES;
    lds_f64* W1 = img + 2 * DOT_MS_DOUBLES;
    lds_f64* part = img + SAMPLE_PART_AT;
    lds_i32* zsel = (lds_i32*)(img + SAMPLE_ZSEL_AT);
    const long long* rk = P.x.rks + (long long)b * (d + 1);
    const double* Xb = P.x.data + (long long)b * P.x.stride;
    const double* Gb = P.genv + (long long)b * P.gbs;
    double* wk = P.work + ((long long)b * gridDim.x + blockIdx.x) * P.wstride;
    double* Vg = wk;
    double* Wg = wk + P.vsz;
    double* Tg = Wg + P.wsz;
    double* Pg = Tg + P.wsz;
    const unsigned long long sub = sample_subseed(P.seed, SAMPLE_DRAW_KIND, (unsigned long long)(P.b0 + b));
    const long long orow = s + P.S * b;                                   // this sample's row of the outputs
    SampleState st;
    st.lp = 0.0; st.clamps = 0; st.dead = !valid;

    // v = [1]: V starts in LDS, all three images clean
    for (int e = tid; e < 3 * DOT_MS_DOUBLES; e += TTN_WG) img[e] = 0.0;
    __syncthreads();
    if (wave == 0) Vi[DOT_AT(0, lane)] = valid ? 1.0 : 0.0;
    __syncthreads();
    bool in_lds = true;

    for (int k = 0; k < d; ++k) {
        const int r = uni32((int)rk[k]), r2 = uni32((int)rk[k + 1]), n = uni32(P.x.dims[k]);
        const double* Xk = Xb + P.x.off[k];
        const double* G = Gb + (long long)(k + 1) * P.gss;
        const bool fit = n == 2 && r <= DOT_RMAX && r2 <= DOT_RMAX;
        double u = 0.5;
        if (wave == 0 && valid) u = P.u ? P.u[k + (long long)d * orow] : sample_uniform(sub, 1ULL + (unsigned long long)k + (unsigned long long)d * (unsigned long long)s);
        int zs = -1;
        if (fit) {
            if (!in_lds) {                                                // V returns to LDS: the GEMMs used the images' memory
                for (int a = wave; a < DOT_RMAX; a += TTN_NWAVES) Vi[DOT_AT(a, lane)] = a < r ? Vg[lane + (long long)SAMPLE_TILE * a] : 0.0;
                __syncthreads();
                in_lds = true;
            }
            sample_site_chip(Xk, G, P.born, r, r2, Vi, W0, W1, part);
            if (wave == 0) {
                double p2[2] = {0.0, 0.0};
                for (int g = 0; g < TTN_NWAVES; ++g) {
                    p2[0] += part[g * SAMPLE_TILE + lane];
                    p2[1] += part[(TTN_NWAVES + g) * SAMPLE_TILE + lane];
                }
                zs = sample_pick(2, [&](int z) { return z ? p2[1] : p2[0]; }, u, st);
                zsel[lane] = zs;
                if (valid) P.idx[k + (long long)d * orow] = zs < 0 ? 1 : zs + 1;
            }
            __syncthreads();
            // step 7: the chosen row, scaled by the binade of its largest entry — 16 partial maxima per sample, then every wave its rows
            zs = zsel[lane];
            const lds_f64* Wz = zs == 1 ? W1 : W0;
            double m = 0.0;
            if (zs >= 0)
                for (int a = wave; a < r2; a += TTN_NWAVES) m = fmax(m, fabs(Wz[DOT_AT(a, lane)]));
            part[wave * SAMPLE_TILE + lane] = m;
            __syncthreads();
            m = 0.0;
            for (int g = 0; g < TTN_NWAVES; ++g) m = fmax(m, part[g * SAMPLE_TILE + lane]);
            const int e = (m > 0.0 && m < __builtin_inf()) ? ilogb(m) : 0;
            const int rows = zs >= 0 ? ((r2 + 3) & ~3) : DOT_RMAX;        // a dead sample: the whole row of V is cleared
            for (int a = wave; a < rows; a += TTN_NWAVES) Vi[DOT_AT(a, lane)] = (zs >= 0 && a < r2) ? ldexp(Wz[DOT_AT(a, lane)], -e) : 0.0;
            __syncthreads();
        } else {
            if (in_lds) {                                                 // V leaves LDS: the GEMMs use the images' memory
                for (int a = wave; a < r; a += TTN_NWAVES) Vg[lane + (long long)SAMPLE_TILE * a] = Vi[DOT_AT(a, lane)];
                __syncthreads();
                in_lds = false;
            }
            const int rows = SAMPLE_TILE * n;                             // (s, z) pairs, s fastest
            {
                // W[s, z + n a] = sum_al V[s, al] A_k[z, al, a]
                const View Vv = mkview(Vg, plain(1), plain(SAMPLE_TILE));
                const View Av = mkview((double*)Xk, plain(n), Idx{n, 1, (long long)n * r});
                const View Wv = mkview(Wg, plain(1), plain(SAMPLE_TILE));
                wg_gemm(SAMPLE_TILE, n * r2, r, Vv, Av, Wv, 1.0, 0.0, lds);
                __syncthreads();
            }
            if (P.born) {
                // T[(s, z), b] = sum_a W[(s, z), a] G[a, b]
                const View Wv = mkview(Wg, plain(1), plain(rows));
                const View Gv = mkview((double*)G, plain(1), plain(r2));
                const View Tv = mkview(Tg, plain(1), plain(rows));
                wg_gemm(rows, r2, r2, Wv, Gv, Tv, 1.0, 0.0, lds);
                __syncthreads();
                for (int i = tid; i < rows; i += TTN_WG) {
                    double acc = 0.0;
                    for (int a = 0; a < r2; ++a) acc = fma(Wg[i + (long long)rows * a], Tg[i + (long long)rows * a], acc);
                    Pg[i] = acc;
                }
            } else {
                for (int i = tid; i < rows; i += TTN_WG) {
                    double acc = 0.0;
                    for (int a = 0; a < r2; ++a) acc = fma(Wg[i + (long long)rows * a], G[a], acc);
                    Pg[i] = acc;
                }
            }
            __syncthreads();
            if (wave == 0) {
                zs = sample_pick(n, [&](int z) { return Pg[lane + (long long)SAMPLE_TILE * z]; }, u, st);
                zsel[lane] = zs;
                if (valid) P.idx[k + (long long)d * orow] = zs < 0 ? 1 : zs + 1;
            }
            __syncthreads();
            zs = zsel[lane];
            const double* Wz = Wg + lane + (long long)SAMPLE_TILE * (zs < 0 ? 0 : zs);
            double m = 0.0;
            if (zs >= 0)
                for (int a = wave; a < r2; a += TTN_NWAVES) m = fmax(m, fabs(Wz[(long long)rows * a]));
            part[wave * SAMPLE_TILE + lane] = m;
            __syncthreads();
            m = 0.0;
            for (int g = 0; g < TTN_NWAVES; ++g) m = fmax(m, part[g * SAMPLE_TILE + lane]);
            const int e = (m > 0.0 && m < __builtin_inf()) ? ilogb(m) : 0;
            for (int a = wave; a < r2; a += TTN_NWAVES) Vg[lane + (long long)SAMPLE_TILE * a] = zs >= 0 ? ldexp(Wz[(long long)rows * a], -e) : 0.0;
            __syncthreads();
        }
    }
    if (wave == 0) {
        if (valid) P.logp[orow] = st.lp;
        if (P.info) {
            unsigned long long nc = (unsigned long long)st.clamps, nd = (valid && st.dead) ? 1ULL : 0ULL;
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) { nc += __shfl_down(nc, sh, 64); nd += __shfl_down(nd, sh, 64); }
            if (lane == 0) {
                if (nc) atomicAdd(P.info + 2 * b, nc);
                if (nd) atomicAdd(P.info + 2 * b + 1, nd);
            }
        }
    }
}
