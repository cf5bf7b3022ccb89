// ttn_zmeasure_kernels.h — site-resolved measurements of a ComplexF64 train x (include/ttn_zmeasure.h): the profile
//       E_O[k]     = <x| O_k |x> / <x|x>                                  (one complex n_k x n_k matrix O_k per site: an operator TABLE)
// and the two-point functions
//       C_PQ[i, j] = <x| P_i Q_j |x> / <x|x>                              for ALL pairs (i, j)
// in O(d) chain work plus O(d^2) short walks per train: the three phases of ttn_measure_kernels.h on interleaved (re, im) cores, the bra
// conjugated.  The first index of a table meets the conjugated bra.
//
//   phase 0   k_zmeasure_chain, grid (batch, 2): L_1 .. L_{d+1} left to right and G_{d+1} .. G_1 right to left, every state kept,
//                 L'[a, b]   = sum_{z, al, be} conj(x_k[z, al, a]) L[al, be] x_k[z, be, b]
//                 G'[al, be] = sum_{z, a, b}   conj(x_k[z, al, a]) G[a, b]   x_k[z, be, b]
//             <x|x> = re L_{d+1}[1, 1].
//   phase 1   k_zmeasure_open, grid (d * tables, batch): workgroup (k, t, b) runs ONE left-to-right site with the ket core O_k x_k, stores
//             V^O_k and reduces E_O[k] = sum V^O_k G_{k+1} / <x|x> in a fixed order.
//   phase 2   k_zmeasure_walk, grid (d - 1, batch, passes), longest walks first: workgroup (j, b) opens right to left at site j with the ket
//             core O1_j x_j on G_{j+1} and carries the state through j - 1, j - 2, ... with the plain step; in front of every i < j it emits
//             sum V^{O2}_i T — the plain complex product, no conjugate: the bra's conjugate is already inside V and T.  Pass 0 runs
//             (O1, O2) = (Q, P) and fills the upper triangle, pass 1 runs (P, Q) and fills the lower one; the diagonal is phase 1 with the
//             table P_k Q_k.
//
// Routes, one per TRAIN (decided from its rank words, as k_zexpect decides): every kernel is a template on the route, the on-chip
// instantiation holds no call and no stack, the general one is separate, and a batch that may hold both classes launches both.
//   on-chip (every n_k = 2 — known on the host — and every rank of the train <= 64): the site step is the two-layer form of
//     braket_site<true, true, 1> (ttn_braket_kernels.h) — bra, ket and a 2 x 2 complex table in between, applied in registers to the
//     accumulators of the first product; both products on the fp64 MFMA on split re / im fragments, conj and the minus of the real part
//     the negate bit; the four waves of a column block meet in two LDS images (re, im) by LDS atomics.  zm_site<LR> runs it in either
//     direction: the left-to-right form is the same code with the roles of the two rank indices of a core exchanged in the loads.  A
//     state lives in workspace as two dense 64 x 64 planes (re, then im; entry (p, q) at p + 64 q), zero outside the current ranks,
//     so the first product reads it without masks; a step reads one state and writes another, nothing rotates through LDS.
//   general (any n, any ranks): O x_k is formed in workspace and a site is two complex products, each four workgroup GEMMs on
//     stride-2 views (braket_gemm); a state is r x r interleaved, column-major.
//
// Reductions: a product sum V T is summed per thread over a fixed set of entries, per wave by shuffles, and the 16 wave sums by one
// thread, all in a fixed order.  The on-chip states come from LDS atomics, whose order is not fixed: results are reproducible to
// rounding, not bitwise.
#pragma once
#include "ttn_common.h"
#include "ttn_wg_gemm.h"
#include "ttn_dot_kernels.h"
#include "ttn_tdvp_kernels.h"
#include "ttn_braket_kernels.h"

#define ZMEASURE_MAX_OPS 16                                               // tables per call (TTN_ZMEASURE_MAX_OPS)
#define ZMEASURE_MAX_D DOT_MAX_D
#define ZMEASURE_RMAX BRAKET_QTT_RMAX                                     // largest rank of the on-chip route
#define ZM_IMG BRAKET_IMG                                                 // doubles of one plane of an on-chip state in workspace
#define ZM_STATE (2 * ZM_IMG)                                             // ... of the state
#define ZM_WORK_DOUBLES ((2 * DOT_MS_DOUBLES) > GEMM_LDS_TOTAL ? (2 * DOT_MS_DOUBLES) : GEMM_LDS_TOTAL)      // two images, or the GEMM's tiles
#define ZM_RED_DOUBLES (2 * 2 * TTN_NWAVES)                               // behind them: two alternating rows of 16 (re, im) wave sums
#define ZM_TAB 2                                                          // ints per site of the table behind those: [0] r_k, [1] off_k
#define ZM_LDS_BYTES(d) (sizeof(double) * (ZM_WORK_DOUBLES + ZM_RED_DOUBLES) + sizeof(int) * ZM_TAB * ((d) + 2))
static_assert(ZM_LDS_BYTES(ZMEASURE_MAX_D) <= 160 * 1024, "k_zmeasure_*: the LDS of a workgroup is 160 KiB");

struct ZMeasureArgs {
    TTDev x;                 // the trains of this launch (a chunk of the handle's batch: data and rks advanced by the host)
    double* env;             // [batch][2][d + 1][W]: L on bond 0 .. d, then G on bond 0 .. d
    long long W;             // doubles of one state slot
    const double* tabs;      // [ntab][2 S]: the operator tables, site k of a table at 2 toff[k], n_k x n_k column-major, interleaved
    const long long* toff;   // [d], in elements
    long long S;
    int ntab;
    double* V;               // [batch][ntab][d][W]: V^O_k
    double* St;              // [batch][passes][d - 1][2][W]: the two states a walk alternates between
    double* ctb;             // general route, k_zmeasure_chain: [batch][2][tsz], the GEMM intermediate of each side
    double* work;            // general route, open and walk: `wstride` doubles per workgroup — O x_k in [0, tsz), the intermediate behind it
    long long wstride, tsz;
    double* out;             // device, interleaved
    long long ob, ot, ok;    // k_zmeasure_open: table t < nemit writes element out[b ob + t ot + k ok]
    int nemit;
    int normalize;           // divide by re <x|x> (a zero train: IEEE 0 / 0)
    int o1[2], o2[2];        // k_zmeasure_walk, per pass: the table that opens at j, the table whose V it meets
    int mirror;              // P and Q are the same table: the one pass writes both triangles
    int skip_fit;            // general kernels: leave the trains of the on-chip class alone (the on-chip kernel of this call took them)
};

__device__ __forceinline__ double zm_wave_sum(double p) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) p += __shfl_down(p, s, 64);
    return p;
}

// The 16 wave sums of (pr, pi) in a fixed order through `row` (2 * TTN_NWAVES LDS doubles); the result is valid in thread 0.  One
// barrier; the caller alternates two rows so that the next reduction does not overwrite what thread 0 still reads.
__device__ __forceinline__ void zm_reduce(double pr, double pi, lds_f64* row, double& sr, double& si) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    pr = zm_wave_sum(pr);
    pi = zm_wave_sum(pi);
    if (lane == 0) { row[2 * wave] = pr; row[2 * wave + 1] = pi; }
    __syncthreads();
    sr = 0.0; si = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < TTN_NWAVES; ++w) { sr += row[2 * w]; si += row[2 * w + 1]; }
}

// Does every rank of the train fit the on-chip route?  The same answer in every thread, through one LDS word (`flag`, free again on return).
__device__ __forceinline__ bool zm_train_fits(const long long* rk, int d, lds_i32* flag) {
    if (threadIdx.x == 0) *flag = 1;
    __syncthreads();
    for (int k = threadIdx.x; k <= d; k += TTN_WG)
        if (rk[k] > ZMEASURE_RMAX) *flag = 0;
    __syncthreads();
    const bool fit = *flag != 0;
    __syncthreads();
    return fit;
}

// ---------------------------------------------------------------------------------------------
// the on-chip route
// ---------------------------------------------------------------------------------------------
// One site.  rin: the rank of the incoming state (LR: the left rank of the core, else the right one), rout: the other one.
//   LR    Mout[a, b]   = sum_{z, z', al, be} conj(Xk[z, al, a]) Min[al, be] O[z, z'] Xk[z', be, b]
//   else  Mout[al, be] = sum_{z, z', a, b}   conj(Xk[z, al, a]) Min[a, b]   O[z, z'] Xk[z', be, b]
//   Min, Mout: states in workspace (two planes of ZM_IMG doubles), Mout != Min; Min is zero outside rin x rin, Mout is written whole
//   Ok : the 2 x 2 complex table as it lies, (z, z') at 2 (z + 2 z'); TAB = false: the identity, Ok is not read
//   img: two LDS images (re, im), all zero on entry and on exit
// The structure is braket_site<true, true, 1>'s: wave w owns tile (tr = w & 3, tc = w >> 2) of U_z' = Min (Xk as ket)[z'], re and im;
// V_z = sum_z' O[z, z'] U_z' on the accumulators; the accumulator layout of V_z is the B-operand layout of the second product.
template <bool LR, bool TAB>
__device__ __forceinline__ void zm_site(const double* Xk, const double* Ok, const double* Min, double* Mout, int rin, int rout, lds_f64* img) {
    const int wave = uni32((int)threadIdx.x >> 6);
    const int tr = wave & 3, tc = wave >> 2;
    const bool active = 16 * tr < rin && 16 * tc < rout;                 // wave-uniform
    mfma_acc_t ur[2], ui[2];
    ur[0] = BK_ZERO; ur[1] = BK_ZERO; ui[0] = BK_ZERO; ui[1] = BK_ZERO;
    lds_f64* imr = img;
    lds_f64* imi = img + DOT_MS_DOUBLES;
    if (active) {
        // ---- first product: U_z'[p, q] = sum_s Min[p, s] Xk[z', (s, q)]: rows p = 16 tr + ., columns q = 16 tc + . ----
        int te = threadIdx.x;
        asm volatile("" : "+v"(te));
        const int li = te & 15, lk = (te >> 4) & 3;
        const int nt = (rin + 3) >> 2;
        const int bq = 16 * tc + li;
        gmem_f64* mrow = (gmem_f64*)Min + (16 * tr + li) + 64 * lk;      // Min[p, s = 4 t + lk]: + 256 t (+ ZM_IMG: im)
        for (int t = 0; t < nt; ++t) {
            const bk_frag y = LR ? bk_load<true>(Xk, 4 * t + lk, bq, rin, rout, rin) : bk_load<true>(Xk, bq, 4 * t + lk, rout, rin, rout);
            const double mr = mrow[256 * t], mi = mrow[256 * t + ZM_IMG];
            ur[0] = BK_MFMA(mr, y.re0, ur[0]);
            ur[1] = BK_MFMA(mr, y.re1, ur[1]);
            ui[0] = BK_MFMA(mi, y.re0, ui[0]);
            ui[1] = BK_MFMA(mi, y.re1, ui[1]);
            ur[0] = BK_MFMA_NEGA(mi, y.im0, ur[0]);
            ur[1] = BK_MFMA_NEGA(mi, y.im1, ur[1]);
            ui[0] = BK_MFMA(mr, y.im0, ui[0]);
            ui[1] = BK_MFMA(mr, y.im1, ui[1]);
        }
        const int nta = (rout + 15) >> 4;
        // One z at a time, as in braket_site: V_0 and V_1 together would stand next to U's four tiles.
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            mfma_acc_t vr, vi;
            if (TAB) {
                const double r0 = Ok[2 * i], i0 = Ok[2 * i + 1], r1 = Ok[2 * i + 4], i1 = Ok[2 * i + 5];      // O[i, 0], O[i, 1]
                vr = BK_ZERO; vi = BK_ZERO;
                vr += r0 * ur[0]; vr -= i0 * ui[0]; vr += r1 * ur[1]; vr -= i1 * ui[1];
                vi += r0 * ui[0]; vi += i0 * ur[0]; vi += r1 * ui[1]; vi += i1 * ur[1];
            } else {
                vr = ur[i]; vi = ui[i];
            }
            // ---- second product, partial over this wave's block of the summed index: sum_r conj(Xk[i, ...]) V_i[16 tr + 4 r + lk, .] ----
            //      re: x.re V.re + x.im V.im      im: x.re V.im - x.im V.re
#pragma unroll
            for (int ta = 0; ta < 4; ++ta) {
                if (ta < nta) {                                           // wave-uniform
                    const int aq = 16 * ta + li;
                    mfma_acc_t pr = BK_ZERO, pi = BK_ZERO;
                    bk_elem x[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        x[r] = LR ? bk_load1<true>(Xk, i, 16 * tr + 4 * r + lk, aq, rin, rout, rin) : bk_load1<true>(Xk, i, aq, 16 * tr + 4 * r + lk, rout, rin, rout);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        pr = BK_MFMA(x[r].re, vr[r], pr);
                        pi = BK_MFMA(x[r].re, vi[r], pi);
                        pr = BK_MFMA(x[r].im, vi[r], pr);
                        pi = BK_MFMA_NEGA(x[r].im, vr[r], pi);
                    }
                    // Mout[16 ta + lk + 4 reg, 16 tc + li] += p[reg]   (entries beyond rout x rout are exact zeros)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int at = DOT_AT(16 * tc + li, 16 * ta + lk + 4 * reg);
                        __hip_atomic_fetch_add(imr + at, pr[reg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_add(imi + at, pi[reg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
        }
    }
    dot_lds_barrier();                                                    // the images are complete
    {
        gmem_wf64* dst = (gmem_wf64*)Mout;
        int te = threadIdx.x;
        asm volatile("" : "+v"(te));
        for (int e = te; e < ZM_IMG; e += TTN_WG) {
            const int at = DOT_AT(e >> 6, e & 63);
            dst[e] = imr[at];
            dst[e + ZM_IMG] = imi[at];
            imr[at] = 0.0;
            imi[at] = 0.0;
        }
    }
    __syncthreads();                                                      // the state is in memory and the images are zero again
}

// sum over the r x r entries of two on-chip states of V T (complex, no conjugate): this thread's share
__device__ __forceinline__ void zm_frob_chip(const double* V, const double* T, int r, double& pr, double& pi) {
    pr = 0.0; pi = 0.0;
#pragma unroll
    for (int u = 0; u < ZM_IMG / TTN_WG; ++u) {
        const int e = threadIdx.x + TTN_WG * u;
        if ((e & 63) < r && (e >> 6) < r) {
            const double vr = V[e], vi = V[e + ZM_IMG], tr = T[e], ti = T[e + ZM_IMG];
            pr = fma(vr, tr, pr); pr = fma(-vi, ti, pr);
            pi = fma(vr, ti, pi); pi = fma(vi, tr, pi);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the general route
// ---------------------------------------------------------------------------------------------
// OX[z, f] = sum_z' O[z, z'] X[z', f] over the `fibres` = r_left r_right fibres of a core, complex
__device__ __forceinline__ void zm_transform(double* OX, const double* X, const double* O, int n, int fibres) {
    for (int f = threadIdx.x; f < fibres; f += TTN_WG) {
        const double* xf = X + 2 * (long long)n * f;
        for (int z = 0; z < n; ++z) {
            double ar = 0.0, ai = 0.0;
            for (int zz = 0; zz < n; ++zz) {
                const double orr = O[2 * (z + n * zz)], oi = O[2 * (z + n * zz) + 1], xr = xf[2 * zz], xi = xf[2 * zz + 1];
                ar = fma(orr, xr, ar); ar = fma(-oi, xi, ar);
                ai = fma(orr, xi, ai); ai = fma(oi, xr, ai);
            }
            OX[2 * ((long long)n * f + z)] = ar;
            OX[2 * ((long long)n * f + z) + 1] = ai;
        }
    }
}

// One site on interleaved column-major states: Xk the bra core (conjugated), Bk the ket core (Xk, or O Xk); rl, rr the ranks of the core.
//   LR    Sin  = L, rl x rl;  T[al, (z, b)]  = sum_be L[al, be] Bk[z, be, b] at z + n al + n rl b;  Sout[a, b]   = sum_{(z, al)} conj(Xk[z, al, a]) T[(z, al), b]
//   else  Sin  = G, rr x rr;  T[a, (z, be)]  = sum_b  G[a, b]  Bk[z, be, b]  at z + n a + n rr be;  Sout[al, be] = sum_{(z, a)}  conj(Xk[z, al, a]) T[(z, a), be]
template <bool LR>
__device__ __noinline__ void zm_site_generic(double* Xk, double* Bk, double* Sin, double* Sout, double* Tb, int n, int rl, int rr, double* lds) {
    Xk = unip(Xk); Bk = unip(Bk); Sin = unip(Sin); Sout = unip(Sout); Tb = unip(Tb); lds = unip(lds);
    n = uni32(n); rl = uni32(rl); rr = uni32(rr);
    if (LR) {
        braket_gemm(rl, n * rr, rl, Sin, plain(1), plain(rl), 2, false, Bk, plain(n), Idx{n, 1, (long long)n * rl}, 2, Tb, plain(n),
                    Idx{n, 1, (long long)n * rl}, lds);
        braket_gemm(rr, rr, n * rl, Xk, plain((long long)n * rl), plain(1), 2, true, Tb, plain(1), plain((long long)n * rl), 2, Sout, plain(1), plain(rr), lds);
    } else {
        braket_gemm(rr, n * rl, rr, Sin, plain(1), plain(rr), 2, false, Bk, plain((long long)n * rl), plain(1), 2, Tb, plain(n),
                    Idx{n, 1, (long long)n * rr}, lds);
        braket_gemm(rl, rl, n * rr, Xk, plain(n), Idx{n, 1, (long long)n * rl}, 2, true, Tb, plain(1), plain((long long)n * rr), 2, Sout, plain(1), plain(rl), lds);
    }
}

__device__ __forceinline__ void zm_frob_generic(const double* V, const double* T, int r, double& pr, double& pi) {
    pr = 0.0; pi = 0.0;
    for (int e = threadIdx.x; e < r * r; e += TTN_WG) {
        const double vr = V[2 * e], vi = V[2 * e + 1], tr = T[2 * e], ti = T[2 * e + 1];
        pr = fma(vr, tr, pr); pr = fma(-vi, ti, pr);
        pi = fma(vr, ti, pi); pi = fma(vi, tr, pi);
    }
}

// ---------------------------------------------------------------------------------------------
// phase 0: block (b, side) — side 0 the L chain, side 1 the G chain
// ---------------------------------------------------------------------------------------------
template <bool CHIP>
__global__ void __launch_bounds__(TTN_WG) k_zmeasure_chain(ZMeasureArgs P) {
    extern __shared__ double lds[];
    const int d = P.x.d, tid = threadIdx.x;
    const int b = blockIdx.x, side = blockIdx.y;
    const long long* rk = P.x.rks + (long long)b * (d + 1);
    const bool fit = zm_train_fits(rk, d, (lds_i32*)((lds_f64*)lds + ZM_WORK_DOUBLES));
    if (CHIP ? !fit : (P.skip_fit && fit)) return;                       // block-uniform
    lds_i32* tab = (lds_i32*)((lds_f64*)lds + ZM_WORK_DOUBLES + ZM_RED_DOUBLES);
    for (int k = tid; k <= d; k += TTN_WG) {
        tab[ZM_TAB * k + 0] = (int)rk[k];
        tab[ZM_TAB * k + 1] = k < d ? (int)P.x.off[k] : 0;               // a train is far below 2^31 doubles (checked by the host)
    }
    __syncthreads();
    double* Xb = P.x.data + (long long)b * P.x.stride;
    double* E = P.env + ((long long)b * 2 + side) * (d + 1) * P.W;       // this side's states, bond 0 .. d
    double* first = E + (side ? (long long)d * P.W : 0);
    if constexpr (CHIP) {
        lds_f64* img = (lds_f64*)lds;
        for (int e = tid; e < 2 * DOT_MS_DOUBLES; e += TTN_WG) img[e] = 0.0;
        for (int e = tid; e < ZM_STATE; e += TTN_WG) first[e] = e == 0 ? 1.0 : 0.0;
        __syncthreads();
        if (side == 0) {
            for (int k = 0; k < d; ++k)
                zm_site<true, false>(unip(Xb + uni32(tab[ZM_TAB * k + 1])), nullptr, E + (long long)k * P.W, E + (long long)(k + 1) * P.W,
                                     uni32(tab[ZM_TAB * k]), uni32(tab[ZM_TAB * (k + 1)]), img);
        } else {
            for (int k = d - 1; k >= 0; --k)
                zm_site<false, false>(unip(Xb + uni32(tab[ZM_TAB * k + 1])), nullptr, E + (long long)(k + 1) * P.W, E + (long long)k * P.W,
                                      uni32(tab[ZM_TAB * (k + 1)]), uni32(tab[ZM_TAB * k]), img);
        }
    } else {
        double* Tb = P.ctb + ((long long)b * 2 + side) * P.tsz;
        if (tid == 0) { first[0] = 1.0; first[1] = 0.0; }
        __syncthreads();
        if (side == 0) {
            for (int k = 0; k < d; ++k) {
                double* Xk = Xb + uni32(tab[ZM_TAB * k + 1]);
                zm_site_generic<true>(Xk, Xk, E + (long long)k * P.W, E + (long long)(k + 1) * P.W, Tb, P.x.dims[k] >> 1, uni32(tab[ZM_TAB * k]),
                                      uni32(tab[ZM_TAB * (k + 1)]), lds);
                __syncthreads();
            }
        } else {
            for (int k = d - 1; k >= 0; --k) {
                double* Xk = Xb + uni32(tab[ZM_TAB * k + 1]);
                zm_site_generic<false>(Xk, Xk, E + (long long)(k + 1) * P.W, E + (long long)k * P.W, Tb, P.x.dims[k] >> 1, uni32(tab[ZM_TAB * k]),
                                       uni32(tab[ZM_TAB * (k + 1)]), lds);
                __syncthreads();
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// phase 1: block (k + d t, b) — V^O_k of table t and its product with G_{k+1}
// ---------------------------------------------------------------------------------------------
template <bool CHIP>
__global__ void __launch_bounds__(TTN_WG) k_zmeasure_open(ZMeasureArgs P) {
    extern __shared__ double lds[];
    const int d = P.x.d, tid = threadIdx.x;
    const int k = blockIdx.x % d, t = blockIdx.x / d, b = blockIdx.y;
    const long long* rk = P.x.rks + (long long)b * (d + 1);
    const bool fit = zm_train_fits(rk, d, (lds_i32*)((lds_f64*)lds + ZM_WORK_DOUBLES));
    if (CHIP ? !fit : (P.skip_fit && fit)) return;                       // block-uniform
    const int r = uni32((int)rk[k]), r2 = uni32((int)rk[k + 1]);
    double* Xk = P.x.data + (long long)b * P.x.stride + P.x.off[k];
    const double* Ok = P.tabs + 2 * ((long long)t * P.S + P.toff[k]);
    const double* E = P.env + (long long)b * 2 * (d + 1) * P.W;
    const double* L = E + (long long)k * P.W;                             // L on bond k, r x r
    const double* G = E + (long long)(d + 1 + k + 1) * P.W;               // G on bond k + 1, r2 x r2
    double* Vk = P.V + (((long long)b * P.ntab + t) * d + k) * P.W;
    lds_f64* red = (lds_f64*)lds + ZM_WORK_DOUBLES;
    double pr, pi;
    if constexpr (CHIP) {
        lds_f64* img = (lds_f64*)lds;
        for (int e = tid; e < 2 * DOT_MS_DOUBLES; e += TTN_WG) img[e] = 0.0;
        __syncthreads();
        zm_site<true, true>(unip(Xk), unip(Ok), unip(L), unip(Vk), r, r2, img);
        zm_frob_chip(Vk, G, r2, pr, pi);
    } else {
        const int n = uni32(P.x.dims[k] >> 1);                            // a complex train keeps 2 n_k in its table
        double* OX = P.work + ((long long)b * gridDim.x + blockIdx.x) * P.wstride;
        double* Tb = OX + P.tsz;
        zm_transform(OX, Xk, Ok, n, r * r2);
        __syncthreads();
        zm_site_generic<true>(Xk, OX, const_cast<double*>(L), Vk, Tb, n, r, r2, lds);
        __syncthreads();
        zm_frob_generic(Vk, G, r2, pr, pi);
    }
    if (t >= P.nemit) return;                                             // block-uniform
    double sr, si;
    zm_reduce(pr, pi, red, sr, si);
    if (tid == 0) {
        if (P.normalize) { const double nn = E[(long long)d * P.W]; sr /= nn; si /= nn; }      // re <x|x> = re L[bond d][1, 1]: the first double in both layouts
        double* o = P.out + 2 * ((long long)b * P.ob + (long long)t * P.ot + (long long)k * P.ok);
        o[0] = sr; o[1] = si;
    }
}

// ---------------------------------------------------------------------------------------------
// phase 2: block (d - 1 - j, b, pass) — the walk that opens at site j (0-based, j = d - 1 first: the longest walk) and ends at site 1
// ---------------------------------------------------------------------------------------------
template <bool CHIP>
__global__ void __launch_bounds__(TTN_WG) k_zmeasure_walk(ZMeasureArgs P) {
    extern __shared__ double lds[];
    const int d = P.x.d, tid = threadIdx.x;
    const int j = d - 1 - (int)blockIdx.x, b = blockIdx.y, pass = blockIdx.z;
    const long long* rk = P.x.rks + (long long)b * (d + 1);
    const bool fit = zm_train_fits(rk, d, (lds_i32*)((lds_f64*)lds + ZM_WORK_DOUBLES));
    if (CHIP ? !fit : (P.skip_fit && fit)) return;                       // block-uniform
    lds_f64* red = (lds_f64*)lds + ZM_WORK_DOUBLES;
    lds_i32* tab = (lds_i32*)(red + ZM_RED_DOUBLES);
    for (int k = tid; k <= d; k += TTN_WG) {
        tab[ZM_TAB * k + 0] = (int)rk[k];
        tab[ZM_TAB * k + 1] = k < d ? (int)P.x.off[k] : 0;
    }
    __syncthreads();
    double* Xb = P.x.data + (long long)b * P.x.stride;
    const double* E = P.env + (long long)b * 2 * (d + 1) * P.W;
    const double* V2 = P.V + ((long long)b * P.ntab + P.o2[pass]) * d * P.W;
    const double* O1 = P.tabs + 2 * ((long long)P.o1[pass] * P.S + P.toff[j]);
    const long long wg = ((long long)b * gridDim.z + pass) * gridDim.x + blockIdx.x;
    double* St = P.St + wg * 2 * P.W;
    double* Cb = P.out + 2 * (long long)b * d * d;
    const double nrm = P.normalize ? E[(long long)d * P.W] : 1.0;
    const double* Sin = E + (long long)(d + 1 + j + 1) * P.W;            // G on bond j + 1
    if constexpr (CHIP) {
        lds_f64* img = (lds_f64*)lds;
        for (int e = tid; e < 2 * DOT_MS_DOUBLES; e += TTN_WG) img[e] = 0.0;
        __syncthreads();
    }
    int step = 0;
    for (int i = j; i >= 1; --i, ++step) {
        const int rr = uni32(tab[ZM_TAB * (i + 1)]), rl = uni32(tab[ZM_TAB * i]);      // the incoming state is rr x rr, the outgoing one rl x rl
        double* Xi = Xb + uni32(tab[ZM_TAB * i + 1]);
        const double* Vi = V2 + (long long)(i - 1) * P.W;                 // V^{O2}_{i-1}, rl x rl
        double* Sout = St + (long long)(step & 1) * P.W;
        double pr, pi;
        if constexpr (CHIP) {
            lds_f64* img = (lds_f64*)lds;
            if (i == j) zm_site<false, true>(unip(Xi), unip(O1), unip(Sin), unip(Sout), rr, rl, img);
            else zm_site<false, false>(unip(Xi), nullptr, unip(Sin), unip(Sout), rr, rl, img);
            zm_frob_chip(Vi, Sout, rl, pr, pi);
        } else {
            const int n = uni32(P.x.dims[i] >> 1);
            double* OX = P.work + wg * P.wstride;
            double* Tb = OX + P.tsz;
            double* Bk = Xi;
            if (i == j) {
                zm_transform(OX, Xi, O1, n, rl * rr);
                __syncthreads();
                Bk = OX;
            }
            zm_site_generic<false>(Xi, Bk, const_cast<double*>(Sin), Sout, Tb, n, rl, rr, lds);
            __syncthreads();
            zm_frob_generic(Vi, Sout, rl, pr, pi);
        }
        double sr, si;
        zm_reduce(pr, pi, red + (step & 1) * 2 * TTN_NWAVES, sr, si);
        if (tid == 0) {
            sr /= nrm; si /= nrm;
            const int io = i - 1;                                         // this step met V of site i - 1
            double* up = Cb + 2 * (io + (long long)d * j);
            double* lo = Cb + 2 * (j + (long long)d * io);
            if (pass == 0) { up[0] = sr; up[1] = si; } else { lo[0] = sr; lo[1] = si; }
            if (P.mirror) { lo[0] = sr; lo[1] = si; }
        }
        Sin = Sout;
    }
}
