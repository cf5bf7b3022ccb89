// ttn_grad_kernels.h — reverse-mode rules of dot(A, B) and H * psi (ext/TensorTrainNumericsChainRulesCoreExt of the reference), and the
// core-wise linear algebra of tangents.  Float64 only.
//
//   environments (ChainRulesCoreExt.jl:8-34), r^A x r^B, column-major [al + r^A be]:
//       L_1 = [1],      L_{k+1}[a, b]  = sum_{z, al, be} A_k[z, al, a] B_k[z, be, b] L_k[al, be]
//       G_{N+1} = [1],  G_k[al, be]    = sum_{z, a, b}   A_k[z, al, a] B_k[z, be, b] G_{k+1}[a, b]
//   pullback of dot (:36-65):    Abar_k[z, al, a] = Delta sum_{be, b} L_k[al, be] B_k[z, be, b] G_{k+1}[a, b]     (Bbar_k: A and B exchanged)
//   pullback of H * psi (:67-88): psibar_k[j, vl, vr] = sum_{i, al, ar} H_k[i, j, al, ar] Ybar_k[i, al + Rl vl, ar + Rr vr]
//
// k_grad_chain      both chains of a train, each ONCE, every state kept: grid (batch, 2) — block (t, 0) walks L left to right, block
//                   (t, 1) walks G right to left.  A site of the k_dot_fused class (n = 2, its four ranks <= 64) runs with the state in
//                   LDS — G on dot_site itself, L on its left-to-right twin grad_site_lr — and copies the finished image to its slot;
//                   any other site runs two workgroup GEMMs on the slots (dot_site_generic / grad_site_generic_rl).  The state moves
//                   into LDS whenever a site of the class follows one outside it, so (psi, H psi) — ramp sites inside, the body
//                   outside — is one launch.
//                   Workspace per train: 2 (d + 1) W + 2 nmax ramax rbmax doubles, W = max_m r^A_m r^B_m (rounded up to even).
// k_grad_sandwich   with both chains stored the 2 N outputs of a train are independent: grid (tiles, 2 N, batch).  An output
//                   O[z, p, q] = Delta sum_{s, t} E1[p, s] C[z, s, t] E2[q, t] is two chained products; a block owns 16 rows p and 64
//                   columns q, forms U[p, t] = sum_s E1[p, s] C[z, s, t] in chunks of 256 t in LDS (never in HBM) and folds each chunk into
//                   its accumulators, both on v_mfma_f64_16x16x4_f64.  Sites whose four ranks all stay below 16 (rank ramps, rank-1
//                   ends) take a plain vector path: one thread per output entry.
// k_apply_pullback  the transpose of k_apply, HBM bound: reads Ybar once (Rl Rr times the output), one thread per output row vl and
//                   TTN_APB_K columns vr, operator core in LDS.
// k_cores_axpby / k_cores_dot   one pass over the arena with the trains' current ranks; the dot reduces per train in a fixed order.
#pragma once
#include "ttn_common.h"
#include "ttn_wg_gemm.h"
#include "ttn_dot_kernels.h"
#include "ttn_stream_kernels.h"

struct GradChainArgs {
    TTDev a, b;
    double* env;            // [batch][2][d + 1][W]: L_1 .. L_{N+1}, then G_1 .. G_{N+1}
    double* tbuf;           // [batch][2][tsz]: the intermediate of the GEMM sites
    long long W, tsz;
    double* out;            // [batch]: L_{N+1}[1, 1] = dot(a_b, b_b), or null
};

// A site outside the LDS-resident class, RIGHT TO LEFT: T[a, (z, be)] = sum_b G[a, b] B_k[z, be, b], G'[al, be] = sum_{z, a} A_k[z, al, a] T
__device__ __noinline__ void grad_site_generic_rl(double* Ak, double* Bk, double* Gc, double* Gn, double* Tb, int n, int ra, int ra2, int rb, int rb2,
                                                  double* lds) {
    Ak = unip(Ak); Bk = unip(Bk); Gc = unip(Gc); Gn = unip(Gn); Tb = unip(Tb); lds = unip(lds);
    n = uni32(n); ra = uni32(ra); ra2 = uni32(ra2); rb = uni32(rb); rb2 = uni32(rb2);
    const View Gv = mkview(Gc, plain(1), plain(ra));
    const View Bv = mkview(Bk, plain((long long)n * rb2), plain(1));                  // B as [b, (z + n be)]
    const View Tv = mkview(Tb, plain(n), Idx{n, 1, (long long)n * ra});               // T as [a, (z + n be)] stored at z + n a + n ra be
    wg_gemm(ra, n * rb2, rb, Gv, Bv, Tv, 1.0, 0.0, lds);
    const View Av = mkview(Ak, plain(n), Idx{n, 1, (long long)n * ra2});              // A as [al, (z + n a)]
    const View T2v = mkview(Tb, plain(1), plain((long long)n * ra));                  // T as [(z + n a), be]
    const View Gnv = mkview(Gn, plain(1), plain(ra2));
    wg_gemm(ra2, rb2, n * ra, Av, T2v, Gnv, 1.0, 0.0, lds);
}

// A site of the LDS-resident class, LEFT TO RIGHT (the L chain): dot_site of ttn_dot_kernels.h with the roles of the two rank indices of
// a core exchanged — the fragment rows walk the RIGHT index (stride r_left), the k-steps the left one.
//   T_z[al, b]  = sum_be L[al, be] B_k[z, be, b]          (tile rows al = 16 tr + ., columns b = 16 tc + .)
//   L'[a, b]   += sum_{z, al in block tr} A_k[z, al, a] T_z[al, b]      (the accumulator register r of T_z is the B fragment of k-step r)
//   ra, rb: LEFT ranks (the incoming state L[al, be] at Mcur[DOT_AT(be, al)]); ra2, rb2: RIGHT ranks (L'[a, b] into Mnxt, all zero on entry)
// Every lane loads 16 bytes 2 r_left doubles apart from its neighbour: this is the form section 4.3 of DESIGN.md found bound by the
// line-request rate of the vector L1 (34 k clk per rank-64 site against 22 k right to left) — and still ahead of the GEMM route.
__device__ __noinline__ void grad_site_lr(const double* Ak, const double* Bk, int ra, int ra2, int rb, int rb2, const lds_f64* Mcur, lds_f64* Mnxt,
                                          lds_f64* Mzero) {
    Ak = unip(Ak); Bk = unip(Bk); ra = uni32(ra); ra2 = uni32(ra2); rb = uni32(rb); rb2 = uni32(rb2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int tr = wave & 3, tc = wave >> 2;
    {
        typedef __attribute__((address_space(3))) dot_f64x2 lds_f64x2;
        lds_f64x2* z2 = (lds_f64x2*)Mzero;
        const dot_f64x2 zero2 = {0.0, 0.0};
        for (int e = threadIdx.x; e < DOT_MS_DOUBLES / 2; e += TTN_WG) z2[e] = zero2;
    }
    if (16 * tr < ra && 16 * tc < rb2) {                                  // wave-uniform
        mfma_acc_t t0 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0}, t1 = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
        const int bq = 16 * tc + li;
        const int nt = (rb + 3) >> 2;                                     // k-steps of four be
        for (int t = 0; t < nt; ++t) {
            const dot_f64x2 bv = dot_load2(Bk, 4 * t + lk, bq, rb, rb2, rb);              // B_k[., be = 4 t + lk, b = bq]
            const double a = Mcur[DOT_AT(4 * t + lk, 16 * tr + li)];
            t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv.x, t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv.y, t1, 0, 0, 0);
        }
        const int nr = min(4, (ra - 16 * tr + 3) >> 2);                   // k-steps of this block that hold rows al < ra
        const int nta = (ra2 + 15) >> 4;
#pragma unroll
        for (int ta = 0; ta < 4; ++ta) {
            if (ta < nta) {                                               // wave-uniform
                mfma_acc_t m = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
                const int aq = 16 * ta + li;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r < nr) {
                        const dot_f64x2 av = dot_load2(Ak, 16 * tr + 4 * r + lk, aq, ra, ra2, ra);      // A_k[., al = 16 tr + 4 r + lk, a = aq]
                        m = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, t0[r], m, 0, 0, 0);
                        m = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, t1[r], m, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)                        // L'[a = 16 ta + lk + 4 reg, b = 16 tc + li]
                    __hip_atomic_fetch_add(Mnxt + DOT_AT(16 * tc + li, 16 * ta + lk + 4 * reg), m[reg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    dot_lds_barrier();
}

// Block (t, 0): L_1 .. L_{N+1} left to right; block (t, 1): G_{N+1} .. G_1 right to left.  "in" / "out" below: the state a site reads
// and the one it produces — slots k, k + 1 for L and k + 1, k for G.
__global__ void __launch_bounds__(TTN_WG) k_grad_chain(GradChainArgs P) {
    extern __shared__ double lds[];
    const int dir = blockIdx.y, t = blockIdx.x;
    const int tid = threadIdx.x;
    const TTDev& A = P.a; const TTDev& B = P.b;
    const int d = A.d;
    lds_f64* img = (lds_f64*)lds;
    lds_i32* tab = (lds_i32*)((lds_f64*)lds + DOT_LDS_DOUBLES);           // the per-site table of k_dot_fused
    for (int k = tid; k <= d; k += TTN_WG) {
        tab[6 * k + 0] = (int)A.rks[(long long)t * (d + 1) + k];
        tab[6 * k + 1] = (int)B.rks[(long long)t * (d + 1) + k];
        tab[6 * k + 2] = k < d ? A.dims[k] : 0;
        tab[6 * k + 3] = k < d ? (int)A.off[k] : 0;
        tab[6 * k + 4] = k < d ? (int)B.off[k] : 0;
    }
    __syncthreads();
    double* Abase = A.data + (long long)t * A.stride;
    double* Bbase = B.data + (long long)t * B.stride;
    double* E = P.env + ((long long)t * 2 + dir) * (d + 1) * P.W;
    double* Tb = P.tbuf + ((long long)t * 2 + dir) * P.tsz;
    {
        // both chains start from e_1 e_1^T (the 1 x 1 matrix [1] in every train the reference builds)
        const int m0 = dir ? d : 0;
        const int r0a = uni32(tab[6 * m0]), r0b = uni32(tab[6 * m0 + 1]);
        double* E0 = E + (long long)m0 * P.W;
        for (int e = tid; e < r0a * r0b; e += TTN_WG) E0[e] = (e == 0) ? 1.0 : 0.0;
        __syncthreads();
    }
    bool in_lds = false;
    int cur = 0;                                                          // image that holds the incoming state while in_lds
    for (int i = 0; i < d; ++i) {
        const int k = dir ? d - 1 - i : i;
        const int kin = dir ? k + 1 : k, kout = dir ? k : k + 1;
        const int n = uni32(tab[6 * k + 2]);
        const int ra = uni32(tab[6 * kin]), rb = uni32(tab[6 * kin + 1]);               // the incoming state
        const int ra2 = uni32(tab[6 * kout]), rb2 = uni32(tab[6 * kout + 1]);           // the outgoing state
        double* Ak = Abase + uni32(tab[6 * k + 3]);
        double* Bk = Bbase + uni32(tab[6 * k + 4]);
        double* Ein = E + (long long)kin * P.W;
        double* Eout = E + (long long)kout * P.W;
        const bool fit = n == 2 && ra <= DOT_RMAX && rb <= DOT_RMAX && ra2 <= DOT_RMAX && rb2 <= DOT_RMAX;
        if (!fit) {
            if (dir) grad_site_generic_rl(Ak, Bk, Ein, Eout, Tb, n, ra, ra2, rb, rb2, lds);
            else dot_site_generic(Ak, Bk, Ein, Eout, Tb, n, ra, ra2, rb, rb2, lds);
            in_lds = false;
            continue;
        }
        if (!in_lds) {                                                    // the state enters LDS: two clean images, the incoming state in the first
            __syncthreads();
            for (int e = tid; e < 2 * DOT_MS_DOUBLES; e += TTN_WG) img[e] = 0.0;
            __syncthreads();
            for (int e = tid; e < ra * rb; e += TTN_WG) img[DOT_AT(e / ra, e % ra)] = Ein[e];
            __syncthreads();
            cur = 0;
            in_lds = true;
        }
        const int nx = cur == 2 ? 0 : cur + 1, sp = nx == 2 ? 0 : nx + 1;
        if (!dir)
            grad_site_lr(Ak, Bk, ra, ra2, rb, rb2, img + cur * DOT_MS_DOUBLES, img + nx * DOT_MS_DOUBLES, img + sp * DOT_MS_DOUBLES);
        else if (ra == DOT_RMAX && ra2 == DOT_RMAX && rb == DOT_RMAX && rb2 == DOT_RMAX)
            dot_site<true>(Ak, Bk, ra, ra2, rb, rb2, img + cur * DOT_MS_DOUBLES, img + nx * DOT_MS_DOUBLES, img + sp * DOT_MS_DOUBLES);
        else
            dot_site_masked(Ak, Bk, ra, ra2, rb, rb2, img + cur * DOT_MS_DOUBLES, img + nx * DOT_MS_DOUBLES, img + sp * DOT_MS_DOUBLES);
        // the finished image to its slot (the next site only reads it)
        const lds_f64* done = img + nx * DOT_MS_DOUBLES;
        for (int e = tid; e < ra2 * rb2; e += TTN_WG) Eout[e] = (double)done[DOT_AT(e / ra2, e % ra2)];
        cur = nx;
    }
    if (dir == 0 && P.out) {
        __syncthreads();
        if (tid == 0) P.out[t] = E[(long long)d * P.W];
    }
}

// ---------------------------------------------------------------------------------------------
// sandwiches
// ---------------------------------------------------------------------------------------------
#define GRAD_SW_TB 256                   // 4 waves: wave w owns columns 16 w .. 16 w + 15 of the block's 64
#define GRAD_SW_JC 256                   // inner columns t of U held in LDS at a time
#define GRAD_SW_UP 17                    // row pitch of U in LDS (doubles): U[p, t] at t * 17 + p

struct GradSandArgs {
    TTDev a, b, abar, bbar;              // abar.data / bbar.data null: that output is not wanted
    const double* env;
    long long W;
    const double* delta;                 // [batch] on the device, or null: 1
};

__global__ void __launch_bounds__(GRAD_SW_TB) k_grad_sandwich(GradSandArgs P) {
    __shared__ double Us[GRAD_SW_JC * GRAD_SW_UP];
    const int k = blockIdx.y >> 1, which = blockIdx.y & 1, t = blockIdx.z;
    const TTDev& dst = which ? P.bbar : P.abar;
    if (!dst.data) return;
    const int d = P.a.d;
    const long long* ar = P.a.rks + (long long)t * (d + 1);
    const long long* br = P.b.rks + (long long)t * (d + 1);
    const int ral = (int)ar[k], rar = (int)ar[k + 1], rbl = (int)br[k], rbr = (int)br[k + 1];
    const int n = P.a.dims[k];
    const double* L = P.env + ((long long)t * 2) * (d + 1) * P.W + (long long)k * P.W;                   // L_k[al + ral be]
    const double* G = P.env + ((long long)t * 2 + 1) * (d + 1) * P.W + (long long)(k + 1) * P.W;         // G_{k+1}[a + rar b]
    // O[z, p, q] = Delta sum_{s, t} E1[p, s] C[z, s, t] E2[q, t]
    //   Abar: p = al, q = a, s = be, t = b, C = B_k;     Bbar: p = be, q = b, s = al, t = a, C = A_k
    const int Pn = which ? rbl : ral, Q = which ? rbr : rar, S = which ? ral : rbl, T = which ? rar : rbr;
    const long long e1p = which ? ral : 1, e1s = which ? 1 : ral, e2q = which ? rar : 1, e2t = which ? 1 : rar;
    const TTDev& src = which ? P.a : P.b;
    const double* C = src.data + (long long)t * src.stride + src.off[k];
    double* O = dst.data + (long long)t * dst.stride + dst.off[k];
    const double dl = P.delta ? P.delta[t] : 1.0;
    const int tid = threadIdx.x;
    const int rmax = max(max(Pn, Q), max(S, T));
    if (rmax < 16) {                                                     // rank ramps and rank-1 ends: one thread per output entry
        if (blockIdx.x != 0) return;
        const int total = n * Pn * Q;
        for (int e = tid; e < total; e += GRAD_SW_TB) {
            const int z = e % n, p = (e / n) % Pn, q = e / (n * Pn);
            double acc = 0.0;
            for (int tt = 0; tt < T; ++tt) {
                double u = 0.0;
                for (int s = 0; s < S; ++s) u = fma(L[p * e1p + s * e1s], C[z + n * (s + S * tt)], u);
                acc = fma(u, G[q * e2q + tt * e2t], acc);
            }
            O[e] = dl * acc;
        }
        return;
    }
    const int rblocks = (Pn + 15) >> 4, cchunks = (Q + 63) >> 6;
    if ((int)blockIdx.x >= rblocks * cchunks) return;
    const int pb = blockIdx.x % rblocks, cc = blockIdx.x / rblocks;
    const int lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int p0 = 16 * pb, q0 = 64 * cc + 16 * w;
    const bool prow = p0 + li < Pn;
    const bool qcol = q0 + li < Q;
    for (int z = 0; z < n; ++z) {
        mfma_acc_t acc = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
        for (int j0 = 0; j0 < T; j0 += GRAD_SW_JC) {
            const int jn = min(GRAD_SW_JC, T - j0), jtiles = (jn + 15) >> 4;
            __syncthreads();                                              // the readers of the previous chunk are done
            // U[p0 + ., j0 + 16 jt + .] = sum_s E1[p, s] C[z, s, t]: the waves share the column tiles of the chunk
            for (int jt = w; jt < jtiles; jt += GRAD_SW_TB / 64) {
                mfma_acc_t u = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
                const int tt = j0 + 16 * jt + li;
                const bool tcol = tt < T;
                for (int s0 = 0; s0 < S; s0 += 4) {
                    const int s = s0 + lk;
                    const double av = (prow && s < S) ? L[(p0 + li) * e1p + s * e1s] : 0.0;
                    const double bv = (tcol && s < S) ? C[z + (long long)n * (s + (long long)S * tt)] : 0.0;
                    u = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, u, 0, 0, 0);
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) Us[(16 * jt + li) * GRAD_SW_UP + lk + 4 * reg] = u[reg];      // U[p = lk + 4 reg, t = 16 jt + li]
            }
            __syncthreads();
            // O[p0 + ., q0 + .] += sum_t U[p, t] E2[q, t] over the chunk (columns beyond T hold exact zeros: masked fragments)
            if (q0 < Q) {                                                 // wave-uniform
                for (int i = 0; i < 4 * jtiles; ++i) {
                    const int tl = 4 * i + lk, tt = j0 + tl;
                    const double av = Us[tl * GRAD_SW_UP + li];
                    const double bv = (qcol && tt < T) ? G[(q0 + li) * e2q + tt * e2t] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                }
            }
        }
        if (qcol) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int p = p0 + lk + 4 * reg;
                if (p < Pn) O[z + (long long)n * (p + (long long)Pn * (q0 + li))] = dl * acc[reg];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Per-train rank checks of the streaming kernels below: every block reads the d + 1 ranks of its train (they are device-resident)
// and the whole train is left alone when they do not fit.  All threads of the block must call it.
// ---------------------------------------------------------------------------------------------
template <class Pred>
__device__ __forceinline__ bool grad_ranks_bad(int d, Pred differ) {
    int bad = 0;
    for (int m = threadIdx.x; m <= d; m += blockDim.x) bad |= differ(m) ? 1 : 0;
    return __syncthreads_or(bad) != 0;
}

// ---------------------------------------------------------------------------------------------
// apply pullback: psibar_k[j, vl, vr] = sum_{i, al, ar} H_k[i, j, al, ar] Ybar_k[i, al + Rl vl, ar + Rr vr].  HBM-read bound: Ybar is
// read once, Rl Rr times the bytes written.  For fixed (ar, vr) the Rl fibres al of an output row are contiguous in Ybar and
// consecutive lanes (vl) continue the run, so a wave reads runs of 64 n Rl doubles.
// ---------------------------------------------------------------------------------------------
#define TTN_APB_K 4                      // output columns vr per thread (n = 2): K loads of a thread in flight together
__global__ void __launch_bounds__(TTN_STREAM_TB) k_apply_pullback(TTODev A, TTDev x, TTDev yb, TTDev xb, int lds_a, int* status) {
    extern __shared__ double apb_smem[];
    const int k = blockIdx.y, b = blockIdx.z, d = x.d;
    const long long* xr = x.rks + (long long)b * (d + 1);
    const long long* yr = yb.rks + (long long)b * (d + 1);
    if (grad_ranks_bad(d, [&](int m) { return yr[m] != A.rks[m] * xr[m]; })) {
        if (threadIdx.x == 0 && blockIdx.x == 0 && k == 0) ttn_set_status(status + b, TTN_ST_RANKS_DIFFER);
        return;
    }
    const int n = x.dims[k];
    const int Rl = (int)A.rks[k], Rr = (int)A.rks[k + 1];
    const int rl = (int)xr[k], rr = (int)xr[k + 1];
    const double* Ak = A.data + A.off[k];
    const int asz = n * n * Rl * Rr;
    const bool in_lds = asz <= lds_a;
    if (in_lds) {
        for (int e = threadIdx.x; e < asz; e += blockDim.x) apb_smem[e] = Ak[e];
        __syncthreads();
    }
    const double* Ap = in_lds ? apb_smem : Ak;
    const double* Yk = yb.data + (long long)b * yb.stride + yb.off[k];
    double* Xk = xb.data + (long long)b * xb.stride + xb.off[k];
    const long long P = (long long)Rl * rl;                               // left rank of Ybar
    if (n == 2) {
        typedef double d2v_t __attribute__((ext_vector_type(2)));
        const unsigned int url = (unsigned int)rl, cgroups = ((unsigned int)rr + TTN_APB_K - 1) / TTN_APB_K, items = url * cgroups;
        for (unsigned int it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
            const int vl = (int)(it % url), c0 = (int)(it / url) * TTN_APB_K;
            d2v_t acc[TTN_APB_K];
#pragma unroll
            for (int j = 0; j < TTN_APB_K; ++j) acc[j] = (d2v_t){0.0, 0.0};
            for (int ar_ = 0; ar_ < Rr; ++ar_) {
                for (int al = 0; al < Rl; ++al) {
                    const double* h = Ap + 4 * (al + Rl * ar_);            // H[i, j, al, ar] at i + 2 j + 4 (al + Rl ar)
                    const double h00 = h[0], h10 = h[1], h01 = h[2], h11 = h[3];
                    d2v_t yv[TTN_APB_K];
#pragma unroll
                    for (int j = 0; j < TTN_APB_K; ++j) {
                        const int vr = min(c0 + j, rr - 1);               // (a column beyond rr re-reads the last one and is not stored)
                        yv[j] = *reinterpret_cast<const d2v_t*>(Yk + 2 * ((long long)al + (long long)Rl * vl + P * ((long long)ar_ + (long long)Rr * vr)));
                    }
#pragma unroll
                    for (int j = 0; j < TTN_APB_K; ++j) {
                        acc[j].x = fma(h10, yv[j].y, fma(h00, yv[j].x, acc[j].x));
                        acc[j].y = fma(h11, yv[j].y, fma(h01, yv[j].x, acc[j].y));
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < TTN_APB_K; ++j)
                if (c0 + j < rr) *reinterpret_cast<d2v_t*>(Xk + 2 * ((long long)vl + (long long)rl * (c0 + j))) = acc[j];
        }
        return;
    }
    const unsigned int total = (unsigned int)n * (unsigned int)rl * (unsigned int)rr;       // one thread per output entry (j, vl, vr)
    for (unsigned int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int j = (int)(e % (unsigned int)n), f = (int)(e / (unsigned int)n), vl = f % rl, vr = f / rl;
        double acc = 0.0;
        for (int ar_ = 0; ar_ < Rr; ++ar_)
            for (int al = 0; al < Rl; ++al) {
                const double* h = Ap + (long long)n * (j + (long long)n * (al + (long long)Rl * ar_));
                const double* y = Yk + (long long)n * ((long long)al + (long long)Rl * vl + P * ((long long)ar_ + (long long)Rr * vr));
                for (int i = 0; i < n; ++i) acc = fma(h[i], y[i], acc);
            }
        Xk[e] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// y_k <- alpha_b x_k + beta_b y_k on every core (x may be y); alpha / beta: device, per train, or null: 1
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TTN_STREAM_TB) k_cores_axpby(TTDev x, TTDev y, const double* alpha, const double* beta, int* status) {
    const int k = blockIdx.y, b = blockIdx.z, d = x.d;
    const long long* xr = x.rks + (long long)b * (d + 1);
    const long long* yr = y.rks + (long long)b * (d + 1);
    if (grad_ranks_bad(d, [&](int m) { return xr[m] != yr[m]; })) {
        if (threadIdx.x == 0 && blockIdx.x == 0 && k == 0) ttn_set_status(status + b, TTN_ST_RANKS_DIFFER);
        return;
    }
    const long long total = (long long)x.dims[k] * xr[k] * xr[k + 1];
    const double* Xk = x.data + (long long)b * x.stride + x.off[k];
    double* Yk = y.data + (long long)b * y.stride + y.off[k];
    const double al = alpha ? alpha[b] : 1.0, be = beta ? beta[b] : 1.0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) Yk[e] = fma(al, Xk[e], be * Yk[e]);
}

// ---------------------------------------------------------------------------------------------
// out[b] = sum_k <x_k, y_k>: one workgroup per train; thread i sums the entries i, i + 1024, ... of core 1, then of core 2, ...; the
// 1024 partial sums are added as a fixed binary tree — the same call gives the same bits.  Ranks that differ: NaN.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TTN_WG) k_cores_dot(TTDev x, TTDev y, double* out) {
    __shared__ double red[TTN_WG];
    const int b = blockIdx.x, d = x.d, tid = threadIdx.x;
    const long long* xr = x.rks + (long long)b * (d + 1);
    const long long* yr = y.rks + (long long)b * (d + 1);
    if (grad_ranks_bad(d, [&](int m) { return xr[m] != yr[m]; })) {
        if (tid == 0) out[b] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    double acc = 0.0;
    for (int k = 0; k < d; ++k) {
        const long long total = (long long)x.dims[k] * xr[k] * xr[k + 1];
        const double* Xk = x.data + (long long)b * x.stride + x.off[k];
        const double* Yk = y.data + (long long)b * y.stride + y.off[k];
        for (long long e = tid; e < total; e += TTN_WG) acc = fma(Xk[e], Yk[e], acc);
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = TTN_WG / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) out[b] = red[0];
}
