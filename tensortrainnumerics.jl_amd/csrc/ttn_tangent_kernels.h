// ttn_tangent_kernels.h — the fixed-rank TT manifold (include/ttn_tangent.h): the orthogonal projection of a train z onto
// the tangent space at x, and the train alpha x + beta xi of a tangent xi.  Float64 only.
//
//   gauges of x (ranks r):   U = orthogonalize(x, d): U_1 .. U_{d-1} left-orthogonal, U_d the centre;   V = orthogonalize(x, 1): V_2 .. V_d
//                            right-orthogonal.  A tangent is a bag of cores dC_1 .. dC_d with x's ranks that stands for
//                            xi = sum_k U_1 .. U_{k-1} dC_k V_{k+1} .. V_d, with U_k^T dC_k = 0 (left unfolding) for k < d.
//   chains, z of ranks rz:   L_1 = [1],      L_{k+1}[a, b] = sum U_k[z, al, a] Z_k[z, be, b] L_k[al, be]        (bra U, left to right)
//                            G_{d+1} = [1],  G_k[al, be]   = sum V_k[z, al, a] Z_k[z, be, b] G_{k+1}[a, b]      (bra V, right to left)
//   components:              dC_k[z, al, a'] = sum_b ( sum_be L_k[al, be] Z_k[z, be, b] - [k < d] sum_a U_k[z, al, a] L_{k+1}[a, b] ) G_{k+1}[a', b]
//                            (the second term is (I - U_k U_k^T) folded into the middle factor: U_k^T (L_k^T Z_k) = L_{k+1}), and
//                            L_{d+1}[1, 1] = <x, z>.
//
// k_tangent_chain     k_grad_chain (ttn_grad_kernels.h) with one bra per direction: grid (batch, 2), block (t, 0) walks L with (U, z), block
//                     (t, 1) walks G with (V, z); every state kept.  The sites are the device functions of ttn_grad_kernels.h /
//                     ttn_dot_kernels.h and their class rule: n = 2 with the four ranks of the site <= 64 keeps the state in LDS, any other
//                     site runs two workgroup GEMMs on the slots.  Workspace per train as there: 2 (d + 1) W + 2 tsz doubles.
// k_tangent_sandwich  k_grad_sandwich's tiling, grid (tiles, d, batch): a block owns 16 rows al and 64 columns a' of dC_k[z, ., .], forms the
//                     middle factor M[al, b] = sum_be L_k Z_k - sum_a U_k L_{k+1} in chunks of 256 b in LDS — the second product runs into
//                     the same accumulators with the sign on the U fragment — and folds each chunk with G_{k+1}; both products on
//                     v_mfma_f64_16x16x4_f64.  Sites whose ranks all stay below 16: one thread per output entry.
// k_tangent_assemble  y = alpha x + beta xi at ranks 2 r, one streaming pass: W_1 = [dC_1, U_1], W_k = [[V_k, 0], [dC_k, U_k]],
//                     W_d = [beta V_d ; beta dC_d + alpha U_d]  (d = 1: alpha U_1 + beta dC_1).  One output row and TTN_TAN_K columns per
//                     thread for n = 2 (k_add's mapping), one fibre per thread otherwise.  Blocks that are copies are copied bit for bit.
// Trains whose U and V (and xi, in the assembly) differ in a rank are left alone and carry TTN_ST_RANKS_DIFFER on the destination.
#pragma once
#include "ttn_common.h"
#include "ttn_wg_gemm.h"
#include "ttn_dot_kernels.h"
#include "ttn_stream_kernels.h"
#include "ttn_grad_kernels.h"

struct TangentChainArgs {
    TTDev u, v, z;
    double* env;            // [batch][2][d + 1][W]: L_1 .. L_{d+1}, then G_1 .. G_{d+1}
    double* tbuf;           // [batch][2][tsz]: the intermediate of the GEMM sites
    long long W, tsz;
    double* out;            // [batch]: L_{d+1}[1, 1] = <x_b, z_b>, or null
};

__global__ void __launch_bounds__(TTN_WG) k_tangent_chain(TangentChainArgs P) {
    extern __shared__ double lds[];
    const int dir = blockIdx.y, t = blockIdx.x;
    const int tid = threadIdx.x;
    const TTDev& A = dir ? P.v : P.u; const TTDev& B = P.z;
    const int d = A.d;
    {
        const long long* ur = P.u.rks + (long long)t * (d + 1);
        const long long* vr = P.v.rks + (long long)t * (d + 1);
        if (grad_ranks_bad(d, [&](int m) { return ur[m] != vr[m]; })) {              // k_tangent_sandwich records the code; the value: NaN
            if (dir == 0 && P.out && tid == 0) P.out[t] = __longlong_as_double(0x7ff8000000000000LL);
            return;
        }
    }
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
// the tangent sandwich
// ---------------------------------------------------------------------------------------------
struct TangentSandArgs {
    TTDev u, v, z, xi;
    const double* env;
    long long W;
    int* status;            // [batch]: xi's
};

__global__ void __launch_bounds__(GRAD_SW_TB) k_tangent_sandwich(TangentSandArgs P) {
    __shared__ double Us[GRAD_SW_JC * GRAD_SW_UP];
    const int k = blockIdx.y, t = blockIdx.z;
    const int d = P.u.d;
    const int tid = threadIdx.x;
    const long long* ur = P.u.rks + (long long)t * (d + 1);
    const long long* vr = P.v.rks + (long long)t * (d + 1);
    const long long* zr = P.z.rks + (long long)t * (d + 1);
    if (grad_ranks_bad(d, [&](int m) { return ur[m] != vr[m]; })) {
        if (tid == 0 && blockIdx.x == 0 && k == 0) ttn_set_status(P.status + t, TTN_ST_RANKS_DIFFER);
        return;
    }
    const int Pn = (int)ur[k], Q = (int)ur[k + 1], S = (int)zr[k], T = (int)zr[k + 1];
    const int n = P.u.dims[k];
    const bool gauge = k < d - 1;                                          // site d is the centre: no projector
    const double* L = P.env + ((long long)t * 2) * (d + 1) * P.W + (long long)k * P.W;                   // L_k[al + Pn be]
    const double* L1 = L + P.W;                                                                            // L_{k+1}[a + Q b]
    const double* G = P.env + ((long long)t * 2 + 1) * (d + 1) * P.W + (long long)(k + 1) * P.W;         // G_{k+1}[a' + Q b]
    const double* C = P.z.data + (long long)t * P.z.stride + P.z.off[k];                                  // Z_k[z, be, b]
    const double* Uk = P.u.data + (long long)t * P.u.stride + P.u.off[k];                                 // U_k[z, al, a]
    double* O = P.xi.data + (long long)t * P.xi.stride + P.xi.off[k];
    const int rmax = max(max(Pn, Q), max(S, T));
    if (rmax < 16) {                                                     // rank ramps and rank-1 ends: one thread per output entry
        if (blockIdx.x != 0) return;
        const int total = n * Pn * Q;
        for (int e = tid; e < total; e += GRAD_SW_TB) {
            const int z = e % n, p = (e / n) % Pn, q = e / (n * Pn);
            double acc = 0.0;
            for (int tt = 0; tt < T; ++tt) {
                double u = 0.0;
                for (int s = 0; s < S; ++s) u = fma(L[p + Pn * s], C[z + n * (s + S * tt)], u);
                if (gauge)
                    for (int a = 0; a < Q; ++a) u = fma(-Uk[z + n * (p + Pn * a)], L1[a + Q * tt], u);
                acc = fma(u, G[q + Q * tt], acc);
            }
            O[e] = acc;
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
            // M[p0 + ., j0 + 16 jt + .] = sum_be L_k[p, be] Z_k[z, be, b] - sum_a U_k[z, p, a] L_{k+1}[a, b]: the waves share the column tiles
            for (int jt = w; jt < jtiles; jt += GRAD_SW_TB / 64) {
                mfma_acc_t u = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
                const int tt = j0 + 16 * jt + li;
                const bool tcol = tt < T;
                for (int s0 = 0; s0 < S; s0 += 4) {
                    const int s = s0 + lk;
                    const double av = (prow && s < S) ? L[(p0 + li) + (long long)Pn * s] : 0.0;
                    const double bv = (tcol && s < S) ? C[z + (long long)n * (s + (long long)S * tt)] : 0.0;
                    u = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, u, 0, 0, 0);
                }
                if (gauge) {                                              // block-uniform
                    for (int a0 = 0; a0 < Q; a0 += 4) {
                        const int a = a0 + lk;
                        const double av = (prow && a < Q) ? -Uk[z + (long long)n * ((p0 + li) + (long long)Pn * a)] : 0.0;
                        const double bv = (tcol && a < Q) ? L1[a + (long long)Q * tt] : 0.0;
                        u = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, u, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) Us[(16 * jt + li) * GRAD_SW_UP + lk + 4 * reg] = u[reg];      // M[p = lk + 4 reg, b = 16 jt + li]
            }
            __syncthreads();
            // dC[p0 + ., q0 + .] += sum_b M[p, b] G_{k+1}[q, b] over the chunk (columns beyond T hold exact zeros: masked fragments)
            if (q0 < Q) {                                                 // wave-uniform
                for (int i = 0; i < 4 * jtiles; ++i) {
                    const int tl = 4 * i + lk, tt = j0 + tl;
                    const double av = Us[tl * GRAD_SW_UP + li];
                    const double bv = (qcol && tt < T) ? G[(q0 + li) + (long long)Q * tt] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                }
            }
        }
        if (qcol) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int p = p0 + lk + 4 * reg;
                if (p < Pn) O[z + (long long)n * (p + (long long)Pn * (q0 + li))] = acc[reg];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// y = alpha x + beta xi at ranks 2 r.  Entry (a, c) of the output core of site k (rl, rr: x's ranks there) is a fibre of n doubles:
//   first site   c < rr: dC_1[a, c]         else U_1[a, c - rr]
//   interior     a < rl: c < rr ? V_k[a, c] : 0          else  c < rr ? dC_k[a - rl, c] : U_k[a - rl, c - rr]
//   last site    a < rl: beta V_d[a, c]     else beta dC_d[a - rl, c] + alpha U_d[a - rl, c]      (d = 1: the second form alone)
// ---------------------------------------------------------------------------------------------
#define TTN_TAN_K 4                      // output columns per thread (n = 2), k_add's mapping

struct TangentAsmArgs {
    TTDev u, v, xi, y;
    const double* alpha;    // [batch] on the device, or null: 1
    const double* beta;
    int* status;            // [batch]: y's
};

// where entry (a, c) comes from: kind 0 an explicit zero, 1 a copy of s1, 2 beta s1, 3 beta s1 + alpha s2 (s1, s2: fibre offsets in doubles / n)
struct TanSrc { int kind; const double* s1; const double* s2; };
__device__ __forceinline__ TanSrc tan_source(int k, int d, int a, int c, int rl, int rr, const double* Uk, const double* Vk, const double* Xk, int n) {
    TanSrc r{0, nullptr, nullptr};
    if (k == d - 1) {
        if (d > 1 && a < rl) { r.kind = 2; r.s1 = Vk + (long long)n * (a + (long long)rl * c); }
        else {
            const int a2 = d > 1 ? a - rl : a;
            r.kind = 3; r.s1 = Xk + (long long)n * (a2 + (long long)rl * c); r.s2 = Uk + (long long)n * (a2 + (long long)rl * c);
        }
    } else if (k == 0) {
        r.kind = 1; r.s1 = (c < rr) ? Xk + (long long)n * (a + (long long)rl * c) : Uk + (long long)n * (a + (long long)rl * (c - rr));
    } else if (a < rl) {
        if (c < rr) { r.kind = 1; r.s1 = Vk + (long long)n * (a + (long long)rl * c); }
    } else {
        r.kind = 1; r.s1 = (c < rr) ? Xk + (long long)n * ((a - rl) + (long long)rl * c) : Uk + (long long)n * ((a - rl) + (long long)rl * (c - rr));
    }
    return r;
}

__global__ void __launch_bounds__(TTN_STREAM_TB) k_tangent_assemble(TangentAsmArgs P) {
    const int k = blockIdx.y, b = blockIdx.z, d = P.u.d;
    const long long* ur = P.u.rks + (long long)b * (d + 1);
    const long long* vr = P.v.rks + (long long)b * (d + 1);
    const long long* xr = P.xi.rks + (long long)b * (d + 1);
    if (grad_ranks_bad(d, [&](int m) { return ur[m] != vr[m] || ur[m] != xr[m] || ((m == 0 || m == d) && ur[m] != 1); })) {
        if (threadIdx.x == 0 && blockIdx.x == 0 && k == 0) ttn_set_status(P.status + b, TTN_ST_RANKS_DIFFER);
        return;
    }
    if (blockIdx.x == 0 && k == 0)
        for (int m = threadIdx.x; m <= d; m += blockDim.x) P.y.rks[(long long)b * (d + 1) + m] = (m == 0 || m == d) ? 1 : 2 * ur[m];
    const int n = P.u.dims[k];
    const int rl = (int)ur[k], rr = (int)ur[k + 1];
    const int zl = (k == 0) ? 1 : 2 * rl, zr = (k == d - 1) ? 1 : 2 * rr;
    const double* Uk = P.u.data + (long long)b * P.u.stride + P.u.off[k];
    const double* Vk = P.v.data + (long long)b * P.v.stride + P.v.off[k];
    const double* Xk = P.xi.data + (long long)b * P.xi.stride + P.xi.off[k];
    double* Yk = P.y.data + (long long)b * P.y.stride + P.y.off[k];
    const double al = P.alpha ? P.alpha[b] : 1.0, be = P.beta ? P.beta[b] : 1.0;
    if (n == 2) {
        typedef double d2v_t __attribute__((ext_vector_type(2)));
        const unsigned int uzl = (unsigned int)zl, uzr = (unsigned int)zr, cgroups = (uzr + TTN_TAN_K - 1) / TTN_TAN_K, items = uzl * cgroups;
        for (unsigned int it = blockIdx.x * blockDim.x + threadIdx.x; it < items; it += gridDim.x * blockDim.x) {
            const int a = (int)(it % uzl), c0 = (int)(it / uzl) * TTN_TAN_K;
            d2v_t v[TTN_TAN_K];
#pragma unroll
            for (int j = 0; j < TTN_TAN_K; ++j) {
                v[j] = (d2v_t){0.0, 0.0};
                if (c0 + j < zr) {
                    const TanSrc s = tan_source(k, d, a, c0 + j, rl, rr, Uk, Vk, Xk, 2);
                    if (s.kind) v[j] = *reinterpret_cast<const d2v_t*>(s.s1);
                    if (s.kind == 2) v[j] *= be;
                    if (s.kind == 3) {
                        const d2v_t w = *reinterpret_cast<const d2v_t*>(s.s2);
                        v[j].x = fma(be, v[j].x, al * w.x);
                        v[j].y = fma(be, v[j].y, al * w.y);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < TTN_TAN_K; ++j)
                if (c0 + j < zr) __builtin_nontemporal_store(v[j], reinterpret_cast<d2v_t*>(Yk + 2LL * ((long long)a + (long long)zl * (c0 + j))));
        }
        return;
    }
    const unsigned int total = (unsigned int)zl * (unsigned int)zr;       // one thread per output fibre (a, c)
    for (unsigned int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int a = (int)(e % (unsigned int)zl), c = (int)(e / (unsigned int)zl);
        const TanSrc s = tan_source(k, d, a, c, rl, rr, Uk, Vk, Xk, n);
        double* yo = Yk + (long long)n * e;
        for (int i = 0; i < n; ++i) {
            double o = 0.0;
            if (s.kind) o = s.s1[i];
            if (s.kind == 2) o *= be;
            if (s.kind == 3) o = fma(be, o, al * s.s2[i]);
            yo[i] = o;
        }
    }
}
