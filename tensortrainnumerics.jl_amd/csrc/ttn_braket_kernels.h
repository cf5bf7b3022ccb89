// ttn_braket_kernels.h — <x| A |y> = sum_{i, j} conj(x_i) A_ij y_j (include/ttn_braket.h) on ComplexF64 operands without forming A y:
// the three-layer transfer recurrence of ttn_expect_kernels.h on interleaved (re, im) cores, one workgroup per train, the scalar the
// only thing that is written per train.
//
// Operand types: the trains x and y share an element type (CX: ComplexF64), the operator is real or complex on its own (CA).  The
// kernel is built for the three forms with a complex operand — (CA, CX) = (1, 1), (0, 1), (1, 0); a real operand stays real in memory
// and is read as it lies, as k_zapply<CA, CX> reads it.  x is conjugated: a sign on its imaginary fragment.
//
//   state, RIGHT TO LEFT on the on-chip route:  M[a, be, b] complex over the right ranks of x_k, A_k, y_k; per site
//     1.  U_j[a, be, bl]   = sum_b M[a, be, b] y_k[j, bl, b]                         fp64 MFMA on split re / im fragments
//     2.  V_i[a, be', bl]  = sum_{j, be} A_k[i, j, be', be] U_j[a, be, bl]          elementwise in (a, bl): acts on the accumulators
//     3.  M'[al, be', bl]  = sum_{i, a} conj(x_k[i, al, a]) V_i[a, be', bl]         fp64 MFMA
//   A complex product is four real MFMA accumulations (two when one factor is real); the minus sign of the real part and the sign of
//   conj are the negate bit of the MFMA's A operand.
//
// The on-chip route (every n_k = 2, train ranks <= BRAKET_QTT_RMAX, operator ranks <= BRAKET_QTT_OPR_MAX) follows expect_site<RM>:
//   * wave w of the 16 owns tile (tr = w & 3, tc = w >> 2) of every U_j[., be, .], re and im: 4 R accumulators (the real kernel: 2 R);
//   * a complex core is stored (re, im) fastest, then z: the 32 bytes of a lane's (z = 0, 1) pair are two 16-byte loads, each giving
//     both planes of one element; the planes go to separate MFMAs;
//   * step 2 is 4 R R' wave-uniform complex coefficients (the operator core, staged in LDS once per site) times those accumulators;
//   * the accumulator layout of V_i is the B-operand layout of step 3, so a wave multiplies its V tiles by x_k's fragments for the four
//     output row blocks and holds PARTIAL sums over its a-block of M'[., be', .], re and im;
//   * the four waves of a column block meet in TWO LDS images (re, im; k_dot's swizzled layout, LDS atomics), one be' at a time.  Four
//     images (the real kernel's rotation, twice) are 164 KiB and do not fit, so a pass ends with two barriers: adds | flush and zero.
//   * the state sits in library workspace as 2 R dense 64 x 64 images per train (plane-split: image 2 be is the real part, 2 be + 1 the
//     imaginary part), zero outside the current ranks, so step 1 reads it without masks.
// From HBM a site reads its three cores and nothing else; U and V never exist in memory.
//
// The general route (any n, any ranks, any R) runs the three steps LEFT TO RIGHT as workgroup-GEMM calls per site on stride-2 views
// of the interleaved arrays (k_tdvp's complex contractions, ttn_tdvp_kernels.h): four real GEMMs per complex product, two when one
// factor is real, conj a sign.  State, U and V (always complex) live in library workspace.
// One train takes one route for the whole chain, decided per train from its rank words: the on-chip route is a kernel of its own
// (no call, no stack), the general route another, and a call whose batch may hold both classes launches the two one after the other.
#pragma once
#include "ttn_common.h"
#include "ttn_wg_gemm.h"
#include "ttn_dot_kernels.h"
#include "ttn_tdvp_kernels.h"

#define BRAKET_QTT_RMAX DOT_RMAX                 // largest train rank of the on-chip route (= TTN_BRAKET_QTT_MAX_RANK of the public header)
#define BRAKET_QTT_OPR_MAX 2                     // largest operator rank of the on-chip route: 4 R accumulator tiles of U (32 R VGPRs) live in a wave
#define BRAKET_MAX_D DOT_MAX_D
#define BRAKET_ACORE_DOUBLES 64                  // >= 8 * BRAKET_QTT_OPR_MAX^2, the staged operator core (behind the two images)
#define BRAKET_LDS_DOUBLES ((2 * DOT_MS_DOUBLES + BRAKET_ACORE_DOUBLES) > GEMM_LDS_TOTAL ? (2 * DOT_MS_DOUBLES + BRAKET_ACORE_DOUBLES) : GEMM_LDS_TOTAL)
#define BRAKET_TAB 7                             // ints per site of the table (behind that region)
#define BRAKET_LDS_BYTES(d) (sizeof(double) * BRAKET_LDS_DOUBLES + sizeof(int) * BRAKET_TAB * ((d) + 2))
static_assert(BRAKET_LDS_BYTES(BRAKET_MAX_D) <= 160 * 1024, "k_zexpect: the LDS of a workgroup is 160 KiB");
static_assert(8 * BRAKET_QTT_OPR_MAX * BRAKET_QTT_OPR_MAX <= BRAKET_ACORE_DOUBLES, "k_zexpect: the staged operator core");
#define BRAKET_IMG (BRAKET_QTT_RMAX * BRAKET_QTT_RMAX)            // doubles of one plane of one be-image of the state in workspace

struct BraketArgs {
    TTDev x, y;
    TTODev A;
    double* scratch;            // per train: max(2 Rmax * BRAKET_IMG, 2 (2 + 2 nmax) rxmax Rmax rymax)
    long long scratch_stride;
    int rxmax, rymax, Rmax, nmax;
    int skip_fit;               // k_zexpect<., ., 0>: leave the trains of the on-chip class alone (the on-chip kernel of this call took them)
    double* out;                // [batch] interleaved (re, im), device
};

// the (z = 0, 1) pair of core element (., p, q), re and im apart; zero outside p < np, q < nq
struct bk_frag { double re0, im0, re1, im1; };
template <bool CX>
__device__ __forceinline__ bk_frag bk_load(const double* core, int p, int q, int np, int nq, int ldp) {
    const bool ok = (p < np) && (q < nq);
    bk_frag f;
    if (CX) {
        const unsigned off = ok ? 4u * (unsigned)(p + ldp * q) : 0u;        // unsigned: a uniform base plus a 32-bit lane offset, one VGPR
        dot_f64x2 e0 = *(gmem_f64x2*)(core + off);
        dot_f64x2 e1 = *(gmem_f64x2*)(core + off + 2u);
        if (!ok) { e0.x = 0.0; e0.y = 0.0; e1.x = 0.0; e1.y = 0.0; }
        f.re0 = e0.x; f.im0 = e0.y; f.re1 = e1.x; f.im1 = e1.y;
    } else {
        const dot_f64x2 v = dot_load2(core, p, q, np, nq, ldp);
        f.re0 = v.x; f.re1 = v.y; f.im0 = 0.0; f.im1 = 0.0;
    }
    return f;
}

// element z of the pair alone: one 16-byte load (complex) or one 8-byte load (real)
struct bk_elem { double re, im; };
template <bool CX>
__device__ __forceinline__ bk_elem bk_load1(const double* core, int z, int p, int q, int np, int nq, int ldp) {
    const bool ok = (p < np) && (q < nq);
    bk_elem f;
    if (CX) {
        const unsigned off = ok ? 4u * (unsigned)(p + ldp * q) + 2u * (unsigned)z : 0u;
        dot_f64x2 e = *(gmem_f64x2*)(core + off);
        if (!ok) { e.x = 0.0; e.y = 0.0; }
        f.re = e.x; f.im = e.y;
    } else {
        const unsigned off = ok ? 2u * (unsigned)(p + ldp * q) + (unsigned)z : 0u;
        const double e = ((gmem_f64*)core)[off];
        f.re = ok ? e : 0.0; f.im = 0.0;
    }
    return f;
}

#define BK_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
// c - a b: on gfx940 and later the BLGP field of the fp64 MFMA holds negate bits (bit 0: A); the sign costs no instruction and no register
#define BK_MFMA_NEGA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 1)
#define BK_ZERO ((mfma_acc_t){0.0, 0.0, 0.0, 0.0})

// One site of the on-chip route.  rx, R, ry: RIGHT ranks of x_k, A_k, y_k (the incoming state); rx2, R2, ry2: their LEFT ranks.
//   Mg : the state, element (a, be, b) of plane p at Mg[(2 be + p) BRAKET_IMG + a + 64 b], zero outside (rx, R, ry); overwritten with M'
//   Ac : LDS, receives the operator core as it lies: (i, j, be', be) at i + 2 (j + 2 (be' + R2 be)), a complex element two doubles
//   img: two LDS images (re, im), all zero on entry and on exit
template <bool CA, bool CX, int RM>
__device__ __forceinline__ void braket_site(const double* Xk, const double* Yk, const double* Ak, double* Mg, int rx, int rx2, int R, int R2, int ry, int ry2,
                                            lds_f64* Ac, lds_f64* img) {
    // tr, tc are scalars; what a lane derives from its index (li, lk, addresses) is derived where it is used, from an opaque copy of the
    // thread index: derived once at the top it is loop invariant, the compiler keeps it in registers across the passes, and next to
    // the 32 R accumulator registers of U that costs a spill frame (the note in ttn_dense_kernels.h, k_fused_merge's epilogue)
    const int wave = uni32((int)threadIdx.x >> 6);
    const int tr = wave & 3, tc = wave >> 2;
    constexpr int EA = CA ? 2 : 1;
    if ((int)threadIdx.x < 4 * EA * R * R2) Ac[threadIdx.x] = ((gmem_f64*)Ak)[threadIdx.x];      // <= 8 RM^2 <= TTN_WG
    const bool active = 16 * tr < rx && 16 * tc < ry2;                   // wave-uniform
    mfma_acc_t ur[RM][2], ui[RM][2];                                     // U_j[., be, .], re and im
#pragma unroll
    for (int be = 0; be < RM; ++be) { ur[be][0] = BK_ZERO; ur[be][1] = BK_ZERO; ui[be][0] = BK_ZERO; ui[be][1] = BK_ZERO; }
    if (active) {
        // ---- step 1: U_j[a, be, bl] = sum_b M[a, be, b] y_k[j, bl, b]: rows a = 16 tr + ., columns bl = 16 tc + . ----
        int te = threadIdx.x;
        asm volatile("" : "+v"(te));
        const int li = te & 15, lk = (te >> 4) & 3;
        const int nt = (ry + 3) >> 2;
        const int bq = 16 * tc + li;
        gmem_f64* mrow = (gmem_f64*)Mg + (16 * tr + li) + 64 * lk;              // M[a, be, b = 4 t + lk]: + 256 t + 2 BRAKET_IMG be (+ BRAKET_IMG: im)
        for (int t = 0; t < nt; ++t) {
            const bk_frag y = bk_load<CX>(Yk, bq, 4 * t + lk, ry2, ry, ry2);
            double mr[RM], mi[RM];
#pragma unroll
            for (int be = 0; be < RM; ++be) {
                mr[be] = be < R ? mrow[256 * t + 2 * BRAKET_IMG * be] : 0.0;
                mi[be] = be < R ? mrow[256 * t + 2 * BRAKET_IMG * be + BRAKET_IMG] : 0.0;
            }
#pragma unroll
            for (int be = 0; be < RM; ++be) {
                if (be < R) {                                             // wave-uniform
                    ur[be][0] = BK_MFMA(mr[be], y.re0, ur[be][0]);
                    ur[be][1] = BK_MFMA(mr[be], y.re1, ur[be][1]);
                    ui[be][0] = BK_MFMA(mi[be], y.re0, ui[be][0]);
                    ui[be][1] = BK_MFMA(mi[be], y.re1, ui[be][1]);
                    if (CX) {
                        ur[be][0] = BK_MFMA_NEGA(mi[be], y.im0, ur[be][0]);
                        ur[be][1] = BK_MFMA_NEGA(mi[be], y.im1, ur[be][1]);
                        ui[be][0] = BK_MFMA(mr[be], y.im0, ui[be][0]);
                        ui[be][1] = BK_MFMA(mr[be], y.im1, ui[be][1]);
                    }
                }
            }
        }
    }
    dot_lds_barrier();                                                    // the staged core is visible; every wave has read the state
    const int nta = (rx2 + 15) >> 4;
    lds_f64* imr = img;
    lds_f64* imi = img + DOT_MS_DOUBLES;
    for (int bp = 0; bp < R2; ++bp) {
        if (active) {
            int te = threadIdx.x;
            asm volatile("" : "+v"(te));
            const int li = te & 15, lk = (te >> 4) & 3;
            // One i at a time: V_0 and V_1 together are 32 VGPRs next to the 32 R of U, and at R = 2 the compiler then keeps a tile of U on
            // the stack across step 3.  The price is that the LDS images take the partial sums of i = 0 and of i = 1 separately.
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                // ---- step 2: V_i[a, bp, bl] = sum_{j, be} A_k[i, j, bp, be] U_j[a, be, bl], on the accumulators ----
                mfma_acc_t vr = BK_ZERO, vi = BK_ZERO;
#pragma unroll
                for (int be = 0; be < RM; ++be) {
                    if (be < R) {
                        const lds_f64* c = Ac + EA * (i + 4 * (bp + R2 * be));      // (i, j) at i + 2 j
                        if (CA) {
                            const double r0 = c[0], i0 = c[1], r1 = c[4], i1 = c[5];
                            // one product per statement: each is an FMA into the accumulator, no temporary tile
                            vr += r0 * ur[be][0]; vr -= i0 * ui[be][0]; vr += r1 * ur[be][1]; vr -= i1 * ui[be][1];
                            vi += r0 * ui[be][0]; vi += i0 * ur[be][0]; vi += r1 * ui[be][1]; vi += i1 * ur[be][1];
                        } else {
                            const double c0 = c[0], c1 = c[2];
                            vr += c0 * ur[be][0]; vr += c1 * ur[be][1];
                            vi += c0 * ui[be][0]; vi += c1 * ui[be][1];
                        }
                    }
                }
                // ---- step 3, partial over a in this wave's block and over this i: sum_r conj(x_k[i, al, 16 tr + 4 r + lk]) V_i[16 tr + 4 r + lk, bp, bl]
                //      — register r of V_i is the B fragment of k-step r as it is; rows a >= rx are masked fragments ----
                //      re: x.re V.re + x.im V.im      im: x.re V.im - x.im V.re
#pragma unroll
                for (int ta = 0; ta < 4; ++ta) {
                    if (ta < nta) {                                       // wave-uniform
                        const int aq = 16 * ta + li;
                        mfma_acc_t pr = BK_ZERO, pi = BK_ZERO;
                        bk_elem x[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) x[r] = bk_load1<CX>(Xk, i, aq, 16 * tr + 4 * r + lk, rx2, rx, rx2);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            pr = BK_MFMA(x[r].re, vr[r], pr);
                            pi = BK_MFMA(x[r].re, vi[r], pi);
                            if (CX) {
                                pr = BK_MFMA(x[r].im, vi[r], pr);
                                pi = BK_MFMA_NEGA(x[r].im, vr[r], pi);
                            }
                        }
                        // M'[al = 16 ta + lk + 4 reg, bp, bl = 16 tc + li] += p[reg]   (entries beyond (rx2, ry2) are exact zeros)
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
        dot_lds_barrier();                                                // images bp are complete
        {
            gmem_wf64* dst = (gmem_wf64*)Mg + 2 * BRAKET_IMG * bp;
            int te = threadIdx.x;
            asm volatile("" : "+v"(te));
            for (int e = te; e < BRAKET_IMG; e += TTN_WG) {
                const int at = DOT_AT(e >> 6, e & 63);
                dst[e] = imr[at];
                dst[e + BRAKET_IMG] = imi[at];
                imr[at] = 0.0;
                imi[at] = 0.0;
            }
        }
        dot_lds_barrier();                                                // ... and zero again before the next pass adds
    }
    __syncthreads();                                                      // the state is in memory before the next site reads it
}

// C (complex) = op(A) B with A of esA and B of esB doubles per element (at least one of them 2), strides in ELEMENTS; conjA: conj(A)
__device__ inline void braket_gemm(int m, int n, int k, const double* A, Idx Ar, Idx Ac, int esA, bool conjA, const double* B, Idx Br, Idx Bc, int esB,
                                   double* C, Idx Cr, Idx Cc, double* lds) {
    const double sg = conjA ? -1.0 : 1.0;
    const View Cre = tv(C, 2, 0, Cr, Cc), Cim = tv(C, 2, 1, Cr, Cc);
    if (esA == 2 && esB == 2) {
        const View Are = tv(A, 2, 0, Ar, Ac), Aim = tv(A, 2, 1, Ar, Ac), Bre = tv(B, 2, 0, Br, Bc), Bim = tv(B, 2, 1, Br, Bc);
        wg_gemm(m, n, k, Are, Bre, Cre, 1.0, 0.0, lds);
        wg_gemm(m, n, k, Aim, Bim, Cre, -sg, 1.0, lds);
        wg_gemm(m, n, k, Are, Bim, Cim, 1.0, 0.0, lds);
        wg_gemm(m, n, k, Aim, Bre, Cim, sg, 1.0, lds);
    } else if (esA == 2) {
        const View Are = tv(A, 2, 0, Ar, Ac), Aim = tv(A, 2, 1, Ar, Ac), Bv = tv(B, 1, 0, Br, Bc);
        wg_gemm(m, n, k, Are, Bv, Cre, 1.0, 0.0, lds);
        wg_gemm(m, n, k, Aim, Bv, Cim, sg, 0.0, lds);
    } else {
        const View Av = tv(A, 1, 0, Ar, Ac), Bre = tv(B, 2, 0, Br, Bc), Bim = tv(B, 2, 1, Br, Bc);
        wg_gemm(m, n, k, Av, Bre, Cre, 1.0, 0.0, lds);
        wg_gemm(m, n, k, Av, Bim, Cim, 1.0, 0.0, lds);
    }
}

// One site of the general route, LEFT TO RIGHT, expect_site_generic's three products: rx, R, ry are the LEFT ranks (incoming state
// Mc[al + rx (be + R bl)]), rx2, R2, ry2 the right ranks (outgoing Mn[a + rx2 (be' + R2 b)]).  U at al + rx (be + R (j + n b)), V at
// i + n (al + rx (be' + R2 b)); Mc, Mn, U, V complex (interleaved), the cores of esX / esA doubles per element.
__device__ __noinline__ void braket_site_generic(double* Xk, double* Yk, double* Ak, double* Mc, double* Mn, double* U, double* V, int n, int rx, int rx2,
                                                 int R, int R2, int ry, int ry2, int esX, int esA, double* lds) {
    Xk = unip(Xk); Yk = unip(Yk); Ak = unip(Ak); Mc = unip(Mc); Mn = unip(Mn); U = unip(U); V = unip(V); lds = unip(lds);
    n = uni32(n); rx = uni32(rx); rx2 = uni32(rx2); R = uni32(R); R2 = uni32(R2); ry = uni32(ry); ry2 = uni32(ry2); esX = uni32(esX); esA = uni32(esA);
    const long long rxR = (long long)rx * R;
    // step 1: U[(al, be), (j, b)] = sum_bl M[(al, be), bl] y_k[j, bl, b]
    braket_gemm(rx * R, n * ry2, ry, Mc, plain(1), plain(rxR), 2, false, Yk, plain(n), Idx{n, 1, (long long)n * ry}, esX, U, plain(1), plain(rxR), lds);
    // step 2: V[(al, b), (i, be')] = sum_{(be, j)} U[(al, b), (be, j)] A_k[i, j, be, be']
    braket_gemm(rx * ry2, n * R2, R * n, U, Idx{rx, 1, rxR * n}, plain(rx), 2, false, Ak, Idx{R, (long long)n * n, n}, Idx{n, 1, (long long)n * n * R}, esA,
                V, Idx{rx, n, (long long)n * rx * R2}, Idx{n, 1, (long long)n * rx}, lds);
    // step 3: M'[a, (be', b)] = sum_{(i, al)} conj(x_k[i, al, a]) V[(i, al), (be', b)]
    braket_gemm(rx2, R2 * ry2, n * rx, Xk, plain((long long)n * rx), plain(1), esX, true, V, plain(1), plain((long long)n * rx), 2, Mn, plain(1), plain(rx2), lds);
}

// CA / CX: the operator / the trains are ComplexF64.
// RM = 1 .. BRAKET_QTT_OPR_MAX: the on-chip route and nothing else — every n_k is 2 and the operator ranks are <= RM (both known on the
//   host); a train with a rank above BRAKET_QTT_RMAX is left alone (the host then launches RM = 0 with skip_fit set for those).  The
//   kernel holds no call and no stack: the general route's out-of-line GEMMs would bring their frames into it.
// RM = 0: the general route; with skip_fit set, only for the trains that the on-chip kernel of the same call left alone.
template <bool CA, bool CX, int RM>
__global__ void __launch_bounds__(TTN_WG) k_zexpect(BraketArgs P) {
    extern __shared__ double lds[];
    const int t = blockIdx.x;
    const int tid = threadIdx.x;
    const TTDev& X = P.x; const TTDev& Y = P.y; const TTODev& A = P.A;
    const int d = X.d;
    double* scr = P.scratch + (long long)t * P.scratch_stride;
    lds_i32* tab = (lds_i32*)((lds_f64*)lds + BRAKET_LDS_DOUBLES);   // [0] rx_k [1] ry_k [2] R_k [3] n_k [4] offx_k [5] offy_k [6] offA_k
    for (int k = tid; k <= d; k += TTN_WG) {
        tab[BRAKET_TAB * k + 0] = (int)X.rks[(long long)t * (d + 1) + k];
        tab[BRAKET_TAB * k + 1] = (int)Y.rks[(long long)t * (d + 1) + k];
        tab[BRAKET_TAB * k + 2] = (int)A.rks[k];
        tab[BRAKET_TAB * k + 3] = k < d ? (CX ? X.dims[k] >> 1 : X.dims[k]) : 0;      // a complex train keeps 2 n_k in its table
        tab[BRAKET_TAB * k + 4] = k < d ? (int)X.off[k] : 0;              // trains and operator are below 2^31 doubles (checked by the host)
        tab[BRAKET_TAB * k + 5] = k < d ? (int)Y.off[k] : 0;
        tab[BRAKET_TAB * k + 6] = k < d ? (int)A.off[k] : 0;
    }
    __syncthreads();
    const double* Xbase = X.data + (long long)t * X.stride;
    const double* Ybase = Y.data + (long long)t * Y.stride;
    const double* Abase = A.data;
    bool fit = true;                                                      // wave-uniform: the route of this train
    if (RM > 0 || P.skip_fit)
        for (int k = 0; k <= d; ++k) fit = fit && uni32(tab[BRAKET_TAB * k]) <= BRAKET_QTT_RMAX && uni32(tab[BRAKET_TAB * k + 1]) <= BRAKET_QTT_RMAX;
    if constexpr (RM > 0) {
        if (!fit) return;
        lds_f64* img = (lds_f64*)lds;
        lds_f64* Ac = img + 2 * DOT_MS_DOUBLES;
        const int Rlast = uni32(tab[BRAKET_TAB * d + 2]);
        for (int e = tid; e < 2 * DOT_MS_DOUBLES; e += TTN_WG) img[e] = 0.0;
        for (int e = tid; e < 2 * Rlast * BRAKET_IMG; e += TTN_WG) scr[e] = (e == 0) ? 1.0 : 0.0;           // e_1 e_1^T e_1 at the right end
        __syncthreads();
        for (int k = d - 1; k >= 0; --k) {
            const lds_i32* s = tab + BRAKET_TAB * k;
            braket_site<CA, CX, RM>(unip(Xbase + uni32(s[4])), unip(Ybase + uni32(s[5])), unip(Abase + uni32(s[6])), scr, uni32(s[BRAKET_TAB]), uni32(s[0]),
                                    uni32(s[BRAKET_TAB + 2]), uni32(s[2]), uni32(s[BRAKET_TAB + 1]), uni32(s[1]), Ac, img);
        }
        if (tid == 0) { P.out[2 * t] = scr[0]; P.out[2 * t + 1] = scr[BRAKET_IMG]; }
    } else {
        if (P.skip_fit && fit) return;
        const long long S = 2 * (long long)P.rxmax * P.Rmax * P.rymax;            // doubles of one complex state
        double* Mc = scr; double* Mn = scr + S;
        double* U = Mn + S; double* V = U + (long long)P.nmax * S;
        if (tid == 0) { Mc[0] = 1.0; Mc[1] = 0.0; }
        __syncthreads();
        for (int k = 0; k < d; ++k) {
            const lds_i32* s = tab + BRAKET_TAB * k;
            braket_site_generic(const_cast<double*>(Xbase) + uni32(s[4]), const_cast<double*>(Ybase) + uni32(s[5]), const_cast<double*>(Abase) + uni32(s[6]), Mc, Mn,
                                U, V, uni32(s[3]), uni32(s[0]), uni32(s[BRAKET_TAB]), uni32(s[2]), uni32(s[BRAKET_TAB + 2]), uni32(s[1]),
                                uni32(s[BRAKET_TAB + 1]), CX ? 2 : 1, CA ? 2 : 1, lds);
            double* tmp = Mc; Mc = Mn; Mn = tmp;
            __syncthreads();
        }
        if (tid == 0) { P.out[2 * t] = Mc[0]; P.out[2 * t + 1] = Mc[1]; }
    }
}
