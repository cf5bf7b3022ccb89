// ttn_grid_kernels.h — train -> dense tensor on the device (ttn_tt_to_dense) and the QTT grid coordinates (ttn_qtt_grid_points).
//
// ttn_tt_to_dense cuts the train at a site m into two partial products,
//     L  (prod_{k <= m} n_k  x  r_m)      R  (r_m  x  prod_{k > m} n_k),
// both about sqrt(total) wide, built core by core with small products (k_dense_chain), and writes out = L R with fp64 MFMA
// (k_dense_product).  The output address of entry (i_1..i_N) is sum_k (i_k - 1) strides[k]; the strides form a mixed-radix system, so
// the address splits into offL[row of L] + offR[column of R], two tables a small kernel fills (k_dense_tables).
//
// Store order.  The rows of L and the columns of R are enumerated IN OUTPUT-ADDRESS ORDER (the tables are sorted by offset).  The
// host takes the sites with the smallest output strides, on whichever side of the cut they sit, until their dimensions multiply to
// at most TTN_DENSE_TILE: the TM rows and TN columns they span cover ONE contiguous, tile-aligned segment of TM*TN outputs.  A
// workgroup computes that tile in 16 x 16 MFMA blocks, scatters the accumulators into LDS at (address - segment base) and then
// writes the segment out front to back, so every wave-wide store instruction covers whole contiguous lines whatever the ordering.
#pragma once
#include "ttn_common.h"

#define TTN_DENSE_TB 256
#define TTN_DENSE_TILE 4096          // doubles of one output tile (32 KB of LDS)
#define TTN_DENSE_CHAIN_SMALL 8192   // chain steps with at most this many outputs share one single-workgroup launch

typedef double grid_f64x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int dense_ld(long long r) { return (int)((r + 3) & ~3LL); }     // leading dimension: the rank padded to the MFMA's K = 4

// ---- offset tables ----------------------------------------------------------------------------------------------------------------
// The sites of one side, sorted by output stride: entry p of the table has the digits of p in that mixed radix (smallest stride fastest).
struct DenseTabArgs {
    int ns;
    int n[TTN_MAX_D];
    long long stride[TTN_MAX_D];     // output stride of the site
    long long rstride[TTN_MAX_D];    // stride of the site in the row index of L / the column index of R (train order, first site fastest)
    long long count;
    long long* off;                  // [count] output offset, ascending
    int* idx;                        // [count] the row of L / column of R with that offset
};

__global__ void __launch_bounds__(TTN_DENSE_TB) k_dense_tables(DenseTabArgs T) {
    for (long long p = (long long)blockIdx.x * TTN_DENSE_TB + threadIdx.x; p < T.count; p += (long long)gridDim.x * TTN_DENSE_TB) {
        long long rem = p, off = 0, r = 0;
        for (int j = 0; j < T.ns; ++j) {
            const long long dg = rem % T.n[j];
            rem /= T.n[j];
            off += dg * T.stride[j];
            r += dg * T.rstride[j];
        }
        T.off[p] = off;
        T.idx[p] = (int)r;
    }
}

// ---- partial products -------------------------------------------------------------------------------------------------------------
// side 0: L_k [(I, i)][b] = sum_a L_{k-1}[I][a] G_k[i, a, b]   (rows: site 1 fastest), sites k0, k0 + 1, ...
// side 1: R_k [(i, J)][a] = sum_b G_k[i, a, b] R_{k+1}[J][b]   (R held transposed: one row per column of R), sites k0, k0 - 1, ...
// Both are stored row by row with the leading dimension dense_ld(rank) and zeros in the padding.  Step g of a chain writes buf[g & 1].
// A launch of several steps must have gridDim.x == 1 (the steps are separated by a workgroup barrier).
struct DenseChainArgs {
    TTDev tt;
    int side, k0, nsteps, par;       // par: parity of the chain's step index of the first step of this launch
    double* buf[2];
    long long buf_stride;            // doubles per train in each buffer
};

__global__ void __launch_bounds__(TTN_DENSE_TB) k_dense_chain(DenseChainArgs A) {
    const int b = blockIdx.y, d = A.tt.d;
    const long long* rk = A.tt.rks + (long long)b * (d + 1);
    const double* cores = A.tt.data + (long long)b * A.tt.stride;
    long long P = 1;                 // rows of the input partial product
    if (A.side == 0) for (int j = 0; j < A.k0; ++j) P *= A.tt.dims[j];
    else for (int j = d - 1; j > A.k0; --j) P *= A.tt.dims[j];
    for (int s = 0; s < A.nsteps; ++s) {
        const int k = A.side == 0 ? A.k0 + s : A.k0 - s;
        const int n = A.tt.dims[k], rl = (int)rk[k], rr = (int)rk[k + 1];
        const bool first = A.side == 0 ? k == 0 : k == d - 1;      // the input is the 1 x 1 matrix [1]
        const int rin = A.side == 0 ? rl : rr, rout = A.side == 0 ? rr : rl;
        const int ldin = dense_ld(rin), ldout = dense_ld(rout);
        const double* G = cores + A.tt.off[k];
        const double* in = A.buf[(A.par + s + 1) & 1] + (long long)b * A.buf_stride;
        double* out = A.buf[(A.par + s) & 1] + (long long)b * A.buf_stride;
        const long long nout = P * n * ldout;
        for (long long e = (long long)blockIdx.x * TTN_DENSE_TB + threadIdx.x; e < nout; e += (long long)gridDim.x * TTN_DENSE_TB) {
            const int c = (int)(e % ldout);
            const long long row = e / ldout;
            const int i = A.side == 0 ? (int)(row / P) : (int)(row % n);
            const long long I = A.side == 0 ? row % P : row / n;
            double acc = 0.0;
            if (c < rout) {
                if (first) acc = G[i + (long long)n * c];
                else if (A.side == 0) for (int a = 0; a < rin; ++a) acc += in[I * ldin + a] * G[i + (long long)n * (a + (long long)rl * c)];
                else for (int a = 0; a < rin; ++a) acc += G[i + (long long)n * (c + (long long)rl * a)] * in[I * ldin + a];
            }
            out[e] = acc;
        }
        P *= n;
        if (s + 1 < A.nsteps) __syncthreads();
    }
}

// ---- out = L R ------------------------------------------------------------------------------------------------------------------
struct DenseArgs {
    const double* L;                 // [PL][ld] per train (strideL doubles apart; 0: the 1 x 1 unit shared by all trains)
    const double* R;                 // [PR][ld] per train (the right side always holds at least one site)
    long long strideL, strideR;
    const long long* rks;            // [batch][d + 1] current ranks
    int d, m;                        // the cut: K = rks[b][m]
    const long long* offL;           // [PL] ascending
    const long long* offR;           // [PR] ascending
    const int* rowL;                 // [PL]
    const int* colR;                 // [PR]
    long long tilesL;                // PL / TM
    int TM, TN;                      // TM * TN <= TTN_DENSE_TILE
    long long total;
    double* out;                     // [batch][total]
    int vec2;                        // 1: every segment is 16-byte aligned and of even length
};

__global__ void __launch_bounds__(TTN_DENSE_TB) k_dense_product(DenseArgs A) {
    __shared__ double tile[TTN_DENSE_TILE];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const long long tp = blockIdx.x % A.tilesL, tq = blockIdx.x / A.tilesL;
    const long long p0 = tp * A.TM, q0 = tq * A.TN;
    const int ld = dense_ld(A.rks[(long long)b * (A.d + 1) + A.m]);
    const double* L = A.L + (long long)b * A.strideL;
    const double* R = A.R + (long long)b * A.strideR;
    const long long baseL = A.offL[p0], baseR = A.offR[q0];
    const int nbi = (A.TM + 15) >> 4, nbj = (A.TN + 15) >> 4;
    for (int blk = wave; blk < nbi * nbj; blk += TTN_DENSE_TB / 64) {
        const int bi = blk % nbi, bj = blk / nbi;
        const int pa = 16 * bi + li, qb = 16 * bj + li;
        const bool va = pa < A.TM, vb = qb < A.TN;
        const double* Lr = L + (long long)A.rowL[p0 + (va ? pa : 0)] * ld;
        const double* Rr = R + (long long)A.colR[q0 + (vb ? qb : 0)] * ld;
        grid_f64x4 acc = (grid_f64x4){0.0, 0.0, 0.0, 0.0};
        int k = 0;
        // the order of the K index is free as long as both operands agree: quarter lk of the wave takes k + 4 lk .. k + 4 lk + 3, one 32-byte load each
        for (; k + 16 <= ld; k += 16) {
            const grid_f64x4 zero = (grid_f64x4){0.0, 0.0, 0.0, 0.0};
            const grid_f64x4 av = va ? *reinterpret_cast<const grid_f64x4*>(Lr + k + 4 * lk) : zero;
            const grid_f64x4 bv = vb ? *reinterpret_cast<const grid_f64x4*>(Rr + k + 4 * lk) : zero;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], bv[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1], bv[1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2], bv[2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[3], bv[3], acc, 0, 0, 0);
        }
        for (; k < ld; k += 4) {
            const double a = va ? Lr[k + lk] : 0.0, bb = vb ? Rr[k + lk] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc, 0, 0, 0);
        }
        // accumulator register `reg` holds row lk + 4 reg, column li of the block
        if (vb) {
            const long long oR = A.offR[q0 + qb] - baseR;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int pr = 16 * bi + lk + 4 * reg;
                if (pr < A.TM) tile[(A.offL[p0 + pr] - baseL) + oR] = acc[reg];
            }
        }
    }
    __syncthreads();
    double* o = A.out + (long long)b * A.total + baseL + baseR;
    const int nt = A.TM * A.TN;
    if (A.vec2) {
        for (int t = 2 * tid; t < nt; t += 2 * TTN_DENSE_TB) *reinterpret_cast<double2*>(o + t) = make_double2(tile[t], tile[t + 1]);
    } else {
        for (int t = tid; t < nt; t += TTN_DENSE_TB) o[t] = tile[t];
    }
}

// ---- dense -> dense permutation of digits (ttn_tto_decomp_dev) ----------------------------------------------------------------------
// out[sum_j v_j ostride_j] = in[sum_j v_j istride_j] over the digits (n_j, istride_j, ostride_j), both stride sets mixed-radix systems
// of the same digits.  One workgroup moves one tile through LDS.  The tile is spanned by
//   SI: the fastest INPUT digits (their product TI, a contiguous run of the input), and
//   SO: the fastest OUTPUT digits not in SI (their product TO),
// with TI * TO <= TTN_DENSE_TILE; every other digit is enumerated by blockIdx.x.  Element e = eh * TI + el of the tile in input order
// (el over SI, eh over SO in output order) is loaded from in[baseI + el + inHi[eh]] — consecutive lanes, consecutive addresses — to
// tile[el + ld * eh].  In output order the tile's leading digits (in SI or SO alike) form contiguous runs of RO outputs: element
// f = fh * RO + fl is stored to out[baseO + fl + outHi[fh]] from tile[posLo[fl] + posHi[fh]], again consecutive lanes on consecutive
// addresses, every output exactly once.  The tables are filled by k_dense_tables from the digit lists (off: global offset, idx: LDS
// position); ld = TI + a pad the host picks so that the 32 lanes of a half wave read distinct banks (8-byte reads: 32 banks).
#define TTN_GATHER_LDS 5120          // doubles: TTN_DENSE_TILE plus room for the padded leading dimension (40 KB)
#define TTN_GATHER_DIGITS 32         // digits with n > 1: total <= 2^27 leaves at most 27

struct GatherArgs {
    const double* in;
    double* out;
    int TI, TO, ld, RO, nt;          // nt = TI * TO
    const long long* inHi;           // [TO] input offset of eh
    const int* posLo;                // [RO] LDS position of fl
    const long long* outHi;          // [nt / RO] output offset of fh
    const int* posHi;                // [nt / RO] LDS position of fh
    int nouter;                      // the digits outside the tile
    int on[TTN_GATHER_DIGITS];
    long long oin[TTN_GATHER_DIGITS], oout[TTN_GATHER_DIGITS];
};

__global__ void __launch_bounds__(TTN_DENSE_TB) k_dense_gather(GatherArgs G) {
    __shared__ double tile[TTN_GATHER_LDS];
    const int tid = threadIdx.x;
    long long baseI = 0, baseO = 0;
    {
        long long rem = blockIdx.x;
        for (int j = 0; j < G.nouter; ++j) {
            const long long dg = rem % G.on[j];
            rem /= G.on[j];
            baseI += dg * G.oin[j];
            baseO += dg * G.oout[j];
        }
    }
    const double* src = G.in + baseI;
    for (int e = tid; e < G.nt; e += TTN_DENSE_TB) {
        const int eh = e / G.TI, el = e - eh * G.TI;
        tile[el + G.ld * eh] = src[el + G.inHi[eh]];
    }
    __syncthreads();
    double* dst = G.out + baseO;
    for (int f = tid; f < G.nt; f += TTN_DENSE_TB) {
        const int fh = f / G.RO, fl = f - fh * G.RO;
        dst[fl + G.outHi[fh]] = tile[G.posLo[fl] + G.posHi[fh]];
    }
}

// ---- QTT grid coordinates ---------------------------------------------------------------------------------------------------------
// Entry e of the (2, ..., 2) tensor (site 1 fastest) has bit (e >> s) & 1 at site s; the bit -> (dim, level) rule of
// src/qtt_tools.jl:820-829 gives the grid index g per dimension.  coord = a + g * h with one rounded multiply and one rounded add
// (no contraction into an FMA), which is what NumPy computes for a + g * h.  HIP's __dmul_rn / __dadd_rn are inline * and + compiled
// with the default contraction, and the compiler fuses them after inlining (seen in the ISA; measured: 1 ulp off NumPy on
// [-2, 3.5]), so the kernel uses plain operators with contraction switched off in its own scope.
__global__ void __launch_bounds__(TTN_DENSE_TB) k_qtt_grid_points(int n_dims, int bits, int interleaved, double a, double h, long long first,
                                                                   long long count, double* X) {
#pragma clang fp contract(off)
    for (long long t = (long long)blockIdx.x * TTN_DENSE_TB + threadIdx.x; t < count; t += (long long)gridDim.x * TTN_DENSE_TB) {
        const unsigned long long e = (unsigned long long)(first + t);
        for (int dim = 0; dim < n_dims; ++dim) {
            unsigned long long g = 0;
            for (int level = 0; level < bits; ++level) {
                const int site = interleaved ? level * n_dims + dim : dim * bits + level;
                g |= ((e >> site) & 1ULL) << (bits - 1 - level);
            }
            const double gh = (double)g * h;               // (plain operators: the flags that count are those of THIS scope)
            X[(long long)dim * count + t] = a + gh;
        }
    }
}
