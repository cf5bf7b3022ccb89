// ttn_resite_kernels.h — to_qtt / to_ttv (src/qtt_tools.jl:254-360): split the physical index of every core into factors, or merge runs
// of consecutive cores into one, on a resident batch.
//   k_split_sites  one workgroup per train (like k_ttv_decomp): the successive SVDs of to_qtt, each one a wg_hsvd_step on a View of the
//                  input core or of the carried remainder — the reference's reshape / permutedims are index arithmetic.
//   k_merge_copy   the rank table of the merged train and its groups of ONE core (plain copies).
//   k_merge_step   one contraction step of every group of >= 2 cores: out[(i1 n2 + i2), a, b] = sum_m P[i1, a, m] C[i2, m, b] on the
//                  fp64 MFMA, grid = tiles x groups x batch.  No SVD: the work is streaming the output.
#pragma once
#include "ttn_hsvd_kernels.h"

// ---- to_qtt -------------------------------------------------------------------------------------------------------------------
struct SplitArgs {
    CompressArgs C;              // scratch / status / Jacobi knobs; C.tt = the OUTPUT handle (its dims are the flattened split lists)
    TTDev x;                     // the input handle
    int nsplit[TTN_MAX_D];       // factors per input site
    double threshold;
    double* work;                // per train: cur0 | cur1 (carry_len doubles each) | M2, then the BondCtx-style scratch (C.scratch)
    long long work_stride, carry_len;
};

__global__ void __launch_bounds__(TTN_WG) k_split_sites(SplitArgs H) {
    extern __shared__ double lds[];
    const CompressArgs& P = H.C;
    const TTDev& Z = P.tt;
    const TTDev& X = H.x;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) P.sweep_stats[b] = 0;
    BondCtx S;
    S.ldsX = lds;
    S.red = lds + GEMM_LDS_TOTAL;
    S.Ts = S.red + 32;
    S.Ss = S.Ts + QR_NB * QR_NB;
    S.taus = S.Ss + QR_NB * QR_NB;
    S.scal = S.taus + QR_NB;
    S.iflag = reinterpret_cast<int*>(S.scal + 8);
    S.nrm2 = S.scal + 16;
    double* scr = P.scratch + (long long)b * P.scratch_stride;
    S.M = nullptr; S.M2 = nullptr;
    S.Vb = scr;                                           // QR_NB x qmax
    S.Wb = S.Vb + (long long)QR_NB * P.qmax;              // pmax x QR_NB
    S.Us = S.Wb + (long long)P.pmax * QR_NB;              // pmax x pmax
    S.Xg = S.Us + (long long)P.pmax * P.pmax;             // pmax x pmax
    S.sig = S.Xg + (long long)P.pmax * P.pmax;
    S.sigs = S.sig + P.pmax;
    S.perm = reinterpret_cast<int*>(S.sigs + P.pmax);
    S.Ga = S.Gb = S.Cc = S.T1 = S.T2 = S.T3 = nullptr;
    double* cur = H.work + (long long)b * H.work_stride;
    double* nxt = cur + H.carry_len;
    double* M2 = nxt + H.carry_len;
    const long long* xr = X.rks + (long long)b * (X.d + 1);
    long long* zr = Z.rks + (long long)b * (Z.d + 1);
    bool alive = xr[0] <= Z.cap[0];
    if (alive && tid == 0) zr[0] = xr[0];
    int zi = 0;                                            // output site
    for (int i = 0; i < X.d && alive; ++i) {
        const int n = X.dims[i], k = H.nsplit[i];
        const int rl = (int)xr[i], rnext = (int)xr[i + 1];
        double* src = X.data + (long long)b * X.stride + X.off[i];
        if (rnext > Z.cap[zi + k]) { alive = false; break; }
        int remaining = n, rprev = rl;
        for (int j = 0; j + 1 < k; ++j, ++zi) {
            const int s = Z.dims[zi];
            const int fine = remaining / s;                // the coarse digit c (size s) goes to the new core, the fine rest f stays
            const int a = rprev * s, bc = fine * rnext;
            // M[(al + rprev c), (f + fine be)] = core[al, c fine + f, be]   (src/qtt_tools.jl:278-283)
            const View Av = (j == 0) ? mkview(src, Idx{rprev, (long long)n, (long long)fine}, Idx{fine, 1, (long long)n * rprev})
                                     : mkview(cur, Idx{rprev, 1, (long long)rprev * fine}, Idx{fine, (long long)rprev, (long long)rprev * remaining});
            double* core = Z.data + (long long)b * Z.stride + Z.off[zi];
            const int r = wg_hsvd_step(P, b, S, Av, a, bc, M2, 0, s, rprev, core, nxt, H.threshold, (int)Z.cap[zi + 1], lds, 3);
            if (r < 0) { alive = false; break; }
            if (tid == 0) zr[zi + 1] = r;
            rprev = r;
            remaining = fine;
            double* t = cur; cur = nxt; nxt = t;
            __syncthreads();
        }
        if (!alive) break;
        // last (or only) core of this site: the carried (rprev, remaining, rnext) as (remaining, rprev, rnext)   (:303)
        double* core = Z.data + (long long)b * Z.stride + Z.off[zi];
        const long long cnt = (long long)remaining * rprev * rnext;
        if (k == 1) {
            for (long long e = tid; e < cnt; e += TTN_WG) core[e] = src[e];
        } else {
            for (long long e = tid; e < cnt; e += TTN_WG) {
                const int f = (int)(e % remaining);
                const long long t2 = e / remaining;
                const int al = (int)(t2 % rprev), be = (int)(t2 / rprev);
                core[e] = cur[al + (long long)rprev * (f + (long long)remaining * be)];
            }
        }
        if (tid == 0) zr[zi + 1] = rnext;
        ++zi;
        __syncthreads();
    }
    if (!alive && tid == 0) ttn_set_status(&P.status[b], TTN_ST_RANK_OVERFLOW);
}

// ---- to_ttv -------------------------------------------------------------------------------------------------------------------
#define TTN_MERGE_TB 256           // 4 waves
#define TTN_MERGE_GROUPS 64        // groups per launch (their table travels in the kernel arguments)
#define TTN_MERGE_NX 16            // (i1, i2) pairs per workgroup: 4 accumulator tiles per wave
#define TTN_MERGE_KC 16            // bond indices per staged chunk
#define TTN_MERGE_LD 17            // leading dimension of the staged panels (odd: the fragment reads of 16 lanes hit 16 banks)

struct MergeArgs {
    TTDev x, z;
    int* status;                     // z's status words
    int ngroups;                     // groups in this launch
    int g0;                          // first output site of this launch
    int step;                        // k_merge_step: contract cores k0 .. k0+step-1 (already merged) with core k0+step
    int k0[TTN_MERGE_GROUPS];        // first input site of each group
    int count[TTN_MERGE_GROUPS];     // cores of each group
    double* work;                    // intermediate products of the groups of >= 3 cores, two buffers (ping-pong) per group:
    long long work_stride;           //   train b, group g, buffer q at work + b * work_stride + work_off[g] + q * work_half[g]
    long long work_off[TTN_MERGE_GROUPS];
    long long work_half[TTN_MERGE_GROUPS];   // (even, like the offsets: the buffers stay 16-byte aligned)
};

// rank table of the merged train (bond g of z = bond k0_g of x) and the groups of one core
__global__ void __launch_bounds__(TTN_MERGE_TB) k_merge_copy(MergeArgs M) {
    const int g = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const TTDev& X = M.x;
    const TTDev& Z = M.z;
    const int k0 = M.k0[g], cnt = M.count[g], zs = M.g0 + g;
    const long long* xr = X.rks + (long long)b * (X.d + 1);
    long long* zr = Z.rks + (long long)b * (Z.d + 1);
    const long long rl = xr[k0], rr = xr[k0 + cnt];
    if (rl > Z.cap[zs] || rr > Z.cap[zs + 1]) { if (blockIdx.x == 0 && tid == 0) ttn_set_status(&M.status[b], TTN_ST_RANK_OVERFLOW); return; }
    if (blockIdx.x == 0 && tid == 0) {
        zr[zs] = rl;
        if (zs + 1 == Z.d) zr[Z.d] = rr;
    }
    if (cnt != 1) return;
    const long long len = (long long)X.dims[k0] * rl * rr;
    const double* src = X.data + (long long)b * X.stride + X.off[k0];
    double* dst = Z.data + (long long)b * Z.stride + Z.off[zs];
    for (long long e = (long long)blockIdx.x * TTN_MERGE_TB + tid; e < len; e += (long long)gridDim.x * TTN_MERGE_TB) dst[e] = src[e];
}

// One contraction step of the groups with more than `step` cores.  A workgroup owns a 16 x 16 tile of (a, b) and up to TTN_MERGE_NX
// consecutive merged indices x = i1 n2 + i2; the bond index m is staged through LDS in chunks of TTN_MERGE_KC.  The loads walk the
// operands' fast index (i1 resp. i2 first, as the cores lie in memory).  The products are collected in LDS in the order of the output
// core (x fastest, then a) and leave as contiguous runs, 16 bytes per lane where the run and its start are even.
__global__ void __launch_bounds__(TTN_MERGE_TB) k_merge_step(MergeArgs M) {
    __shared__ __attribute__((aligned(16))) double sm[(TTN_MERGE_NX + 1) * TTN_MERGE_KC * TTN_MERGE_LD];    // CI + CJ <= NX + 1 panels; later the 256 x NX outputs
    const int g = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const TTDev& X = M.x;
    const TTDev& Z = M.z;
    const int k0 = M.k0[g], cnt = M.count[g], step = M.step;
    if (cnt <= step) return;
    const long long* xr = X.rks + (long long)b * (X.d + 1);
    const int rl = (int)xr[k0], rm = (int)xr[k0 + step], rr = (int)xr[k0 + step + 1];
    const int zs = M.g0 + g;
    if (rl > Z.cap[zs] || xr[k0 + cnt] > Z.cap[zs + 1]) return;               // k_merge_copy has recorded the overflow
    int nA = 1;
    for (int s = 0; s < step; ++s) nA *= X.dims[k0 + s];
    const int n2 = X.dims[k0 + step];
    const long long nout = (long long)nA * n2;
    // chunk of merged indices: CJ values of i2 times CI values of i1 (CI > 1 only when the chunk holds all of i2: the run stays contiguous)
    const int CJ = n2 < TTN_MERGE_NX ? n2 : TTN_MERGE_NX;
    int CI = TTN_MERGE_NX / CJ;
    if (CI > nA) CI = nA;
    const int nci = (nA + CI - 1) / CI, ncj = (n2 + CJ - 1) / CJ;
    const int ta = (rl + 15) >> 4, tb = (rr + 15) >> 4;
    const long long ntile = (long long)nci * ncj * ta * tb;
    if ((long long)blockIdx.x >= ntile) return;
    int t = blockIdx.x;
    const int xc = t % (nci * ncj); t /= nci * ncj;
    const int a0 = (t % ta) << 4, b0 = (t / ta) << 4;
    const int i10 = (xc / ncj) * CI, i20 = (xc % ncj) * CJ;
    const int vi = (nA - i10 < CI) ? nA - i10 : CI, vj = (n2 - i20 < CJ) ? n2 - i20 : CJ;     // valid digits of this chunk
    double* wsp = M.work + (long long)b * M.work_stride + M.work_off[g];
    const double* Pp = (step == 1) ? X.data + (long long)b * X.stride + X.off[k0] : wsp + ((step - 2) & 1) * M.work_half[g];
    const double* Cp = X.data + (long long)b * X.stride + X.off[k0 + step];
    double* Op = (step == cnt - 1) ? Z.data + (long long)b * Z.stride + Z.off[zs] : wsp + ((step - 1) & 1) * M.work_half[g];
    double* As = sm;                                                  // As[(ci KC + kk) LD + a]
    double* Bs = sm + CI * TTN_MERGE_KC * TTN_MERGE_LD;               // Bs[(cj KC + kk) LD + b]
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int npair = CI * CJ;
    mfma_acc_t acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = (mfma_acc_t){0.0, 0.0, 0.0, 0.0};
    for (int m0 = 0; m0 < rm; m0 += TTN_MERGE_KC) {
        __syncthreads();
        for (int e = tid; e < CI * 16 * TTN_MERGE_KC; e += TTN_MERGE_TB) {
            const int ci = e % CI, a = (e / CI) & 15, kk = e / (CI * 16);
            const bool ok = ci < vi && a0 + a < rl && m0 + kk < rm;
            As[(ci * TTN_MERGE_KC + kk) * TTN_MERGE_LD + a] = ok ? Pp[(i10 + ci) + (long long)nA * ((a0 + a) + (long long)rl * (m0 + kk))] : 0.0;
        }
        for (int e = tid; e < CJ * TTN_MERGE_KC * 16; e += TTN_MERGE_TB) {
            const int cj = e % CJ, kk = (e / CJ) % TTN_MERGE_KC, bb = e / (CJ * TTN_MERGE_KC);
            const bool ok = cj < vj && m0 + kk < rm && b0 + bb < rr;
            Bs[(cj * TTN_MERGE_KC + kk) * TTN_MERGE_LD + bb] = ok ? Cp[(i20 + cj) + (long long)n2 * ((m0 + kk) + (long long)rm * (b0 + bb))] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = wave + 4 * u;
            if (p < npair) {                                          // wave-uniform
                const double* ap = As + ((p / CJ) * TTN_MERGE_KC + lk) * TTN_MERGE_LD + li;
                const double* bp = Bs + ((p % CJ) * TTN_MERGE_KC + lk) * TTN_MERGE_LD + li;
#pragma unroll
                for (int ks = 0; ks < TTN_MERGE_KC / 4; ++ks)
                    acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * ks * TTN_MERGE_LD], bp[4 * ks * TTN_MERGE_LD], acc[u], 0, 0, 0);
            }
        }
    }
    __syncthreads();
    // Os[(bb 16 + a) npair + p]: the order of the output core inside the tile
    double* Os = sm;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int p = wave + 4 * u;
        if (p < npair) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) Os[(li * 16 + lk + 4 * reg) * npair + p] = acc[u][reg];
        }
    }
    __syncthreads();
    const int nxv = (CJ == n2) ? vi * CJ : vj;                        // valid, contiguous merged indices of the chunk
    const long long x0 = (long long)i10 * n2 + i20;
    const bool vec2 = ((npair | nxv) & 1) == 0 && ((x0 | nout) & 1) == 0 && ((reinterpret_cast<uintptr_t>(Op) & 15) == 0);
    if (vec2) {
        const int hp = npair >> 1;
        for (int e = tid; e < 256 * hp; e += TTN_MERGE_TB) {
            const int p = (e % hp) << 1, a = (e / hp) & 15, bb = e / (hp * 16);
            if (p < nxv && a0 + a < rl && b0 + bb < rr) {
                const double2 v = *reinterpret_cast<const double2*>(Os + (bb * 16 + a) * npair + p);
                *reinterpret_cast<double2*>(Op + x0 + p + nout * ((a0 + a) + (long long)rl * (b0 + bb))) = v;
            }
        }
    } else {
        for (int e = tid; e < 256 * npair; e += TTN_MERGE_TB) {
            const int p = e % npair, a = (e / npair) & 15, bb = e / (npair * 16);
            if (p < nxv && a0 + a < rl && b0 + bb < rr) Op[x0 + p + nout * ((a0 + a) + (long long)rl * (b0 + bb))] = Os[(bb * 16 + a) * npair + p];
        }
    }
}
