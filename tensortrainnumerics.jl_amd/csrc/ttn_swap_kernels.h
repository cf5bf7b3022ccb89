// ttn_swap_kernels.h — site-swap chains: programs of two-site swap SVDs and site-wise contractions on one train per workgroup.
//
// Provides: ChainArgs, k_swap_chain.
// Needs: ttn_dense_kernels.h (CompressArgs, BondIO, wg_bond_step_io<1>) and through it wg_gemm and the uniform pins.
// Used by: the translation units only (ttn_api.hip launches it for hadamard_ttm and the QTT reorder).
#pragma once
#include "ttn_dense_kernels.h"

// -------------------------------------------------------------------------------------------------
// Site-swap chains: hadamard_ttm (src/tt_operations.jl:398-422) and QTT reorder (src/qtt_tools.jl:733-775).
// Both are sequences of two-site swap SVDs (wg_bond_step_io<1>) on a chain of cores with one physical dimension n; the TTM
// Hadamard product additionally contracts neighbours site-wise (_ttm_contract!, :384-396), which shortens the chain.  One
// workgroup owns one train for the whole program; the host turns the reference's loops into a list of (type, slotA, slotB)
// ops on fixed storage slots, so a deleted core is simply a slot no later op names.
// -------------------------------------------------------------------------------------------------
struct ChainArgs {
    CompressArgs C;              // tolerance / rank rule / scratch / status (C.tt = the handle for kind 2)
    int kind;                    // 1: hadamard_ttm (slots in `arena`, x and y copied in, result copied to z); 2: reorder in place
    int n, nslots, nops, d;
    const int* ops;              // device [nops][3]: type (0 swap, 1 contract), slotA, slotB
    const int* final_slots;      // device [d] (kind 1): slots of the final chain, left to right
    double* arena;               // kind 1: per train nslots * slot_doubles
    long long arena_stride, slot_doubles;
    int cap;                     // kind 1: rank capacity of every slot
    long long* srk;              // per train [2*nslots + 2]: left ranks, right ranks, new-rank word
    long long srk_stride;
    TTDev x, y, z;               // kind 1
};

__global__ void TTN_KERNEL_BOUNDS k_swap_chain(ChainArgs Q) {
    extern __shared__ double lds[];
    const CompressArgs& P = Q.C;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = Q.n, ns = Q.nslots;
    long long* srl = Q.srk + (long long)b * Q.srk_stride;
    long long* srr = srl + ns;
    long long* rword = srr + ns;
    if (tid == 0) P.sweep_stats[b] = 0;
    __syncthreads();
    // ---- set-up ----
    if (Q.kind == 1) {
        const int d = Q.d;
        const long long* xr = Q.x.rks + (long long)b * (d + 1);
        const long long* yr = Q.y.rks + (long long)b * (d + 1);
        for (int k = 0; k < d; ++k) {
            const int rl = uni32((int)xr[k]), rr = uni32((int)xr[k + 1]);
            const double* src = Q.x.data + (long long)b * Q.x.stride + Q.x.off[k];
            double* dst = Q.arena + (long long)b * Q.arena_stride + (long long)k * Q.slot_doubles;
            for (int e = tid; e < n * rl * rr; e += TTN_WG) dst[e] = src[e];
            if (tid == 0) { srl[k] = rl; srr[k] = rr; }
        }
        for (int k = 0; k < d; ++k) {                          // slot d + k <- permutedims(y[d-1-k], (1,3,2))   (tt_operations.jl:411)
            const int ky = d - 1 - k;
            const int rl = uni32((int)yr[ky]), rr = uni32((int)yr[ky + 1]);
            const double* src = Q.y.data + (long long)b * Q.y.stride + Q.y.off[ky];
            double* dst = Q.arena + (long long)b * Q.arena_stride + (long long)(d + k) * Q.slot_doubles;
            for (int e = tid; e < n * rl * rr; e += TTN_WG) {
                const int s_ = e % n, t = e / n, a = t % rl, c = t / rl;
                dst[s_ + n * (c + (long long)rr * a)] = src[e];
            }
            if (tid == 0) { srl[d + k] = rr; srr[d + k] = rl; }
        }
    } else {
        const long long* rks = P.tt.rks + (long long)b * (P.tt.d + 1);
        for (int k = tid; k < ns; k += TTN_WG) { srl[k] = rks[k]; srr[k] = rks[k + 1]; }
    }
    __syncthreads();
    // ---- the program ----
    bool alive = true;
    for (int o = 0; o < Q.nops; ++o) {
        if (!alive) break;
        const int type = Q.ops[3 * o], sA = Q.ops[3 * o + 1], sB = Q.ops[3 * o + 2];
        double* cA = (Q.kind == 1) ? Q.arena + (long long)b * Q.arena_stride + (long long)sA * Q.slot_doubles
                                   : P.tt.data + (long long)b * P.tt.stride + P.tt.off[sA];
        double* cB = (Q.kind == 1) ? Q.arena + (long long)b * Q.arena_stride + (long long)sB * Q.slot_doubles
                                   : P.tt.data + (long long)b * P.tt.stride + P.tt.off[sB];
        const int rL = uni32((int)srl[sA]), rM = uni32((int)srr[sA]), rR = uni32((int)srr[sB]);
        if (type == 0) {
            BondIO io;
            io.ck = cA; io.ck1 = cB;
            io.n1 = n; io.n2 = n; io.Dl = rL; io.rm = rM; io.Dr = rR;
            io.rank_out = rword;
            io.cap = (Q.kind == 1) ? Q.cap : uni32((int)P.tt.cap[sB]);
            wg_bond_step_io<1>(P, b, io, sA, o, lds, false);
            const int r = uni32((int)*rword);
            if (r < 0) alive = false;
            else if (tid == 0) { srr[sA] = r; srl[sB] = r; }
            __syncthreads();
        } else {
            // Pi[s] = A[s] * B[s]   (rL x rM)(rM x rR) for every physical index s; the product replaces A's slot
            double* tmp = P.scratch + (long long)b * P.scratch_stride;
            for (int s_ = 0; s_ < n; ++s_) {
                const View Av = mkview(cA + s_, plain(n), plain((long long)n * rL));
                const View Bv = mkview(cB + s_, plain(n), plain((long long)n * rM));
                const View Cv = mkview(tmp + s_, plain(n), plain((long long)n * rL));
                wg_gemm(rL, rR, rM, Av, Bv, Cv, 1.0, 0.0, lds);
            }
            __syncthreads();
            for (int e = tid; e < n * rL * rR; e += TTN_WG) cA[e] = tmp[e];
            if (tid == 0) srr[sA] = rR;
            __syncthreads();
        }
    }
    // ---- results ----
    if (Q.kind == 1) {
        const int d = Q.d;
        long long* zr = Q.z.rks + (long long)b * (d + 1);
        if (alive) {
            for (int k = 0; k < d; ++k) {
                const int sl = Q.final_slots[k];
                const int rl = uni32((int)srl[sl]), rr = uni32((int)srr[sl]);
                if (rl > Q.z.cap[k] || rr > Q.z.cap[k + 1]) { if (tid == 0) ttn_set_status(&P.status[b], TTN_ST_RANK_OVERFLOW); alive = false; break; }
                const double* src = Q.arena + (long long)b * Q.arena_stride + (long long)sl * Q.slot_doubles;
                double* dst = Q.z.data + (long long)b * Q.z.stride + Q.z.off[k];
                for (int e = tid; e < n * rl * rr; e += TTN_WG) dst[e] = src[e];
                if (tid == 0) { zr[k] = rl; zr[k + 1] = rr; }
            }
        }
    } else if (alive) {
        long long* rks = P.tt.rks + (long long)b * (P.tt.d + 1);
        for (int k = tid; k < ns; k += TTN_WG) rks[k + 1] = srr[k];
    }
}
