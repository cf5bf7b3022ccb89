// ttn_opbatch_kernels.h — operator batches (include/ttn_opbatch.h): B operators of equal dims and ranks in one handle,
// operator b, core k at data + b * stride + off[k] (TTODev::stride; 0 for a single operator).  The kernels that read an operator per
// train only add train * stride where they form the operator pointer (k_apply, k_apply_axpby, k_expect, the three kernels of
// ttn_sandwich_pullback, k_two_site_eig through AC); this file holds the one kernel of its own, the packing of a batch of trains.
#pragma once
#include "ttn_common.h"
#include "ttn_stream_kernels.h"

// ttn_tto_from_tt_batch: grid (tiles, d, B).  Train b of x (dims n_k^2, slots laid out by the CAPACITY ranks, every core compact at the
// start of its slot) into operator b of A (slots laid out by the common ranks A.rks): the core (n^2, r_l, r_r) is byte for byte the
// operator core (n, n, r_l, r_r), so this is a copy of n^2 r_l r_r doubles between two 16-byte aligned slots — 16 bytes per lane, and
// one scalar element behind them when the count is odd.  The host has checked that every train holds the ranks A.rks.
__global__ void __launch_bounds__(TTN_STREAM_TB) k_tto_pack(TTDev x, TTODev A, double* out) {
    typedef double d2v_t __attribute__((ext_vector_type(2)));
    const int k = blockIdx.y, b = blockIdx.z;
    const long long total = (long long)x.dims[k] * A.rks[k] * A.rks[k + 1];
    const double* Xk = x.data + (long long)b * x.stride + x.off[k];
    double* Ok = out + (long long)b * A.stride + A.off[k];
    const long long t2 = total >> 1;
    const d2v_t* X2 = reinterpret_cast<const d2v_t*>(Xk);
    d2v_t* O2 = reinterpret_cast<d2v_t*>(Ok);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < t2; e += (long long)gridDim.x * blockDim.x) O2[e] = X2[e];
    if ((total & 1) && blockIdx.x == 0 && threadIdx.x == 0) Ok[total - 1] = Xk[total - 1];
}
