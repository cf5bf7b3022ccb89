/*
 * ttn_dense.h — the dense bridge for TT operators of libttn_hip.so: operator -> dense array and dense array -> operator, on the device.
 * Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.  Float64 only.
 *
 * Replaces tto_to_tensor (src/tt_tools.jl:375-392), qtto_to_matrix (src/qtt_tools.jl:180-188) and tto_decomp (src/tt_tools.jl:338-362).
 *
 * Both calls address the dense array through two stride tables of d entries each:
 *     address(x_1..x_d ; y_1..y_d) = sum_k (x_k - 1) xstrides[k] + (y_k - 1) ystrides[k]
 * over N^2 doubles, N = prod(n_k).  The 2 d (stride, n) pairs ("digits") sorted by stride must form a mixed-radix system: the
 * smallest stride is 1, each next one is the previous stride times that digit's n; digits with n = 1 are ignored.  That makes the map
 * a bijection onto [0, N^2).  Both tables NULL: the reference's tto_to_tensor array, Julia column-major over [x_1..x_d, y_1..y_d],
 *     xstrides[k] = prod_{j<k} n_j      ystrides[k] = N prod_{j<k} n_j.
 * qtto_to_matrix's matrix (column-major N x N, row and column with site 1 most significant) is
 *     xstrides[k] = prod_{j>k} n_j      ystrides[k] = N prod_{j>k} n_j.
 */
#ifndef TTN_DENSE_H
#define TTN_DENSE_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tto_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

/* d_out[address(x ; y)] = A(x_1..x_d ; y_1..y_d); d_out is DEVICE memory of N^2 doubles.  The operator is read in place as a train on
 * n_k^2 sites and goes through the kernels of ttn_tt_to_dense (cut, two chains, out = L R by fp64 MFMA, stores in output-address
 * order); an operator site carries two digits, so a tile may split a site between its x and its y.  Asynchronous on the library's
 * stream.  Refused before any launch, with a message that names the call:
 *   TTN_ERR_ARG          A or d_out null; only one of the two tables given; digits that are not a mixed-radix system
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 operator; more than 2^27 entries; an n_k above 4096; more than 64 sites; end ranks other than 1 */
int ttn_tto_to_dense(ttn_tto_t A, const int64_t* xstrides, const int64_t* ystrides, double* d_out);

/* tto_decomp(tensor; index) with ttv_decomp's absolute threshold exposed (the reference always uses 1e-12): d_tensor is DEVICE memory
 * of N^2 doubles addressed as above (both tables NULL: the reference's [x.., y..] array) and is only read.  A gather kernel permutes
 * it into the array (n_1^2, ..., n_d^2) with merged index x_k + n_k (y_k - 1), the hierarchical SVD of ttn_ttv_decomp_dev runs on a
 * working train of rank capacity min(prod_{j<=k} n_j^2, prod_{j>k} n_j^2, rank_cap), and *out receives the operator with the gauge
 * flags -1 / 0 / +1 around `index`.  Synchronises.
 *   TTN_ERR_ARG          a null pointer; d outside 1..64; a dimension below 1; index outside 1..d; only one table given; digits that
 *                        are not a mixed-radix system; tol < 0 (or NaN); rank_cap < 1
 *   TTN_ERR_UNSUPPORTED  more than 2^27 entries; an n_k above 4096; an unfolding with a short side above 4096 (lower rank_cap)
 *   TTN_ERR_CAPACITY     a rank above rank_cap (found on the device, reported by this call; no operator is returned) */
int ttn_tto_decomp_dev(int64_t d, const int64_t* dims, const double* d_tensor, const int64_t* xstrides, const int64_t* ystrides,
                       int64_t index, double tol, int64_t rank_cap, ttn_tto_t* out);

/* What the host chose for the last launch, for diagnostics (tools/diag_dense_operator.py): out3 = {cut m (sites 0..m-1 form L), TM, TN}
 * of the last ttn_tt_to_dense / ttn_tto_to_dense — a tile is TM rows of L x TN columns of R, computed in 16 x 16 MFMA blocks, so a side
 * below 16 leaves padded blocks —; out4 = {TI, TO, ld, RO} of the gather of the last ttn_tto_decomp_dev.  TTN_ERR_ARG before any such
 * launch.  The environment variable TTN_GATHER_PAD = 0..32 replaces the gather's searched LDS pad by a fixed one (diagnostic only). */
int ttn_debug_dense_plan(int64_t* out3);
int ttn_debug_gather_plan(int64_t* out4);

#ifdef __cplusplus
}
#endif
#endif /* TTN_DENSE_H */
