/*
 * ttn_contract.h — partial contraction of resident trains, of libttn_hip.so: a subset of the sites of every train of a batch is
 * contracted against weight vectors and the result is a train on the remaining sites (csrc/ttn_contract_kernels.h).
 * With all-ones weights that is a marginal, with unit vectors a slice, with the grid's coordinates a moment: what the PDE examples
 * of the reference compute from the dense array (sum(P, dims = 2), P[:, j], the means and variances).
 * Included by ttn.h; the conventions (column-major arrays, int64_t integers, 1-based sites, return codes) are stated there.  Float64 only.
 *
 * x has d sites, dims n_k and per-train ranks r_0 = 1, r_1, .., r_d = 1; C is the set of contracted sites, a proper subset, and w_k a
 * vector of n_k doubles for every k in C.  With M_k = sum_z w_k[z] X_k[z, :, :] (r_{k-1} x r_k) the result y is the train on the kept
 * sites in their order, with the kept dims:
 *     a run of contracted sites in front of a kept site k (behind the previous kept site p, or from the left end) is multiplied into k
 *     from the left:               Y_k[z] = (M_{p+1} ... M_{k-1}) X_k[z]
 *     the run behind the LAST kept site is multiplied into it from the right (a chain of matrix-vector products, r_d = 1):
 *                                  Y_k[z] <- Y_k[z] (M_{k+1} ... M_d)
 *     a kept site with no run next to it is copied bit for bit.
 * So y's ranks are 1 at both ends and the bond between consecutive kept sites p < k carries x's rank at the right of p.  y's gauge flags
 * are zeros; its ranks are written per train on the device.  No atomics anywhere: two identical calls give identical bits, and train b
 * of a batch gives the bits of the same call on that train alone (handles of the same dims and capacities).
 *
 * Library workspace, doubles per train, with r = max_m (x's host-side rank bound), n = max_k n_k, v = 4 r + n r (rounded up to even):
 *     v   for the first kept site when a run from the left end stands in front of it (a chain of vector-matrix products),
 *   + v   for the last kept site when a run stands behind it and none, or the one from the left end, in front of it,
 *   + (3 r^2 + 2 r + n r, rounded up to even) per kept site with a run behind another kept site in front of it — only on the general
 *         route (a site with n_k != 2 or a rank capacity of x above 64); the on-chip route keeps those products in LDS.
 * The number of trains is never a reason to refuse: a batch is processed in chunks of at most 65535 trains whose workspace stays within
 * TTN_CONTRACT_CHUNK_BYTES, or is that of ONE train where a single train needs more.
 */
#ifndef TTN_CONTRACT_H
#define TTN_CONTRACT_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

#define TTN_CONTRACT_CHUNK_BYTES 1073741824      /* 1 GiB: the workspace bound of one chunk of trains */

/* y <- x with the `ncontract` sites `sites` (1-based, strictly increasing) contracted, asynchronously on the library stream.
 * `weights` is a host array of wbatch * S doubles, S = sum_{k in C} n_k: the vectors w_k back to back in the order of `sites`, one such
 * table for all trains (wbatch == 1) or one per train (wbatch == batch, table b at weights + b S); it is copied before the call
 * returns.  y is created by the caller with the kept dims and a rank capacity (the ttn_tt_kron convention) and x's batch.
 * Every check runs before y is touched:
 *   TTN_ERR_ARG          a null handle or pointer; y == x; ncontract < 1; a site out of 1..d, repeated or unsorted; no kept site
 *                        (ncontract == d: that is ttn_dot with the rank-1 train of the weights); wbatch neither 1 nor the batch
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle; a core (slot) of x or y of 2^31 doubles or more (32-bit element indices)
 *   TTN_ERR_DIMS         y's number of sites, dims or batch; an end rank of x whose host-side bound is not 1
 *   TTN_ERR_CAPACITY     y's capacity at a bond below x's host-side rank bound there (the bond left of kept site k carries the bound of
 *                        x's bond left of the run in front of k) */
int ttn_tt_contract_sites(ttn_tt_t x, int64_t ncontract, const int64_t* sites, int64_t wbatch, const double* weights, ttn_tt_t y);

#ifdef __cplusplus
}
#endif
#endif /* TTN_CONTRACT_H */
