/*
 * ttn_zmeasure.h — site-resolved measurements on resident batches of ComplexF64 trains, of libttn_hip.so: the profile <sigma^mu_k> and
 * the two-point functions <P_i Q_j> of every train for ALL pairs, in O(d) chain work plus O(d^2) short walks (DESIGN.md 4.36,
 * csrc/ttn_zmeasure_kernels.h) instead of one product operator and one ttn_braket per site or per pair.  The complex twin of
 * ttn_measure.h, under new names: ttn_site_expect / ttn_correlation stay Float64 only.
 * Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.  ComplexF64 only; the bra
 * and the ket are the same train, the bra conjugated.
 *
 * An operator TABLE is one complex n_k x n_k matrix per site, the matrices concatenated, interleaved (re, im): 2 S doubles with
 * S = sum_k n_k^2, site k at offset 2 sum_{m < k} n_m^2, column-major.  With x a train of the batch,
 *     E_O[k]     = sum conj(x[.. z_k ..]) O_k[z_k, z'_k] x[.. z'_k ..] / <x|x>   (the first index of O_k meets the conjugated bra, the
 *                                                                                second the ket, as the output / input index of A in
 *                                                                                ttn_braket)
 *     C_PQ[i, j] = <x| P_i Q_j |x> / <x|x>                                       (the diagonal is E_{P Q}[i], the matrix product on one
 *                                                                                site; for i != j the two act on different sites and commute)
 * Results are complex, interleaved (re, im).  A lone sigma_y is measured as it stands.  C_PQ is in general neither symmetric nor
 * Hermitian when P != Q.  normalize == 0 leaves the division by re <x|x> out.  A zero train with normalize != 0 gives the IEEE 0 / 0
 * (NaN); it is not treated specially.
 *
 * Every check runs before any launch:
 *   TTN_ERR_ARG          a null pointer; nops < 1 or nops > TTN_ZMEASURE_MAX_OPS
 *   TTN_ERR_UNSUPPORTED  a Float64 handle (ttn_site_expect / ttn_correlation measure those); a chain longer than 480 sites; a train, or
 *                        the workspace of one train, of 2^31 doubles or more
 * The number of trains is never a reason to refuse: a batch is processed in chunks of at most 65535 trains whose library workspace
 * stays within TTN_ZMEASURE_CHUNK_BYTES, or is that of ONE train where a single train needs more.
 *
 * Routes, one per train: a train whose ranks are all <= 64, in a handle whose n_k are all 2, runs on chip (fp64 MFMA on split re / im
 * fragments, the states as two dense 64 x 64 planes in workspace); any other train runs the general route (workgroup GEMMs on
 * stride-2 views, the states r x r interleaved).  Per train the workspace is, with r = max_m r_m (the handle's bounds), n = max_k n_k,
 *     W = max(8192 if every n_k = 2, 2 r^2 if a train can lie outside the on-chip class)      one state
 *     N = 2 n r^2                                                                              one core-sized intermediate
 * and T = nops, p = 0 for ttn_zsite_expect, T = 3, p = 2 for ttn_zcorrelation (T = 2, p = 1 when P and Q are bitwise equal):
 *     2 (d + 1) W                             both environment chains, every state kept
 *   + T d W                                   the states V^O_k
 *   + 2 p (d - 1) W                           the two states every walk alternates between
 *   + 2 N + max(T d, p (d - 1)) 2 N           only when a train can lie outside the on-chip class: the general route's intermediates
 * doubles.  Results are reproducible to rounding, not bitwise (the on-chip site step adds with LDS atomics).
 */
#ifndef TTN_ZMEASURE_H
#define TTN_ZMEASURE_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

#define TTN_ZMEASURE_MAX_OPS 16
#define TTN_ZMEASURE_CHUNK_BYTES 1073741824      /* 1 GiB: the workspace bound of one chunk of trains */

/* out[2 (k + d (t + nops b))] (re, then im) = E_{O^t}[k] of train b for the `nops` tables that `ops` holds back to back (host,
 * nops * 2 S doubles): all tables share one pair of environment chains.  `out` is a host array of 2 * d * nops * batch doubles; the
 * call synchronises. */
int ttn_zsite_expect(ttn_tt_t x, int64_t nops, const double* ops, int64_t normalize, double* out);

/* The same into DEVICE memory, asynchronously on the library stream (`ops` is still a host array; it is copied before the call
 * returns). */
int ttn_zsite_expect_dev(ttn_tt_t x, int64_t nops, const double* ops, int64_t normalize, double* d_out);

/* out[2 (i + d (j + d b))] (re, then im) = C_PQ[i, j] of train b; P and Q are host tables (2 S doubles each; they may be the same
 * array).  When the two tables are bitwise equal only one pass of walks runs and the lower triangle is the plain copy of the upper one
 * (no conjugate: for i != j the two factors commute).  `out` is a host array of 2 * d * d * batch doubles; the call synchronises. */
int ttn_zcorrelation(ttn_tt_t x, const double* P, const double* Q, int64_t normalize, double* out);

/* The same into DEVICE memory, asynchronously on the library stream. */
int ttn_zcorrelation_dev(ttn_tt_t x, const double* P, const double* Q, int64_t normalize, double* d_out);

#ifdef __cplusplus
}
#endif
#endif /* TTN_ZMEASURE_H */
