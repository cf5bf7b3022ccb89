/*
 * ttn_measure.h — site-resolved measurements on resident batches, of libttn_hip.so: the magnetisation profile <Z_k> and the two-point
 * functions <Z_i Z_j>, <S+_i S-_j> of every train for ALL pairs, in O(d) chain work plus O(d^2) short walks (DESIGN.md 4.28,
 * csrc/ttn_measure_kernels.h) instead of one product operator and one ttn_sandwich per pair.
 * Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.  Float64 only; the bra and
 * the ket are the same train.
 *
 * An operator TABLE is one real n_k x n_k matrix per site, the matrices concatenated: S = sum_k n_k^2 doubles, site k at offset
 * sum_{m < k} n_m^2, column-major.  With x a train of the batch,
 *     E_O[k]     = sum x[.. z_k ..] O_k[z_k, z'_k] x[.. z'_k ..] / <x, x>        (the first index of O_k meets the bra, the second the ket,
 *                                                                                as the output / input index of A in ttn_sandwich)
 *     C_PQ[i, j] = <x| P_i Q_j |x> / <x, x>                                      (the diagonal is E_{P Q}[i], the matrix product on one site;
 *                                                                                for i != j the two act on different sites and commute)
 * x is real, so E_O sees only the symmetric part of O.  A correlator sees antisymmetric factors: P = Q = [[0, 1], [-1, 0]] (= i sigma_y)
 * gives -<sigma_y sigma_y>, which is how a Float64 caller obtains YY correlations.  C_PQ is in general not symmetric when P != Q.
 * normalize == 0 leaves the division out.  A zero train with normalize != 0 gives the IEEE 0 / 0 (NaN); it is not treated specially.
 *
 * Every check runs before any launch:
 *   TTN_ERR_ARG          a null pointer; nops < 1 or nops > TTN_MEASURE_MAX_OPS
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle; a chain longer than 480 sites; a train, or the workspace of one train, of 2^31 doubles or more
 * The number of trains is never a reason to refuse: a batch is processed in chunks of at most 65535 trains (the launch limit of the
 * core-gradient kernels these calls share) whose library workspace stays within TTN_MEASURE_CHUNK_BYTES, or is that of ONE train
 * where a single train needs more.  Per train the workspace is, with r = max_m r_m, W = r^2 and N = max_k n_k r^2 (both rounded up to
 * even), T = nops and p = 0 for ttn_site_expect, T = 3 and p = 2 for ttn_correlation (T = 2 and p = 1 when P and Q are bitwise equal):
 *     2 (d + 1) W + 2 N                     both environment chains (ttn_dot_pullback's)
 *   + T d W                                 the states V^O_k
 *   + max(T d, p (d - 1)) (2 N + 2 W)       only when a site can lie outside n_k = 2, ranks <= 64: the general route's workgroups
 * doubles.  Results are reproducible to rounding, not bitwise (the on-chip transfer step adds with LDS atomics).
 */
#ifndef TTN_MEASURE_H
#define TTN_MEASURE_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

#define TTN_MEASURE_MAX_OPS 16
#define TTN_MEASURE_CHUNK_BYTES 1073741824      /* 1 GiB: the workspace bound of one chunk of trains */

/* out[k + d (t + nops b)] = E_{O^t}[k] of train b for the `nops` tables that `ops` holds back to back (host, nops * S doubles): all
 * tables share one pair of environment chains.  `out` is a host array of d * nops * batch doubles; the call synchronises. */
int ttn_site_expect(ttn_tt_t x, int64_t nops, const double* ops, int64_t normalize, double* out);

/* The same into DEVICE memory, asynchronously on the library stream (`ops` is still a host array; it is copied before the call
 * returns). */
int ttn_site_expect_dev(ttn_tt_t x, int64_t nops, const double* ops, int64_t normalize, double* d_out);

/* out[i + d (j + d b)] = C_PQ[i, j] of train b; P and Q are host tables (S doubles each; they may be the same array).  When the two
 * tables are bitwise equal the lower triangle is the mirrored upper one and only one pass of walks runs.  `out` is a host array of
 * d * d * batch doubles; the call synchronises. */
int ttn_correlation(ttn_tt_t x, const double* P, const double* Q, int64_t normalize, double* out);

/* The same into DEVICE memory, asynchronously on the library stream. */
int ttn_correlation_dev(ttn_tt_t x, const double* P, const double* Q, int64_t normalize, double* d_out);

#ifdef __cplusplus
}
#endif
#endif /* TTN_MEASURE_H */
