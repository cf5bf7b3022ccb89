/*
 * ttn_step.h — what a time step does around its linear solve, of libttn_hip.so: the fused update z = alpha x + beta (A y) and the
 * public increase_ranks.  Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.
 *
 * ttn_apply_axpby serves the steppers of src/solvers/euler.jl: the Crank-Nicolson right-hand side (I + (h/2) A) u (:162), the explicit
 * Euler update u + h (A u) (:81-82) and the residuals of the return_error branches (:91, :137, :185) are all alpha x + beta (A y).
 * ttn_tt_increase_ranks is increase_ranks(x, max_bond; rks, noise), src/tt_tools.jl:443-489.  Float64 only.
 */
#ifndef TTN_STEP_H
#define TTN_STEP_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t, ttn_tto_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

/* z_b = alpha[b] x_b + beta[b] (A y_b) for every train b, in one streaming launch, asynchronously.  alpha and beta are host arrays of
 * `batch` doubles; NULL means 1 (the convention of ttn_scale_batch).  The result is, bit for bit, what the composition
 *     ttn_apply(A, y, t); ttn_scale_batch(beta, t, t2); ttn_scale_batch(alpha, x, x2); ttn_add(x2, t2, z)
 * leaves in z:
 *     ranks        z.rks[m] = x.rks[m] + A.rks[m] * y.rks[m], both ends 1; gauge flags zeros
 *     cores        first [X~_1, Y~_1], middle diag(X~_k, Y~_k) with the off-diagonal blocks written as zeros, last [X~_d; Y~_d]
 *     Y~_k[i, a' + R_l v', a + R_r v] = sum_j A_k[i, j, a', a] Y_k[j, v', v], accumulated as ttn_apply accumulates it
 *                  (acc = A[i,0] y_0, then one fma per j >= 1) and rounded once; core 1 is then multiplied by beta[b]
 *     X~_k = X_k,  multiplied by alpha[b] in the core ttn_scale_batch scales: the first with gauge flag 0, else core 1
 *     a zero factor writes an all-zero block in every core
 * x == y is allowed.  d >= 2, as ttn_add.  Every check runs before z is touched:
 *   TTN_ERR_ARG          a null handle; z == x or z == y
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle; d == 1; a core of 2^31 fibres or more (32-bit element indices, as ttn_apply)
 *   TTN_ERR_DIMS         dimensions or batch sizes that differ
 *   TTN_ERR_CAPACITY     z's capacity below x's host-side rank bound + A.rks * y's at some bond */
int ttn_apply_axpby(const double* alpha, ttn_tt_t x, const double* beta, ttn_tto_t A, ttn_tt_t y, ttn_tt_t z);

/* y_b = x_b zero-padded to the ranks new_rks (d + 1 entries, both ends 1) for every train; with noise != 0 the new blocks receive
 * noise * Q as increase_ranks_noise places them, Q orthonormal from the seeded splitmix64 stream ttn_als_eigsolve uses (keyed by seed,
 * site and entry, not by the train).  y's gauge flags are zeros.  Synchronises (the current ranks of x are read back for the check).
 *   TTN_ERR_ARG          a null pointer; y == x; an end rank that is not 1; a new rank below a current rank of any train; noise not finite
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle; with noise != 0 a new rank above 1024 or a core above 65 536 entries
 *   TTN_ERR_DIMS         dimensions or batch sizes that differ
 *   TTN_ERR_CAPACITY     a new rank above y's capacity */
int ttn_tt_increase_ranks(ttn_tt_t x, const int64_t* new_rks, double noise, uint64_t seed, ttn_tt_t y);

#ifdef __cplusplus
}
#endif
#endif /* TTN_STEP_H */
