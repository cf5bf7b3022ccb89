/*
 * ttn_expect_grad.h — the pullback of <x, A y> on resident batches without forming A y, of libttn_hip.so: the gradient behind the
 * reference's Rayleigh-quotient descent on fixed-rank cores (test/test_ad.jl, examples/manopt_ttvector_gradient_descent.jl,
 * optimize_methods.jl, variational_solver.jl).  Included by ttn.h; the conventions are stated there and in ttn_expect.h.  Float64 only.
 */
#ifndef TTN_EXPECT_GRAD_H
#define TTN_EXPECT_GRAD_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t, ttn_tto_t (ttn.h includes this file at its end: either order works) */
#include "ttn_expect.h"   /* TTN_EXPECT_QTT_MAX_RANK, TTN_EXPECT_QTT_MAX_OP_RANK: the on-chip class is the one of ttn_sandwich */

#ifdef __cplusplus
extern "C" {
#endif

/* The pullback of s_b = <x_b, A y_b> for a cotangent delta_b per train, on the three-layer environments — A y, a train of ranks R r or
 * a cotangent of that size never exist (csrc/ttn_expect_grad_kernels.h):
 *     xbar_k[i, al, a] = delta_b sum L_k[al, rl, bl] A_k[i, j, rl, rho] y_k[j, bl, b] G_{k+1}[a, rho, b],      ybar_k likewise,
 * L and G the left and right environments of <x, A y>, each computed once per call.  The conventions of ttn_dot_pullback: `delta` is a
 * HOST array of `batch` doubles (NULL: 1); xbar / ybar may each be NULL (not both) and receive the current ranks of x / y per train
 * (copied on the device), gauge flags 0; `out` is HOST or NULL — non-NULL: it receives s_b (not scaled by delta) and the call
 * synchronises; out and delta both NULL: the call is asynchronous.  x and y may be the same handle (both tangents are still computed
 * separately); the operands are only read.  A train of the on-chip class (every n_k = 2, ranks <= TTN_EXPECT_QTT_MAX_RANK, operator
 * ranks <= TTN_EXPECT_QTT_MAX_OP_RANK) keeps every intermediate of a gradient in registers and LDS; any other train runs workgroup GEMMs.
 * Workspace per train, in doubles, with W = max_m rx_m R_m ry_m (rounded up to even), S = max rx * max R * max ry (host-side bounds):
 *     2 (d + 1) W  +  2 max(2 nmax S, 4096 max R on the on-chip class)  +  4 d nmax S
 * the last term absent when the bounds put every train in the on-chip class, and one 32-bit route word per train.  Boundary ranks
 * above 1 (a segment of a train) are taken at the [1, 1, 1] entry, as ttn_sandwich takes them.  Every check runs before any launch, nothing is written:
 *   TTN_ERR_ARG          null x / A / y; both tangents NULL; a tangent that is x, y or the other tangent
 *   TTN_ERR_DIMS         "Incompatible dimensions" when the dims of x, A and y (and the tangents) differ; "batch sizes differ"
 *   TTN_ERR_CAPACITY     a tangent's capacity below its source's host-side rank bounds
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle; the limits of ttn_sandwich (480 sites, 2^31 doubles); more than 65535 trains
 * and the allocator's error when the workspace cannot be had. */
int ttn_sandwich_pullback(ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, const double* delta, ttn_tt_t xbar, ttn_tt_t ybar, double* out);

#ifdef __cplusplus
}
#endif
#endif /* TTN_EXPECT_GRAD_H */
