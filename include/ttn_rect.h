/*
 * ttn_rect.h — rectangular TT operators of libttn_hip.so: the part of the C ABI that carries its own handle type.
 * Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.
 *
 * Replaces *(A::TToperator{T,M}, v::TTvector{T,N}) with M == N + 1, src/tt_operations.jl:116-148.  A has M sites with cores
 *     operator core k: (n_out_k, n_in_k, R_{k-1}, R_k)      offset i + n_out*(j + n_in*(a + R_{k-1}*b))
 * and exactly one site s with n_in == 1 (the singleton site), which consumes no site of the train; the other sites meet the train's
 * sites in order.  With c(b) = b - [b >= s] (sites 1-based, boundaries 0-based) the input sites left of boundary b:
 *     ranks          y.rks[b] = A.rks[b] * x.rks[c(b)]
 *     regular site   Y_k[i, a' + R_l v', a + R_r v] = sum_j A_k[i, j, a', a] X[j, v', v]        (n_out != n_in allowed)
 *     singleton site Y_s[i, a' + R_l v', a + R_r v] = A_s[i, 1, a', a] [v' == v],  v', v < x.rks[s - 1]: every entry is written,
 *                    the zeros included (the arena is not cleared)
 * and y's gauge flags are zeros.  Float64 only.
 */
#ifndef TTN_RECT_H
#define TTN_RECT_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

/* One rectangular operator in device memory: immutable, ranks known on the host, shared by every train of a batch.  A distinct
 * type: the entry points of ttn.h that take a ttn_tto_t read cores as (n, n, R_l, R_r) and must never see one of these. */
typedef struct ttn_rtto_s* ttn_rtto_t;

/* cores[k] points at out_dims[k]*in_dims[k]*rks[k]*rks[k+1] doubles (host memory, column-major); 1 <= M <= 64.  Any in_dims are
 * accepted here: how many singleton sites there are is checked where the operator is applied, as in the reference. */
int ttn_rtto_create(int64_t M, const int64_t* out_dims, const int64_t* in_dims, const int64_t* rks, const double* const* cores,
                    ttn_rtto_t* out);
int ttn_rtto_free(ttn_rtto_t h);
/* any of the outputs may be NULL: *M the number of sites, out_dims / in_dims M entries each, rks M + 1 */
int ttn_rtto_ranks(ttn_rtto_t h, int64_t* M, int64_t* out_dims, int64_t* in_dims, int64_t* rks);

/* y = A * x on every train of the batch, asynchronously; x has M - 1 sites, y has M sites with A's output dimensions and receives its
 * ranks per train on the device.  Every check runs before y is touched:
 *   TTN_ERR_ARG          a null handle, y == x
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle; a destination core of 2^31 fibres or more (32-bit element indices, as ttn_apply)
 *   TTN_ERR_DIMS         M != N + 1; not exactly one singleton site; input dimensions that are not x's; a right end rank of x that
 *                        is not 1; y's dimensions or batch
 *   TTN_ERR_CAPACITY     y's capacity below A.rks[b] * (x's host-side rank bound at c(b)) at some boundary */
int ttn_apply_rect(ttn_rtto_t A, ttn_tt_t x, ttn_tt_t y);

/* The stateless form for one train, beside ttn_apply_f64: X has M - 1 sites (X_rks: M entries); Y_cores[k] is caller-allocated with
 * out_dims[k] * yr[k] * yr[k+1] doubles, yr[b] = A_rks[b] * X_rks[c(b)]. */
int ttn_apply_rect_f64(int64_t M, const int64_t* out_dims, const int64_t* in_dims,
                       const double* const* A_cores, const int64_t* A_rks,
                       const double* const* X_cores, const int64_t* X_rks,
                       double* const* Y_cores);

#ifdef __cplusplus
}
#endif
#endif /* TTN_RECT_H */
