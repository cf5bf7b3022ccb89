/*
 * ttn_expect.h — <x, A y> on resident batches without forming A y, of libttn_hip.so: the scalar behind the reference's
 * real(dot(psi, H * psi)) / real(dot(psi, psi)) (examples/Schrodinger_groundstate.jl, ising_model.jl, variational_solver.jl, ...).
 * Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.  Float64 only.
 */
#ifndef TTN_EXPECT_H
#define TTN_EXPECT_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t, ttn_tto_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

/* The limits of the on-chip route of the kernel (csrc/ttn_expect_kernels.h): every n_k = 2, every rank of both trains
 * <= TTN_EXPECT_QTT_MAX_RANK, every rank of the operator <= TTN_EXPECT_QTT_MAX_OP_RANK.  A train outside them takes the general route
 * (workgroup GEMMs, state in library workspace): the same number, more memory traffic.  Nothing is refused because of them. */
#define TTN_EXPECT_QTT_MAX_RANK 64
#define TTN_EXPECT_QTT_MAX_OP_RANK 5

/* out[b] = <x_b, A y_b> = sum_{i, j} x_b[i] A[i, j] y_b[j] for every train b: one sweep over the three cores of every site, one
 * workgroup per train.  A's first physical index is the output index, as ttn_apply reads it, and the result is what
 * ttn_dot(x, ttn_apply(A, y)) returns up to the order of the rounding errors.  x and y may be the same handle; one operator serves the
 * whole batch; ragged ranks inside a batch are read from the per-train rank words.  `out` is a host array of `batch` doubles;
 * the call synchronises, as ttn_dot does.  Every check runs before any launch:
 *   TTN_ERR_ARG          a null pointer
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle; a chain longer than 480 sites; a train or an operator of 2^31 doubles or more; ranks
 *                        whose three-layer state r_x R r_y (times 2 + 2 max n_k, the workspace of one train) reaches 2^31 doubles
 *   TTN_ERR_DIMS         "Incompatible dimensions" when the dims of x, A and y differ; "batch sizes differ" */
int ttn_sandwich(ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, double* out);

/* The same into DEVICE memory (`batch` doubles), asynchronously on the library stream: nothing crosses to the host. */
int ttn_sandwich_dev(ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, double* d_out);

#ifdef __cplusplus
}
#endif
#endif /* TTN_EXPECT_H */
