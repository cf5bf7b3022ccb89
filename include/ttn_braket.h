/*
 * ttn_braket.h — <x| A |y> = sum_{i, j} conj(x_i) A_ij y_j on resident batches without forming A y, of libttn_hip.so: what the
 * reference's dot(psi, H * psi) computes when psi or H is ComplexF64 (a state from real-time tdvp, the QFT, sigma_y).  ttn_sandwich
 * (ttn_expect.h) is the bilinear form on Float64 handles and keeps refusing complex ones; this is the sesquilinear form, for either
 * element type.  Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.
 */
#ifndef TTN_BRAKET_H
#define TTN_BRAKET_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t, ttn_tto_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

/* The limits of the on-chip route of the kernel (csrc/ttn_braket_kernels.h): every n_k = 2, every rank of both trains
 * <= TTN_BRAKET_QTT_MAX_RANK, every rank of the operator <= TTN_BRAKET_QTT_MAX_OP_RANK.  A train outside them takes the general route
 * (workgroup GEMMs on the re / im planes, state in library workspace): the same number, more memory traffic.  Nothing is refused
 * because of them. */
#define TTN_BRAKET_QTT_MAX_RANK 64
#define TTN_BRAKET_QTT_MAX_OP_RANK 2

/* out[2 b], out[2 b + 1] = re, im of <x_b| A |y_b> = sum_{i, j} conj(x_b[i]) A[i, j] y_b[j] for every train b: one sweep over the
 * three cores of every site, one workgroup per train.  A's first physical index is the output index, as ttn_apply reads it, and the
 * result is what ttn_dot(x, ttn_apply(A, y)) returns up to the order of the rounding errors.  x and y share an element type; the
 * operator is Float64 or ComplexF64 on its own, and a Float64 operand is read as it lies (no promoted copy).  With all three Float64
 * the real part is ttn_sandwich's number bit for bit and the imaginary part is +0.0.  x and y may be the same handle; one operator
 * serves the whole batch; ragged ranks inside a batch are read from the per-train rank words.  `out` is a host array of 2 * batch
 * doubles; the call synchronises, as ttn_dot does.  Every check runs before any launch:
 *   TTN_ERR_ARG          a null pointer
 *   TTN_ERR_UNSUPPORTED  x and y of different element types; an operator batch (ttn_opbatch.h); a chain longer than 480 sites; a train
 *                        or an operator of 2^31 doubles or more; ranks whose three-layer state r_x R r_y (times 2 + 2 max n_k, the
 *                        workspace of one train, a complex element counting as two doubles) reaches 2^31 doubles
 *   TTN_ERR_DIMS         "Incompatible dimensions" when the dims of x, A and y differ; "batch sizes differ" */
int ttn_braket(ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, double* out);

/* The same into DEVICE memory (2 * batch doubles), asynchronously on the library stream: nothing crosses to the host. */
int ttn_braket_dev(ttn_tt_t x, ttn_tto_t A, ttn_tt_t y, double* d_out);

#ifdef __cplusplus
}
#endif
#endif /* TTN_BRAKET_H */
