/*
 * ttn_opbatch.h — operator batches of libttn_hip.so: B TT operators of equal dims and ranks in ONE ttn_tto handle, operator b for train b
 * of a batch of trains.  The parameter families the reference's examples loop over on the host (examples/ising_model.jl: H(g) for 21
 * values of g; a drift, a volatility or a step size per run) become one launch per operation.
 * Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.  Float64 only.
 *
 * A batch is a field of the handle, not a handle type of its own: dims, ranks and gauge flags are common to the B operators, host-known
 * and immutable as for one operator; the cores of operator b lie `stride` doubles behind those of operator b - 1.
 *
 * These entry points take an operator batch, which must hold as many operators as the trains hold trains (TTN_ERR_DIMS "batch sizes
 * differ" otherwise); with one operator in the handle they do what they always did, bit for bit:
 *     ttn_apply (Float64), ttn_apply_axpby, ttn_sandwich, ttn_sandwich_dev, ttn_sandwich_pullback, ttn_dmrg_eigsolve, ttn_mals_eigsolve,
 *     ttn_tto_ranks, ttn_tto_dtype, ttn_tto_free and the five below.
 * EVERY other entry point with a ttn_tto_t operand returns TTN_ERR_UNSUPPORTED ("... an operator batch is not supported here") before
 * any launch: ttn_apply_compress, ttn_apply_begin / ttn_apply_sweep, ttn_apply_pullback, the operator algebra (ttn_tto_mul, _inner, _add,
 * _scale, _kron, _to_tt, _compress, _set_ot, _download), ttn_tto_to_dense, the linear solvers, ttn_als_eigsolve, ttn_als_gen_eigsolve (both
 * operands) and the ComplexF64 form of ttn_apply.  ttn_tto_select gives them one operator of the batch.
 */
#ifndef TTN_OPBATCH_H
#define TTN_OPBATCH_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t, ttn_tto_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

/* `batch` operators of dims (n_k) and ranks rks[0..d] from host cores: cores[b * d + k] is core k of operator b, (n_k, n_k, r_k, r_k+1)
 * column-major Float64.  batch == 1 gives an ordinary operator.  Gauge flags: zeros.
 *   TTN_ERR_ARG  a null pointer, d < 1, batch < 1, a dim or a rank < 1 */
int ttn_tto_create_batch(int64_t d, const int64_t* dims, const int64_t* rks, int64_t batch, const double* const* cores, ttn_tto_t* out);

/* ttv_to_tto of EVERY train of v (dims n_k^2) into one operator batch, on the device: one packing launch (k_tto_pack) from the
 * capacity-strided slots of v into compact operator slots.  Every train must currently hold the same ranks; they are read once
 * (synchronises).  Gauge flags: those of the trains when all trains carry the same, zeros otherwise.
 *   TTN_ERR_DIMS         "the ranks of train b differ from those of train 0 at bond m"; dims that are not perfect squares
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle */
int ttn_tto_from_tt_batch(ttn_tt_t v, ttn_tto_t* out);

/* Number of operators in the handle (1 for an ordinary operator). */
int ttn_tto_batch(ttn_tto_t A, int64_t* batch);

/* Operator b of the batch as a NEW single operator (one device copy). */
int ttn_tto_select(ttn_tto_t A, int64_t b, ttn_tto_t* out);

/* ttn_tto_download of operator b. */
int ttn_tto_download_b(ttn_tto_t A, int64_t b, double* const* cores);

#ifdef __cplusplus
}
#endif
#endif /* TTN_OPBATCH_H */
