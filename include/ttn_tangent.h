/*
 * ttn_tangent.h — the fixed-rank TT manifold on resident batches, of libttn_hip.so: the orthogonal projection of a train onto the
 * tangent space at a point x, and the train alpha x + beta xi of a tangent xi at twice x's ranks (the input of a retraction).  Float64
 * only.  Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.
 *
 * A point is handed over as its two gauges, which the caller computes once per point with ttn_orthogonalize:
 *     U = orthogonalize(x, d)    U_1 .. U_{d-1} left-orthogonal, U_d the centre core
 *     V = orthogonalize(x, 1)    V_2 .. V_d right-orthogonal
 * A tangent xi is a bag of cores dC_1 .. dC_d with x's ranks (an ordinary ttn_tt handle that is never contracted as a train) and stands
 * for sum_k U_1 .. U_{k-1} dC_k V_{k+1} .. V_d, with U_k^T dC_k = 0 in the left unfolding for k < d.  Under that gauge condition the
 * inner product of two tangents AS TENSORS is sum_k <dC_k, dD_k>: what ttn_tt_cores_dot returns.
 *
 * U and V must be gauges of the SAME x.  The calls cannot verify that; they do check, per train on the device, that the ranks of U
 * and V (and of xi in ttn_tangent_to_tt) agree and that the boundary ranks are 1: a train where they do not is left alone, carries a
 * per-train failure code on the destination (TTN_ERR_DIMS from ttn_compress_status / ttn_status_all), and the other trains are computed.
 */
#ifndef TTN_TANGENT_H
#define TTN_TANGENT_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

#define TTN_TANGENT_CHUNK_BYTES 1073741824     /* 1 GiB: the workspace bound of one chunk of trains of ttn_tangent_project */

/* xi = P_x z, the orthogonal projection of the train z (any ranks rz) onto the tangent space at x:
 *     dC_k[z, al, a'] = sum_b ( sum_be L_k[al, be] Z_k[z, be, b] - [k < d] sum_a U_k[z, al, a] L_{k+1}[a, b] ) G_{k+1}[a', b]
 * with L the left environments of (U, z) and G the right environments of (V, z), each chain computed once.  xi receives U's current
 * ranks per train (copied on the device) and gauge flags 0.  `out` is a HOST array of `batch` doubles or NULL: non-NULL, it receives
 * <x_b, z_b> (= L_{d+1}) and the call synchronises; NULL, the call is asynchronous on the library stream.
 * Workspace from the library buffer, per train: 2 (d + 1) W + 2 nmax rmax rzmax doubles, W = max_m r_m rz_m rounded up to even; batches
 * whose workspace exceeds TTN_TANGENT_CHUNK_BYTES run in chunks of trains (one train at least).
 * Before any launch, with nothing written:
 *   TTN_ERR_ARG          a null handle; xi is U, V or z
 *   TTN_ERR_DIMS         dims or batch sizes differ
 *   TTN_ERR_CAPACITY     xi's rank capacity below U's rank bounds
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle; more than 480 sites; a train, or the workspace of one train, of 2^31 doubles or more */
int ttn_tangent_project(ttn_tt_t U, ttn_tt_t V, ttn_tt_t z, ttn_tt_t xi, double* out);

/* y = alpha_b x_b + beta_b xi_b as a train of ranks 2 r on the interior bonds (gauge flags 0), one streaming pass:
 *     W_1 = [dC_1, U_1],   W_k = [[V_k, 0], [dC_k, U_k]],   W_d = [beta V_d ; beta dC_d + alpha U_d]      (d = 1: alpha U_1 + beta dC_1)
 * Blocks that are copies are copied bit for bit and the off-diagonal block is written as explicit zeros.  `alpha`, `beta`: HOST arrays
 * of `batch` doubles each, NULL = 1.  Asynchronous unless a coefficient array is given (its upload synchronises).
 * Before any launch, with nothing written:
 *   TTN_ERR_ARG          a null handle; y is U, V or xi
 *   TTN_ERR_DIMS         dims or batch sizes differ
 *   TTN_ERR_CAPACITY     y's rank capacity below 2 r (U's rank bounds) on an interior bond
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle; a train of 2^31 doubles or more; 2^31 or more fibres in one core of y; more than 65535 trains */
int ttn_tangent_to_tt(ttn_tt_t U, ttn_tt_t V, ttn_tt_t xi, const double* alpha, const double* beta, ttn_tt_t y);

#ifdef __cplusplus
}
#endif
#endif /* TTN_TANGENT_H */
