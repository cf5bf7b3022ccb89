/*
 * ttn_cross_batch.h — MaxVol cross interpolation for a batch of functions, of libttn_hip.so (csrc/ttn_cross_batch_kernels.h,
 * DESIGN.md 4.24).  Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.
 *
 * The three entry points are the per-site work of tt_cross(f, domain, ::MaxVol) (src/tt_cross_interpolation.jl:189-317) for A functions
 * at once.  Every pointer is a device pointer, every call is enqueued on the library stream and returns without waiting.  Indices are
 * int64, 1-based.  A per-function array is contiguous with the function axis leading: function a starts at a times the size of one.
 * Float64 only.  Every argument check runs before anything is launched.  A <= 65535.
 */
#ifndef TTN_CROSS_BATCH_H
#define TTN_CROSS_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Index matrices and coordinates.  mode 0: the fibre of site `site` (1..N) of every function, P = rl n rr points in the order of
 * _build_fiber_indices (i fastest, then the left, then the right rank index), from L [A][rl x (site - 1)] (ignored when site = 1) and
 * R [A][rr x (N - site)] (ignored when site = N).  mode 2: the shared index matrix idx_in (P x N), the same for every function.
 * doff: N + 1 offsets of the concatenated domain arrays dom.  idx_out and X are [A][P x N]; either may be NULL, not both.
 *   TTN_ERR_ARG          a missing pointer, a bad mode / site / size / rank, P that differs from rl n rr
 *   TTN_ERR_UNSUPPORTED  A above 65535 */
int ttn_cross_batch_points(int mode, int64_t A, int64_t N, int64_t site, int64_t n, int64_t rl, int64_t rr, const int64_t* L, const int64_t* R,
                           const int64_t* idx_in, int64_t P, const int64_t* doff, const double* dom, int64_t* idx_out, double* X);

/* One site step of every function, one workgroup per function.  V: [A][rl n rr], the values of the fibre of `site` in the order above.
 * dir 0 (left-to-right, site 1..N-1): the matrix is V reshaped to m = rl n rows and r = rr columns; set_in = lsets[site],
 *   [A][rl x (site - 1)] (NULL when site = 1); set_out = lsets[site + 1], [A][r x site], row c = [set_in[local_r(c), :], local_i(c)];
 *   core: [A][n x rl x r].
 * dir 1 (right-to-left, site 2..N): the matrix has m = n rr rows and r = rl columns, entry (i + n b, a) = V[i, a, b]; set_in =
 *   rsets[site], [A][rr x (N - site)] (NULL when site = N); set_out = rsets[site - 1], [A][r x (N - site + 1)], row c = [local_i(c),
 *   set_in[local_r(c), :]]; core: [A][n x r x rr].
 * The matrix is scaled by the power of two of its largest modulus, Q of its Householder QR goes through maxvol (tol, maxiter; the
 * rules of ttn_cross_maxvol), core = Q / Q[piv, :] in the layout above, piv [A][r] the pivot rows, local_i = (piv - 1) % n + 1,
 * local_r = (piv - 1) / n.  info [A][2] = {0 or TTN_ERR_SINGULAR, swaps}; singular: a zero or NaN pivot in maxvol, or an all-zero fibre.
 * A singular function gets a zero core and in-range pivots, the others are not affected.  Needs m >= r.
 *   TTN_ERR_ARG          a missing pointer, a bad dir / site / size / rank, m < r, maxiter < 0
 *   TTN_ERR_UNSUPPORTED  r above 1024, m above 2^20, A above 65535 */
int ttn_cross_batch_site(int64_t A, int dir, int64_t N, int64_t site, int64_t n, int64_t rl, int64_t rr, const double* V, double tol,
                         int64_t maxiter, const int64_t* set_in, int64_t* set_out, double* core, int64_t* piv, int64_t* info);

/* A trains at once.  cores: host array of N device pointers, cores[k] = [A][n_k x r_k x r_{k+1}]; dims and rks (N + 1 entries, both ends
 * 1) are host arrays.  Point form (idx, P x N, shared by all functions): out [A][P]; with yref [A][P] also err [A],
 * err_a = ||yref_a - out_a|| / max(||yref_a||, tol), every entry scaled by a power of two before it is squared.  Weight form (w, the
 * concatenated weight vectors, idx NULL, P = 1): out [A] = the contraction of every site with its weights.
 *   TTN_ERR_ARG          a missing pointer, both or neither of idx and w, w with P != 1, yref without err
 *   TTN_ERR_DIMS         an end rank that is not 1
 *   TTN_ERR_UNSUPPORTED  a rank above 1024, A above 65535 */
int ttn_cross_batch_eval(int64_t A, int64_t N, int64_t P, const double* const* cores, const int64_t* dims, const int64_t* rks,
                         const int64_t* idx, const double* w, double* out, const double* yref, double tol, double* err);

#ifdef __cplusplus
}
#endif
#endif /* TTN_CROSS_BATCH_H */
