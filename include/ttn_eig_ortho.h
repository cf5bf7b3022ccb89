/*
 * ttn_eig_ortho.h — excited states with the two-site eigensolvers of libttn_hip.so: ttn_dmrg_eigsolve / ttn_mals_eigsolve with a penalty
 * against given trains (csrc/ttn_eig_ortho_kernels.h).
 * Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.  Float64, real symmetric
 * operators, two-site windows: the limits of the plain entry points.
 *
 * With phi_1 .. phi_m given (m = n_ortho <= TTN_EIG_ORTHO_MAX) every train b of the batch is driven to the smallest eigenpair of
 *     A_b + sum_j w[b][j] |phi_j><phi_j| / <phi_j, phi_j>
 * on the walk, rank rules and core moves of the plain solvers: the local problem of a window is the symmetrised two-site matrix plus
 * the rank-m term sum_j w_j p_j p_j^T, p_j the projection of phi_j / ||phi_j|| onto the window's basis.  The rank-m term is never
 * formed as an operator.  With the phi_j the eigenstates below the wanted one and every w_j above the distance from their level to
 * the wanted one, the result is the next level, orthogonal to the phi_j up to the accuracy of the solve.
 *
 *   phi[j]     has the d and dims of x, its own ranks and capacity, and need not be normalised: its norm is taken once per call.  Its
 *              batch is that of x (train b penalises train b) or 1 (shared by all trains).  It is only read.
 *   weights    HOST array, weights[j + n_ortho * b] = w[b][j], finite and > 0.
 *   E          the history, as in ttn_dmrg_eigsolve; an entry is the local eigenvalue of the PENALISED problem, i.e.
 *              <x, A x> + sum_j w_j <phi_j, x>^2 / <phi_j, phi_j> in the local basis.  It equals the energy only where the overlaps
 *              vanish: take the energy with ttn_sandwich (or ttn_dot of ttn_apply) on the result.
 *   ovl        HOST array, ovl[j + n_ortho * b] = <phi_j, x> / ||phi_j|| of the final state of train b.
 *   A          ONE operator: like every entry point outside the list of ttn_opbatch.h these two refuse an operator batch
 *              (TTN_ERR_UNSUPPORTED, before anything else); ttn_tto_select gives one operator of it.
 * n_ortho == 0 is the plain call: the same kernel, the same bits; phi, weights and ovl are then not read.
 *
 * Every check runs before the solve is launched and before x is written:
 *   TTN_ERR_ARG          n_ortho outside 0 .. TTN_EIG_ORTHO_MAX; a null pointer or handle; a phi[j] that is x or x0; a phi[j] whose batch
 *                        is neither that of x nor 1; a weight that is not finite or not > 0; ||phi_j|| zero or not finite for some train
 *   TTN_ERR_DIMS         a phi[j] of other dims
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle
 *   TTN_ERR_CAPACITY     the workspace does not fit in device memory
 *   and everything ttn_dmrg_eigsolve / ttn_mals_eigsolve refuse.
 * Workspace per train, in doubles, on top of the plain solver's: with c = the largest capacity rank of x, q_j = the largest rank
 * bound of phi[j], q = max_j q_j, M = max_k n_k c, N = max_i n_i c_i n_{i+1} c_{i+2}:
 *     sum_j 2 (d + 1) c q_j        both overlap chains of every phi_j
 *   + n_ortho N                    the projected vectors
 *   + 2 M q + 8                    the intermediates of a projection, the coefficients of the matrix-free term
 */
#ifndef TTN_EIG_ORTHO_H
#define TTN_EIG_ORTHO_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t, ttn_tto_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

#define TTN_EIG_ORTHO_MAX 8

int ttn_dmrg_eigsolve_ortho(ttn_tto_t A, ttn_tt_t x0, ttn_tt_t x, int64_t n_ortho, const ttn_tt_t* phi, const double* weights,
                            double tol, int64_t n_stages, const int64_t* sweep_schedule, const int64_t* rmax_schedule,
                            int it_solver, int64_t maxiter, double linsolv_tol, int64_t itslv_thresh,
                            int64_t hist_len, double* E, int64_t* r_hist, double* ovl);

int ttn_mals_eigsolve_ortho(ttn_tto_t A, ttn_tt_t x0, ttn_tt_t x, int64_t n_ortho, const ttn_tt_t* phi, const double* weights,
                            double tol, int64_t n_stages, const int64_t* sweep_schedule, const int64_t* rmax_schedule,
                            int it_solver, int64_t maxiter, double linsolv_tol, int64_t itslv_thresh,
                            int64_t hist_len, double* E, int64_t* r_hist, double* ovl);

#ifdef __cplusplus
}
#endif
#endif /* TTN_EIG_ORTHO_H */
