/*
 * ttn_sample.h — sampling of resident trains, of libttn_hip.so: configurations z = (z_1 .. z_d) drawn from a Float64 train x of a
 * resident batch, with their log-probabilities (csrc/ttn_sample_kernels.h).
 * Included by ttn.h; the conventions (column-major arrays, int64_t integers, return codes) are stated there.  A core is
 * A_k[z, al, a], column-major (n_k, r_{k-1}, r_k).  Sites and indices are 1-based in the outputs, as the index sets of the cross
 * interpolation are.
 *
 *   TTN_SAMPLE_BORN     p(z) = x(z)^2 / <x, x>.       Right environments G_{d+1} = [1], G_k = sum_z A_k[z] G_{k+1} A_k[z]^T.
 *   TTN_SAMPLE_DENSITY  p(z) = x(z) / sum_z x(z), for a train that represents a non-negative function.
 *                                                     Right environments g_{d+1} = [1], g_k = sum_z A_k[z] g_{k+1}.
 * The environments are computed once per call.  One sample starts from v = [1] and does at site k = 1 .. d, with n = n_k:
 *   1. w_z = v A_k[z] for every z;
 *   2. p_z = w_z G_{k+1} w_z^T (Born) or p_z = w_z g_{k+1} (density);
 *   3. every p_z < 0 is set to 0 and counted as a CLAMP;
 *   4. c_z = p_0 + .. + p_z, summed in this order; tot = c_{n-1};
 *   5. with t = u_k tot the drawn z is the smallest z with t < c_z; if there is none, z = n - 1;
 *   6. logp += log(p_z / tot);
 *   7. v <- w_z 2^-e with 2^e the binade of max |w_z|: exact, so it changes no ratio; it only keeps v in range over 480 sites;
 *   8. if tot is 0 or not finite the sample is DEAD: its remaining indices (this site included) are 1, its logp is -inf, it is counted
 *      as dead and nothing is raised — the analogue of the IEEE 0 / 0 of ttn_site_expect on a zero train.
 * The environments themselves are not rescaled: a train whose environments over- or underflow is the caller's to normalise first.
 *
 * Uniforms.  d_u[k + d (s + S b)] in [0, 1) (k 0-based), device memory; or NULL, and the kernel generates them — nothing of size
 * B S d is allocated: u is the 53-bit uniform (word >> 11) 2^-53 of word j = 1 + k + d s of the splitmix64 stream
 * word_j = mix(sub + j 0x9E3779B97F4A7C15) whose sub-seed is sub = ((seed p + 6) p + b) p mod 2^64, p = 1000003 (the draw kind 6 of the
 * Python layer's sub-seeds).  The stream is counter based, so the first S samples of train b do not depend on S.
 *
 * Reproducibility: every reduction of the sampling kernel has a fixed order; the Born environments come from the chain kernel of
 * ttn_dot_pullback, whose on-chip sites add with LDS atomics.  A call is reproducible to rounding, not bitwise: two calls can differ
 * only in a sample whose t lies within rounding of a c_z.
 *
 * Every check runs before any launch:
 *   TTN_ERR_ARG          a null handle or null d_idx / d_logp (idx / logp); nsamples < 1; an unknown mode
 *   TTN_ERR_UNSUPPORTED  a ComplexF64 handle; a chain longer than 480 sites; a train, or the workspace of one train, of 2^31 doubles or more
 * Neither the number of trains nor the number of samples is a reason to refuse: a call works in chunks of at most 65535 trains and of
 * as many 64-sample tiles as keep the library workspace within TTN_SAMPLE_CHUNK_BYTES (or that of ONE train and ONE tile where that
 * needs more).  With r = max_m r_m, n = max_k n_k, W = r^2 and N = n r^2 (both rounded up to even) the workspace is
 *     per train   2 (d + 1) W + 2 N   (Born: both chains of ttn_dot_pullback's kernel)   or   (d + 1) r   (density)
 *     per tile    64 (r + 2 n r + n)  only when a site can lie outside n_k = 2, ranks <= 64 (the general route's products)
 * doubles.  Operator handles, conditional sampling with some sites fixed and sampling without replacement are not offered.
 */
#ifndef TTN_SAMPLE_H
#define TTN_SAMPLE_H

#include <stdint.h>
#include "ttn.h"      /* ttn_tt_t (ttn.h includes this file at its end: either order works) */

#ifdef __cplusplus
extern "C" {
#endif

#define TTN_SAMPLE_BORN 0
#define TTN_SAMPLE_DENSITY 1
#define TTN_SAMPLE_TILE 64                     /* samples one workgroup carries through the sites */
#define TTN_SAMPLE_CHUNK_BYTES 1073741824      /* 1 GiB: the workspace bound of one chunk of trains and tiles */

/* nsamples = S samples of every train of x into DEVICE memory, asynchronously on the library stream.  x is not modified.
 *   d_u     device, [k + d (s + S b)], or NULL (generated from `seed`; `seed` is ignored otherwise)
 *   d_idx   device, [k + d (s + S b)], 1-based indices
 *   d_logp  device, [s + S b]
 *   d_info  device, [2 b + 0] clamps, [2 b + 1] dead samples of train b; may be NULL */
int ttn_tt_sample_dev(ttn_tt_t x, int64_t mode, int64_t nsamples, int64_t seed, const double* d_u, int64_t* d_idx, double* d_logp, int64_t* d_info);

/* The same with HOST outputs (d_u stays device memory or NULL; info may be NULL); the call synchronises. */
int ttn_tt_sample(ttn_tt_t x, int64_t mode, int64_t nsamples, int64_t seed, const double* d_u, int64_t* idx, double* logp, int64_t* info);

/* Milliseconds the environments and the sweeps of the last ttn_tt_sample / ttn_tt_sample_dev took on the device (event pairs on the
 * library stream around the two phases, summed over the call's chunks of trains); synchronises.  TTN_ERR_ARG for a null pointer or
 * when no such call has run. */
int ttn_tt_sample_last_ms(double* env_ms, double* sweep_ms);

#ifdef __cplusplus
}
#endif
#endif /* TTN_SAMPLE_H */
