// ttn_selftest_kernels.h — unit-test hooks of the workgroup layers.
//
// Provides: k_selftest_gemm (wg_gemm, wg_syrk, wg_gemm_ra on plain operands), k_selftest_syrk2, k_selftest_gemm_ra2 (wg_syrk2, wg_gemm_ra2: two products in one call).
// Needs: ttn_wg_gemm.h.
// Used by: the translation units only (ttn_selftest_gemm, ttn_selftest_syrk2, ttn_selftest_gemm_ra2 and their 512-thread twins).
#pragma once
#include "ttn_wg_gemm.h"

// -------------------------------------------------------------------------------------------------
// kernel unit-test hook for wg_gemm (tests/test_gpu_kernels.py): one workgroup, plain row-major operands
// (optionally viewed transposed so both LDS staging maps are exercised)
// -------------------------------------------------------------------------------------------------
__global__ void TTN_KERNEL_BOUNDS k_selftest_gemm(int m, int n, int k, double* A, double* B, double* C, double alpha,
                                                         double beta, int ta, int tb) {
    extern __shared__ double lds[];
    const View Av = (ta & 1) ? mkview(A, plain(1), plain(m)) : mkview(A, plain(k), plain(1));     // ta & 1: A stored k x m
    const View Bv = tb ? mkview(B, plain(1), plain(k)) : mkview(B, plain(n), plain(1));     // tb: B stored n x k
    if (ta & 2) wg_syrk(m, k, Av, mkview(C, plain(n), plain(1)), alpha, lds);               // ta & 2: C = alpha A A^T (n == m; B, beta unused)
    else if (ta & 4) wg_gemm_ra(m, n, k, Av, Bv, mkview(C, plain(n), plain(1)), alpha, lds);   // ta & 4: the register-A form (beta unused)
    else wg_gemm(m, n, k, Av, Bv, mkview(C, plain(n), plain(1)), alpha, beta, lds);
}

// wg_syrk2 on plain operands: G_i (p_i x p_i, row-major) = alpha_i A_i A_i^T, A_i stored p_i x q_i row-major, or q_i x p_i if ta_i.
// pair = 0 runs the same two products as two wg_syrk calls in the same launch: what the paired call is compared with, bits and time.
__global__ void TTN_KERNEL_BOUNDS k_selftest_syrk2(int p1, int q1, double* A1, double* G1, double alpha1, int ta1,
                                                   int p2, int q2, double* A2, double* G2, double alpha2, int ta2, int pair) {
    extern __shared__ double lds[];
    const View A1v = ta1 ? mkview(A1, plain(1), plain(p1)) : mkview(A1, plain(q1), plain(1));
    const View A2v = ta2 ? mkview(A2, plain(1), plain(p2)) : mkview(A2, plain(q2), plain(1));
    const View G1v = mkview(G1, plain(p1), plain(1)), G2v = mkview(G2, plain(p2), plain(1));
    if (pair) wg_syrk2(p1, q1, A1v, G1v, alpha1, p2, q2, A2v, G2v, alpha2, lds);
    else { wg_syrk(p1, q1, A1v, G1v, alpha1, lds); wg_syrk(p2, q2, A2v, G2v, alpha2, lds); }
}

// wg_gemm_ra2 on plain operands: C_i (m_i x n_i) = alpha_i A_i B_i.  f_i & 1: A_i stored k x m, & 2: B_i stored n x k, & 4: C_i stored n x m
// (route F passes its left product with all three transposed), else row-major.  pair = 0: two wg_gemm_ra calls in the same launch.
__global__ void TTN_KERNEL_BOUNDS k_selftest_gemm_ra2(int m1, int n1, int k1, double* A1, double* B1, double* C1, double alpha1, int f1,
                                                      int m2, int n2, int k2, double* A2, double* B2, double* C2, double alpha2, int f2, int pair) {
    extern __shared__ double lds[];
    const View A1v = (f1 & 1) ? mkview(A1, plain(1), plain(m1)) : mkview(A1, plain(k1), plain(1));
    const View B1v = (f1 & 2) ? mkview(B1, plain(1), plain(k1)) : mkview(B1, plain(n1), plain(1));
    const View C1v = (f1 & 4) ? mkview(C1, plain(1), plain(m1)) : mkview(C1, plain(n1), plain(1));
    const View A2v = (f2 & 1) ? mkview(A2, plain(1), plain(m2)) : mkview(A2, plain(k2), plain(1));
    const View B2v = (f2 & 2) ? mkview(B2, plain(1), plain(k2)) : mkview(B2, plain(n2), plain(1));
    const View C2v = (f2 & 4) ? mkview(C2, plain(1), plain(m2)) : mkview(C2, plain(n2), plain(1));
    if (pair) wg_gemm_ra2(m1, n1, k1, A1v, B1v, C1v, alpha1, m2, n2, k2, A2v, B2v, C2v, alpha2, lds);
    else { wg_gemm_ra(m1, n1, k1, A1v, B1v, C1v, alpha1, lds); wg_gemm_ra(m2, n2, k2, A2v, B2v, C2v, alpha2, lds); }
}
