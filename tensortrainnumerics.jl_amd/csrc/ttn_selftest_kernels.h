// ttn_selftest_kernels.h — unit-test hooks of the workgroup layers.
//
// Provides: k_selftest_gemm (wg_gemm, wg_syrk, wg_gemm_ra on plain operands).
// Needs: ttn_wg_gemm.h.
// Used by: the translation units only (ttn_selftest_gemm and its 512-thread twin).
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
