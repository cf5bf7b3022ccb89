// ttn_wg512.h — the launchers of the 512-thread build of k_compress and its building blocks (ttn_wg512.hip: two workgroups per CU).
//
// The one declaration of what crosses the boundary between the two translation units of libttn_hip.so.  ttn_wg512.hip includes it, so
// the compiler holds every definition against its prototype; ttn_api.hip and the host headers that call across include it too.  Both
// sides are extern "C": a prototype written out a second time would link whatever it said.
#ifndef TTN_WG512_H
#define TTN_WG512_H
#include <hip/hip_runtime.h>
#include <stddef.h>

extern "C" {
int ttn_wg512_init(void);
size_t ttn_wg512_compress_args_bytes(void);
size_t ttn_wg512_lds_bytes(void);
int ttn_wg512_launch_compress(const void* args, size_t nbytes, int grid, hipStream_t stream);
int ttn_wg512_selftest_eig(const double* G, double* Vst, int n, int r, int nev, double* sig, double* Xout, long long* clk, hipStream_t stream);
int ttn_wg512_selftest_gemm(int m, int n, int k, double* A, double* B, double* C, double alpha, double beta, int ta, int tb, hipStream_t stream);
int ttn_wg512_selftest_syrk2(int p1, int q1, double* A1, double* G1, double alpha1, int ta1, int p2, int q2, double* A2, double* G2, double alpha2, int ta2,
                             int pair, hipStream_t stream);
int ttn_wg512_selftest_gemm_ra2(int m1, int n1, int k1, double* A1, double* B1, double* C1, double alpha1, int f1,
                                int m2, int n2, int k2, double* A2, double* B2, double* C2, double alpha2, int f2, int pair, hipStream_t stream);
}
#endif  // TTN_WG512_H
