// ttn_host_lds.h — host API: the one {kernel, bytes} table of dynamic LDS that ttn_init applies.
//
// Included FIRST among the host headers, before any launch: a kernel template is instantiated where the translation unit first names
// it, and that order is the order of the instantiations in the code object.  This table has always been the first to name them (it
// stood at the top of ttn_init); it stays first so that the device code does not depend on the order of the host headers.
#ifndef TTN_HOST_LDS_H
#define TTN_HOST_LDS_H
#include "ttn_dense_kernels.h"
#include "ttn_swap_kernels.h"
#include "ttn_selftest_kernels.h"
#include "ttn_dot_kernels.h"
#include "ttn_ortho_kernels.h"
#include "ttn_ortho512.h"
#include "ttn_hsvd_kernels.h"
#include "ttn_resite_kernels.h"
#include "ttn_als_kernels.h"
#include "ttn_als_grid.h"
#include "ttn_eigsolve_kernels.h"
#include "ttn_eig_ortho_kernels.h"
#include "ttn_als_eig_kernels.h"
#include "ttn_eig_kernels.h"
#include "ttn_tdvp_kernels.h"
#include "ttn_cross_kernels.h"
#include "ttn_cross_batch_kernels.h"
#include "ttn_cplx_kernels.h"
#include "ttn_grad_kernels.h"
#include "ttn_expect_kernels.h"
#include "ttn_expect_grad_kernels.h"
#include "ttn_measure_kernels.h"
#include "ttn_sample_kernels.h"
#include "ttn_braket_kernels.h"
#include "ttn_tangent_kernels.h"
#include "ttn_contract_kernels.h"
#include "ttn_zmeasure_kernels.h"

#include <cstddef>

namespace {
// the kernels that use more than the default 64 KiB of dynamic LDS
const struct { const void* fn; size_t lds; } lds_limits[] = {
    {(const void*)k_compress, COMPRESS_LDS_BYTES},
    {(const void*)k_selftest_eig128, COMPRESS_LDS_BYTES},
    {(const void*)k_mals_linsolve, COMPRESS_LDS_BYTES},
    {(const void*)k_als_linsolve, COMPRESS_LDS_BYTES},
    {(const void*)k_two_site_eig, COMPRESS_LDS_BYTES},
    {(const void*)k_two_site_eig_ortho, COMPRESS_LDS_BYTES},
    {(const void*)k_als_eig, COMPRESS_LDS_BYTES},
    {(const void*)k_increase_ranks, COMPRESS_LDS_BYTES},
    {(const void*)k_ttv_decomp, COMPRESS_LDS_BYTES},
    {(const void*)k_split_sites, COMPRESS_LDS_BYTES},
    {(const void*)k_swap_chain, COMPRESS_LDS_BYTES},
    {(const void*)k_orthogonalize, ORTHO_LDS_BYTES},
    {(const void*)k_ortho512, O5_LDS_BYTES(TTN_MAX_D * 8)},
    {(const void*)k_dot_fused, DOT_LDS_BYTES(DOT_MAX_D)},
    {(const void*)k_grad_chain, DOT_LDS_BYTES(DOT_MAX_D)},
    {(const void*)k_selftest_gemm, sizeof(double) * GEMM_LDS_TOTAL},
    {(const void*)k_selftest_syrk2, sizeof(double) * GEMM_LDS_TOTAL},
    {(const void*)k_selftest_gemm_ra2, sizeof(double) * GEMM_LDS_TOTAL},
    {(const void*)k_tdvp, TDVP_LDS_BYTES},
    {(const void*)k_lu_panel, LU_PANEL_LDS_BYTES},
    {(const void*)k_lu_trail, sizeof(double) * GEMM_LDS_TOTAL},
    {(const void*)k_selftest_lu, COMPRESS_LDS_BYTES},
    {(const void*)k_selftest_two_site_apply, COMPRESS_LDS_BYTES},
    {(const void*)k_cross_maxvol<false>, TTN_XV_LDS_BYTES},
    {(const void*)k_cross_maxvol<true>, TTN_XV_LDS_BYTES},
    {(const void*)k_zcompress, TTN_ZC_LDS_BYTES},
    {(const void*)k_cross_batch_site, TTN_XB_LDS_BYTES},
    {(const void*)k_expect<0>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expect<1>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expect<2>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expect<3>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expect<4>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expect<5>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expgrad_chain<0>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expgrad_chain<1>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expgrad_chain<2>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expgrad_chain<3>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expgrad_chain<4>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expgrad_chain<5>, EXPECT_LDS_BYTES(EXPECT_MAX_D)},
    {(const void*)k_expgrad_core_gen<false>, sizeof(double) * GEMM_LDS_TOTAL},
    {(const void*)k_expgrad_core_gen<true>, sizeof(double) * GEMM_LDS_TOTAL},
    {(const void*)k_measure_open, MEASURE_LDS_BYTES(MEASURE_MAX_D)},
    {(const void*)k_measure_walk, MEASURE_LDS_BYTES(MEASURE_MAX_D)},
    {(const void*)k_sample_sweep, SAMPLE_LDS_BYTES},
    {(const void*)k_zexpect<true, true, 0>, BRAKET_LDS_BYTES(BRAKET_MAX_D)},
    {(const void*)k_zexpect<true, true, 1>, BRAKET_LDS_BYTES(BRAKET_MAX_D)},
    {(const void*)k_zexpect<true, true, 2>, BRAKET_LDS_BYTES(BRAKET_MAX_D)},
    {(const void*)k_zexpect<false, true, 0>, BRAKET_LDS_BYTES(BRAKET_MAX_D)},
    {(const void*)k_zexpect<false, true, 1>, BRAKET_LDS_BYTES(BRAKET_MAX_D)},
    {(const void*)k_zexpect<false, true, 2>, BRAKET_LDS_BYTES(BRAKET_MAX_D)},
    {(const void*)k_zexpect<true, false, 0>, BRAKET_LDS_BYTES(BRAKET_MAX_D)},
    {(const void*)k_zexpect<true, false, 1>, BRAKET_LDS_BYTES(BRAKET_MAX_D)},
    {(const void*)k_zexpect<true, false, 2>, BRAKET_LDS_BYTES(BRAKET_MAX_D)},
    {(const void*)k_tangent_chain, DOT_LDS_BYTES(DOT_MAX_D)},
    {(const void*)k_contract_chip, CONTRACT_CHIP_LDS_BYTES},
    {(const void*)k_contract_gen, sizeof(double) * GEMM_LDS_TOTAL},
    {(const void*)k_zmeasure_chain<true>, ZM_LDS_BYTES(ZMEASURE_MAX_D)},
    {(const void*)k_zmeasure_chain<false>, ZM_LDS_BYTES(ZMEASURE_MAX_D)},
    {(const void*)k_zmeasure_open<true>, ZM_LDS_BYTES(ZMEASURE_MAX_D)},
    {(const void*)k_zmeasure_open<false>, ZM_LDS_BYTES(ZMEASURE_MAX_D)},
    {(const void*)k_zmeasure_walk<true>, ZM_LDS_BYTES(ZMEASURE_MAX_D)},
    {(const void*)k_zmeasure_walk<false>, ZM_LDS_BYTES(ZMEASURE_MAX_D)},
};
}  // namespace
#endif  // TTN_HOST_LDS_H
