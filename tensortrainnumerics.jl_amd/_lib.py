"""ctypes binding of libttn_hip.so (the C ABI declared in include/ttn.h).

This is what a Julia ``ccall`` would bind.  There is NO CPU fallback:
if the shared library is missing or cannot be loaded the import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TTN_LIB") or os.path.join(_HERE, "libttn_hip.so")   # TTN_LIB: experiment builds
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

# error codes of include/ttn.h
TTN_OK = 0
TTN_ERR_DIMS = -1
TTN_ERR_BOND_INDEX = -2
TTN_ERR_SWEEPS = -3
TTN_ERR_CENTER = -4
TTN_ERR_CAPACITY = -5
TTN_ERR_ARG = -6
TTN_ERR_NOT_INIT = -7
TTN_ERR_UNSUPPORTED = -8
TTN_ERR_NO_CONVERGENCE = -9
TTN_ERR_SINGULAR = -10

i64 = C.c_int64
p_i64 = C.POINTER(C.c_int64)
p_f64 = C.POINTER(C.c_double)
pp_f64 = C.POINTER(C.POINTER(C.c_double))
handle = C.c_void_p
p_handle = C.POINTER(C.c_void_p)

# name -> (restype, argtypes): every symbol include/ttn.h declares
SIGNATURES = {
    "ttn_init": (C.c_int, [C.c_int]),
    "ttn_finalize": (C.c_int, []),
    "ttn_version": (C.c_char_p, []),
    "ttn_last_error_string": (C.c_char_p, []),
    "ttn_sync": (C.c_int, []),
    "ttn_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "ttn_tt_create": (C.c_int, [i64, p_i64, p_i64, i64, p_handle]),
    "ttn_tt_free": (C.c_int, [handle]),
    "ttn_tt_upload": (C.c_int, [handle, i64, pp_f64, p_i64, p_i64]),
    "ttn_tt_replicate": (C.c_int, [handle, i64]),
    "ttn_tt_ranks": (C.c_int, [handle, i64, p_i64, p_i64]),
    "ttn_tt_max_ranks": (C.c_int, [handle, p_i64]),
    "ttn_tt_download": (C.c_int, [handle, i64, pp_f64]),
    "ttn_tt_batch": (C.c_int, [handle, p_i64]),
    "ttn_tt_copy": (C.c_int, [handle, handle]),
    "ttn_tto_create": (C.c_int, [i64, p_i64, p_i64, pp_f64, p_handle]),
    "ttn_tto_free": (C.c_int, [handle]),
    "ttn_tto_mul": (C.c_int, [handle, handle, p_handle]),
    "ttn_tto_inner": (C.c_int, [handle, handle, p_handle]),
    "ttn_tto_add": (C.c_int, [handle, handle, p_handle]),
    "ttn_tto_scale": (C.c_int, [C.c_double, handle, p_handle]),
    "ttn_tto_kron": (C.c_int, [handle, handle, p_handle]),
    "ttn_tt_outer": (C.c_int, [handle, handle, i64, p_handle]),
    "ttn_tt_diag_tto": (C.c_int, [handle, i64, p_handle]),
    "ttn_tt_kron": (C.c_int, [handle, handle, handle]),
    "ttn_tto_to_tt": (C.c_int, [handle, handle]),
    "ttn_tto_from_tt": (C.c_int, [handle, i64, p_handle]),
    "ttn_tto_compress": (C.c_int, [handle, i64, C.c_double, i64, p_handle]),
    "ttn_tto_ranks": (C.c_int, [handle, p_i64, p_i64, p_i64, p_i64]),
    "ttn_tto_set_ot": (C.c_int, [handle, p_i64]),
    "ttn_tto_download": (C.c_int, [handle, pp_f64]),
    "ttn_apply": (C.c_int, [handle, handle, handle]),
    "ttn_compress": (C.c_int, [handle, i64, C.c_double, i64]),
    "ttn_compress_status": (C.c_int, [handle, p_i64]),
    "ttn_status_all": (C.c_int, []),
    "ttn_compress_rank_bound": (C.c_int, [i64, p_i64, p_i64, i64, i64, i64, p_i64, p_i64]),
    "ttn_bond_truncate": (C.c_int, [handle, i64, i64, C.c_double]),
    "ttn_apply_compress": (C.c_int, [handle, handle, handle, i64, C.c_double, i64]),
    "ttn_sweep": (C.c_int, [handle, i64, i64, i64, C.c_double]),
    "ttn_apply_begin": (C.c_int, [handle, handle, handle]),
    "ttn_apply_sweep": (C.c_int, [handle, handle, handle, i64, i64, i64, C.c_double, C.c_int]),
    "ttn_stream_handle": (C.c_int, [C.POINTER(C.c_void_p)]),
    "ttn_tt_core_extent": (C.c_int, [handle, i64, p_i64, p_i64, p_i64]),
    "ttn_tt_core_export": (C.c_int, [handle, i64, C.c_void_p, C.c_void_p]),
    "ttn_tt_core_import": (C.c_int, [handle, i64, C.c_void_p, C.c_void_p, i64, i64]),
    "ttn_dot": (C.c_int, [handle, handle, p_f64]),
    "ttn_norm": (C.c_int, [handle, p_f64]),
    "ttn_last_launch_ms": (C.c_int, [C.POINTER(C.c_float)]),
    "ttn_debug_ortho_state": (C.c_int, [i64, p_i64]),
    "ttn_dot_pullback": (C.c_int, [handle, handle, p_f64, handle, handle, p_f64]),
    "ttn_apply_pullback": (C.c_int, [handle, handle, handle, handle]),
    "ttn_tt_cores_axpby": (C.c_int, [p_f64, handle, p_f64, handle]),
    "ttn_tt_cores_dot": (C.c_int, [handle, handle, p_f64]),
    "ttn_hadamard": (C.c_int, [handle, handle, handle]),
    "ttn_hadamard_ttm": (C.c_int, [handle, handle, handle, C.c_double, i64, i64]),
    "ttn_swap_sites": (C.c_int, [handle, i64, p_i64, C.c_double]),
    "ttn_ttv_decomp": (C.c_int, [handle, C.c_void_p, i64, C.c_double]),
    "ttn_ttv_decomp_dev": (C.c_int, [handle, C.c_void_p, i64, C.c_double]),
    "ttn_tt_split_sites": (C.c_int, [handle, handle, p_i64, p_i64, C.c_double]),
    "ttn_tt_merge_sites": (C.c_int, [handle, handle, p_i64, i64]),
    "ttn_tt_to_dense": (C.c_int, [handle, p_i64, C.c_void_p]),
    "ttn_qtt_grid_points": (C.c_int, [i64, i64, C.c_int, C.c_double, C.c_double, i64, i64, C.c_void_p]),
    "ttn_als_linsolve": (C.c_int, [handle, handle, handle, handle, i64]),
    "ttn_mals_linsolve": (C.c_int, [handle, handle, handle, handle, C.c_double, i64]),
    "ttn_dmrg_linsolve": (C.c_int, [handle, handle, handle, handle, C.c_double, i64, p_i64, p_i64]),
    "ttn_dmrg_linsolve_it": (C.c_int, [handle, handle, handle, handle, C.c_double, i64, p_i64, p_i64, C.c_int, i64, C.c_double, i64]),
    "ttn_dmrg_cg_iterations": (C.c_int, [i64, p_i64]),
    "ttn_dmrg_eigsolve": (C.c_int, [handle, handle, handle, C.c_double, i64, p_i64, p_i64, C.c_int, i64, C.c_double, i64, i64, p_f64, p_i64]),
    "ttn_mals_eigsolve": (C.c_int, [handle, handle, handle, C.c_double, i64, p_i64, p_i64, C.c_int, i64, C.c_double, i64, i64, p_f64, p_i64]),
    "ttn_eigsolve_history_len": (C.c_int, [C.c_int, i64, i64, p_i64, p_i64]),
    "ttn_als_eigsolve": (C.c_int, [handle, handle, handle, i64, p_i64, p_i64, p_f64, i64, C.c_int, i64, C.c_double, i64, i64, p_f64]),
    "ttn_als_gen_eigsolve": (C.c_int, [handle, handle, handle, handle, i64, p_i64, p_i64, C.c_int, i64, i64, p_f64]),
    "ttn_eigsolve_stats": (C.c_int, [i64, p_i64, p_f64]),
    "ttn_tdvp_apply_h1": (C.c_int, [C.c_int, i64, i64, i64, i64, i64, i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "ttn_tdvp_apply_h0": (C.c_int, [C.c_int, i64, i64, i64, i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ttn_tdvp_update_left_env": (C.c_int, [C.c_int, i64, i64, i64, i64, i64, i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "ttn_tdvp_update_right_env": (C.c_int, [C.c_int, i64, i64, i64, i64, i64, i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "ttn_tdvp_apply_h2": (C.c_int, [C.c_int, i64, i64, i64, i64, i64, i64, i64, i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "ttn_dense_qr": (C.c_int, [C.c_int, i64, i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ttn_dense_svd": (C.c_int, [C.c_int, i64, i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ttn_cross_maxvol": (C.c_int, [C.c_int, i64, i64, C.c_void_p, C.c_double, i64, C.c_void_p, C.c_void_p, C.c_void_p, p_i64]),
    "ttn_cross_points": (C.c_int, [C.c_int, C.c_int, i64, i64, i64, i64, i64, i64, C.c_void_p, C.c_void_p, C.c_void_p, i64, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "ttn_cross_eval": (C.c_int, [C.c_int, i64, i64, pp_f64, p_i64, p_i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                 C.c_void_p]),
    "ttn_tdvp_contract_f64": (C.c_int, [C.c_int, C.c_int, i64, p_i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "ttn_selftest_eig128": (C.c_int, [C.c_void_p, i64, i64, i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ttn_selftest_sym_eig": (C.c_int, [i64, i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ttn_selftest_poison": (C.c_int, [C.c_int, C.c_uint64]),
    "ttn_selftest_workspace_peek": (C.c_int, [i64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ttn_selftest_tt_peek": (C.c_int, [handle, i64, i64, i64, p_f64]),
    "ttn_add": (C.c_int, [handle, handle, handle]),
    "ttn_scale": (C.c_int, [C.c_double, handle, handle]),
    "ttn_scale_batch": (C.c_int, [p_f64, handle, handle]),
    "ttn_orthogonalize": (C.c_int, [handle, i64, handle]),
    "ttn_sv_capture": (C.c_int, [handle, C.c_int]),
    "ttn_sv_get": (C.c_int, [handle, i64, i64, p_f64, i64, p_i64]),
    "ttn_timer_begin": (C.c_int, []),
    "ttn_timer_end": (C.c_int, [C.POINTER(C.c_float)]),
    "ttn_selftest_gemm": (C.c_int, [i64, i64, i64, p_f64, p_f64, p_f64, C.c_double, C.c_double, C.c_int, C.c_int]),
    "ttn_selftest_syrk2": (C.c_int, [i64, i64, p_f64, p_f64, C.c_double, C.c_int, i64, i64, p_f64, p_f64, C.c_double, C.c_int, C.c_int]),
    "ttn_selftest_gemm_ra2": (C.c_int, [i64, i64, i64, p_f64, p_f64, p_f64, C.c_double, C.c_int, i64, i64, i64, p_f64, p_f64, p_f64, C.c_double, C.c_int, C.c_int]),
    "ttn_selftest_lu_solve": (C.c_int, [i64, p_f64, p_f64, p_f64, p_i64, C.c_int]),
    "ttn_selftest_two_site_apply": (C.c_int, [i64, i64, i64, p_f64, p_f64, p_f64, p_f64]),
    "ttn_event_record": (C.c_int, [i64]),
    "ttn_event_elapsed": (C.c_int, [i64, i64, C.POINTER(C.c_float)]),
    "ttn_apply_f64": (C.c_int, [i64, p_i64, pp_f64, p_i64, pp_f64, p_i64, pp_f64]),
    "ttn_dot_f64": (C.c_int, [i64, p_i64, pp_f64, p_i64, pp_f64, p_i64, p_f64]),
    "ttn_hadamard_f64": (C.c_int, [i64, p_i64, pp_f64, p_i64, pp_f64, p_i64, pp_f64]),
    "ttn_add_f64": (C.c_int, [i64, p_i64, pp_f64, p_i64, pp_f64, p_i64, pp_f64]),
    "ttn_scale_f64": (C.c_int, [i64, p_i64, C.c_double, pp_f64, p_i64, p_i64, pp_f64, p_i64]),
    "ttn_orthogonalize_f64": (C.c_int, [i64, p_i64, pp_f64, p_i64, i64, pp_f64, p_i64, p_i64]),
    "ttn_compress_f64": (C.c_int, [i64, p_i64, pp_f64, p_i64, i64, C.c_double, i64]),
    "ttn_apply_compress_rank_bound": (C.c_int, [i64, p_i64, p_i64, p_i64, i64, i64, p_i64]),
    "ttn_apply_compress_f64": (C.c_int, [i64, p_i64, pp_f64, p_i64, pp_f64, p_i64, pp_f64, p_i64, i64, C.c_double, i64]),
    "ttn_bond_truncate_f64": (C.c_int, [i64, p_i64, pp_f64, p_i64, i64, i64, C.c_double]),
    "ttn_r_and_d_to_rks": (C.c_int, [i64, p_i64, i64, p_i64, i64, p_i64]),
    # ComplexF64 handles and stateless entry points (interleaved re / im doubles)
    "ttn_tt_create_c64": (C.c_int, [i64, p_i64, p_i64, i64, p_handle]),
    "ttn_tto_create_c64": (C.c_int, [i64, p_i64, p_i64, pp_f64, p_handle]),
    "ttn_tt_dtype": (C.c_int, [handle, C.POINTER(C.c_int)]),
    "ttn_tto_dtype": (C.c_int, [handle, C.POINTER(C.c_int)]),
    "ttn_scale_c64": (C.c_int, [C.c_double, C.c_double, handle, handle]),
    "ttn_scale_batch_c64": (C.c_int, [p_f64, handle, handle]),
    "ttn_apply_c64": (C.c_int, [i64, p_i64, pp_f64, p_i64, pp_f64, p_i64, pp_f64, C.c_int, C.c_int]),
    "ttn_dot_c64": (C.c_int, [i64, p_i64, pp_f64, p_i64, pp_f64, p_i64, p_f64]),
    "ttn_hadamard_c64": (C.c_int, [i64, p_i64, pp_f64, p_i64, pp_f64, p_i64, pp_f64]),
    "ttn_add_c64": (C.c_int, [i64, p_i64, pp_f64, p_i64, pp_f64, p_i64, pp_f64]),
    "ttn_scale_host_c64": (C.c_int, [i64, p_i64, C.c_double, C.c_double, pp_f64, p_i64, p_i64, pp_f64, p_i64]),
    "ttn_compress_c64": (C.c_int, [i64, p_i64, pp_f64, p_i64, i64, C.c_double, i64]),
    "ttn_bond_truncate_c64": (C.c_int, [i64, p_i64, pp_f64, p_i64, i64, i64, C.c_double]),
    "ttn_apply_compress_c64": (C.c_int, [i64, p_i64, pp_f64, p_i64, pp_f64, p_i64, pp_f64, p_i64, i64, C.c_double, i64, C.c_int, C.c_int]),
}

# the rectangular operators of include/ttn_rect.h (a handle type of their own, ttn_rtto_t)
RECT_SIGNATURES = {
    "ttn_rtto_create": (C.c_int, [i64, p_i64, p_i64, p_i64, pp_f64, p_handle]),
    "ttn_rtto_free": (C.c_int, [handle]),
    "ttn_rtto_ranks": (C.c_int, [handle, p_i64, p_i64, p_i64, p_i64]),
    "ttn_apply_rect": (C.c_int, [handle, handle, handle]),
    "ttn_apply_rect_f64": (C.c_int, [i64, p_i64, p_i64, pp_f64, p_i64, pp_f64, p_i64, pp_f64]),
}

# the dense bridge for operators of include/ttn_dense.h
DENSE_SIGNATURES = {
    "ttn_tto_to_dense": (C.c_int, [handle, p_i64, p_i64, C.c_void_p]),
    "ttn_tto_decomp_dev": (C.c_int, [i64, p_i64, C.c_void_p, p_i64, p_i64, i64, C.c_double, i64, p_handle]),
    "ttn_debug_dense_plan": (C.c_int, [p_i64]),
    "ttn_debug_gather_plan": (C.c_int, [p_i64]),
}

# the time-step entry points of include/ttn_step.h
STEP_SIGNATURES = {
    "ttn_apply_axpby": (C.c_int, [p_f64, handle, p_f64, handle, handle, handle]),
    "ttn_tt_increase_ranks": (C.c_int, [handle, p_i64, C.c_double, C.c_uint64, handle]),
}

# MaxVol cross for a batch of functions, include/ttn_cross_batch.h (device pointers throughout; the core table of the evaluation is host)
CROSS_BATCH_SIGNATURES = {
    "ttn_cross_batch_points": (C.c_int, [C.c_int, i64, i64, i64, i64, i64, i64, C.c_void_p, C.c_void_p, C.c_void_p, i64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "ttn_cross_batch_site": (C.c_int, [i64, C.c_int, i64, i64, i64, i64, i64, C.c_void_p, C.c_double, i64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "ttn_cross_batch_eval": (C.c_int, [i64, i64, i64, pp_f64, p_i64, p_i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                       C.c_void_p]),
}

# <x, A y> without forming A y, include/ttn_expect.h
EXPECT_SIGNATURES = {
    "ttn_sandwich": (C.c_int, [handle, handle, handle, p_f64]),
    "ttn_sandwich_dev": (C.c_int, [handle, handle, handle, C.c_void_p]),
}

# the pullback of <x, A y>, include/ttn_expect_grad.h
EXPECT_GRAD_SIGNATURES = {
    "ttn_sandwich_pullback": (C.c_int, [handle, handle, handle, p_f64, handle, handle, p_f64]),
}

# operator batches, include/ttn_opbatch.h
OPBATCH_SIGNATURES = {
    "ttn_tto_create_batch": (C.c_int, [i64, p_i64, p_i64, i64, pp_f64, p_handle]),
    "ttn_tto_from_tt_batch": (C.c_int, [handle, p_handle]),
    "ttn_tto_batch": (C.c_int, [handle, p_i64]),
    "ttn_tto_select": (C.c_int, [handle, i64, p_handle]),
    "ttn_tto_download_b": (C.c_int, [handle, i64, pp_f64]),
}

# site-resolved measurements, include/ttn_measure.h (the tables are host arrays; `out` is host, `d_out` device memory)
MEASURE_SIGNATURES = {
    "ttn_site_expect": (C.c_int, [handle, i64, p_f64, i64, p_f64]),
    "ttn_site_expect_dev": (C.c_int, [handle, i64, p_f64, i64, C.c_void_p]),
    "ttn_correlation": (C.c_int, [handle, p_f64, p_f64, i64, p_f64]),
    "ttn_correlation_dev": (C.c_int, [handle, p_f64, p_f64, i64, C.c_void_p]),
}

# sampling, include/ttn_sample.h (`d_u` is device memory or NULL; the plain form writes host arrays, the _dev form device memory)
SAMPLE_SIGNATURES = {
    "ttn_tt_sample": (C.c_int, [handle, i64, i64, i64, C.c_void_p, p_i64, p_f64, p_i64]),
    "ttn_tt_sample_dev": (C.c_int, [handle, i64, i64, i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ttn_tt_sample_last_ms": (C.c_int, [p_f64, p_f64]),
}

# excited states, include/ttn_eig_ortho.h (`phi` is a host array of handles; weights and ovl are host arrays [batch][n_ortho])
EIG_ORTHO_SIGNATURES = {
    "ttn_dmrg_eigsolve_ortho": (C.c_int, [handle, handle, handle, i64, p_handle, p_f64, C.c_double, i64, p_i64, p_i64, C.c_int, i64, C.c_double, i64,
                                          i64, p_f64, p_i64, p_f64]),
    "ttn_mals_eigsolve_ortho": (C.c_int, [handle, handle, handle, i64, p_handle, p_f64, C.c_double, i64, p_i64, p_i64, C.c_int, i64, C.c_double, i64,
                                          i64, p_f64, p_i64, p_f64]),
}

# <x| A |y> on ComplexF64 or Float64 operands, include/ttn_braket.h (`out`: 2 * batch host doubles, `d_out`: device memory)
BRAKET_SIGNATURES = {
    "ttn_braket": (C.c_int, [handle, handle, handle, p_f64]),
    "ttn_braket_dev": (C.c_int, [handle, handle, handle, C.c_void_p]),
}

# the fixed-rank manifold, include/ttn_tangent.h (`out`, `alpha`, `beta`: host arrays of `batch` doubles, or NULL)
TANGENT_SIGNATURES = {
    "ttn_tangent_project": (C.c_int, [handle, handle, handle, handle, p_f64]),
    "ttn_tangent_to_tt": (C.c_int, [handle, handle, handle, p_f64, p_f64, handle]),
}

# partial contraction, include/ttn_contract.h (`sites` and `weights` are host arrays)
CONTRACT_SIGNATURES = {
    "ttn_tt_contract_sites": (C.c_int, [handle, i64, p_i64, i64, p_f64, handle]),
}

# site-resolved measurements on ComplexF64 trains, include/ttn_zmeasure.h (interleaved host tables; `out` is host, `d_out` device memory)
ZMEASURE_SIGNATURES = {
    "ttn_zsite_expect": (C.c_int, [handle, i64, p_f64, i64, p_f64]),
    "ttn_zsite_expect_dev": (C.c_int, [handle, i64, p_f64, i64, C.c_void_p]),
    "ttn_zcorrelation": (C.c_int, [handle, p_f64, p_f64, i64, p_f64]),
    "ttn_zcorrelation_dev": (C.c_int, [handle, p_f64, p_f64, i64, C.c_void_p]),
}

_lib = None


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/ttn_api.hip (the host API of csrc/ttn_host_*.h on the kernel headers) and csrc/ttn_wg512.hip for gfx950 into
    libttn_hip.so (in-tree).  hipcc cross-compiles without a GPU."""
    srcs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))]
    srcs += [os.path.join(INCLUDE, f) for f in sorted(os.listdir(INCLUDE)) if f.endswith(".h")]
    if not force and os.path.exists(LIB_PATH):
        newest = max(os.path.getmtime(s) for s in srcs)
        if os.path.getmtime(LIB_PATH) >= newest:
            return LIB_PATH
    cmd = ["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value", "-Wno-pass-failed",
           "-o", LIB_PATH, os.path.join(CSRC, "ttn_api.hip"), os.path.join(CSRC, "ttn_wg512.hip")]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


def lib() -> C.CDLL:
    """Load the shared library (once).  Fails loudly if it is missing: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for table in (SIGNATURES, RECT_SIGNATURES, DENSE_SIGNATURES, STEP_SIGNATURES, CROSS_BATCH_SIGNATURES, EXPECT_SIGNATURES, EXPECT_GRAD_SIGNATURES,
                  OPBATCH_SIGNATURES, MEASURE_SIGNATURES, SAMPLE_SIGNATURES, EIG_ORTHO_SIGNATURES, BRAKET_SIGNATURES,
                  TANGENT_SIGNATURES, CONTRACT_SIGNATURES, ZMEASURE_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(L, name)       # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
    _lib = L
    return L


def last_error() -> str:
    return lib().ttn_last_error_string().decode()


class TTNError(RuntimeError):
    pass


# messages of the reference's @assert sites (src/tt_operations.jl:11,102,240,344; src/tt_tools.jl:513,744,773)
_ASSERT_CODES = {TTN_ERR_DIMS, TTN_ERR_BOND_INDEX, TTN_ERR_SWEEPS, TTN_ERR_CENTER}


def check(rc: int) -> None:
    """Map a return code to the exception type the reference throws."""
    if rc == 0:
        return
    msg = last_error()
    if rc in _ASSERT_CODES:
        raise AssertionError(msg)
    raise TTNError(f"ttn error {rc}: {msg}")


_initialised = False


def ensure_init(device: int | None = None) -> None:
    global _initialised
    if _initialised and device is None:
        return
    if device is None:
        device = int(os.environ.get("TTN_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    check(lib().ttn_init(device))
    _initialised = True


def finalize() -> None:
    global _initialised
    if _lib is not None:
        _lib.ttn_finalize()
    _initialised = False
