"""Every device call on POISONED workspace and handle slack.

The library carves the workspace of every launch out of one buffer that is never cleared, creates train handles zeroed and keeps cores
compactly at the start of capacity-sized slots: a kernel that reads a byte nobody wrote reads plausible stale numbers or zeros, and the
oracle comparisons cannot see it.  ``ttn_selftest_poison`` (host side only, no kernel differs) fills the workspace at every acquisition,
the slack of new handles and the self-test hooks' allocations with an 8-byte pattern.  This module

* proves with two probes that the fills happen (without that the rest proves nothing),
* re-runs the smallest oracle comparisons of every module that launches kernels, with their own tolerances, under two patterns:
  a quiet NaN (survives any sum and any mask by multiplication) and 1e300 (survives the ``fmax``-style reductions and comparisons
  that drop a NaN),
* and demands of the calls documented as reproducible that clean and poisoned runs agree in every bit: pollution below a 1e-9
  oracle tolerance still shows.
"""
import ctypes as C

import numpy as np
import pytest

import tests.test_gpu_als as ALS
import tests.test_gpu_als_eig as ALSE
import tests.test_gpu_braket as BK
import tests.test_gpu_complex as CX
import tests.test_gpu_cross as CR
import tests.test_gpu_cross_batch as CRB
import tests.test_gpu_dense_operator as DOP
import tests.test_gpu_densefact as DF
import tests.test_gpu_dmrg as DMRG
import tests.test_gpu_eig_ortho as EO
import tests.test_gpu_eigsolve as ES
import tests.test_gpu_expect as EX
import tests.test_gpu_expect_grad as EG
import tests.test_gpu_grad as G
import tests.test_gpu_kernels as K
import tests.test_gpu_lu as LU
import tests.test_gpu_mals as MALS
import tests.test_gpu_measure as ME
import tests.test_gpu_opalg as OA
import tests.test_gpu_opbatch as OB
import tests.test_gpu_parity as P
import tests.test_gpu_prolongation as PR
import tests.test_gpu_qttnd as QN
import tests.test_gpu_resite as RS
import tests.test_gpu_sample as SA
import tests.test_gpu_steppers as ST
import tests.test_gpu_swap_chain as SW
import tests.test_gpu_sym_eig as SE
import tests.test_gpu_tdvp as TD
import tests.test_gpu_ttv_decomp as TV
from oracle import tt_oracle as O
from tests.helpers import to_oracle, to_product
from tests.test_gpu_cross import torch            # noqa: F401  (module-scoped fixtures of the re-run modules, used under their own names)
from tests.test_gpu_measure import class_case     # noqa: F401
from tests.test_gpu_prolongation import D         # noqa: F401

pytestmark = pytest.mark.gpu

QNAN = 0x7FF8000000000000
BIG = int(np.float64(1e300).view(np.uint64))
PATTERNS = [pytest.param(QNAN, id="qnan"), pytest.param(BIG, id="1e300")]


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _mode(T, on, pattern=0):
    assert T._lib.lib().ttn_selftest_poison(int(on), C.c_uint64(pattern)) == 0


@pytest.fixture(autouse=True, params=PATTERNS)
def pattern(T, request):
    _mode(T, 1, request.param)
    try:
        yield request.param
    finally:
        _mode(T, 0)


# ---- positive controls: the fills happen ---------------------------------------------------------------------------------------------
def _peek_workspace(T, nbytes):
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert T._lib.lib().ttn_selftest_workspace_peek(nbytes, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _peek_train(T, h, b, off, n):
    out = np.zeros(n)
    assert T._lib.lib().ttn_selftest_tt_peek(h.h, b, off, n, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return out.view(np.uint64)


def test_workspace_is_filled_at_every_acquisition(T, pattern):
    """First and last word of the whole buffer, after a call that wrote real numbers into it, and for a size that is no multiple of 8."""
    x = T.DeviceTT.from_host(to_product(O.rand_tt((2,) * 6, 3, np.random.default_rng(0))))
    assert np.isfinite(T.device.dot(x, x)).all()                      # leaves its partial products in the workspace
    assert _peek_workspace(T, 8) == (pattern, pattern)
    assert _peek_workspace(T, (1 << 20) + 12) == (pattern, pattern)  # grows the buffer


def test_new_handle_has_poisoned_slack_and_a_zero_live_block(T, pattern):
    """dims (2, 3), capacity (1, 4, 1), two trains, Float64 and ComplexF64: slot k holds el n_k zeros (the rank-1 zero train), then the
    pattern up to the end of the slot; ranks, upload and download behave as ever."""
    for dtype, el in ((np.float64, 1), (np.complex128, 2)):
        h = T.DeviceTT((2, 3), [1, 4, 1], batch=2, dtype=dtype)
        slots = [(0, el * 2, el * 8), (el * 8, el * 3, el * 12)]         # (offset, live doubles, slot doubles)
        for b in range(2):
            assert list(h.ranks(b)[0]) == [1, 1, 1]
            for off, live, size in slots:
                w = _peek_train(T, h, b, off, size)
                assert not w[:live].any(), (dtype, b, off)
                assert (w[live:] == pattern).all(), (dtype, b, off)
            z = h.download(b)
            assert all(not np.asarray(c).any() for c in z.ttv_vec)
        h.free()
    x = to_product(O.rand_tt((2, 3), 2, np.random.default_rng(1)))
    h = T.DeviceTT.from_host(x, cap_rks=[1, 4, 1])
    assert all(np.array_equal(a, b) for a, b in zip(h.download(0).ttv_vec, x.ttv_vec))
    w = _peek_train(T, h, 0, 0, 8)                        # slot 0 after the upload of a (2, 1, 2) core: 4 live doubles, 4 of slack
    assert not (w[:4] == pattern).any() and (w[4:] == pattern).all()
    h.free()


def test_mode_off_shows_what_it_shows_today(T, pattern):
    other = pattern ^ 0xFFFF
    _mode(T, 1, other)
    assert _peek_workspace(T, 8) == (other, other)
    _mode(T, 0)
    assert _peek_workspace(T, 8) == (other, other)                   # an acquisition leaves the buffer as the last call left it
    h = T.DeviceTT((2, 3), [1, 4, 1], batch=2)
    for b in range(2):
        assert not _peek_train(T, h, b, 0, 20).any()                 # a new handle is zeroed whole
    h.free()


# ---- re-runs of the other modules' oracle comparisons (their tolerances, their code) -------------------------------------------------
@pytest.fixture(params=[0, 1], ids=["wg1024", "wg512"])
def build(request, monkeypatch):
    """The compress cases once per build of k_compress"""
    if request.param:
        monkeypatch.setenv("TTN_WG512", "1")
    return request.param


def test_parity_apply_compress_vs_oracle(T, build):
    P.test_apply_compress_vs_oracle(T, 12, 16, 2)


def test_parity_ragged_batch_different_ranks_per_train(T, build):
    P.test_ragged_batch_different_ranks_per_train(T)


def test_parity_compress_fuzz_ragged_ranks(T, build):
    P.test_compress_fuzz_ragged_ranks(T)


def test_parity_orthogonalize_fuzz_ragged_ranks(T):
    P.test_orthogonalize_fuzz_ragged_ranks(T)


@pytest.mark.parametrize("name", list("abce"))
def test_parity_golden_random_small(T, build, name):
    P.test_golden_random_small(T, name)


def test_parity_golden_config1(T, build):
    P.test_golden_config1(T)


def test_parity_apply_beyond_the_lds_staging_and_long_ragged_dots(T):
    P.test_apply_with_operator_cores_beyond_the_lds_staging_and_long_ragged_dots(T)


MNK = [(1, 1, 1), (17, 33, 5), (130, 70, 37)]


@pytest.mark.parametrize("m,n,k", MNK)
@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_kernels_gemm_exact_on_integers(T, m, n, k, ta, tb):
    K.test_wg_gemm_exact_on_integers(T, m, n, k, ta, tb)


@pytest.mark.parametrize("p,q", [(1, 1), (17, 33), (130, 70)])
@pytest.mark.parametrize("ta", [0, 1])
def test_kernels_syrk_exact_on_integers(T, monkeypatch, p, q, ta):
    K.test_wg_syrk_exact_on_integers(T, monkeypatch, p, q, ta, 0)


@pytest.mark.parametrize("m,n,k", MNK)                   # (130, 70, 37) is beyond the register-A form: the general GEMM takes it
@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 1)])
def test_kernels_gemm_ra_exact_on_integers(T, monkeypatch, m, n, k, ta, tb):
    K.test_wg_gemm_ra_exact_on_integers(T, monkeypatch, m, n, k, ta, tb, 0)


@pytest.mark.parametrize("n,r,nev,decades,seed", [(128, 64, 64, 1.5, 0), (64, 20, 64, 2.0, 5)])
def test_kernels_eig_selftest(T, n, r, nev, decades, seed):
    K.test_eig_selftest(n, r, nev, decades, seed)


@pytest.mark.parametrize("N", [31, 32, 33])
def test_sym_eig_families_around_the_panel_width(T, N):
    SE.test_families(T, N)


@pytest.mark.parametrize("N", [31, 32, 33])
def test_lu_pivots_and_backward_error(T, N):
    LU.test_lu_pivots_and_backward_error_vs_lapack(T, N)


def test_lu_grid_form(T):
    LU.test_lu_grid_form_equals_one_workgroup_form(T, 33)


@pytest.mark.parametrize("na,nb,Rz", [(1, 1, 1), (17, 33, 5)])
def test_lu_two_site_apply_exact_on_integers(T, na, nb, Rz):
    LU.test_two_site_apply_is_exact_on_integers(T, na, nb, Rz)


def test_expect_d1_and_d2(T):
    EX.test_d1_and_d2()


def test_expect_general_route_mixed_dims_ragged_batch_and_zero_train(T):
    EX.test_general_route_mixed_dims_ragged_batch_and_zero_train()


def test_expect_one_batch_two_routes(T):
    EX.test_one_batch_two_routes()


def test_expect_limits_of_the_qtt_route(T):
    EX.test_limits_of_the_qtt_route_inside_and_outside()


@pytest.mark.parametrize("ca,cx", BK.FORMS)
def test_braket_d1_and_d2(T, ca, cx):
    BK.test_d1_and_d2(ca, cx)


@pytest.mark.parametrize("ca,cx", BK.FORMS)
def test_braket_general_route_mixed_dims_ragged_batch_and_zero_train(T, ca, cx):
    BK.test_general_route_mixed_dims_ragged_batch_and_zero_train(ca, cx)


@pytest.mark.parametrize("ca,cx", BK.FORMS)
def test_braket_one_batch_two_routes(T, ca, cx):
    BK.test_one_batch_two_routes(ca, cx)


@pytest.mark.parametrize("ca,cx", BK.FORMS)
def test_braket_limits_of_the_on_chip_route(T, ca, cx):
    BK.test_limits_of_the_on_chip_route_inside_and_outside(ca, cx)


def test_measure_general_route_mixed_dims(T):
    ME.test_general_route("mixed_dims")


@pytest.mark.parametrize("dims", [(2,), (3, 2)])
def test_measure_edges_d1_d2(T, dims):
    ME.test_edges_d1_d2_single_train(dims)


def test_measure_on_chip_class(T, class_case):
    ME.test_class_site_expect_three_tables_at_once(class_case)
    ME.test_class_correlation_matrix(class_case)


@pytest.mark.parametrize("born", [True, False], ids=["born", "density"])
def test_sample_mixed_dims_d1_d2_and_on_chip_class(T, born):
    SA.test_general_route("mixed_dims", 200, 13, born)
    SA.test_edge_sizes("d1", 65, 14, born)
    SA.test_edge_sizes("d2", 65, 15, born)
    SA.test_on_chip_class(born)


def test_grad_dot_pullback_ragged_batch_and_single_outputs(T):
    G.test_dot_pullback_ragged_batch_and_single_outputs(T)


def test_grad_apply_pullback_ragged(T):
    G.test_apply_pullback(T, "ragged")


def test_expect_grad_ragged_batch_zero_train_and_single_outputs(T):
    EG.test_general_route_ragged_batch_zero_train_and_single_outputs(T)


def test_expect_grad_d1_and_d2(T):
    EG.test_d1_and_d2(T)


@pytest.mark.parametrize("grid", [0, 1])
def test_als_batch_with_ragged_rhs_ranks(T, monkeypatch, grid):
    ALS.test_als_batch_with_ragged_rhs_ranks(T, monkeypatch, grid)


def test_mals_ragged_batch(T):
    MALS.test_mals_ragged_batch(T)


def test_dmrg_ragged_batch(T):
    DMRG.test_dmrg_ragged_batch(T)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("it_solver", [False, True])
def test_eigsolve_ragged_batch_equals_single_calls(T, mode, it_solver):
    ES.test_ragged_batch_equals_single_calls(T, mode, it_solver)


def test_als_eig_batch_and_zero_noise_padding(T):
    ALSE.test_batch_equals_single_calls(T)
    ALSE.test_noise_zero_is_exact_padding(T)


@pytest.mark.parametrize("mode,n_ortho,case", [(1, 1, 0), (0, 3, 2)])
def test_eig_ortho_parity_dense(T, mode, n_ortho, case):
    EO.test_parity_dense(T, mode, n_ortho, *EO.PARITY[case])


def test_complex_compress_random_batches(T):
    CX.test_compress_random_batches()


def test_complex_apply_add_hadamard_dot(T):
    CX.test_apply_against_oracle(2, "cc")
    CX.test_apply_against_oracle(1, "rc")
    CX.test_add_hadamard_scale(2)
    CX.test_dot_norm(2)


def test_opalg_ragged_product_sum_kron_and_rounding(T):
    OA.test_mul(*OA.CASES[0])
    OA.test_add_sub_scale(*OA.SMALL[2])
    OA.test_inner_and_kron(*OA.SMALL[2])
    OA.test_ornstein_generator_dense_d4()


@pytest.mark.parametrize("cap", [None, [1, 5, 4, 1]])
def test_opbatch_from_tt_batch_packs_capacity_strided_slots(T, cap):
    OB.test_from_tt_batch_packs_capacity_strided_slots(cap)


def test_opbatch_lincomb_and_apply(T):
    OB.test_lincomb()
    OB.test_apply("mixed")


def test_resite_one_split_one_merge(T):
    RS.test_split_batch_with_different_ranks()
    RS.test_merge_batch_with_different_ranks()


def test_prolongation_rounded_three_train_case(T, D):
    PR.test_batch_with_different_current_ranks(T, D)


def test_steppers_apply_axpby_ragged_and_exact_zero_pad(T):
    ST.test_apply_axpby_equals_the_composition_in_every_bit(*OA.CASES[0])
    ST.test_device_increase_ranks_zero_noise()


@pytest.mark.parametrize("d,rx,ry,seed", [(2, 2, 2, 5), (6, 2, 3, 0)])
def test_swap_chain_hadamard_ttm(T, d, rx, ry, seed):
    SW.test_hadamard_ttm_random_vs_oracle(T, d, rx, ry, seed)


def test_ttv_decomp_batch_and_capacity(T):
    TV.test_ttv_decomp_batch_and_capacity(T)


def test_cross_smallest_maxvol_parity(T, torch):
    CR.test_maxvol_matches_restatement(torch, 7, 1, True)
    CR.test_maxvol_matches_restatement(torch, 64, 8, False)
    CR.test_cross_parity_with_restatement(torch, CR.PARITY[0])


def test_cross_batch_smallest_maxvol_parity(T, torch):
    CRB.test_site_kernel_matches_restatement(torch, 65, 3, 5, 13, 3, 0)
    CRB.test_driver_parity_per_function(torch, CRB.PARITY[0])


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,n", [(1, 1), (7, 16), (33, 130)])
def test_densefact_qr_and_svd(T, cplx, m, n):
    DF.test_dense_qr(T, cplx, m, n)
    DF.test_dense_svd(T, cplx, m, n)


@pytest.mark.parametrize("cplx", [False, True])
def test_densefact_svd_zero_columns(T, cplx):
    DF.test_dense_svd_zero_columns_and_rows(T, cplx, 40, 12)


@pytest.mark.parametrize("cplx", [False, True])
def test_tdvp_two_shapes_per_contraction(T, cplx):
    for s in (TD.SHAPES[0], TD.SHAPES[2]):
        TD.test_applyH1_vs_oracle(T, cplx, *s)
    for s in ((3, 2, 4), (40, 64, 4)):
        TD.test_applyH0_vs_oracle(T, cplx, *s)
    for s in ((2, 3, 4, 2, 5), (64, 2, 33, 3, 3)):
        TD.test_env_updates_vs_oracle(T, cplx, *s)
    for s in ((2, 2, 3, 2, 2, 3, 2), (16, 2, 2, 24, 3, 3, 3)):
        TD.test_applyH2_vs_oracle(T, cplx, *s)


def test_qttnd_to_dense_and_decomp(T):
    QN.test_to_dense_batch_of_three()
    QN.test_ttv_decomp_dev_is_bitwise_ttv_decomp()


def test_dense_operator_to_dense_and_from_dense(T):
    DOP.test_to_dense_entrywise_both_layouts((3, 2, 2, 3), 3, 5)
    DOP.test_from_dense_matrix_layout_round_trip()


# ---- the other routes of the same modules: thresholds between kernels, tile edges, the iterative local solvers --------------------------
@pytest.mark.parametrize("d,ra,rb,seed", [(9, 5, 13, 0), (7, 16, 17, 4), (2, 2, 2, 5)])
def test_parity_dot_lds_resident_path_odd_ranks(T, d, ra, rb, seed):
    P.test_dot_lds_resident_path_odd_ranks(T, d, ra, rb, seed)


def test_parity_orthogonalize_every_kernel(T, monkeypatch):
    P.test_orthogonalize_vs_oracle(T, 12, 20, 7)
    P.test_orthogonalize_three_launch_form(T, monkeypatch, 16, 37, 1, 2)
    P.test_orthogonalize_three_launch_form(T, monkeypatch, 9, 5, 2, 5)
    P.test_orthogonalize_hand_over_between_the_kernels(T, monkeypatch)


def test_parity_compress_odd_sizes_fallback_and_long_panel(T, build):
    P.test_compress_general_dims_and_odd_sizes(T)
    P.test_compress_short_side_above_128_uses_fallback(T)
    P.test_compress_long_panel_householder(T)
    P.test_bond_truncate_every_bond(T)


@pytest.mark.parametrize("d,kind,xr,max_bond,truncerr,seed", [(12, 0, 64, 64, 0.0, 0), (12, 1, 64, 33, 0.0, 2), (12, 2, 64, 64, 1e-8, 3), (12, 0, 32, 32, 0.0, 6)])
def test_parity_apply_compress_eigen_routes(T, build, d, kind, xr, max_bond, truncerr, seed):
    P.test_apply_compress_eigen_routes_vs_oracle(T, d, kind, xr, max_bond, truncerr, seed)


def test_parity_fused_merge_mixed_dims_and_sweep_ranges(T, monkeypatch, build):
    P.test_fused_apply_compress_equals_apply_then_compress(T, monkeypatch, (2, 3, 2, 2, 3, 2, 2), [1, 2, 3, 2, 4, 2, 3, 1], 5, 6)
    P.test_sweep_ranges_and_core_handoff_reproduce_compress(T)


def test_parity_compress_blocked_jacobi_rank_100(T, build):
    P.test_compress_ranks_up_to_128_blocked_jacobi(T, 14, 100, 100)


def test_expect_and_braket_on_chip_routes(T):
    EX.test_qtt_route_dense_nonsymmetric_operator(9, 5, 13, 3)
    EX.test_qtt_route_dense_nonsymmetric_operator(7, 16, 17, 1)
    for ca, cx in BK.FORMS:
        BK.test_on_chip_route_dense_nonsymmetric_operator(9, 5, 13, 2, ca, cx)
    BK.test_on_chip_route_zero_train_is_exactly_zero()


def test_gradients_tile_edges_and_two_routes(T):
    for name in ("d1", "tile_edges", "mixed_dims"):
        G.test_dot_pullback_shapes(T, name)
    EG.test_on_chip_tile_edges(T, 15, 16)
    EG.test_on_chip_tile_edges(T, 16, 17)
    EG.test_one_batch_two_routes(T)


@pytest.mark.parametrize("born", [True, False], ids=["born", "density"])
def test_measure_and_sample_rank_80(T, born):
    if born:
        ME.test_general_route("rank80_d14")
    SA.test_general_route("rank80_d10", 130, 12, born)


def test_linear_solvers_grid_form_pivoting_and_matrix_free(T, monkeypatch):
    ALS.test_als_grid_form_equals_one_workgroup_form(T, monkeypatch, 8, 4, 0.5, 3)
    ALS.test_als_pivoting_operator_vs_oracle(T, monkeypatch, 2, 1)
    MALS.test_mals_mixed_dims_vs_oracle(T)
    DMRG.test_dmrg_matrix_free_cg_vs_oracle_and_dense(T, 6, 2, 2, 2.0, 1e-10, [2], [8], 1e-12, 0)
    DMRG.test_dmrg_itslv_thresh_switches_per_system(T)
    DMRG.test_dmrg_mixed_dims_vs_oracle(T, True)


@pytest.mark.parametrize("mode", [1, 0])
def test_eigensolvers_lanczos_and_mixed_dims(T, mode):
    ES.test_lanczos_vs_dense(T, mode)
    ES.test_mixed_dims_parity_dense(T, mode, ES.MIXED[0])
    EO.test_lanczos_vs_dense(T, mode)
    if mode:
        ALSE.test_matrix_free_against_dense(T)


@pytest.mark.parametrize("N", [64, 255, 256])
def test_sym_eig_families_larger(T, N):
    SE.test_families(T, N)


@pytest.mark.parametrize("N", [65, 257, 513])
def test_lu_beyond_one_panel(T, N):
    LU.test_lu_pivots_and_backward_error_vs_lapack(T, N)
    if N == 513:
        LU.test_lu_grid_form_equals_one_workgroup_form(T, 544)


def test_swap_chain_reorder_and_swap_sites(T):
    SW.test_reorder_is_the_axis_permutation(T, 2, 3, 3, 0)
    SW.test_swap_sites_batch_and_errors(T)


def test_resite_wide_merge_and_threshold(T):
    RS.test_merge_wide_second_operand((3, 20), (1, 17, 1), [2])
    RS.test_merge_wide_second_operand((2, 3, 37), (1, 2, 18, 2), [3])
    RS.test_split_threshold()


def test_opbatch_pullback_eigensolver_and_axpby(T):
    for route in ("qtt", "general"):
        OB.test_sandwich_pullback(route)
    OB.test_two_site_eigensolvers(1)
    OB.test_apply_axpby("mixed")


def test_complex_bond_step_and_qft_product(T):
    CX.test_bond_step_singular_values()
    CX.test_compress_qft_products("qtt_sin")


@pytest.mark.parametrize("cplx", [False, True])
def test_densefact_larger_shapes(T, cplx):
    for m, n in ((128, 64), (257, 12)):
        DF.test_dense_qr(T, cplx, m, n)
        DF.test_dense_svd(T, cplx, m, n)


def test_cross_maxvol_beyond_one_tile(T, torch):
    CR.test_maxvol_matches_restatement(torch, 180, 90, False)
    CR.test_maxvol_matches_restatement(torch, 130, 64, True)


def test_ttv_decomp_and_dense_export_other_shapes(T):
    TV.test_ttv_decomp_full_rank_vs_oracle(T, (3, 2, 4, 2, 3), 1, 3)
    QN.test_to_dense_shapes((2, 3, 4, 2, 5), 4)
    QN.test_to_dense_shapes((2, 2, 64), 4)
    DOP.test_to_dense_entrywise_both_layouts((65, 2), 3, 1)
    DOP.test_tto_decomp_of_the_dense_laplacian(4, 2)


# ---- clean against poisoned, bit for bit ---------------------------------------------------------------------------------------------
def _bits(out, tag, t):
    out[tag] = b"".join(np.ascontiguousarray(c).tobytes() for c in t.ttv_vec) + np.asarray(list(t.ttv_rks) + list(t.ttv_ot), dtype=np.int64).tobytes()


def _reproducible_calls(T):
    """The calls documented as reproducible, each into FRESH handles whose capacity lies above the ranks (so there is slack), on fixed
    inputs.  Returns {label: bytes of every downloaded live core, rank, gauge flag and host output}.
    The ranks stay at 3: dot, sandwich, site_expect, Born sampling and dot_pullback add with LDS atomics on their on-chip routes and
    are bitwise reproducible only while one wave per column block adds, i.e. up to rank 16 (DESIGN §4.3, §4.25, §4.28, §4.29;
    tests/test_gpu_host_state.py relies on the same)."""
    Dv = T.device
    out = {}
    own = []                                     # every handle made here, freed on every way out

    def keep(h):
        own.append(h)
        return h

    try:
        _run_reproducible_calls(T, Dv, out, keep)
    finally:
        for h in reversed(own):
            h.free()
    return out


def _run_reproducible_calls(T, Dv, out, keep):
    d, B = 8, 3
    dims = (2,) * d
    rng = np.random.default_rng(4)
    cap = [1] + [24] * (d - 1) + [1]
    rks = ([1, 2, 3, 3, 3, 3, 3, 2, 1], [1, 2, 2, 2, 2, 2, 2, 2, 1], [1, 1, 2, 3, 2, 3, 2, 1, 1])       # a ragged batch

    def ragged():
        h = keep(T.DeviceTT(dims, cap, batch=B))
        for b in range(B):
            h.upload(b, to_product(O.rand_tt(dims, list(rks[b]), rng)))
        return h

    A = keep(T.DeviceTTO(to_product(O.tto_add(O.Delta(d), O.tto_scale(1.5, O.id_tto(d))))))
    x, y = ragged(), ragged()
    for name, fn in (("apply", lambda z: Dv.apply(A, x, z)), ("add", lambda z: Dv.add(x, y, z)), ("hadamard", lambda z: Dv.hadamard(x, y, z)),
                     ("scale_batch", lambda z: Dv.scale_batch([0.5, -2.0, 3.0], x, z)), ("orthogonalize", lambda z: Dv.orthogonalize(x, 4, z))):
        z = keep(T.DeviceTT(dims, cap, batch=B))
        fn(z)
        for b in range(B):
            _bits(out, "%s train %d" % (name, b), z.download(b))
    out["dot"] = np.ascontiguousarray(Dv.dot(x, y)).tobytes()
    out["sandwich"] = np.ascontiguousarray(Dv.sandwich(x, A, y)).tobytes()
    z = keep(T.DeviceTT(dims, cap, batch=B))
    Dv.hadamard(x, y, z)
    Dv.tt_compress_(z, 5, truncerr=1e-10)
    Dv.compress_status(z)
    for b in range(B):
        _bits(out, "tt_compress_ train %d" % b, z.download(b))
    out["site_expect"] = np.ascontiguousarray(Dv.site_expect(x, np.diag([1.0, -1.0]))).tobytes()
    idx, logp, _ = Dv.sample(x, 64, "born", seed=7)
    out["sample idx"] = np.ascontiguousarray(idx).tobytes()
    out["sample logp"] = np.ascontiguousarray(logp).tobytes()
    val, abar, bbar = T.grad.dot_pullback(x, y, delta=[0.5, -2.0, 1.0])
    keep(abar), keep(bbar)
    out["dot_pullback value"] = np.ascontiguousarray(val).tobytes()
    for b in range(B):
        _bits(out, "dot_pullback abar %d" % b, abar.download(b))
        _bits(out, "dot_pullback bbar %d" % b, bbar.download(b))
    # dmrg_eigsolve_ on the inputs of tests/test_gpu_host_state.py::test_finalize_then_init_repeats_bitwise
    ising = keep(T.DeviceTTO(to_product(to_oracle(T.ising_tto(d, J=1.0, h=1.5)))))
    e0 = keep(T.DeviceTT.from_host(to_product(O.rand_tt(dims, 4, np.random.default_rng(44))), batch=2))
    ev = keep(T.DeviceTT(dims, T.solvers.dmrg_capacity(dims, e0.cap, 8), batch=2))
    E, rh = T.solvers.dmrg_eigsolve_(ising, e0, ev, 1e-12, [3], [8])
    out["dmrg_eigsolve_ E"] = np.asarray(E, dtype=np.float64).tobytes()
    out["dmrg_eigsolve_ ranks"] = np.asarray(rh, dtype=np.int64).tobytes()
    for b in range(2):
        _bits(out, "dmrg_eigsolve_ train %d" % b, ev.download(b))
    Dv.status_all()


@pytest.fixture(scope="module")
def clean_run(T):
    """The reference of the bitwise check: computed once with the mode off, left unchanged.  An off-mode acquisition leaves the
    workspace as the last call left it, and here that is an earlier test's pattern: a kernel that read unwritten workspace would read
    the same 1e300 in the reference as in the poisoned run and match it.  So the residue is scrubbed first — one filling acquisition
    with the pattern 0, of 64 MiB so that the calls below (a few MiB) never grow the buffer into raw memory — and the reference sees
    what a young process shows: zeros where nobody wrote."""
    _mode(T, 1, 0)
    assert _peek_workspace(T, 64 << 20) == (0, 0)
    _mode(T, 0)
    return _reproducible_calls(T)


def test_clean_and_poisoned_runs_agree_in_every_bit(T, clean_run, pattern):
    _mode(T, 1, pattern)          # (clean_run ends with the mode off whenever it is set up)
    got = _reproducible_calls(T)
    assert got.keys() == clean_run.keys()
    differ = [k for k in got if got[k] != clean_run[k]]
    assert not differ, differ
