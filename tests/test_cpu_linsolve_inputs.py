"""CPU pins of what the linear-solver GPU tests (test_gpu_als / _mals / _dmrg, tests/linsolve_reference.py) take for granted about
their inputs and about the oracle.  Above all: on a non-symmetric operator the reference's dense two-site solve `Hermitian(K) \\ b`
(mals.jl:156,167; dmrg.jl:53,174) reads only the upper triangle of K, so mals_linsolve does NOT return A \\ b even with full ranks.
That is the reference's behaviour, restated by the oracle and mirrored by the device; the pin below keeps a later reader from
"fixing" the oracle to the Galerkin solution and the GPU tests to a device that solves the full K."""
import numpy as np

from oracle import tt_oracle as O
from tests.linsolve_reference import A_cd, A_piv, mixed_dims_operator, pivot_spy, tt_to_vector, tto_to_matrix


def test_operators_are_what_the_tests_say():
    M = O.qtto_to_matrix(A_piv(8))
    assert abs(np.linalg.cond(M) - 3.4) < 0.1 and np.linalg.norm(M - M.T) > 0.1 * np.linalg.norm(M)
    M = O.qtto_to_matrix(A_cd(6))
    assert abs(np.linalg.norm(M - M.T) / np.linalg.norm(M) - 0.56) < 0.01
    assert abs(np.linalg.cond(M) - 8.9) < 0.1
    assert abs(np.min(np.linalg.eigvalsh(0.5 * (M + M.T))) - 0.50) < 0.01
    dims = (2, 3, 2, 3, 2)
    A = mixed_dims_operator(dims, np.random.default_rng(63))
    M = tto_to_matrix(A)
    assert M.shape == (72, 72) and np.linalg.norm(M - M.T) > 0.05 * np.linalg.norm(M)
    assert np.min(np.linalg.eigvalsh(0.5 * (M + M.T))) >= 2.0 - 1e-12 and np.linalg.cond(M) <= 3.0 + 1e-12
    x = O.rand_tt(dims, 2, np.random.default_rng(1))
    assert np.allclose(tt_to_vector(O.apply(A, x)), M @ tt_to_vector(x), rtol=1e-12, atol=1e-12)


def test_oracle_mals_on_a_nonsymmetric_operator_is_not_the_dense_solution():
    """Full ranks on A_cd: a solver on the full K would return A \\ b; the reference's upper-triangle solve is 0.6 away from it."""
    d = 6
    rng = np.random.default_rng(61)
    A = A_cd(d)
    b, x0 = O.rand_tt((2,) * d, 2, rng), O.rand_tt((2,) * d, 2, rng)
    ref = O.mals_linsolve(A, b, x0, tol=0.0, rmax=64)
    assert list(ref.ttv_rks) == [1, 2, 4, 8, 4, 2, 1]
    dense = np.linalg.solve(O.qtto_to_matrix(A), O.qtt_to_vector(b))
    assert np.linalg.norm(O.qtt_to_vector(ref) - dense) > 0.1 * np.linalg.norm(dense)
    # on the symmetric part of the same operator it IS the dense solution
    S = O.toeplitz_to_qtto(2.5, -1.0, -1.0, d)
    ref = O.mals_linsolve(S, b, x0, tol=0.0, rmax=64)
    dense = np.linalg.solve(O.qtto_to_matrix(S), O.qtt_to_vector(b))
    assert np.linalg.norm(O.qtt_to_vector(ref) - dense) < 1e-10 * np.linalg.norm(dense)


def test_oracle_dmrg_cg_and_dense_branches_differ_on_a_nonsymmetric_operator():
    d = 8
    rng = np.random.default_rng(62)
    b, x0 = O.rand_tt((2,) * d, 2, rng), O.rand_tt((2,) * d, 3, rng)
    kw = dict(tol=1e-10, sweep_schedule=[2], rmax_schedule=[8])
    cg = O.qtt_to_vector(O.dmrg_linsolve(A_cd(d), b, x0, it_solver=True, linsolv_tol=1e-12, **kw))
    de = O.qtt_to_vector(O.dmrg_linsolve(A_cd(d), b, x0, **kw))
    assert np.linalg.norm(cg - de) > 1e-3 * np.linalg.norm(de)


def test_pivot_spy_sees_no_exchange_beyond_the_first_panel_on_the_old_inputs_and_all_on_a_piv():
    """The gap the A_piv tests close: Delta + sigma I never exchanges rows at a step >= 32 (d = 10, r = 6 of test_als_vs_oracle),
    A_piv does in every local system with N > 32."""
    rng = np.random.default_rng(3)
    A = O.tto_add(O.Delta(10), O.id_tto(10))
    with pivot_spy() as log:
        O.als_linsolve(A, O.rand_tt((2,) * 10, 2, rng), O.rand_tt((2,) * 10, 6, rng), sweep_count=2)
    assert len(log.beyond_first_panel()) == 12 and all(e[1] == 0 for e in log)
    assert O.np.linalg.solve is np.linalg.solve                     # the spy restored what it patched
    rng = np.random.default_rng(42)
    with pivot_spy() as log:
        O.als_linsolve(A_piv(8), O.rand_tt((2,) * 8, 3, rng), O.rand_tt((2,) * 8, 8, rng), sweep_count=2)
    assert len(log.beyond_first_panel()) == 8
    log.assert_pivots_beyond_first_panel(at_least=8)
