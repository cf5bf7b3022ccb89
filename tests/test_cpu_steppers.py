"""CPU tests of the stepper family (no GPU): the NumPy restatement (tests/stepper_reference.py) against dense solves at the reference's
own bars (test/test_euler.jl), the host increase_ranks at noise = 0 (test/test_tt_tools.jl:949-967), the argument handling that needs
no device, and the C header include/ttn_step.h against the ctypes table."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import stepper_reference as R
from tests.helpers import to_oracle, to_product

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = [0.05]


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    return ttn_amd


def _dense(x):
    return R.dense_sequential(x)                      # (the product's ttv_to_tensor runs on the device; this one is padding-invariant)


def _case(d, rks, seed):
    rng = np.random.default_rng(seed)
    return R.heat_operator(d), O.rand_tt((2,) * d, rks, rng)


# ---- the restatement against dense solves (test/test_euler.jl) ---------------------------------------------------------------------------
def test_restatement_implicit_euler_dmrg():
    """:34-58, bar 1e-5"""
    A, u0 = _case(4, [1, 2, 2, 2, 1], 1)
    sol = R.implicit_euler_method(A, u0, u0, STEPS, normalize=False, tt_solver="dmrg")
    assert R.rel(O.qtt_to_vector(sol), R.dense_implicit_euler(A, u0, STEPS)) < 1.0e-5


def test_restatement_crank_nicholson_mals():
    """:87-110, bar 1e-5; and the d = 6 case at the default rmax, which truncates (2.8e-6 in the issue's table)"""
    A, u0 = _case(4, [1, 2, 2, 2, 1], 2)
    sol = R.crank_nicholson_method(A, u0, u0, STEPS, normalize=False, tt_solver="mals")
    assert R.rel(O.qtt_to_vector(sol), R.dense_crank_nicholson(A, u0, STEPS)) < 1.0e-5
    A, u0 = _case(6, [1, 2, 3, 3, 3, 2, 1], 3)
    sol = R.crank_nicholson_method(A, u0, u0, STEPS * 3, normalize=False, tt_solver="mals")
    assert R.rel(O.qtt_to_vector(sol), R.dense_crank_nicholson(A, u0, STEPS * 3)) < 1.0e-5


@pytest.mark.parametrize("d,rks", [(4, [1, 2, 4, 2, 1]), (6, [1, 2, 4, 8, 4, 2, 1])])
@pytest.mark.parametrize("method", ["ie", "cn"])
def test_restatement_full_rank_als(d, rks, method):
    """ALS at full rank solves every step exactly: 1e-10 after three steps (the measured figures are 1e-15)"""
    A, u0 = _case(d, rks, 4)
    steps = STEPS * 3
    if method == "ie":
        sol, ref = R.implicit_euler_method(A, u0, u0, steps, normalize=False, tt_solver="als"), R.dense_implicit_euler(A, u0, steps)
    else:
        sol, ref = R.crank_nicholson_method(A, u0, u0, steps, normalize=False, tt_solver="als"), R.dense_crank_nicholson(A, u0, steps)
    assert sol.ttv_rks == rks
    assert R.rel(O.qtt_to_vector(sol), ref) < 1.0e-10


def test_restatement_explicit_euler_and_rk4_error():
    """:5-31 explicit Euler < 1e-6; :300-313 RK4 return_error < 1e-10"""
    A, u0 = _case(4, [1, 2, 2, 2, 1], 5)
    sol, err = R.euler_method(A, u0, STEPS, normalize=False, return_error=True)
    ud = O.qtt_to_vector(u0)
    assert R.rel(O.qtt_to_vector(sol), ud + STEPS[0] * (R.dense(A) @ ud)) < 1.0e-6
    assert np.isfinite(err)
    _, rk_err = R.rk4_method(A, u0, STEPS, 8, normalize=False, return_error=True)
    assert rk_err < 1.0e-10


def test_restatement_return_error_is_the_dense_residual():
    """the residual formulas of :134-139 and :181-187 against the same formulas on dense vectors (normalize = true as at :237-266)"""
    A, u0 = _case(3, [1, 2, 2, 1], 6)
    steps = [0.02]
    Ad, I = R.dense(A), np.eye(8)
    sol, err = R.implicit_euler_method(A, u0, u0, steps, normalize=True, return_error=True, tt_solver="als")
    s, p = O.qtt_to_vector(sol), O.qtt_to_vector(u0)
    assert abs(np.linalg.norm(s) - 1.0) < 1.0e-10
    assert abs(err - np.linalg.norm((I - 0.02 * Ad) @ s - p) / np.linalg.norm(s)) < 1.0e-8
    sol, err = R.crank_nicholson_method(A, u0, u0, steps, normalize=True, return_error=True, tt_solver="dmrg")
    s = O.qtt_to_vector(sol)
    assert abs(err - np.linalg.norm((I - 0.01 * Ad) @ s - (I + 0.01 * Ad) @ p) / np.linalg.norm(s)) < 1.0e-8


# ---- host increase_ranks at noise = 0 (test/test_tt_tools.jl:949-967) --------------------------------------------------------------------
def test_increase_ranks_zero_noise_preserves_the_tensor(T):
    x = T.rand_tt((2, 3, 2, 2), [1, 2, 3, 2, 1], seed=7)
    x.ttv_ot = [1, 0, -1, -1]
    y = T.increase_ranks(x, 5)
    assert y.ttv_rks == T.r_and_d_to_rks([1, 5, 5, 5, 1], x.ttv_dims, rmax=5) == [1, 2, 4, 2, 1]
    assert y.ttv_rks == R.increase_ranks(to_oracle(x), 5).ttv_rks
    assert y.ttv_ot == [0, 0, 0, 0]
    assert np.array_equal(_dense(y), _dense(x))
    for g, r in zip(y.ttv_vec, R.increase_ranks(to_oracle(x), 5).ttv_vec):
        assert g.shape == r.shape and np.array_equal(g, r)
    z = T.increase_ranks(x, 6, rks=[1, 2, 4, 2, 1])
    assert z.ttv_rks == [1, 2, 4, 2, 1] and np.array_equal(_dense(z), _dense(x))


def test_increase_ranks_reference_case(T):
    """ranks [1, 2, 2, 1] from [1, 1, 1, 1] at max_bond = 2; max_bond = 1 is 'New bond dimension too low'"""
    x = T.rand_tt((2, 2, 2), [1, 1, 1, 1], seed=8)
    y = T.increase_ranks(x, 2)
    assert y.ttv_rks == [1, 2, 2, 1]
    assert [c.shape for c in y.ttv_vec] == [(2, 1, 2), (2, 2, 2), (2, 2, 1)]
    assert np.array_equal(_dense(y), _dense(x))
    with pytest.raises(AssertionError, match="New bond dimension too low"):
        T.increase_ranks(x, 1)
    with pytest.raises(T.TTNError, match="below the current ranks"):
        T.increase_ranks(y, 3, rks=[1, 1, 3, 1])


def test_tt_up_rks_warns_and_qttvector_keeps_its_metadata(T):
    x = T.rand_tt((2,) * 4, [1, 1, 2, 1, 1], seed=9)
    with pytest.warns(DeprecationWarning, match="tt_up_rks"):
        y = T.tt_up_rks(x, 3)
    assert y.ttv_rks == T.increase_ranks(x, 3).ttv_rks == [1, 2, 3, 2, 1]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T.increase_ranks(x, 3)                                # the new name does not warn
    q = T.QTTvector(x, 2, 2, "serial")
    for up in (q.increase_ranks(3), T.increase_ranks(q, 3)):
        assert isinstance(up, T.QTTvector)
        assert (up.n_dims, up.bits_per_dim, up.ordering) == (2, 2, "serial")
        assert up.ttv_rks == [1, 2, 3, 2, 1]
        assert np.array_equal(_dense(up.ttvector()), _dense(x))


# ---- argument handling that needs no device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["implicit_euler_method", "crank_nicholson_method"])
def test_unknown_solver_and_unknown_keyword(T, name):
    A = to_product(R.heat_operator(3))
    u = T.rand_tt((2,) * 3, [1, 2, 2, 1], seed=10)
    f = getattr(T, name)
    with pytest.raises(ValueError, match="Unknown TT solver: cg"):
        f(A, u, u, STEPS, tt_solver="cg")
    for solver, bad in (("als", "tol"), ("mals", "sweep_count"), ("dmrg", "rmax"), ("krylov", "sweep_count"), ("als", "return_info")):
        with pytest.raises(TypeError, match=bad):
            f(A, u, u, STEPS, tt_solver=solver, **{bad: 1})
    with pytest.raises(T.TTNError, match="N = 2"):
        f(A, u, u, STEPS, tt_solver="dmrg", N=1)


def test_exports(T):
    for name in ("euler_method", "implicit_euler_method", "crank_nicholson_method", "rk4_method", "krylov_linsolve", "increase_ranks", "tt_up_rks"):
        assert name in T.__all__ and callable(getattr(T, name))
    assert callable(T.device.apply_axpby) and callable(T.DeviceTT.increase_ranks)


# ---- the C ABI of include/ttn_step.h -----------------------------------------------------------------------------------------------------
def test_step_header_and_ctypes_table_agree(T):
    hdr = open(os.path.join(ROOT, "include", "ttn_step.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert {n for n, _ in protos} == set(T._lib.STEP_SIGNATURES) == {"ttn_apply_axpby", "ttn_tt_increase_ranks"}
    assert not set(T._lib.STEP_SIGNATURES) & (set(T._lib.SIGNATURES) | set(T._lib.RECT_SIGNATURES) | set(T._lib.DENSE_SIGNATURES))
    L = ctypes
    table = {"int64_t*": L.POINTER(L.c_int64), "double": L.c_double, "double*": L.POINTER(L.c_double), "uint64_t": L.c_uint64,
             "ttn_tt_t": L.c_void_p, "ttn_tto_t": L.c_void_p}
    lib = T._lib.lib()
    for name, args in protos:
        res, argt = T._lib.STEP_SIGNATURES[name]
        assert res is L.c_int and hasattr(lib, name)
        types = []
        for a in [x.strip() for x in args.split(",")]:
            t = re.sub(r"\s*[A-Za-z_][A-Za-z0-9_]*$", "", re.sub(r"\bconst\b", "", a).strip())
            types.append(re.sub(r"\s+", "", t))
        assert len(types) == len(argt), name
        for ct, at in zip(types, argt):
            want = table[ct]
            assert at is want or (hasattr(at, "_type_") and hasattr(want, "_type_") and at._type_ is want._type_), (name, ct)
    assert '#include "ttn_step.h"' in open(os.path.join(ROOT, "include", "ttn.h")).read()
