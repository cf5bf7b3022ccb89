"""CPU tests of the expectation-value layer (no GPU): the Pauli-sum constructors against dense Kronecker sums, the periodic Ising operator
of examples/ising_model.jl, the refusals of a lone sigma_y, the NumPy three-layer recurrence (tests/expect_reference.py) against the
oracle's dot(x, A * y) — the yardstick of tests/test_gpu_expect.py — and the host entry points' exports, header and loud failure."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import expect_reference as R
from tests.helpers import to_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = ("x", "z")
PAIRS = (("x", "x"), ("x", "z"), ("z", "x"), ("z", "z"), ("y", "y"))


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    return ttn_amd


def mixed_case():
    """The mixed-dims case of the GPU tests: dims (2, 3, 2, 4), x ranks [1, 2, 5, 3, 1], y ranks [1, 3, 4, 2, 1], A ranks [1, 2, 3, 2, 1]."""
    rng = np.random.default_rng(20)
    dims = (2, 3, 2, 4)
    x = O.rand_tt(dims, [1, 2, 5, 3, 1], rng)
    y = O.rand_tt(dims, [1, 3, 4, 2, 1], rng)
    Ar = [1, 2, 3, 2, 1]
    A = O.TToperator(4, [rng.standard_normal((dims[k], dims[k], Ar[k], Ar[k + 1])) for k in range(4)], dims, Ar, [0] * 4)
    return x, A, y


def _dense(A):
    """The (2^d, 2^d) matrix of a product-side operator, through the oracle."""
    Ao = to_oracle(A)
    M = O.qtto_to_matrix(Ao)
    assert np.array_equal(M, O.tto_to_tensor(Ao).reshape(M.shape))
    return M


@pytest.mark.parametrize("d", [1, 2, 3, 5])
@pytest.mark.parametrize("mu", AXES)
def test_pauli_sum_tto(T, mu, d):
    A = T.pauli_sum_tto(mu, d)
    assert A.tto_rks == ([1, 1] if d == 1 else [1] + [2] * (d - 1) + [1])
    assert A.tto_dims == (2,) * d and A.tto_ot == [0] * d
    assert [c.shape for c in A.tto_vec] == [(2, 2, A.tto_rks[k], A.tto_rks[k + 1]) for k in range(d)]
    assert np.max(np.abs(_dense(A) - R.pauli_sum_dense(mu, d))) <= 1e-14
    B = T.H_mu(mu, d)
    assert all(np.array_equal(a, b) for a, b in zip(A.tto_vec, B.tto_vec))


@pytest.mark.parametrize("d", [2, 3, 5])
@pytest.mark.parametrize("pair", PAIRS)
def test_pauli_pair_sum_tto(T, pair, d):
    A = T.pauli_pair_sum_tto(pair[0], pair[1], d)
    assert A.tto_rks == [1] + [3] * (d - 1) + [1]
    assert A.tto_dims == (2,) * d and A.tto_ot == [0] * d
    assert np.max(np.abs(_dense(A) - R.pauli_pair_sum_dense(pair[0], pair[1], d))) <= 1e-14
    B = T.H_munu(pair[0], pair[1], d)
    assert all(np.array_equal(a, b) for a, b in zip(A.tto_vec, B.tto_vec))


def test_pauli_matrix(T):
    assert np.array_equal(T.pauli_matrix("x"), [[0.0, 1.0], [1.0, 0.0]])
    assert np.array_equal(T.pauli_matrix(":z"), [[1.0, 0.0], [0.0, -1.0]])
    assert np.array_equal(T.pauli_sum_tto("z", 1).tto_vec[0][:, :, 0, 0], T.pauli_matrix("z"))


def test_xy_tto_is_heisenberg_without_zz(T):
    for d, jx, jy, h, field in [(2, 1.0, 1.0, 0.0, "z"), (4, 0.7, -1.3, 0.4, "z"), (5, 2.0, 0.5, -0.6, "x")]:
        A = T.xy_tto(d, jx, jy, h, field)
        B = T.heisenberg_xyz_tto(d, jx=jx, jy=jy, jz=0.0, lam=h, field=field)
        assert A.tto_rks == B.tto_rks and A.tto_dims == B.tto_dims
        for a, b in zip(A.tto_vec, B.tto_vec):
            assert np.array_equal(a, b)
    assert np.array_equal(T.xy_tto(3).tto_vec[1], T.heisenberg_xyz_tto(3, jx=1.0, jy=1.0, jz=0.0, lam=0.0, field="z").tto_vec[1])


def periodic_ising(T, d, g):
    """periodic_transverse_field_ising_tto of examples/ising_model.jl from the new constructors and the oracle's + and scalar *."""
    Z = T.pauli_matrix("z")
    cores = [np.eye(2).reshape(2, 2, 1, 1).copy() for _ in range(d)]
    cores[0] = Z.reshape(2, 2, 1, 1).copy()
    cores[d - 1] = Z.reshape(2, 2, 1, 1).copy()
    boundary = O.TToperator(d, cores, (2,) * d, [1] * (d + 1), [0] * d)
    zz = O.tto_add(to_oracle(T.pauli_pair_sum_tto("z", "z", d)), boundary)
    return O.tto_add(O.tto_scale(-1.0, zz), O.tto_scale(-g, to_oracle(T.pauli_sum_tto("x", d))))


@pytest.mark.parametrize("g", [0.5, 1.5])
def test_periodic_ising_operator_d4(T, g):
    H = periodic_ising(T, 4, g)
    assert np.max(np.abs(O.qtto_to_matrix(H) - R.periodic_ising_dense(4, g))) <= 1e-14
    assert np.array_equal(O.qtto_to_matrix(H), O.qtto_to_matrix(H).T)


def test_single_sigma_y_is_refused(T):
    with pytest.raises(T.TTNError, match="sigma_y"):
        T.pauli_matrix("y")
    for d in (1, 3):
        with pytest.raises(T.TTNError, match="sigma_y"):
            T.pauli_sum_tto("y", d)
    with pytest.raises(T.TTNError, match="sigma_y"):
        T.H_mu(":y", 4)
    for pair in (("x", "y"), ("y", "x"), ("z", "y"), ("y", "z")):
        with pytest.raises(T.TTNError, match="sigma_y"):
            T.pauli_pair_sum_tto(pair[0], pair[1], 3)
    with pytest.raises(T.TTNError, match="unknown Pauli axis"):
        T.pauli_sum_tto("w", 3)
    assert T.pauli_pair_sum_tto("y", "y", 3).tto_rks == [1, 3, 3, 1]


def test_restatement_matches_oracle_on_mixed_dims():
    """Pins the yardstick: the three-layer recurrence equals dot(x, A * y) to 1e-13 of ||x|| ||A y||."""
    x, A, y = mixed_case()
    Ay = O.apply(A, y)
    ref = O.dot(x, Ay)
    assert abs(R.sandwich(x, A, y) - ref) <= 1e-13 * O.norm(x) * O.norm(Ay)
    dense = O.ttv_to_tensor(x).reshape(-1) @ O.ttv_to_tensor(Ay).reshape(-1)
    assert abs(ref - dense) <= 1e-13 * O.norm(x) * O.norm(Ay)
    # a transposed read of the operator is a different number
    At = O.TToperator(A.N, [np.swapaxes(c, 0, 1) for c in A.tto_vec], A.tto_dims, A.tto_rks, A.tto_ot)
    assert abs(R.sandwich(x, At, y) - ref) > 1e-6 * O.norm(x) * O.norm(Ay)
    assert abs(R.sandwich(y, At, x) - ref) <= 1e-13 * O.norm(x) * O.norm(Ay)


def test_restatement_dense_helpers():
    psi = np.zeros(8)
    psi[0] = 1.0                                   # all spins up
    assert R.z_magnetization(psi) == 1.0
    psi[:] = 1.0
    assert R.z_magnetization(psi) == 0.0
    assert np.array_equal(R.pauli_sum_dense("z", 2), np.diag([2.0, 0.0, 0.0, -2.0]))


def test_exports_and_loud_failure_without_gpu(T):
    for name in ("sandwich", "expect", "rayleigh", "pauli_matrix", "pauli_sum_tto", "pauli_pair_sum_tto", "H_mu", "H_munu", "xy_tto"):
        assert name in T.__all__ and callable(getattr(T, name))
    for name in ("sandwich", "sandwich_dev", "expect", "rayleigh"):
        assert callable(getattr(T.device, name))
    import torch
    x = T.rand_tt((2,) * 4, 3, seed=1)
    A = T.Delta(4)
    if torch.cuda.is_available():               # with a device the same calls answer
        ref = R.sandwich(to_oracle(x), to_oracle(A), to_oracle(x))
        assert abs(T.expect(A, x) - ref) <= 1e-12 * abs(ref) and abs(T.sandwich(x, A, x) - ref) <= 1e-12 * abs(ref)
        return
    for call in (lambda: T.sandwich(x, A, x), lambda: T.expect(A, x), lambda: T.rayleigh(A, x)):
        with pytest.raises(T.TTNError):
            call()


def test_expect_header_and_ctypes_table_agree(T):
    hdr_raw = open(os.path.join(ROOT, "include", "ttn_expect.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_raw, flags=re.S)
    protos = re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert {n for n, _ in protos} == set(T._lib.EXPECT_SIGNATURES) == {"ttn_sandwich", "ttn_sandwich_dev"}
    others = set(T._lib.SIGNATURES) | set(T._lib.RECT_SIGNATURES) | set(T._lib.DENSE_SIGNATURES) | set(T._lib.STEP_SIGNATURES) | set(T._lib.CROSS_BATCH_SIGNATURES)
    assert not set(T._lib.EXPECT_SIGNATURES) & others
    lib = T._lib.lib()
    for name, args in protos:
        res, argt = T._lib.EXPECT_SIGNATURES[name]
        assert res is ctypes.c_int and hasattr(lib, name)
        assert len([a for a in args.split(",")]) == len(argt) == 4
    assert '#include "ttn_expect.h"' in open(os.path.join(ROOT, "include", "ttn.h")).read()
    # the limits of the on-chip route: the header, the kernels and the Python layer state the same numbers
    defs = dict(re.findall(r"#define\s+(TTN_EXPECT_QTT_MAX_[A-Z_]+)\s+(\d+)", hdr))
    assert int(defs["TTN_EXPECT_QTT_MAX_RANK"]) == T.device.EXPECT_QTT_MAX_RANK
    assert int(defs["TTN_EXPECT_QTT_MAX_OP_RANK"]) == T.device.EXPECT_QTT_MAX_OP_RANK
