"""CPU tests of the braket layer (no GPU): the NumPy three-layer recurrence with a conjugated bra (tests/braket_reference.py) against
the oracle's dot(x, A * y) and the dense np.vdot — the yardstick of tests/test_gpu_braket.py — the complex Pauli constructors against
dense Kronecker sums, and the entry points' exports, header, ctypes table and loud failure without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import braket_reference as R
from tests import expect_reference as RE
from tests.helpers import to_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = ("x", "y", "z")
FORMS = [(True, True), (False, True), (True, False)]          # (complex operator, complex trains): the three forms the kernel handles


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    return ttn_amd


# ---- inputs (crand_tt / crand_tto of tests/test_gpu_complex.py, restated) -----------------------------------------------------------
def crand(shape, rng, cplx=True):
    re = rng.standard_normal(shape)
    return np.asfortranarray(re + 1j * rng.standard_normal(shape)) if cplx else np.asfortranarray(re)


def crand_tt(dims, rks, rng, cplx=True):
    d = len(dims)
    if isinstance(rks, (int, np.integer)):
        rks = O.r_and_d_to_rks([int(rks)] * (d + 1), tuple(dims))
    return O.TTvector(d, [crand((dims[k], rks[k], rks[k + 1]), rng, cplx) for k in range(d)], tuple(dims), list(rks), [0] * d)


def crand_tto(dims, rks, rng, cplx=True):
    d = len(dims)
    if isinstance(rks, (int, np.integer)):
        rks = [1] + [int(rks)] * (d - 1) + [1]
    return O.TToperator(d, [crand((dims[k], dims[k], rks[k], rks[k + 1]), rng, cplx) for k in range(d)], tuple(dims), list(rks), [0] * d)


def reference(x, A, y):
    """(ref, scale) = (dot(x, A y), ||x|| ||A y||) from the oracle: dot conjugates its first argument."""
    Ay = O.apply(A, y)
    return complex(O.dot(x, Ay)), float(O.norm(x) * O.norm(Ay))


YARDSTICK_CASES = [((3,), [1, 1], [1, 1], [1, 1]), ((2, 3), [1, 2, 1], [1, 3, 1], [1, 2, 1]),
                   ((2, 3, 4, 2), [1, 2, 5, 3, 1], [1, 3, 4, 2, 1], [1, 2, 3, 2, 1]), ((2,) * 9, 5, 7, 3)]


@pytest.mark.parametrize("ca,cx", FORMS)
@pytest.mark.parametrize("dims,rx,ry,ra", YARDSTICK_CASES)
def test_restatement_matches_oracle_and_dense(dims, rx, ry, ra, ca, cx):
    """Pins the yardstick: the recurrence equals dot(x, A * y) and the dense vdot to 1e-13 of ||x|| ||A y||."""
    rng = np.random.default_rng(len(dims) * 10 + 2 * ca + cx)
    x, y, A = crand_tt(dims, rx, rng, cx), crand_tt(dims, ry, rng, cx), crand_tto(dims, ra, rng, ca)
    ref, scale = reference(x, A, y)
    got = R.braket(x, A, y)
    dense = complex(np.vdot(O.ttv_to_tensor(x).reshape(-1), O.ttv_to_tensor(O.apply(A, y)).reshape(-1)))
    print(f"dims {dims} ca {ca} cx {cx}: |got - ref| / scale {abs(got - ref) / scale:.2e}  |ref - dense| / scale {abs(ref - dense) / scale:.2e}")
    assert abs(got - ref) <= 1e-13 * scale
    assert abs(ref - dense) <= 1e-13 * scale


def test_restatement_is_sesquilinear_and_conjugates_the_bra():
    rng = np.random.default_rng(4)
    dims = (2, 3, 4, 2)
    x, A = crand_tt(dims, [1, 2, 5, 3, 1], rng), crand_tto(dims, [1, 2, 3, 2, 1], rng)
    ref, scale = reference(x, A, x)
    ix = O.TTvector(x.N, [x.ttv_vec[0] * 1j] + [c.copy() for c in x.ttv_vec[1:]], x.ttv_dims, x.ttv_rks, x.ttv_ot)
    assert abs(R.braket(ix, A, x) - (-1j) * R.braket(x, A, x)) <= 1e-13 * scale          # braket(i x, A, x) = -i braket(x, A, x)
    assert abs(R.braket(x, A, ix) - 1j * R.braket(x, A, x)) <= 1e-13 * scale
    # a non-conjugated read of the bra is a different number
    assert abs(R.braket(x, A, x, conj_x=False) - ref) > 1e-6 * scale
    # on real operands the recurrence is the bilinear one of tests/expect_reference.py
    xr, Ar = crand_tt(dims, [1, 2, 5, 3, 1], rng, False), crand_tto(dims, [1, 2, 3, 2, 1], rng, False)
    b = R.braket(xr, Ar, xr)
    assert b.imag == 0.0 and abs(b.real - RE.sandwich(xr, Ar, xr)) <= 1e-13 * reference(xr, Ar, xr)[1]


# ---- the complex Pauli constructors ---------------------------------------------------------------------------------------------------
def _dense(A):
    """The (2^d, 2^d) matrix of a product-side operator from its cores: site 1 the most significant bit."""
    M = np.ones((1, 1, 1), dtype=np.complex128)                     # (rows, cols, bond)
    for c in A.tto_vec:
        M = np.einsum("pqa,ijab->piqjb", M, np.asarray(c, dtype=np.complex128)).reshape(M.shape[0] * 2, M.shape[1] * 2, c.shape[3])
    return M[:, :, 0]


@pytest.mark.parametrize("d", [1, 2, 3, 5])
@pytest.mark.parametrize("mu", AXES)
def test_complex_pauli_sum_tto(T, mu, d):
    A = T.pauli_sum_tto(mu, d, dtype=np.complex128)
    assert A.tto_rks == ([1, 1] if d == 1 else [1] + [2] * (d - 1) + [1])
    assert A.tto_dims == (2,) * d and A.tto_ot == [0] * d
    assert all(c.dtype == np.complex128 and c.shape == (2, 2, A.tto_rks[k], A.tto_rks[k + 1]) for k, c in enumerate(A.tto_vec))
    assert np.max(np.abs(_dense(A) - R.pauli_sum_dense(mu, d))) <= 1e-14
    B = T.H_mu(mu, d, dtype=np.complex128)
    assert all(np.array_equal(a, b) for a, b in zip(A.tto_vec, B.tto_vec))
    if mu != "y":                                                   # the complex x / z forms hold the real ones' numbers
        Ar = T.pauli_sum_tto(mu, d)
        assert all(a.dtype == np.float64 and np.array_equal(a, b) for a, b in zip(Ar.tto_vec, A.tto_vec))
        assert np.max(np.abs(_dense(Ar) - RE.pauli_sum_dense(mu, d))) <= 1e-14


@pytest.mark.parametrize("d", [2, 3, 5])
@pytest.mark.parametrize("mu", AXES)
@pytest.mark.parametrize("nu", AXES)
def test_complex_pauli_pair_sum_tto(T, mu, nu, d):
    A = T.pauli_pair_sum_tto(mu, nu, d, dtype=np.complex128)
    assert A.tto_rks == [1] + [3] * (d - 1) + [1]
    assert A.tto_dims == (2,) * d and A.tto_ot == [0] * d
    assert all(c.dtype == np.complex128 for c in A.tto_vec)
    assert np.max(np.abs(_dense(A) - R.pauli_pair_sum_dense(mu, nu, d))) <= 1e-14
    B = T.H_munu(mu, nu, d, dtype=np.complex128)
    assert all(np.array_equal(a, b) for a, b in zip(A.tto_vec, B.tto_vec))
    if "y" not in (mu, nu) or (mu, nu) == ("y", "y"):              # ... and so do the pairs that are real
        Ar = T.pauli_pair_sum_tto(mu, nu, d)
        assert all(a.dtype == np.float64 and np.array_equal(a, b) for a, b in zip(Ar.tto_vec, A.tto_vec))


def test_complex_pauli_matrix_and_unchanged_defaults(T):
    assert np.array_equal(T.pauli_matrix("y", dtype=np.complex128), np.array([[0.0, -1.0j], [1.0j, 0.0]]))
    for mu in ("x", "z"):
        m = T.pauli_matrix(mu, dtype=np.complex128)
        assert m.dtype == np.complex128 and np.array_equal(m, T.pauli_matrix(mu)) and T.pauli_matrix(mu).dtype == np.float64
    for m, sq in ((T.pauli_matrix(a, dtype=np.complex128), a) for a in AXES):
        assert np.array_equal(m @ m, np.eye(2)) and np.array_equal(m, m.conj().T)
    # the default keeps refusing a lone sigma_y
    with pytest.raises(T.TTNError, match="sigma_y"):
        T.pauli_matrix("y")
    with pytest.raises(T.TTNError, match="sigma_y"):
        T.pauli_sum_tto("y", 3)
    with pytest.raises(T.TTNError, match="sigma_y"):
        T.pauli_pair_sum_tto("x", "y", 3)
    with pytest.raises(TypeError, match="dtype"):
        T.pauli_matrix("x", dtype=np.float32)


def test_restatement_on_the_complex_pauli_sums(T):
    """<psi| sum_k sigma_y |psi> and <psi| sum_k sigma_x sigma_y |psi> on a random complex state at d = 6 against the dense matrices."""
    d = 6
    rng = np.random.default_rng(8)
    psi = crand_tt((2,) * d, 4, rng)
    v = O.ttv_to_tensor(psi).reshape(-1)
    for A, M in ((T.pauli_sum_tto("y", d, dtype=np.complex128), R.pauli_sum_dense("y", d)),
                 (T.pauli_pair_sum_tto("x", "y", d, dtype=np.complex128), R.pauli_pair_sum_dense("x", "y", d))):
        ref = complex(np.vdot(v, M @ v))
        scale = np.linalg.norm(v) * np.linalg.norm(M @ v)
        assert abs(R.braket(psi, to_oracle(A), psi) - ref) <= 1e-13 * scale
        assert abs(ref.imag) <= 1e-13 * scale                       # Hermitian


# ---- header, ctypes table, exports ----------------------------------------------------------------------------------------------------
def test_braket_header_and_ctypes_table_agree(T):
    hdr_raw = open(os.path.join(ROOT, "include", "ttn_braket.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_raw, flags=re.S)
    protos = re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert {n for n, _ in protos} == set(T._lib.BRAKET_SIGNATURES) == {"ttn_braket", "ttn_braket_dev"}
    others = set()
    for name in dir(T._lib):
        if name.endswith("SIGNATURES") and name != "BRAKET_SIGNATURES":
            others |= set(getattr(T._lib, name))
    assert "ttn_sandwich" in others and not set(T._lib.BRAKET_SIGNATURES) & others
    lib = T._lib.lib()
    for name, args in protos:
        res, argt = T._lib.BRAKET_SIGNATURES[name]
        assert res is ctypes.c_int and hasattr(lib, name)
        assert len(args.split(",")) == len(argt) == 4
    assert '#include "ttn_braket.h"' in open(os.path.join(ROOT, "include", "ttn.h")).read()
    # ttn_expect.h keeps its own two prototypes
    assert "ttn_braket" not in open(os.path.join(ROOT, "include", "ttn_expect.h")).read()
    # the limits of the on-chip route: the header, the kernels and the Python layer state the same numbers
    defs = dict(re.findall(r"#define\s+(TTN_BRAKET_QTT_MAX_[A-Z_]+)\s+(\d+)", hdr))
    assert int(defs["TTN_BRAKET_QTT_MAX_RANK"]) == T.device.BRAKET_QTT_MAX_RANK == 64
    assert int(defs["TTN_BRAKET_QTT_MAX_OP_RANK"]) == T.device.BRAKET_QTT_MAX_OP_RANK >= 2
    kern = open(os.path.join(ROOT, "tensortrainnumerics.jl_amd", "csrc", "ttn_braket_kernels.h")).read()
    assert int(re.search(r"#define\s+BRAKET_QTT_OPR_MAX\s+(\d+)", kern).group(1)) == T.device.BRAKET_QTT_MAX_OP_RANK


def test_exports_and_loud_failure_without_gpu(T):
    for name in ("braket", "energy", "pauli_matrix", "pauli_sum_tto", "pauli_pair_sum_tto", "H_mu", "H_munu"):
        assert name in T.__all__ and callable(getattr(T, name))
    for name in ("braket", "braket_dev", "energy"):
        assert callable(getattr(T.device, name))
    import torch
    rng = np.random.default_rng(2)
    from tests.helpers import to_product
    x = to_product(crand_tt((2,) * 4, 3, rng))
    A = T.pauli_sum_tto("y", 4, dtype=np.complex128)
    if torch.cuda.is_available():               # with a device the same calls answer
        ref, scale = reference(to_oracle(x), to_oracle(A), to_oracle(x))
        got = T.braket(x, A, x)
        assert isinstance(got, complex) and abs(got - ref) <= 1e-12 * scale
        assert isinstance(T.energy(A, x), float)
        return
    for call in (lambda: T.braket(x, A, x), lambda: T.energy(A, x), lambda: T.braket(T.rand_tt((2,) * 4, 3, seed=1), T.Delta(4), T.rand_tt((2,) * 4, 3, seed=1))):
        with pytest.raises(T.TTNError):
            call()
