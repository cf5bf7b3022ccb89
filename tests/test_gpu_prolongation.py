"""Rectangular operators on the GPU (csrc/ttn_rect_kernels.h, include/ttn_rect.h) against the NumPy restatement
(tests/rect_reference.py) and the dense matrices of the reference's testsets (test/test_tt_operators.jl:436-523).

Tolerances (fp64):
  dense products of the reference's cases ............ atol 1e-12 (tests/test_gpu_parity.py's level for apply)
  cores of the reference's cases ..................... that file's 4-ulp rule; bit-exact for the constant prolongation (it only copies)
  cores of the random operators ....................... |got - ref| <= 2 n_in eps (|A_k| * |X_k|) entry by entry: an n_in-term dot
                                                      product in any order, with or without FMA, is within n_in eps (|A| * |X|) of the
                                                      exact value, and so is the restatement's; 0 at the singleton site
  prolong + round ...................................... 1e-10 max|ref| on the dense vector (test_gpu_parity.py's level for apply + round)
"""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import rect_reference as R
from tests.helpers import to_oracle, to_product

pytestmark = pytest.mark.gpu

ULP4 = 4 * np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


@pytest.fixture(scope="module")
def D(T):
    from ttn_amd import device
    return device


def _cores_close(got, ref, rtol):
    """tests/test_gpu_parity.py's _cores_equal: bit-exact for rtol == 0, else rtol relative with rtol max|ref| absolute per core."""
    assert list(got.ttv_rks) == list(ref.ttv_rks)
    assert tuple(got.ttv_dims) == tuple(ref.ttv_dims)
    assert list(got.ttv_ot) == list(ref.ttv_ot) == [0] * ref.N
    for ca, cb in zip(got.ttv_vec, ref.ttv_vec):
        ca, cb = np.asarray(ca), np.asarray(cb)
        assert ca.shape == cb.shape
        if rtol == 0.0:
            assert np.array_equal(ca, cb)
        else:
            assert np.allclose(ca, cb, rtol=rtol, atol=rtol * np.max(np.abs(cb)))


def _cores_within_bound(got, A, x):
    ref, bound = R.apply_rect(A, x), R.apply_rect_bound(A, x)
    assert list(got.ttv_rks) == list(ref.ttv_rks) and tuple(got.ttv_dims) == tuple(ref.ttv_dims) and list(got.ttv_ot) == [0] * ref.N
    for k, (ca, cb, bd) in enumerate(zip(got.ttv_vec, ref.ttv_vec, bound)):
        ca = np.asarray(ca)
        assert ca.shape == cb.shape, k
        assert np.all(np.abs(ca - cb) <= bd), (k, float(np.max(np.abs(ca - cb) - bd)))


def _check_reference_case(T, P, u, P_dense, exact):
    """One product of the reference's testsets: dense against P_dense @ u at 1e-12, cores against the restatement."""
    y = P * u
    assert isinstance(y, T.TTvector) and y.N == P.N and y.ttv_dims == tuple(P.tto_dims)
    want = P_dense @ T.qtt_to_function(u)
    assert np.allclose(T.qtt_to_function(y), want, rtol=0, atol=1e-12)
    _cores_close(y, R.apply_rect(to_oracle(P), to_oracle(u)), 0.0 if exact else ULP4)
    return y


# ---- the reference's testsets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["constant", "linear"])
def test_reference_basis_columns_and_functions(T, kind):
    """test/test_tt_operators.jl:455-463 and :499-511."""
    d = 3
    make = T.qtto_constant_prolongation if kind == "constant" else T.qtto_linear_prolongation
    dense = R.constant_prolongation_matrix if kind == "constant" else R.linear_prolongation_matrix
    P, P_dense = make(d), dense(d)
    for col in range(1, 2 ** d + 1):
        y = _check_reference_case(T, P, T.qtt_basis_vector(d, col), P_dense, kind == "constant")
        assert np.allclose(T.qtt_to_function(y), P_dense[:, col - 1], rtol=0, atol=1e-12)
    f = (lambda x: math.cos(math.pi * x)) if kind == "constant" else (lambda x: math.sin(math.pi * x))
    u = T.function_to_qtt(f, d)
    assert np.allclose(T.qtt_to_function(u), [f(k / (2 ** d - 1)) for k in range(2 ** d)], rtol=0, atol=1e-12)
    ref_u = R.function_to_qtt(f, d)
    assert u.ttv_rks == ref_u.ttv_rks
    assert np.allclose(T.qtt_to_function(u), O.qtt_to_vector(ref_u), rtol=0, atol=1e-12)
    _check_reference_case(T, P, u, P_dense, kind == "constant")
    if kind == "linear":
        y1 = T.qtto_linear_prolongation(1) * T.qtt_basis_vector(1, 2)
        assert np.allclose(T.qtt_to_function(y1), [0.0, 0.5, 1.0, 0.5], rtol=0, atol=1e-12)
        _cores_close(y1, R.apply_rect(R.qtto_linear_prolongation(1), R.qtt_basis_vector(1, 2)), ULP4)


@pytest.mark.parametrize("kind", ["constant", "linear"])
def test_reference_two_dimensional_chains(T, kind):
    """:465-474 and :513-522: Py = id ⊗ P (singleton last), then Px = P ⊗ id (singleton in the middle), at d2 = 2."""
    d2 = 2
    make = T.qtto_constant_prolongation if kind == "constant" else T.qtto_linear_prolongation
    P2 = (R.constant_prolongation_matrix if kind == "constant" else R.linear_prolongation_matrix)(d2)
    u2 = T.kron(T.function_to_qtt(lambda x: 1 + x, d2), T.function_to_qtt(lambda x: 2 - x, d2))
    Py = T.kron(T.id_tto(d2), make(d2))
    uy = _check_reference_case(T, Py, u2, np.kron(np.eye(2 ** d2), P2), kind == "constant")
    Px = T.kron(make(d2), T.id_tto(d2 + 1))
    uxy = _check_reference_case(T, Px, uy, np.kron(P2, np.eye(2 ** (d2 + 1))), kind == "constant")
    assert uxy.N == 2 * d2 + 2


# ---- random rectangular operators: where the singleton sits, dimensions, the edges of the n_out = 2 mapping ---------------------------
#   (out_dims, in_dims, A_rks, x_rks); x's dims are in_dims without the singleton
RANDOM_CASES = {
    "singleton_first_nu1_and_3x2": ((2, 2, 3, 2), (1, 2, 2, 2), [1, 2, 3, 2, 1], [1, 3, 2, 1]),
    "singleton_last_and_2x4": ((2, 2, 2), (2, 4, 1), [1, 3, 2, 1], [1, 3, 1]),
    "singleton_middle_Rl2_Rr3_nu3_nout3": ((2, 3, 2), (2, 1, 2), [1, 2, 3, 1], [1, 3, 1]),
    "singleton_middle_Rl2_Rr3_nu3_nout2": ((2, 2, 2), (2, 1, 2), [1, 2, 3, 1], [1, 3, 1]),
    "columns_15_not_a_multiple_of_4": ((2, 2, 2), (2, 2, 1), [1, 3, 2, 1], [1, 5, 1]),
    "left_rank_64": ((2, 2, 2), (2, 2, 1), [1, 4, 4, 1], [1, 64, 1]),
    "left_rank_65_two_blocks": ((2, 2, 2), (2, 2, 1), [1, 4, 4, 1], [1, 65, 1]),
    "core_too_large_for_lds_Rl40_Rr40": ((2, 2, 2), (2, 2, 1), [1, 40, 40, 1], [1, 3, 1]),
}


def _random_case(name):
    out_dims, in_dims, A_rks, x_rks = RANDOM_CASES[name]
    rng = np.random.default_rng(sorted(RANDOM_CASES).index(name) + 100)
    A = R.rand_rect_tto(out_dims, in_dims, A_rks, rng)
    xd = tuple(n for n in in_dims if n != 1)
    x = O.TTvector(len(xd), [np.asfortranarray(rng.standard_normal((xd[k], x_rks[k], x_rks[k + 1]))) for k in range(len(xd))], xd, list(x_rks),
                   [0] * len(xd))
    return A, x


@pytest.mark.parametrize("name", sorted(RANDOM_CASES))
def test_random_rectangular_operators(T, D, name):
    A, x = _random_case(name)
    pA, px = to_product(A), to_product(x)
    y = T.apply(pA, px)                                                      # stateless
    _cores_within_bound(y, A, x)
    dA, dx = D.DeviceRectTTO(pA), D.DeviceTT.from_host(px)                   # on handles: identical cores
    assert dA.ranks() == list(A.tto_rks) and len(dA.singleton_sites()) == 1
    dy = D.DeviceTT(dA.dims, D.rect_rank_capacity(dA.rks, dA.singleton_sites()[0], dx.cap))
    z = D.apply_rect(dA, dx, dy).download()
    assert z.ttv_rks == y.ttv_rks and z.ttv_ot == [0] * A.N
    for a, b in zip(z.ttv_vec, y.ttv_vec):
        assert np.array_equal(a, b)
    dense = R.rect_to_matrix(A) @ np.reshape(O.ttv_to_tensor(x), -1)
    got = np.reshape(O.ttv_to_tensor(to_oracle(y)), -1)
    assert np.allclose(got, dense, rtol=0, atol=1e-12 * max(1.0, float(np.max(np.abs(dense)))))


def test_batch_with_different_current_ranks(T, D):
    """Three trains in one handle; a rounding first makes their device-resident ranks differ (and leaves the host-side bounds loose):
    k_apply_rect must read each train's own ranks."""
    d = 5
    a = T.rand_tt((2,) * d, [1, 2, 2, 2, 2, 1], seed=11)
    trains = [T.rand_tt((2,) * d, [1, 2, 4, 4, 2, 1], seed=12), T.add(a, a), T.rand_tt((2,) * d, [1, 2, 3, 3, 2, 1], seed=13)]
    dx = D.DeviceTT((2,) * d, [1, 4, 4, 4, 4, 1], batch=3)
    for b, t in enumerate(trains):
        dx.upload(b, t)
    D.tt_compress_(dx, 4, truncerr=1e-12)
    D.compress_status(dx)
    rounded = [dx.download(b) for b in range(3)]
    assert rounded[0].ttv_rks == [1, 2, 4, 4, 2, 1] and rounded[1].ttv_rks == [1, 2, 2, 2, 2, 1]      # a + a is rounded harder
    for name, s in (("linear", d + 1), ("kron", 3)):
        P = T.qtto_linear_prolongation(d) if name == "linear" else T.kron(T.qtto_linear_prolongation(2), T.id_tto(3))
        dP = D.DeviceRectTTO(P)
        assert dP.singleton_sites() == [s]
        dy = D.DeviceTT((2,) * (d + 1), D.rect_rank_capacity(P.tto_rks, s, dx.cap), batch=3)
        D.apply_rect(dP, dx, dy)
        for b in range(3):
            got = dy.download(b)
            _cores_close(got, R.apply_rect(to_oracle(P), to_oracle(rounded[b])), ULP4)
        assert dy.download(0).ttv_rks != dy.download(1).ttv_rks


def test_prolong_serial_2d_on_handles(T, D):
    """examples/heat_equation_prolongation.jl: prolong_serial_2d at d = 4 on qtt_sin ⊗ qtt_sin, resident from upload to download: Py,
    then Px with the rounding tt_compress!(., 16; truncerr = 1e-12, sweeps = 2)."""
    d = 4
    for make, ref_make in ((T.qtto_constant_prolongation, R.qtto_constant_prolongation), (T.qtto_linear_prolongation, R.qtto_linear_prolongation)):
        u = T.kron(T.qtt_sin(d), T.qtt_sin(d))
        Py, Px = T.kron(T.id_tto(d), make(d)), T.kron(make(d), T.id_tto(d + 1))
        dPy, dPx, du = D.DeviceRectTTO(Py), D.DeviceRectTTO(Px), D.DeviceTT.from_host(u)
        cap_y = D.rect_rank_capacity(Py.tto_rks, 2 * d + 1, du.cap)
        cap_xy = D.rect_rank_capacity(Px.tto_rks, d + 1, cap_y)
        need, _ = D.compress_rank_bound((2,) * (2 * d + 2), cap_xy, 16, sweeps=2)
        duy = D.DeviceTT((2,) * (2 * d + 1), cap_y)
        duf = D.DeviceTT((2,) * (2 * d + 2), [max(a, b) for a, b in zip(cap_xy, need)])
        D.apply_rect(dPy, du, duy)
        D.prolong_compress_(dPx, duy, duf, 16, truncerr=1e-12, sweeps=2)
        D.compress_status(duf)
        got = duf.download()
        ou = to_oracle(u)
        ref_y = R.apply_rect(to_oracle(Py), ou)
        ref = O.tt_compress_(R.apply_rect(to_oracle(Px), ref_y), 16, truncerr=1e-12, sweeps=2)
        ref_dense = O.qtt_to_vector(ref)
        assert max(got.ttv_rks) <= 16
        if make is T.qtto_constant_prolongation:
            assert got.ttv_rks == ref.ttv_rks
        assert np.allclose(T.qtt_to_function(got), ref_dense, rtol=0, atol=1e-10 * np.max(np.abs(ref_dense)))
        # and it is the prolongation: P ⊗ P of the coarse samples
        Pd = (R.constant_prolongation_matrix if make is T.qtto_constant_prolongation else R.linear_prolongation_matrix)(d)
        want = np.kron(Pd, Pd) @ T.qtt_to_function(u)
        assert np.allclose(T.qtt_to_function(got), want, rtol=0, atol=1e-10 * np.max(np.abs(want)))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_untouched(T, D):
    L, E = T._lib.lib(), T._lib
    d = 3
    P = T.qtto_linear_prolongation(d)
    x = T.rand_tt((2,) * d, [1, 2, 2, 1], seed=5)
    dP, dx = D.DeviceRectTTO(P), D.DeviceTT.from_host(x)
    cap = D.rect_rank_capacity(P.tto_rks, d + 1, dx.cap)
    dy = D.DeviceTT((2,) * (d + 1), cap)
    before = D.apply_rect(dP, dx, dy).download()
    _cores_close(before, R.apply_rect(to_oracle(P), to_oracle(x)), ULP4)

    def refused(code, A, xx, yy, msg):
        assert L.ttn_apply_rect(A.h, xx.h, yy.h) == code
        assert msg in E.last_error()

    none = D.DeviceRectTTO(T.Delta(d + 1))                                                     # zero singleton sites
    two = D.DeviceRectTTO(T.kron(T.qtto_constant_prolongation(1), T.qtto_constant_prolongation(1)))
    refused(E.TTN_ERR_DIMS, none, dx, dy, "exactly one singleton input site")
    refused(E.TTN_ERR_DIMS, two, dx, dy, "exactly one singleton input site")
    refused(E.TTN_ERR_DIMS, D.DeviceRectTTO(T.qtto_linear_prolongation(d + 1)), dx, dy, "one additional output site")      # M != N + 1
    refused(E.TTN_ERR_DIMS, D.DeviceRectTTO(T.qtto_linear_prolongation(d - 1)), dx, dy, "one additional output site")
    x23 = D.DeviceTT.from_host(T.rand_tt((2, 3, 2), [1, 2, 2, 1], seed=6))
    refused(E.TTN_ERR_DIMS, dP, x23, dy, "Incompatible input dimensions")
    xopen = D.DeviceTT.from_host(T.rand_tt((2,) * d, [1, 2, 2, 2], seed=7))
    refused(E.TTN_ERR_DIMS, dP, xopen, dy, "closed right boundary rank")
    y_dims = D.DeviceTT((2, 2, 3, 2), cap)
    refused(E.TTN_ERR_DIMS, dP, dx, y_dims, "output dimensions")
    y_sites = D.DeviceTT((2,) * d, cap[:-1])
    refused(E.TTN_ERR_DIMS, dP, dx, y_sites, "output dimensions")
    small = list(cap)
    small[2] -= 1
    y_small = D.DeviceTT((2,) * (d + 1), small)
    refused(E.TTN_ERR_CAPACITY, dP, dx, y_small, "capacity too small")
    xc = D.DeviceTT((2,) * d, dx.cap, dtype=np.complex128)
    yc = D.DeviceTT((2,) * (d + 1), cap, dtype=np.complex128)
    refused(E.TTN_ERR_UNSUPPORTED, dP, xc, dy, "Float64 only")
    refused(E.TTN_ERR_UNSUPPORTED, dP, dx, yc, "Float64 only")
    with pytest.raises(AssertionError, match="exactly one singleton input site"):          # the Python layer maps TTN_ERR_DIMS as elsewhere
        D.apply_rect(two, dx, dy)
    with pytest.raises(T.TTNError, match="ttn error -5"):
        D.apply_rect(dP, dx, y_small)
    with pytest.raises(TypeError):
        D.apply_rect(D.DeviceTTO(T.Delta(d + 1)), dx, dy)                       # a square-operator handle is not taken
    with pytest.raises(TypeError, match="Float64 only"):
        D.DeviceRectTTO(T.TToperator(P.N, [c.astype(np.complex128) for c in P.tto_vec], P.tto_dims, P.tto_rks, P.tto_ot))
    # nothing was touched: y as before, the refused destinations still the rank-1 zero trains they were created as
    after = dy.download()
    assert after.ttv_rks == before.ttv_rks and after.ttv_ot == before.ttv_ot
    for a, b in zip(after.ttv_vec, before.ttv_vec):
        assert np.array_equal(a, b)
    for h in (y_dims, y_sites, y_small):
        assert h.ranks()[0] == [1] * (h.N + 1)
    # and an ordinary call on the same handles still succeeds
    x2 = T.rand_tt((2,) * d, [1, 2, 2, 1], seed=8)
    dx.upload(0, x2)
    _cores_close(D.apply_rect(dP, dx, dy).download(), R.apply_rect(to_oracle(P), to_oracle(x2)), ULP4)
    D.status_all()
