"""TT operator algebra without a GPU: the NumPy restatement (tests/opalg_reference.py) pinned to the cases of the reference's own tests
(test/test_tt_operations.jl:125-200, test/test_tt_tools.jl for concatenate / tto_to_ttv) at their atol of 1e-12, the new host
constructors against the oracle, the host-side regrouping functions, and the refusals that are decided before the library is called."""
import numpy as np
import pytest

import ttn_amd as T
from oracle import tt_oracle as O
from tests import opalg_reference as R
from tests.helpers import to_oracle, to_product

ATOL = 1.0e-12


def _dense(A):
    """reshape(tto_to_tensor(A), n, n) with the oracle's densifier."""
    n = int(np.prod(A.tto_dims))
    return np.reshape(O.tto_to_tensor(A), (n, n), order="F")


@pytest.mark.parametrize("dims", [(2, 3), (2, 3, 2)])
def test_mul_is_the_matrix_product(dims):
    rng = np.random.default_rng(1)
    A, B = O.rand_tto(dims, 2, rng), O.rand_tto(dims, 2, rng)
    Cm = R.tto_mul(A, B)
    assert Cm.tto_dims == A.tto_dims
    assert Cm.tto_rks == [a * b for a, b in zip(A.tto_rks, B.tto_rks)]
    assert np.allclose(_dense(Cm), _dense(A) @ _dense(B), atol=ATOL, rtol=0)
    assert np.allclose(R.tto_matrix(Cm), _dense(Cm), atol=ATOL, rtol=0)       # the helper's densifier agrees with the oracle's


def test_inner_core_product():
    rng = np.random.default_rng(42)
    A1, B1 = O.rand_tto((3,), 1, rng), O.rand_tto((4,), 1, rng)
    C1 = R.tto_inner(A1, B1)
    assert C1.tto_dims == (12,) and C1.tto_rks == [1, 1]
    assert np.allclose(_dense(C1), np.kron(_dense(A1), _dense(B1)), atol=ATOL, rtol=0)
    A, B = O.rand_tto((2, 2, 2), 2, rng), O.rand_tto((2, 2, 2), 3, rng)
    Cc = R.tto_inner(A, B)
    assert Cc.N == 3 and Cc.tto_dims == (4, 4, 4) and Cc.tto_rks == [a * b for a, b in zip(A.tto_rks, B.tto_rks)]
    # (2, 3) ⨝ (3, 2): every dense entry is the product of the matching entries, A index major and B index minor
    As, Bs = O.rand_tto((2, 3), 2, rng), O.rand_tto((3, 2), 2, rng)
    TA, TB, TC = O.tto_to_tensor(As), O.tto_to_tensor(Bs), O.tto_to_tensor(R.tto_inner(As, Bs))
    assert TC.shape == (6, 6, 6, 6)
    ref = np.einsum("abcd,ABCD->aAbBcCdD", TA, TB).reshape(6, 6, 6, 6)    # C order: the later (B) index of a pair is the minor one
    assert np.allclose(TC, ref, atol=ATOL, rtol=0)


def test_kron_concatenate_and_conversions():
    rng = np.random.default_rng(3)
    A, B = O.rand_tto((2, 3), 2, rng), O.rand_tto((3, 2, 2), 3, rng)
    K = R.kron(A, B)
    assert K.tto_dims == (2, 3, 3, 2, 2) and K.tto_rks == A.tto_rks[:-1] + B.tto_rks
    # site 1 is the fastest index of the dense matrix, so kron(A, B) is np.kron(B_mat, A_mat)
    assert np.allclose(_dense(K), np.kron(_dense(B), _dense(A)), atol=ATOL, rtol=0)
    x, y = O.rand_tt((2, 3), [1, 2, 1], rng), O.rand_tt((4, 2), [1, 3, 1], rng)
    assert np.allclose(R.ttv_vector(R.kron(x, y)), np.kron(R.ttv_vector(y), R.ttv_vector(x)), atol=ATOL, rtol=0)
    # concatenate joins open trains at a common rank and refuses a mismatch
    L, Rt = R.rand_tto((2, 2), [1, 3, 4], rng), R.rand_tto((3,), [4, 1], rng)
    J = R.concatenate(L, Rt)
    assert J.tto_rks == [1, 3, 4, 1] and J.tto_dims == (2, 2, 3)
    with pytest.raises(ValueError):
        R.concatenate(L, R.rand_tto((3,), [3, 1], rng))
    v = R.tto_to_ttv(A)
    assert v.ttv_dims == (4, 9) and v.ttv_rks == A.tto_rks
    # dense: the vector's site index is i + n j, i.e. tensor[x1, x2, y1, y2] read as [(x1, y1), (x2, y2)]
    assert np.allclose(O.ttv_to_tensor(v).reshape(-1, order="F"), np.einsum("abcd->acbd", O.tto_to_tensor(A)).reshape(-1, order="F"), atol=ATOL, rtol=0)
    back = R.ttv_to_tto(v)
    assert back.tto_dims == A.tto_dims and all(np.array_equal(p, q) for p, q in zip(back.tto_vec, A.tto_vec))


def test_diag_outer_add_scale():
    rng = np.random.default_rng(4)
    x, y = O.rand_tt((2, 3, 2), [1, 2, 3, 1], rng), O.rand_tt((2, 3, 2), [1, 3, 2, 1], rng)
    xv, yv = R.ttv_vector(x), R.ttv_vector(y)
    assert np.allclose(R.tto_matrix(R.ttv_to_diag_tto(x)), np.diag(xv), atol=ATOL, rtol=0)
    P = R.outer_product(x, y)
    assert P.tto_rks == [1, 6, 6, 1]
    assert np.allclose(R.tto_matrix(P), np.outer(xv, yv), atol=ATOL, rtol=0)
    A, B = O.rand_tto((2, 3, 2), 3, rng), O.rand_tto((2, 3, 2), 2, rng)
    S = R.tto_add(A, B)
    assert S.tto_rks == [1] + [a + b for a, b in zip(A.tto_rks[1:-1], B.tto_rks[1:-1])] + [1]
    assert np.allclose(_dense(S), _dense(A) + _dense(B), atol=ATOL, rtol=0)
    assert all(np.array_equal(p, q) for p, q in zip(S.tto_vec, O.tto_add(A, B).tto_vec))          # the oracle's own + agrees bit for bit
    assert np.allclose(_dense(R.tto_sub(A, B)), _dense(A) - _dense(B), atol=ATOL, rtol=0)
    A.tto_ot = [1, 0, -1]
    Sc = R.tto_scale(-2.5, A)
    assert np.array_equal(Sc.tto_vec[1], -2.5 * A.tto_vec[1]) and np.array_equal(Sc.tto_vec[0], A.tto_vec[0]) and Sc.tto_ot == [1, 0, -1]
    Z = R.tto_scale(0.0, A)
    assert Z.tto_rks == A.tto_rks and Z.tto_ot == [0, 0, 0] and all(not c.any() for c in Z.tto_vec)


def test_ornstein_generator_ranks_of_the_restatement():
    A = R.ornstein2d_coupled(8, R.HostOps)
    assert A.tto_rks == [1] + [28] * 7 + [6] + [28] * 7 + [1]
    assert R.tto_compress(A, truncerr=1e-6).tto_rks == [1, 4, 6, 6, 6, 6, 6, 6, 4, 6, 6, 6, 6, 6, 6, 4, 1]
    D2 = R.tto_mul(O.Delta(8), O.Delta(8))
    assert R.tto_compress(D2, truncerr=1e-6).tto_rks == [1, 4, 5, 5, 5, 5, 5, 4, 1]


# ---- the product's host code -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 8])
def test_nabla_and_qtt_polynom_match_the_oracle(d):
    N, Nref = T.Nabla(d), O.toeplitz_to_qtto(1, 0, -1, d)
    assert N.tto_rks == Nref.tto_rks and all(np.array_equal(p, q) for p, q in zip(N.tto_vec, Nref.tto_vec))
    M = O.qtto_to_matrix(to_oracle(N))
    assert np.array_equal(M, np.eye(2 ** d) - np.eye(2 ** d, k=-1))
    for coef, a, b in (([-2.0, 1.0], -6.0, 6.0), ([0.5, -1.0, 0.25, 2.0], 0.0, 1.0)):
        p, pref = T.qtt_polynom(coef, d, a, b), O.qtt_polynom(coef, d, a, b)
        assert p.ttv_rks == pref.ttv_rks and p.ttv_dims == pref.ttv_dims
        assert all(np.array_equal(u, v) for u, v in zip(p.ttv_vec, pref.ttv_vec))
        xs = np.linspace(a, b, 2 ** d)
        assert np.allclose(T.qtt_to_vector(p), np.polyval(coef[::-1], xs), atol=1e-11, rtol=0)


def test_host_regrouping_matches_the_restatement():
    rng = np.random.default_rng(5)
    A, B = O.rand_tto((2, 3), 2, rng), O.rand_tto((3, 2, 2), 3, rng)
    A.tto_ot = [1, 0]
    K = T.kron(to_product(A), to_product(B))
    Kr = R.kron(A, B)
    assert isinstance(K, T.TToperator) and K.N == 5 and K.tto_dims == Kr.tto_dims and K.tto_rks == Kr.tto_rks and K.tto_ot == Kr.tto_ot
    assert all(np.array_equal(p, q) for p, q in zip(K.tto_vec, Kr.tto_vec))
    x, y = O.rand_tt((2, 3), [1, 2, 1], rng), O.rand_tt((4, 2), [1, 3, 1], rng)
    k = T.kron(to_product(x), to_product(y))
    assert isinstance(k, T.TTvector) and k.ttv_dims == (2, 3, 4, 2) and k.ttv_rks == [1, 2, 1, 3, 1]
    assert all(np.array_equal(p, q) for p, q in zip(k.ttv_vec, x.ttv_vec + y.ttv_vec))
    L, Rt = R.rand_tto((2, 2), [1, 3, 4], rng), R.rand_tto((3,), [4, 1], rng)
    J = T.concatenate(to_product(L), to_product(Rt))
    assert J.tto_rks == [1, 3, 4, 1] and J.tto_dims == (2, 2, 3)
    v = T.tto_to_ttv(to_product(A))
    vr = R.tto_to_ttv(A)
    assert v.ttv_dims == vr.ttv_dims and v.ttv_rks == vr.ttv_rks and v.ttv_ot == [1, 0]
    assert all(np.array_equal(p, q) and p.shape == q.shape for p, q in zip(v.ttv_vec, vr.ttv_vec))
    back = T.ttv_to_tto(v)
    assert back.tto_dims == A.tto_dims and all(np.array_equal(p, q) for p, q in zip(back.tto_vec, A.tto_vec))


def test_refusals_that_need_no_device():
    rng = np.random.default_rng(6)
    A, B = to_product(O.rand_tto((2, 3), 2, rng)), to_product(O.rand_tto((3, 2), 2, rng))
    x = to_product(O.rand_tt((2, 3), [1, 2, 1], rng))
    for f in (T.tto_mul, T.tto_add, T.tto_sub):
        with pytest.raises(AssertionError, match="Incompatible dimensions"):
            f(A, B)
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        A * B
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        A + B
    with pytest.raises(AssertionError, match="same number of cores"):
        T.tto_inner(A, to_product(O.rand_tto((2, 2, 2), 2, rng)))
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        T.outer_product(x, to_product(O.rand_tt((3, 2), [1, 2, 1], rng)))
    with pytest.raises(ValueError, match="final rank"):
        T.concatenate(to_product(R.rand_tto((2,), [1, 3], rng)), to_product(R.rand_tto((2,), [2, 1], rng)))
    with pytest.raises(ValueError, match="final rank"):
        T.concatenate(to_product(R.rand_ttv((2,), [1, 3], rng)), to_product(R.rand_ttv((2,), [2, 1], rng)))
    with pytest.raises(AssertionError, match="DimensionMismatch"):
        T.ttv_to_tto(x)                                        # dims (2, 3) are not squares
    with pytest.raises(TypeError):
        T.tto_mul(A, x)
    with pytest.raises(TypeError):
        T.kron(A, x)
    with pytest.raises(TypeError):
        T.ttv_to_diag_tto(A)
    with pytest.raises(TypeError):
        A * "two"
    with pytest.raises(TypeError):
        A + 1.0
    with pytest.raises(TypeError, match="complex"):
        T.tto_scale(1j, A)
    Ac = T.TToperator(A.N, [c.astype(complex) for c in A.tto_vec], A.tto_dims, A.tto_rks, A.tto_ot)
    with pytest.raises(TypeError, match="complex"):
        T.tto_mul(Ac, A)
    with pytest.raises(AssertionError, match="sweeps must be >= 1"):
        T.tto_compress_(A, 4, sweeps=0)
    with pytest.raises(AssertionError):
        T.qtt_polynom([1.0, 2.0], 1)
