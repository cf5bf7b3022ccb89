"""The multi-dimensional QTT layer on the CPU: the NumPy restatement (tests/qttnd_reference.py) against the known answers of the
reference's test/test_qtt_multidim.jl, and the host-only pieces of the package (constructors, stride tables, metadata checks,
check_compat, repr, every refusal that is decided before the library is called) against the restatement."""
import math

import numpy as np
import pytest

import ttn_amd as T
from oracle import tt_oracle as O
from tests import qttnd_reference as R
from tests.helpers import to_product

ORDERINGS = ("serial", "interleaved")


def _grid(bits, a=0.0, b=1.0):
    n = 2 ** bits
    h = (b - a) / (n - 1)
    return np.array([a + h * i for i in range(n)])


# ---- test/test_qtt_multidim.jl:139-180 --------------------------------------------------------------------------------------------------
def test_ref_function_to_qttv_round_trips():
    d = 4
    f1d = lambda x: math.sin(math.pi * x[0])
    arr_il = R.qttv_to_array(R.function_to_qttv(f1d, 1, d, "interleaved"))
    arr_sr = R.qttv_to_array(R.function_to_qttv(f1d, 1, d, "serial"))
    assert np.max(np.abs(arr_il - arr_sr)) < 1e-12
    assert arr_il.shape == (2 ** d,)
    assert np.max(np.abs(arr_il - np.sin(math.pi * _grid(d)))) < 1e-12
    bits = 3
    f2d = lambda x: math.sin(math.pi * x[0]) * math.sin(math.pi * x[1])
    a_il = R.qttv_to_array(R.function_to_qttv(f2d, 2, bits, "interleaved"))
    a_sr = R.qttv_to_array(R.function_to_qttv(f2d, 2, bits, "serial"))
    assert a_il.shape == a_sr.shape == (2 ** bits, 2 ** bits)
    assert np.max(np.abs(a_il - a_sr)) < 1e-12
    g = _grid(bits)
    ref = np.sin(math.pi * g)[:, None] * np.sin(math.pi * g)[None, :]
    assert np.max(np.abs(a_il - ref)) < 1e-12


# ---- :393, :418, :433 ----------------------------------------------------------------------------------------------------------------
def test_ref_3d_both_orderings():
    bits = 3
    g = _grid(bits)
    s = np.sin(math.pi * g)
    ref = s[:, None, None] * s[None, :, None] * s[None, None, :]
    f = lambda x: math.sin(math.pi * x[0]) * math.sin(math.pi * x[1]) * math.sin(math.pi * x[2])
    arrs = {}
    for ordering in ORDERINGS:
        q = R.function_to_qttv(f, 3, bits, ordering)
        assert q.ttv.N == 9
        arrs[ordering] = R.qttv_to_array(q)
        assert arrs[ordering].shape == (8, 8, 8)
        assert np.max(np.abs(arrs[ordering] - ref)) < 1e-12
    assert np.max(np.abs(arrs["serial"] - arrs["interleaved"])) < 1e-12


def test_ref_gaussian_non_separable():
    bits = 5
    g = _grid(bits)
    ref = np.exp(-10 * ((g[:, None] - 0.3) ** 2 + (g[None, :] - 0.7) ** 2))
    f = lambda x: math.exp(-10 * ((x[0] - 0.3) ** 2 + (x[1] - 0.7) ** 2))
    a_il = R.qttv_to_array(R.function_to_qttv(f, 2, bits, "interleaved"))
    a_sr = R.qttv_to_array(R.function_to_qttv(f, 2, bits, "serial"))
    assert np.max(np.abs(a_il - ref)) < 1e-12
    assert np.max(np.abs(a_sr - ref)) < 1e-12
    assert np.max(np.abs(a_il - a_sr)) < 1e-12


def test_ref_custom_interval():
    a, b, bits = -1.0, 2.0, 4
    g = _grid(bits, a, b)
    ref = np.sin(g)[:, None] * np.cos(g)[None, :]
    f = lambda x: math.sin(x[0]) * math.cos(x[1])
    for ordering in ORDERINGS:
        assert np.max(np.abs(R.qttv_to_array(R.function_to_qttv(f, 2, bits, ordering, a, b)) - ref)) < 1e-12


def test_ref_fast_sampler_equals_the_literal_loop():
    f = lambda x: math.exp(-x[0]) * (1.0 + x[1]) + 0.25 * x[2]
    fv = lambda X: np.exp(-X[:, 0]) * (1.0 + X[:, 1]) + 0.25 * X[:, 2]
    for ordering in ORDERINGS:
        slow = R.sample_tensor(f, 3, 2, ordering, -2.0, 3.5)
        fast = R.sample_tensor_fast(fv, 3, 2, ordering, -2.0, 3.5)
        assert np.max(np.abs(slow - fast)) <= 4 * np.finfo(float).eps * np.max(np.abs(slow))


# ---- :207-283 -----------------------------------------------------------------------------------------------------------------------
def test_ref_qtt_laplacian():
    d = 4
    n = 2 ** d
    A1 = R.qtt_laplacian(1, d, "serial", bc="DN")
    assert (A1.n_dims, A1.bits_per_dim, A1.ordering, A1.tto.N) == (1, d, "serial", d)
    assert R.qtt_laplacian(1, d, "interleaved", bc="DN").ordering == "interleaved"
    A2s = R.qtt_laplacian(2, d, "serial", bc="DD")
    assert (A2s.n_dims, A2s.bits_per_dim, A2s.ordering, A2s.tto.N) == (2, d, "serial", 2 * d)
    A2i = R.qtt_laplacian(2, d, "interleaved", bc="DD")
    assert (A2i.ordering, A2i.tto.N) == ("interleaved", 2 * d)
    h = 1.0 / (n - 1)
    M1d = O.qtto_to_matrix(O.Delta(d)) / h ** 2
    M_ref = np.kron(M1d, np.eye(n)) + np.kron(np.eye(n), M1d)
    assert np.linalg.norm(R.qtto_to_matrix(A2s) - M_ref) < 1e-8
    ev_s = np.sort(np.linalg.eigvals(R.qtto_to_matrix(R.qtt_laplacian(2, 3, "serial", bc="DD"))).real)
    ev_i = np.sort(np.linalg.eigvals(R.qtto_to_matrix(R.qtt_laplacian(2, 3, "interleaved", bc="DD"))).real)
    assert np.max(np.abs(ev_s - ev_i)) < 1e-8
    for bc in ("DD", "DN", "ND"):
        assert R.qtt_laplacian(2, d, "serial", bc=bc).tto.N == 2 * d
    with pytest.raises(AssertionError):
        R.qtt_laplacian(2, d, "serial", bc="NN")
    assert R.qtt_laplacian(1, d, "serial", bc="NN").tto.tto_rks[0] == 4
    A3 = R.qtt_laplacian(3, 3, "serial", bc="DD")
    assert (A3.n_dims, A3.tto.N) == (3, 9)


def test_ref_grid_matrix_is_ordering_independent():
    # on the grid vector both orderings are the same matrix: kron(I, M) + kron(M, I) with dimension 1 fastest
    d = 3
    n = 2 ** d
    h = 1.0 / (n - 1)
    M1d = O.qtto_to_matrix(O.Delta(d)) / h ** 2
    M_ref = np.kron(np.eye(n), M1d) + np.kron(M1d, np.eye(n))
    for ordering in ORDERINGS:
        M = R.grid_matrix(R.qtt_laplacian(2, d, ordering, bc="DD"))
        assert np.max(np.abs(M - M_ref)) < 1e-8 * np.max(np.abs(M_ref))


def _tridiag(n):
    return 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


@pytest.mark.parametrize("d", [4, 6])
def test_ref_boundary_condition_matrices(d):
    n = 2 ** d
    dn, nd = _tridiag(n), _tridiag(n)
    dn[-1, -1] = 1.0
    nd[0, 0] = 1.0
    assert np.array_equal(O.qtto_to_matrix(R.Delta_DN(d)), dn)
    assert np.array_equal(O.qtto_to_matrix(R.Delta_ND(d)), nd)


# ---- :81 ------------------------------------------------------------------------------------------------------------------------------
def test_ref_entropy_bell_pair():
    bell = np.zeros((2, 2))
    bell[0, 0] = bell[1, 1] = 1 / math.sqrt(2)
    psi = O.ttv_decomp(bell)
    assert np.allclose(R.entanglemententropy(psi), [math.log(2)])
    assert np.allclose(R.entanglemententropy(psi, base=2), [1.0])
    with pytest.raises(AssertionError):
        R.entanglemententropy(psi, base=1)
    one = O.TTvector(1, [np.ones((2, 1, 1))], (2,), [1, 1], [0])
    assert R.entanglemententropy(one).shape == (0,)


def test_ref_entropy_is_the_dense_schmidt_spectrum():
    psi = O.rand_tt((2,) * 6, 4, np.random.default_rng(5))
    full = O.ttv_to_tensor(psi)
    got = R.entanglemententropy(psi)
    for k in range(1, 6):
        s = np.linalg.svd(full.reshape(2 ** k, -1), compute_uv=False)
        p = s ** 2 / np.sum(s ** 2)
        p = p[p > 1e-300]
        assert abs(got[k - 1] + np.sum(p * np.log(p))) < 1e-12


# ---- the package's host-only pieces ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 6])
def test_constructors_equal_the_restatement(d):
    for mine, ref in ((T.Delta_DN, R.Delta_DN), (T.Delta_ND, R.Delta_ND), (T.Delta_NN, R.Delta_NN)):
        a, b = mine(d), ref(d)
        assert list(a.tto_rks) == list(b.tto_rks) and tuple(a.tto_dims) == tuple(b.tto_dims) and list(a.tto_ot) == list(b.tto_ot)
        for ca, cb in zip(a.tto_vec, b.tto_vec):
            assert ca.shape == cb.shape and np.array_equal(ca, cb)
    assert T.Delta_NN(d).tto_rks[0] == 4 and T.Delta_NN(d).tto_rks[-1] == 4
    for ctor in (T.Delta_DN, T.Delta_ND, T.Delta_NN):
        with pytest.raises(AssertionError):
            ctor(3)


def test_stride_tables():
    assert T.grid_strides(2, 3, "interleaved") == [4, 32, 2, 16, 1, 8]
    assert T.grid_strides(2, 3, "serial") == [4, 2, 1, 32, 16, 8]
    for n_dims, bits in ((1, 5), (2, 3), (3, 2), (3, 4)):
        for ordering in ORDERINGS:
            assert T.grid_strides(n_dims, bits, ordering) == R.grid_strides(n_dims, bits, ordering)
            assert sorted(T.grid_strides(n_dims, bits, ordering)) == [2 ** k for k in range(n_dims * bits)]
    # the table against the literal loop of qttv_to_array: a unit tensor entry lands where the strides say
    for ordering in ORDERINGS:
        st = T.grid_strides(2, 2, ordering)
        for idx in np.ndindex(2, 2, 2, 2):
            t = np.zeros((2, 2, 2, 2))
            t[idx] = 1.0
            arr = R.qttv_to_array(R.QTTv(O.ttv_decomp(t), 2, 2, ordering))
            assert np.argmax(np.abs(np.ravel(arr, order="F"))) == sum(i * s for i, s in zip(idx, st))


def _ttv(N=6, seed=1):
    return to_product(O.rand_tt((2,) * N, 2, np.random.default_rng(seed)))


def _tto(N=6, seed=2):
    return to_product(O.rand_tto((2,) * N, 2, np.random.default_rng(seed)))


def test_metadata_checks_and_repr():
    ttv = _ttv()
    q = T.QTTvector(ttv, 2, 3, "interleaved")
    assert (q.N, q.n_dims, q.bits_per_dim, q.ordering) == (6, 2, 3, "interleaved")
    assert repr(q) == "QTT-MPS{Float64}(6 sites, 2d×3bits, interleaved)"
    A = T.QTToperator(_tto(), 3, 2, "serial")
    assert repr(A) == "QTT-MPO{Float64}(6 sites, 3d×2bits, serial)"
    back = q.ttvector()
    assert isinstance(back, T.TTvector) and not isinstance(back, T.QTTvector) and back.ttv_vec[0] is ttv.ttv_vec[0]
    assert isinstance(A.ttoperator(), T.TToperator)
    with pytest.raises(T.TTNError, match="must equal ttv.N"):
        T.QTTvector(ttv, 2, 4, "interleaved")
    with pytest.raises(T.TTNError, match="ordering must be"):
        T.QTTvector(ttv, 2, 3, "zigzag")
    three = to_product(O.rand_tt((2, 3, 2, 2, 2, 2), 2, np.random.default_rng(3)))
    with pytest.raises(T.TTNError, match="must be 2"):
        T.QTTvector(three, 2, 3, "serial")
    with pytest.raises(T.TTNError, match="must equal tto.N"):
        T.QTToperator(_tto(), 4, 2, "serial")
    with pytest.raises(T.TTNError, match="ordering must be"):
        T.QTToperator(_tto(), 2, 3, "Serial")
    with pytest.raises(TypeError):
        T.QTTvector(_tto(), 2, 3, "serial")
    qc = q.copy()
    assert isinstance(qc, T.QTTvector) and qc.ordering == "interleaved" and qc.ttv_vec[0] is not q.ttv_vec[0]
    Ac = A.copy()
    assert isinstance(Ac, T.QTToperator) and Ac.tto_vec[0] is not A.tto_vec[0] and np.array_equal(Ac.tto_vec[0], A.tto_vec[0])


def test_check_compat():
    ttv, tto = _ttv(), _tto()
    q1, q2, q3 = T.QTTvector(ttv, 2, 3, "interleaved"), T.QTTvector(ttv, 2, 3, "interleaved"), T.QTTvector(ttv, 2, 3, "serial")
    q4, q5 = T.QTTvector(ttv, 3, 2, "interleaved"), T.QTTvector(ttv, 1, 6, "interleaved")
    A, B = T.QTToperator(tto, 2, 3, "interleaved"), T.QTToperator(tto, 2, 3, "serial")
    assert T.check_compat(q1, q2) is None and T.check_compat(A, q1) is None and T.check_compat(A, A) is None
    assert T.check_compat(ttv, ttv) is None and T.check_compat(tto, ttv) is None
    with pytest.raises(T.TTNError, match="QTTvector ordering mismatch"):
        T.check_compat(q1, q3)
    with pytest.raises(T.TTNError, match="QTTvector n_dims mismatch"):
        T.check_compat(q1, q4)
    with pytest.raises(T.TTNError, match="n_dims mismatch"):
        T.check_compat(q1, q5)
    with pytest.raises(T.TTNError, match="QTToperator/QTTvector ordering mismatch"):
        T.check_compat(A, q3)
    with pytest.raises(T.TTNError, match="QTToperator ordering mismatch"):
        T.check_compat(A, B)
    # the operations run the check before anything is computed
    for op in (lambda: q1 + q3, lambda: q1 - q3, lambda: T.qttnd.hadamard(q1, q3), lambda: T.qttnd.dot(q1, q3), lambda: A * q3, lambda: A + B,
               lambda: A - B):
        with pytest.raises(T.TTNError, match="mismatch"):
            op()


def test_refusals_before_the_library_is_called():
    f = lambda X: X[:, 0]
    with pytest.raises(T.TTNError, match="ordering must be"):
        T.function_to_qttv(f, 2, 3, ordering="zigzag")
    with pytest.raises(T.TTNError, match="2\\^27"):
        T.function_to_qttv(f, 4, 7)
    with pytest.raises(T.TTNError, match="at least 1"):
        T.function_to_qttv(f, 0, 3)
    with pytest.raises(T.TTNError, match="bc=:NN is only supported for n_dims=1"):
        T.qtt_laplacian(2, 4, bc="NN")
    with pytest.raises(T.TTNError, match="bc must be"):
        T.qtt_laplacian(2, 4, bc="PP")
    with pytest.raises(T.TTNError, match="ordering must be"):
        T.qtt_laplacian(2, 4, ordering="zigzag")
    with pytest.raises(T.TTNError, match="n_dims must be at least 1"):
        T.qtt_laplacian(0, 4)
    with pytest.raises(AssertionError):
        T.qtt_laplacian(2, 3, bc="DN")                  # Δ_DN needs d >= 4
    q = T.QTTvector(_ttv(), 2, 3, "serial")
    for base in (1, 0, -2.0):
        with pytest.raises(T.TTNError, match="base must be positive"):
            T.entanglemententropy(q, base=base)
    with pytest.raises(TypeError):
        T.entanglemententropy(_tto())
    with pytest.raises(T.TTNError, match="ordering must be"):
        q.reorder("zigzag")
    with pytest.raises(TypeError):
        T.qttv_to_array(_ttv())
    with pytest.raises(T.TTNError, match="ordering must be"):
        T.grid_strides(2, 3, "zigzag")
    one = T.TTvector(1, [np.ones((2, 1, 1), order="F")], (2,), [1, 1], [0])
    assert T.entanglemententropy(one).shape == (0,)


def test_nn_laplacian_is_the_scaled_host_constructor():
    d = 4
    A = T.qtt_laplacian(1, d, ordering="serial", bc="NN")
    ref = R.qtt_laplacian(1, d, "serial", bc="NN")
    assert isinstance(A, T.QTToperator) and (A.n_dims, A.bits_per_dim, A.ordering) == (1, d, "serial")
    assert A.tto_rks[0] == 4 and A.tto_rks[-1] == 4 and list(A.tto_rks) == list(ref.tto.tto_rks)
    for ca, cb in zip(A.tto_vec, ref.tto.tto_vec):
        assert np.array_equal(ca, cb)


def test_same_ordering_reorder_returns_a_copy():
    q = T.QTTvector(_ttv(), 2, 3, "serial")
    r = q.reorder("serial")
    assert isinstance(r, T.QTTvector) and r.ordering == "serial" and r.ttv_vec[0] is not q.ttv_vec[0]
    assert all(np.array_equal(a, b) for a, b in zip(r.ttv_vec, q.ttv_vec))
    A = T.QTToperator(_tto(), 2, 3, "interleaved")
    assert isinstance(A.reorder("interleaved"), T.QTToperator)
