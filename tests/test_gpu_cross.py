"""TT-cross on the device (tensortrainnumerics.jl_amd/cross.py, csrc/ttn_cross_kernels.h) against the NumPy restatement
(tests/cross_reference.py), the reference's own cases (test/test_tt_cross_interpolation.jl), closed forms and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import ttn_amd as T
from tests import cross_reference as R
from tests.test_cpu_cross import ACCURACY, _dense_relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    T.ensure_init(0)
    T.tdvp._dev()
    return _t


def _np(X):
    return X.cpu().numpy() if hasattr(X, "cpu") else np.asarray(X)


def dev_f(g):
    """a NumPy function of the (P, N) coordinate matrix as the f tt_cross calls"""
    return lambda X: g(_np(X))


# ---- maxvol --------------------------------------------------------------------------------------------------------------------------
MAXVOL_SIZES = [(1, 1, False), (7, 1, True), (64, 8, False), (180, 90, False), (200, 90, False), (128, 64, True), (130, 64, True),
                (256, 256, False), (4096, 256, False), (1000, 200, True)]


@pytest.mark.parametrize("m,r,cplx", MAXVOL_SIZES, ids=[f"{m}x{r}{'c' if c else 'r'}" for m, r, c in MAXVOL_SIZES])
def test_maxvol_matches_restatement(torch, m, r, cplx):
    rng = np.random.default_rng(m * 7 + r)
    A = rng.standard_normal((m, r)) + (1j * rng.standard_normal((m, r)) if cplx else 0)
    piv, Cd, swaps = T.cross.maxvol(A, 1.05, 100)
    rp, Cr, rs = R.maxvol(A, 1.05, 100)
    assert np.array_equal(piv, rp) and swaps == rs
    assert np.max(np.abs(Cd - Cr)) <= 1e-12 * max(1.0, np.max(np.abs(Cr)))


def test_maxvol_tol_maxiter_and_dominant_input(torch):
    rng = np.random.default_rng(3)
    A = rng.standard_normal((300, 20))
    for tol, maxiter in [(1.05, 0), (1.05, 1), (1.05, 3), (2.0, 100), (1e9, 100)]:
        piv, Cd, swaps = T.cross.maxvol(A, tol, maxiter)
        rp, Cr, rs = R.maxvol(A, tol, maxiter)
        assert np.array_equal(piv, rp) and swaps == rs <= maxiter
        if swaps < maxiter:
            assert np.max(np.abs(Cd)) <= tol * (1 + 1e-12)
    B = np.vstack([np.eye(6), 0.5 * rng.uniform(-1, 1, (50, 6))])
    piv, Cd, swaps = T.cross.maxvol(B)
    assert swaps == 0 and list(piv) == list(range(1, 7))


def test_maxvol_tie_rules(torch):
    """Exact ties in both phases.  getf2 takes the FIRST maximum of |Re| + |Im|; the swaps take the smallest column-major index among
    equal |C_ij|.  Hand-checked cases, then tie-laden matrices against the restatement, which encodes both rules."""
    A = np.array([[1.0, 0.0], [0.0, 1.0], [3.0, 3.0], [3.0, -3.0]])       # column 1: rows 3 and 4 tie at 3
    piv, _, swaps = T.cross.maxvol(A)
    assert list(piv) == [3, 4] and swaps == 0                              # the last maximum would give [4, 3]
    B = np.array([[0.5 + 0.5j, 1.0], [0.2, 1j], [1.0, 0.3]])               # |Re| + |Im| ties at 1: row 1 (modulus 0.71) before row 3 (1)
    piv, _, _ = T.cross.maxvol(B, 1.05, 0)
    assert piv[0] == 1
    cases = [np.array([[1.0, 0.0], [0.0, 1.0], [2.0, 2.0], [2.0, -2.0], [2.0, 2.0]]),                 # duplicated rows
             np.array([[1, 0], [0, 1], [1.5j, 1.5], [-1.5, -1.5j], [1.5j, 1.5], [1.5, 1.5j]]),         # entries of modulus 1.5: ±1.5, ±1.5i
             np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]),   # duplicates of pivots
             np.vstack([B, B]), np.kron(np.ones((3, 1)), np.array([[1.0, -1.0], [1j, 1.0]]))]
    for M in cases:
        for tol, maxiter in [(1.05, 100), (0.5, 4), (1.0, 100)]:
            piv, Cd, swaps = T.cross.maxvol(M, tol, maxiter)
            rp, Cr, rs = R.maxvol(M, tol, maxiter)
            assert list(piv) == list(rp) and swaps == rs, (M, tol, piv, rp, swaps, rs)
            assert np.max(np.abs(Cd - Cr)) <= 1e-12


def test_maxvol_refusals(torch):
    L = T._lib.lib()
    A = torch.zeros((3, 10), dtype=torch.float64, device="cuda")        # Julia 10 x 3, all zero: the first pivot is zero
    A[1] = 1.0
    piv = torch.empty((3,), dtype=torch.int64, device="cuda")
    Cm = torch.empty_like(A)
    info = (C.c_int64 * 2)()
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    assert L.ttn_cross_maxvol(0, 10, 3, p(A), 1.05, 10, p(piv), p(Cm), None, info) == T._lib.TTN_ERR_SINGULAR
    assert set(piv.cpu().tolist()) <= set(range(1, 11))
    assert L.ttn_cross_maxvol(0, 2000, 1025, p(A), 1.05, 10, p(piv), p(Cm), None, info) == T._lib.TTN_ERR_UNSUPPORTED
    assert L.ttn_cross_maxvol(0, (1 << 20) + 1, 1, p(A), 1.05, 10, p(piv), p(Cm), None, info) == T._lib.TTN_ERR_UNSUPPORTED
    with pytest.raises(T.TTNError):
        T.cross.maxvol(np.zeros((5, 2)))
    piv2, _, _ = T.cross.maxvol(np.eye(4)[:, :2] + 0.1)                  # the next ordinary call works
    assert len(piv2) == 2


# ---- evaluation kernel and index matrices ----------------------------------------------------------------------------------------
def _rand_train(rng, dims, rks, cplx):
    return [rng.standard_normal((n, a, b)) + (1j * rng.standard_normal((n, a, b)) if cplx else 0) for n, a, b in zip(dims, rks[:-1], rks[1:])]


@pytest.mark.parametrize("cplx", [False, True])
def test_evaluation_point_and_weight_forms(torch, cplx):
    rng = np.random.default_rng(11 + cplx)
    for dims, rks in [((3,), (1, 1)), ((2, 5, 3, 4), (1, 2, 7, 3, 1)), ((4, 2, 3), (1, 4, 512, 1)), ((2, 3, 2, 2), (1, 2, 6, 300, 1))]:
        cores = _rand_train(rng, dims, rks, cplx)
        idx = np.stack([rng.integers(1, n + 1, 300) for n in dims], axis=1)
        got = T.cross._evaluate_tt(cores, idx, len(dims))
        ref = R._evaluate_tt(cores, idx, len(dims))
        assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
        w = [rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0) for n in dims]
        gw, rw = T.cross._contract_with_weights(cores, w), R._contract_with_weights(cores, w)
        assert abs(gw - rw) <= 1e-12 * max(1.0, abs(rw))
    assert T.cross._evaluate_tt([np.array([1.0, 2.0]).reshape(2, 1, 1), np.array([1.0, 10.0, 100.0]).reshape(3, 1, 1)],
                                np.array([[1, 1], [1, 2], [2, 3]]), 2).tolist() == [1.0, 10.0, 200.0]


def test_index_matrices_equal_restatement(torch):
    rng = np.random.default_rng(2)
    N, Is = 5, [None, 3, 4, 2, 5, 3]
    Rs = [None, 1, 3, 4, 6, 2, 1]
    lsets = [None, np.ones((1, 0), np.int64)] + [np.stack([rng.integers(1, Is[c + 1] + 1, Rs[j]) for c in range(j - 1)], 1) for j in range(2, N + 1)]
    rsets = [None] + [np.stack([rng.integers(1, Is[c] + 1, Rs[j + 1]) for c in range(j + 1, N + 1)], 1) for j in range(1, N)] + [np.ones((1, 0), np.int64)]
    domain = [np.linspace(0, 1, Is[k]) for k in range(1, N + 1)]
    with torch.cuda.stream(T.tdvp._dev()[1]):
        pb = T.cross._Problem(lambda X: X[:, 0], domain)
        dset = lambda a: None if a.shape[1] == 0 else T.cross._dev_set(a)     # noqa: E731
        for j in range(1, N + 1):
            X, idx = pb.points(0, j, Is[j], 1, dset(lsets[j]), dset(rsets[j]), want_idx=True)
            ref = R._build_fiber_indices(lsets, rsets, j, Is, Rs, N)
            assert np.array_equal(idx.cpu().numpy().T, ref)
            assert np.array_equal(X.cpu().numpy().T, np.stack([domain[d][ref[:, d] - 1] for d in range(N)], 1))
        I_l = lsets
        I_g = [None] + [rsets[k] for k in range(1, N)] + [np.ones((1, 0), np.int64)]
        for k in range(1, N):
            X, idx = pb.points(1, k, Is[k], Is[k + 1], dset(I_l[k]), dset(I_g[k + 1]), want_idx=True)
            assert np.array_equal(idx.cpu().numpy().T, R._superblock_indices(I_l, I_g, k, Is, N))


# ---- end-to-end parity ----------------------------------------------------------------------------------------------------------
def _gauss(X):
    return np.exp(-np.sum(X ** 2, axis=1))


def _sin6(X):
    return np.sin(np.sum(X, axis=1))


def _osc5(X):
    return np.cos(37.1 * X[:, 0] + 53.3 * X[:, 1] * X[:, 2] + 71.7 * X[:, 3] ** 2 + 29.9 * X[:, 4] * X[:, 0] + 11.0 * X[:, 2] * X[:, 4])


def _gauss_off(X):
    return np.exp(-np.sum((X - 0.13 * np.arange(1, X.shape[1] + 1)) ** 2, axis=1))


_TABLE5 = np.random.default_rng(55).uniform(-1.0, 1.0, (24,) * 5)


def _rand5(X):
    """a random tensor on the 24-point grid of [0, 1]^5 (looked up by grid index): its fibre matrices are random matrices, of full
    rank and well conditioned, and its values are the same bits whichever side computes them"""
    i = np.rint(np.real(X) * 23.0).astype(np.int64)
    return _TABLE5[i[:, 0], i[:, 1], i[:, 2], i[:, 3], i[:, 4]]


# Parity needs pivot searches without exact ties and fibre matrices of full numerical rank (in a rank-deficient fibre the trailing
# columns of Q are rounding noise, different on two machines).  README example 2 (exp(-|x|^2), rank 1, on a symmetric grid) has
# mirror-image rows of equal modulus, and sin(sum x) on a uniform grid has equal sums along anti-diagonals: the parity runs move the
# centre, give MaxVol the function's rank, and use graded grids that differ per axis (sin(sum x) is symmetric in its arguments); the
# originals are held to their accuracy below.
GRADED = 0.05 + 3.0 * (np.arange(8) / 7.0) ** 1.3
PARITY = [
    ("readme2-offcentre-maxvol", "maxvol", _gauss_off, [np.linspace(-1, 1, 8)] * 4, dict(tol=1e-8), dict(ranks=1)),
    ("readme2-offcentre-dmrg", "dmrg", _gauss_off, [np.linspace(-1, 1, 8)] * 4, dict(tol=1e-8), dict(ranks=2)),
    ("sin6-maxvol", "maxvol", _sin6, [GRADED * (1 + 0.07 * k) for k in range(6)], dict(tol=1e-12), dict(ranks=2)),
    ("sin6-dmrg", "dmrg", _sin6, [GRADED * (1 + 0.07 * k) for k in range(6)], dict(tol=1e-8, maxiter=25), dict(ranks=4)),
    # random right sets drawn with replacement can repeat a row, which makes a fibre rank deficient: seed 2 draws distinct rows
    ("global-route-maxvol", "maxvol", _rand5, [np.linspace(0, 1, 24)] * 5, dict(tol=1e-10, maxiter=2, rmax=60, kickrank=None),
     dict(ranks=[24, 60, 24, 6], seed=2)),
]


@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_cross_parity_with_restatement(torch, case):
    name, alg, g, domain, akw, kw = case
    if alg == "maxvol":
        tt = T.tt_cross(dev_f(g), domain, T.MaxVol(verbose=False, **akw), **kw)
        cores, rks, tr = R.cross_maxvol(g, domain, **akw, **kw)
        sets = [("lsets", range(2, len(domain) + 1)), ("rsets", range(1, len(domain)))]
    else:
        tt = T.tt_cross(dev_f(g), domain, T.DMRG(verbose=False, **akw), **kw)
        cores, rks, tr = R.cross_dmrg(g, domain, **akw, **kw)
        sets = [("I_l", range(2, len(domain) + 1)), ("I_g", range(1, len(domain)))]
    last = T.cross._LAST
    assert tt.ttv_rks == rks and last["sweeps"] == tr["sweeps"]
    for key, ks in sets:
        for k in ks:
            assert np.array_equal(last[key][k], tr[key][k]), (key, k)
    for a, b in zip(last["eps"], tr["eps"]):
        assert abs(a - b) <= max(1e-8 * abs(b), 1e-13), (last["eps"], tr["eps"])
    rng = np.random.default_rng(0)
    idx = np.stack([rng.integers(1, len(d) + 1, 10000) for d in domain], 1)
    yd, yr = R._evaluate_tt(tt.ttv_vec, idx, len(domain)), R._evaluate_tt(cores, idx, len(domain))
    assert np.linalg.norm(yd - yr) <= 1e-10 * np.linalg.norm(yr)
    if name.startswith("global"):
        assert tt.ttv_rks == [1, 24, 60, 24, 6, 1] and 24 * 24 * 60 * 8 > 128 * 1024    # site 2's fibres took the global-memory maxvol


def test_readme_example_2_and_sin6_accuracy(torch):
    domain = [np.linspace(-1, 1, 8)] * 4
    for alg in (T.MaxVol(verbose=False, tol=1e-8), T.DMRG(verbose=False, tol=1e-8)):
        tt = T.tt_cross(dev_f(_gauss), domain, alg, ranks=2)
        assert _dense_relerr(tt.ttv_vec, _gauss, domain) < 1e-8
    domain = [np.linspace(0, math.pi, 8)] * 6                                  # examples/cross.jl:40-50
    tt = T.tt_cross(dev_f(_sin6), domain, T.MaxVol(verbose=False, tol=1e-12), ranks=25)
    rng = np.random.default_rng(6)
    idx = np.stack([rng.integers(1, 9, 10000) for _ in range(6)], 1)
    y = R._evaluate_on_domain(_sin6, domain, idx)
    assert np.linalg.norm(R._evaluate_tt(tt.ttv_vec, idx, 6) - y) <= 1e-10 * np.linalg.norm(y)


def test_stopped_without_converging_returns_core_ranks(torch):
    domain = [np.linspace(0, 1, 10)] * 4
    g = lambda X: np.cos(917.0 * X[:, 0] * X[:, 2] + 613.0 * X[:, 1] ** 2 + 1013.0 * X[:, 2] * X[:, 3] + 411.0 * X[:, 0] * X[:, 3])  # noqa: E731
    akw = dict(tol=1e-12, maxiter=2, kickrank=5)
    tt = T.tt_cross(dev_f(g), domain, T.MaxVol(verbose=False, **akw))
    cores, rks, tr = R.cross_maxvol(g, domain, **akw)
    assert tr["eps"][-1] > 1e-12 and T.cross._LAST["sweeps"] == 2
    assert tt.ttv_rks == [1] + [c.shape[2] for c in tt.ttv_vec] == rks
    assert all(c.shape[1] == r for c, r in zip(tt.ttv_vec, tt.ttv_rks))
    rng = np.random.default_rng(1)
    idx = np.stack([rng.integers(1, 11, 10000) for _ in range(4)], 1)
    yd, yr = R._evaluate_tt(tt.ttv_vec, idx, 4), R._evaluate_tt(cores, idx, 4)
    assert np.linalg.norm(yd - yr) <= 1e-10 * np.linalg.norm(yr)


def test_interpolation_property(torch):
    domain = [np.linspace(0, 1, 9)] * 4
    g = lambda X: 1.0 / (1.0 + np.sum(X, axis=1) ** 2 + X[:, 0] * X[:, 2])     # noqa: E731
    tt = T.tt_cross(dev_f(g), domain, T.MaxVol(verbose=False, tol=1e-30, maxiter=1, kickrank=None), ranks=3)
    rset = T.cross._LAST["rsets"][1]                                           # the right set core 1 was evaluated with
    idx = np.array([[i] + list(row) for row in rset for i in range(1, 10)], dtype=np.int64)
    y = R._evaluate_on_domain(g, domain, idx)
    yhat = R._evaluate_tt(tt.ttv_vec, idx, 4)
    assert np.linalg.norm(y - yhat) <= 1e-12 * np.linalg.norm(y)


# ---- the reference's cases through the device --------------------------------------------------------------------------------------
def test_reference_basic_cases(torch):
    tt = T.tt_cross(dev_f(lambda X: np.sin(X.sum(axis=1))), [np.linspace(0, 1, 10)] * 4, T.MaxVol(verbose=False, tol=1e-6))
    assert isinstance(tt, T.TTvector) and tt.N == 4 and tt.ttv_dims == (10,) * 4 and tt.ttv_rks[0] == tt.ttv_rks[-1] == 1
    assert tt.ttv_ot == [0] * 4 and all(c.dtype == np.float64 for c in tt.ttv_vec)
    tt = T.tt_cross(dev_f(_gauss), [np.linspace(-1, 1, 12)] * 4, T.DMRG(verbose=False, tol=1e-6))
    assert tt.N == 4
    tt = T.tt_cross(dev_f(lambda X: X.sum(axis=1)), [np.arange(1.0, 6.0)] * 3, alg=T.MaxVol(verbose=False))
    assert isinstance(tt, T.TTvector)
    tt = T.tt_cross(lambda X: torch.ones(X.shape[0], dtype=torch.float64, device=X.device), (4, 5, 6), alg=T.MaxVol(verbose=False))
    assert tt.ttv_dims == (4, 5, 6)
    tt = T.tt_cross(lambda X: X.sum(dim=1), [4, 5, 6, 7], alg=T.MaxVol(verbose=False))      # a torch f, values on the device
    assert tt.N == 4
    assert np.allclose(R.full_tensor(tt.ttv_vec), np.add.outer(np.add.outer(np.add.outer(np.arange(1, 5), np.arange(1, 6)), np.arange(1, 7)),
                                                               np.arange(1, 8)), atol=1e-10)


def test_reference_complex_domain(torch):
    domain = [np.linspace(0.0, 1.0, 5) + 1j * np.linspace(0.0, 0.4, 5)] * 3
    g = lambda X: np.exp(X[:, 0] + 0.7 * X[:, 1] - 0.3 * X[:, 2])     # noqa: E731
    rng = np.random.default_rng(91)
    idx = np.stack([rng.integers(1, 6, 150) for _ in range(3)], 1)
    for alg in (T.MaxVol(verbose=False, tol=1e-8, maxiter=20, rmax=30), T.DMRG(verbose=False, tol=1e-8, maxiter=15, rmax=30)):
        tt = T.tt_cross(dev_f(g), domain, alg, ranks=2, val_size=600)
        y = R._evaluate_on_domain(g, domain, idx)
        assert tt.ttv_vec[0].dtype == np.complex128
        assert np.linalg.norm(y - T.cross._evaluate_tt(tt.ttv_vec, idx, 3)) / np.linalg.norm(y) < 1e-6




@pytest.mark.parametrize("case", ACCURACY, ids=[c[0] for c in ACCURACY])
@pytest.mark.parametrize("alg", ["maxvol", "dmrg"])
def test_reference_accuracy_sets(torch, case, alg):
    name, domain, g, tol, maxiter, rmax, bar = case
    A = T.MaxVol if alg == "maxvol" else T.DMRG
    tt = T.tt_cross(dev_f(g), domain, A(verbose=False, tol=tol, maxiter=maxiter, rmax=rmax))
    assert _dense_relerr(tt.ttv_vec, g, domain) < bar
    if name == "rank2 complex":
        assert max(tt.ttv_rks) <= 4


# ---- deep QTT ---------------------------------------------------------------------------------------------------------------------
def test_deep_qtt_sin_feeds_the_solvers(torch):
    d = 30
    h = 1.0 / (2 ** d - 1)
    wts = torch.tensor([h * 2.0 ** (d - k) for k in range(1, d + 1)], dtype=torch.float64, device="cuda")

    def f(X):                                                          # the function behind qtt_sin(30, lam=π), bits of x, site 1 first
        return torch.sin(math.pi * math.pi * (X @ wts))

    y = T.tt_cross(f, [np.array([0.0, 1.0])] * d, T.MaxVol(verbose=False, tol=1e-10, maxiter=3, kickrank=None), ranks=2)
    assert max(y.ttv_rks) <= 2
    ref = T.qtt_sin(d, lam=math.pi)
    rng = np.random.default_rng(4)
    idx = rng.integers(1, 3, (10000, d))
    w = np.array([h * 2.0 ** (d - k) for k in range(1, d + 1)])
    x = (idx - 1) @ w
    assert np.max(np.abs(R._evaluate_tt(y.ttv_vec, idx, d) - np.sin(math.pi ** 2 * x))) <= 1e-10
    # The issue's check, tt_compress_(Delta(30) * y, 8) against the same chain on qtt_sin.  Measured as norm(a - b) / norm(b), the
    # difference of two trains whose norms (0.43) nearly cancel, the comparison has a floor near 1e-5 whatever y is: qtt_sin itself in
    # another gauge (core k times M, core k + 1 times M^-1) gives 0 to 9e-6 against qtt_sin.  The restatement's train, built from the same
    # pivots by LAPACK, gives 2.6e-5 there and the device train 2.9e-5.  So that measure is held relative to the restatement's, and the
    # chain's values are held to the issue's 1e-9 pointwise, at 10^4 points and the four corners, where no cancellation enters.
    D = T.Delta(d)
    a, b = T.tt_compress_(D * y, 8), T.tt_compress_(D * ref, 8)
    cores_r, rks_r, _ = R.cross_maxvol(lambda X: np.sin(math.pi ** 2 * (X @ w)), [np.array([0.0, 1.0])] * d, tol=1e-10, maxiter=3,
                                       kickrank=None, ranks=2)
    yr = T.TTvector(d, [np.asfortranarray(c) for c in cores_r], (2,) * d, rks_r, [0] * d)
    ar = T.tt_compress_(D * yr, 8)
    rel, rel_r = T.norm(T.sub(a, b)) / T.norm(b), T.norm(T.sub(ar, b)) / T.norm(b)
    print(f"Delta chain vs the chain on qtt_sin: device {rel:.3e}, restatement {rel_r:.3e}")
    assert rel <= 2.0 * rel_r
    pts = np.vstack([idx, np.ones((1, d), np.int64), 2 * np.ones((1, d), np.int64), np.r_[np.ones(d - 1), 2][None].astype(np.int64),
                     np.r_[2 * np.ones(d - 1), 1][None].astype(np.int64)])
    va, vb = R._evaluate_tt(a.ttv_vec, pts, d), R._evaluate_tt(b.ttv_vec, pts, d)
    assert np.max(np.abs(va - vb)) <= 1e-9 * T.norm(b)


# ---- tt_integrate -------------------------------------------------------------------------------------------------------------------
def test_integrate_reference_cases(torch):
    ones = lambda X: np.ones(X.shape[0])       # noqa: E731
    assert T.tt_integrate(dev_f(ones), 3, alg=T.DMRG(verbose=False)) == pytest.approx(1.0, abs=1e-6)
    assert T.tt_integrate(dev_f(ones), [0.0, 0.0], [2.0, 3.0], alg=T.DMRG(verbose=False)) == pytest.approx(6.0, abs=1e-6)
    assert T.tt_integrate(dev_f(lambda X: X[:, 0] ** 2), 1, alg=T.DMRG(verbose=False), nquad=10) == pytest.approx(1 / 3, abs=1e-6)


def test_integrate_sin6_closed_form(torch):
    got = T.tt_integrate(dev_f(_sin6), 6, alg=T.MaxVol(verbose=False, tol=1e-12))
    exact = ((np.exp(1j) - 1) ** 6 / 1j ** 6).imag
    assert abs(got - exact) <= 1e-10 * abs(exact)


@pytest.mark.parametrize("d", [10, 20, 50])
def test_integrate_gaussian_high_dim(torch, d):
    got = T.tt_integrate(lambda X: torch.exp(-(X * X).sum(dim=1)), d, lower=-5.0, upper=5.0, alg=T.MaxVol(verbose=False, tol=1e-12))
    x, w = T.cross._gauss_legendre(20, -5.0, 5.0)
    one = float(np.dot(w, np.exp(-x ** 2)))
    assert abs(got - one ** d) <= 1e-10 * one ** d
    print(f"d = {d}: relative distance to pi^(d/2) = {abs(got - math.pi ** (d / 2)) / math.pi ** (d / 2):.3e}")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_library_usable(torch):
    dom = [np.linspace(0, 1, 5)] * 3
    ok = dev_f(lambda X: np.exp(X.sum(axis=1)))
    with pytest.raises(T.TTNError, match="Greedy"):
        T.tt_cross(ok, dom, T.Greedy(verbose=False))
    with pytest.raises(T.TTNError, match="MaxVolPivot"):
        T.tt_cross(ok, dom, T.MaxVol(verbose=False, pivot=T.RandomPivot()))
    with pytest.raises(T.TTNError, match="MaxVolPivot"):
        T.tt_cross(ok, dom, T.DMRG(verbose=False, pivot=T.RandomPivot()))
    with pytest.raises(T.TTNError, match="values for"):
        T.tt_cross(dev_f(lambda X: np.ones(X.shape[0] + 1)), dom, T.MaxVol(verbose=False))
    with pytest.raises(T.TTNError, match="non-finite"):
        T.tt_cross(dev_f(lambda X: np.where(X[:, 1] > 0.6, np.nan, 1.0 + X[:, 0])), dom, T.MaxVol(verbose=False), val_size=3)
    with pytest.raises(T.TTNError, match="non-finite"):
        T.tt_cross(dev_f(lambda X: np.where(X[:, 1] > 0.6, np.inf, 1.0 + X[:, 0])), dom, T.DMRG(verbose=False))
    with pytest.raises(T.TTNError):
        T.cross._evaluate_tt([np.ones((2, 1, 1025)), np.ones((2, 1025, 1))], np.ones((1, 2)), 2)
    with pytest.raises(T.TTNError, match="DimensionMismatch"):                  # cores that do not chain: refused on the host
        T.cross._evaluate_tt([np.ones((2, 1, 2)), np.ones((2, 3, 1))], np.ones((1, 2)), 2)
    with pytest.raises(T.TTNError, match="BoundsError"):
        T.cross._evaluate_tt([np.ones((2, 1, 2)), np.ones((2, 2, 1))], np.array([[1, 3]]), 2)
    with pytest.raises(T.TTNError, match="DimensionMismatch"):
        T.cross._contract_with_weights([np.ones((2, 1, 2)), np.ones((3, 2, 1))], [np.ones(2), np.ones(2)])
    tt = T.tt_cross(ok, dom, T.MaxVol(verbose=False))
    assert np.allclose(R.full_tensor(tt.ttv_vec), np.exp(np.add.outer(np.add.outer(dom[0], dom[1]), dom[2])), rtol=1e-9)
