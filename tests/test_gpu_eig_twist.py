"""The eigenvector phase of the symmetric eigensolver (wg_twisted, csrc/ttn_eig_kernels.h) at the inputs that reach what r03l changed
(DESIGN §4.2): twist indices at both ends of the matrix and in the rows of every one of the four waves that hold D- in registers
(n / 4 rows each), the pivot floor, lanes without a vector, a partly filled last pair of columns in the back-transformation, and the new
barriers.  Single-workgroup launches of the self-test hook, both builds (TTN_WG512_SELFTEST), n = 128 and n = 64.

Reference and tolerances are those of test_gpu_kernels.py::test_eig_selftest: numpy.linalg.eigh; eigenvalues to 1e-13 of the largest,
orthonormality and residual of the returned vectors to 1e-11."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BUILDS = [0, 1]              # TTN_WG512_SELFTEST: the 1024-thread build, the 512-thread build
SIZES = [128, 64]


def run_eig(G, n, r, nev):
    import ttn_amd as T
    T.ensure_init(0)
    G = np.asfortranarray(G)
    sig = np.zeros(128)
    X = np.zeros((128, 64), order="F")
    tk = (C.c_int64 * 6)()
    T._lib.check(T._lib.lib().ttn_selftest_eig128(G.ctypes.data_as(C.c_void_p), n, r, nev, sig.ctypes.data_as(C.c_void_p),
                                                  X.ctypes.data_as(C.c_void_p), tk))
    assert tk[1] == 0
    return sig, X


def check(G, w, n, r, nev, sig, X):
    """w: eigenvalues of G, descending (numpy.linalg.eigvalsh)"""
    assert np.max(np.abs(sig[:nev] ** 2 - w[:nev])) <= 1e-13 * w[0]
    Ux = X[:n, :r] / sig[:r]
    assert np.max(np.abs(Ux.T @ Ux - np.eye(r))) <= 1e-11
    assert np.max(np.abs(G @ Ux - Ux * w[:r])) <= 1e-11 * w[0]


@functools.lru_cache(maxsize=None)
def matrix(kind, n):
    """(G, eigenvalues descending); computed once per (kind, n) and shared, never modified"""
    rng = np.random.default_rng({"diagonal": 11, "localised": 12, "workload": 13}[kind] + n)
    if kind == "diagonal":
        # distinct positive entries in a shuffled order, the two largest at rows 0 and n - 1: the tridiagonal is G itself, every
        # eigenvector a unit vector, D+ and D- vanish at the twist (the pivot floor replaces them), and the 64 kept eigenvalues
        # sit at rows spread over the whole matrix
        d = np.linspace(1.0, 2.0, n)
        mid = rng.permutation(d[:-2])
        G = np.diag(np.concatenate(([d[-1]], mid, [d[-2]])))
    elif kind == "localised":
        P = rng.standard_normal((n, n))
        G = 0.37 * (np.diag(np.linspace(1.0, 2.0, n)) + 1e-3 * (P + P.T) / 2)
    else:
        M = rng.standard_normal((n, 3 * n))
        U, s, Vt = np.linalg.svd(M, full_matrices=False)
        M = (U * (s[0] * 10.0 ** (-1.5 * np.arange(n) / (n - 1)))) @ Vt
        M /= np.max(np.abs(M))
        G = M @ M.T
    G = np.asfortranarray(G)
    w = np.linalg.eigvalsh(G)[::-1].copy()
    G.setflags(write=False)
    w.setflags(write=False)
    return G, w


@pytest.mark.parametrize("wg512", BUILDS)
@pytest.mark.parametrize("n", SIZES)
def test_diagonal_matrix(monkeypatch, n, wg512):
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    G, w = matrix("diagonal", n)
    r = nev = 64
    sig, X = run_eig(G, n, r, nev)
    check(G, w, n, r, nev, sig, X)
    rows = np.argmax(np.abs(X[:n, :r]), axis=0)
    assert rows[0] == 0 and rows[1] == n - 1                              # the two ends
    assert set(rows // (n // 4)) == set(range(4))                         # every holder's rows hold a twist


@pytest.mark.parametrize("wg512", BUILDS)
@pytest.mark.parametrize("n", SIZES)
def test_localised_vectors(monkeypatch, n, wg512):
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    G, w = matrix("localised", n)
    sig, X = run_eig(G, n, 64, 64)
    check(G, w, n, 64, 64, sig, X)


@pytest.mark.parametrize("wg512", BUILDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("r,all_values", [(1, False), (17, False), (63, False), (1, True), (17, True), (63, True)])
def test_vector_counts(monkeypatch, n, r, all_values, wg512):
    """fewer vectors than lanes (r = 1, 17), an odd count (a column pair of the back-transformation half filled), with a few more
    eigenvalues than vectors and with all n"""
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    G, w = matrix("workload", n)
    nev = n if all_values else min(n, r + 4 + r // 2)
    assert nev > r
    sig, X = run_eig(G, n, r, nev)
    check(G, w, n, r, nev, sig, X)


@pytest.mark.parametrize("wg512", BUILDS)
@pytest.mark.parametrize("n", SIZES)
def test_same_input_same_bytes(monkeypatch, n, wg512):
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    G, _ = matrix("localised", n)
    sig1, X1 = run_eig(G, n, 64, 64)
    sig2, X2 = run_eig(G, n, 64, 64)
    assert sig1.tobytes() == sig2.tobytes()
    assert X1.tobytes() == X2.tobytes()
