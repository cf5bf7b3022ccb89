"""The eigenvalue phase of the symmetric eigensolver (wg_bisect, csrc/ttn_eig_kernels.h) after r03m: every wave runs its
own multisection loop and leaves when its own groups have converged (a wave-level vote instead of a workgroup barrier per round),
waves without an eigenvalue never enter, and a group's section points are counted by DPP.  Single-workgroup launches of the
eigensolver's self-test hook, both builds (TTN_WG512_SELFTEST), n = 64 and 128, nev in {1, 32, 33, 64}: one group in one wave; the
largest count of the 8-lane form (TL = 8: four full waves); the smallest of the 4-lane form (TL = 4: two full waves and ONE group in
a third); the benchmark's count (four full waves).

Matrices, all symmetric positive definite:
  graded     eigenvalues 1 ... 1e-12, log-spaced: the stopping rule is relative to each eigenvalue, so the waves that hold the small
             ones need more rounds than the others and every wave leaves at a round of its own
  cluster    eight equal eigenvalues among distinct ones: eight groups converge on one point, some of them across two waves
  identity   c I: every Sturm count jumps from 0 to n at one point
  diagonal   distinct diagonal entries, no coupling: the leading minors are the products of (d_i - x), so a minor is EXACTLY zero
             whenever a section point equals a diagonal entry.  In its last rounds a group's interval is 3 to 15 ulps wide around an
             entry that is itself a floating-point number, and four or eight of the few numbers inside are section points: over the
             groups of a launch some of them land on the entry (a float64 emulation of the rounds on these two matrices: in 13 of 32 groups
             at nev = 32, in 36 to 38 of 64 at nev = 64; not asserted here, the kernel does not report it).  Those lanes repeat the
             count by the guarded recurrence, a divergent call between the wave-level vote and the DPP sum

Reference: numpy.linalg.eigvalsh; the eigenvalues (the squares of the returned sqrt(lam)) agree to 1e-13 ||A||_2."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BUILDS = [0, 1]              # TTN_WG512_SELFTEST: the 1024-thread build, the 512-thread build
SIZES = [64, 128]
NEVS = [1, 32, 33, 64]
KINDS = ["graded", "cluster", "identity", "diagonal"]


@functools.lru_cache(maxsize=None)
def matrix(kind, n):
    """(G, eigenvalues descending by numpy.linalg.eigvalsh); computed once per (kind, n) and shared, never modified"""
    rng = np.random.default_rng({"graded": 21, "cluster": 22, "identity": 23, "diagonal": 24}[kind] + n)
    if kind in ("graded", "cluster"):
        if kind == "graded":
            lam = 10.0 ** (-12.0 * np.arange(n) / (n - 1))
        else:
            lam = np.linspace(2.0, 1.0, n)
            lam[3:11] = lam[3]                                            # inside the 32 largest
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        G = (Q * lam) @ Q.T
        G = 0.5 * (G + G.T)
    elif kind == "identity":
        G = 0.37 * np.eye(n)
    else:
        G = np.diag(rng.permutation(np.linspace(1.0, 2.0, n)))
    G = np.asfortranarray(G)
    w = np.linalg.eigvalsh(G)[::-1].copy()
    assert w[-1] > 0.0
    G.setflags(write=False)
    w.setflags(write=False)
    return G, w


def eigenvalues(G, n, nev):
    import ttn_amd as T
    T.ensure_init(0)
    sig = np.zeros(128)
    X = np.zeros((128, 64), order="F")
    tk = (C.c_int64 * 2)()
    T._lib.check(T._lib.lib().ttn_selftest_eig128(G.ctypes.data_as(C.c_void_p), n, 1, nev, sig.ctypes.data_as(C.c_void_p),
                                                  X.ctypes.data_as(C.c_void_p), tk))
    assert tk[1] == 0
    return sig[:nev] ** 2


@pytest.mark.parametrize("wg512", BUILDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nev", NEVS)
@pytest.mark.parametrize("kind", KINDS)
def test_eigenvalues(monkeypatch, kind, nev, n, wg512):
    monkeypatch.setenv("TTN_WG512_SELFTEST", str(wg512))
    G, w = matrix(kind, n)
    lam = eigenvalues(G, n, nev)
    err = np.max(np.abs(lam - w[:nev]))
    print(f"{kind} n={n} nev={nev} wg512={wg512}: max |lam - eigvalsh| = {err:.2e}, bound {1e-13 * w[0]:.2e}")
    assert err <= 1e-13 * w[0]
