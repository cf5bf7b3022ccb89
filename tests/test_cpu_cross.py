"""TT-cross without a GPU: the reference's tests of the algorithm defaults and of the host helpers (test/test_tt_cross_interpolation.jl),
the NumPy restatement (tests/cross_reference.py) against the reference's accuracy bars, the device entry points failing loudly, and
the register report of the new kernels."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ttn_amd as T
from tests import cross_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- defaults (:7-71) -------------------------------------------------------------------------------------------------------------
def test_pivot_defaults():
    p = T.MaxVolPivot()
    assert p.tol == pytest.approx(1.05) and p.maxiter == 100
    p = T.MaxVolPivot(tol=1.1, maxiter=50)
    assert p.tol == pytest.approx(1.1) and p.maxiter == 50
    p = T.RandomPivot()
    assert p.nsamples == 1000 and p.seed is None
    p = T.RandomPivot(nsamples=500, seed=42)
    assert p.nsamples == 500 and p.seed == 42


def test_algorithm_defaults():
    a = T.MaxVol()
    assert (a.maxiter, a.rmax, a.kickrank, a.verbose) == (50, 500, 5, True) and a.tol == pytest.approx(1e-10)
    assert isinstance(a.pivot, T.MaxVolPivot)
    a = T.MaxVol(maxiter=50, tol=1e-6, rmax=100, kickrank=None, verbose=False)
    assert (a.maxiter, a.rmax, a.kickrank, a.verbose) == (50, 100, None, False) and a.tol == pytest.approx(1e-6)
    g = T.Greedy()
    assert (g.maxiter, g.rmax, g.verbose, g.nsamples) == (50, 500, True, 1000) and g.tol == pytest.approx(1e-10)
    assert isinstance(g.pivot, T.RandomPivot)
    g = T.Greedy(maxiter=100, tol=1e-8, nsamples=500, verbose=False)
    assert (g.maxiter, g.nsamples, g.verbose) == (100, 500, False) and g.tol == pytest.approx(1e-8)
    d = T.DMRG()
    assert (d.maxiter, d.rmax, d.verbose) == (50, 500, True) and d.tol == pytest.approx(1e-10)
    assert isinstance(d.pivot, T.MaxVolPivot)
    d = T.DMRG(maxiter=30, tol=1e-12, kickrank=5)
    assert d.maxiter == 30 and d.tol == pytest.approx(1e-12)


# ---- helpers (:483-555, :605-629) -------------------------------------------------------------------------------------------------
def test_cap_ranks():
    Rs = [None, 1, 10, 10, 10, 1]
    T.cross._cap_ranks_(Rs, [None, 3, 4, 5, 6], 100)
    assert Rs[1] == 1 and Rs[-1] == 1 and all(r <= 100 for r in Rs[2:-1])
    Rs = [None, 1, 100, 100, 1]
    T.cross._cap_ranks_(Rs, [None, 2, 2, 2], 50)
    assert Rs[2] <= 2 and Rs[3] <= 4


def test_evaluate_on_domain_and_evaluate_tt_restated():
    dom = [np.array([1.0, 2.0, 3.0]), np.array([10.0, 20.0])]
    got = R._evaluate_on_domain(lambda x: x.sum(axis=1), dom, np.array([[1, 1], [2, 2], [3, 1]]))
    assert np.allclose(got, [11.0, 22.0, 13.0])
    cores = [np.array([1.0, 2.0]).reshape(2, 1, 1), np.array([1.0, 10.0, 100.0]).reshape(3, 1, 1)]
    assert np.allclose(R._evaluate_tt(cores, np.array([[1, 1], [1, 2], [2, 3]]), 2), [1.0, 10.0, 200.0])
    w = [np.array([0.5, 0.5]), np.array([1 / 3, 1 / 3, 1 / 3])]
    assert R._contract_with_weights([cores[0], np.array([1.0, 2.0, 3.0]).reshape(3, 1, 1)], w) == pytest.approx(3.0)


def test_sample_superblock_and_combine_indices_restated():
    dom = [np.array([1.0, 2.0]), np.array([10.0, 20.0]), np.array([100.0, 200.0])]
    I_l = [None, np.ones((1, 0), dtype=np.int64), np.array([[1], [2]]), np.array([[1, 1], [2, 2]])]
    I_g = [None, np.array([[1, 1], [2, 2]]), np.array([[1], [2]]), np.ones((1, 0), dtype=np.int64)]
    sb = R._sample_superblock(lambda x: x.sum(axis=1), dom, I_l, I_g, 1, [None, 2, 2, 2], 3)
    assert sb.shape == (1, 2, 2, 2)
    assert sb[0, 1, 0, 1] == 2.0 + 10.0 + 200.0
    res = R._combine_indices_left(np.array([[1, 2], [3, 4]]), 3)
    assert res.shape == (6, 3) and list(res[0]) == [1, 2, 1] and list(res[2]) == [1, 2, 2]
    res = R._combine_indices_right(3, np.array([[1, 2], [3, 4]]))
    assert res.shape == (6, 3) and list(res[0]) == [1, 1, 2] and list(res[3]) == [1, 3, 4]


def test_gauss_legendre():
    x, w = T.cross._gauss_legendre(5, 0.0, 1.0)
    assert len(x) == 5 and len(w) == 5 and sum(w) == pytest.approx(1.0) and np.all((0 < x) & (x < 1))
    x, w = T.cross._gauss_legendre(3, -2.0, 2.0)
    assert len(x) == 3 and sum(w) == pytest.approx(4.0) and np.all((-2 < x) & (x < 2))
    x, w = T.cross._gauss_legendre(10, 0.0, 1.0)
    assert float(np.dot(w, x ** 2)) == pytest.approx(1 / 3, abs=1e-14)


def test_draw_indices_are_seeded_and_in_range():
    a = T.cross.draw_indices(7, T.cross.DRAW_KICK, 3, 2, 500, [2, 5, 9])
    b = T.cross.draw_indices(7, T.cross.DRAW_KICK, 3, 2, 500, [2, 5, 9])
    c = T.cross.draw_indices(7, T.cross.DRAW_KICK, 3, 1, 500, [2, 5, 9])
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    for col, hi in enumerate([2, 5, 9]):
        assert a[:, col].min() == 1 and a[:, col].max() == hi
    assert R.draw_indices is T.cross.draw_indices


# ---- restatement against the reference's accuracy bars (:243-480) and README example 2 ---------------------------------------------
def _dense_relerr(cores, f, domain):
    approx = R.full_tensor(cores)
    grids = np.meshgrid(*domain, indexing="ij")
    exact = f(np.stack([g.reshape(-1) for g in grids], axis=1)).reshape(approx.shape)
    return np.linalg.norm(approx - exact) / max(np.linalg.norm(exact), np.finfo(float).eps)


ACCURACY = [
    ("rank1 real", [np.linspace(0.1, 1.0, 6)] * 4, lambda X: np.prod(np.sin(X), axis=1), 1e-10, 30, 500, 1e-8),
    ("polynomial", [np.linspace(0.0, 1.0, 8)] * 3, lambda X: np.sum(X, axis=1) ** 2, 1e-8, 30, 10, 1e-6),
    ("gaussian", [np.linspace(-1.0, 1.0, 8)] * 4, lambda X: np.exp(-np.sum(X ** 2, axis=1)), 1e-6, 50, 20, 1e-4),
    ("rank1 complex", [np.linspace(0.0, 1.0, 5)] * 3, lambda X: np.prod(np.exp(1j * X), axis=1), 1e-10, 30, 500, 1e-8),
    ("complex grid", [np.linspace(1.0 + 0.5j, 2.0 + 1.0j, 5)] * 3, lambda X: np.prod(X, axis=1), 1e-10, 30, 500, 1e-8),
    ("smooth complex", [np.linspace(0.0, 1.0, 6)] * 3, lambda X: np.exp(1j * np.sum(X ** 2, axis=1)), 1e-6, 50, 20, 1e-4),
    ("rank2 complex", [np.linspace(0.0, math.pi, 7)] * 3,
     lambda X: np.prod(np.sin(X), axis=1) + 1j * np.prod(np.cos(X), axis=1), 1e-10, 30, 4, 1e-8),
    ("lorentzian", [np.linspace(-1.0, 1.0, 8)] * 3, lambda X: 1.0 / (0.3j + np.sum(X ** 2, axis=1)), 1e-6, 40, 20, 1e-4),
    ("4d separable", [np.linspace(0.0, 1.0, 6)] * 4, lambda X: np.prod(1.0 + 1j * X, axis=1), 1e-10, 20, 500, 1e-8),
]


@pytest.mark.parametrize("case", ACCURACY, ids=[c[0] for c in ACCURACY])
@pytest.mark.parametrize("alg", ["maxvol", "dmrg"])
def test_restatement_meets_reference_accuracy(case, alg):
    name, domain, f, tol, maxiter, rmax, bar = case
    run = R.cross_maxvol if alg == "maxvol" else R.cross_dmrg
    cores, rks, _ = run(f, domain, tol=tol, maxiter=maxiter, rmax=rmax)
    assert _dense_relerr(cores, f, domain) < bar
    if name == "rank2 complex":
        assert max(rks) <= 4


def test_restatement_readme_example_2():
    domain = [np.linspace(-1.0, 1.0, 8)] * 4
    f = lambda X: np.exp(-np.sum(X ** 2, axis=1))      # noqa: E731
    cores, _, tr = R.cross_maxvol(f, domain, tol=1e-8, ranks=2)
    assert _dense_relerr(cores, f, domain) < 1e-8


def test_restatement_maxvol_properties():
    rng = np.random.default_rng(5)
    for m, r, cplx in [(40, 7, False), (33, 33, False), (64, 10, True), (12, 1, True)]:
        A = rng.standard_normal((m, r)) + (1j * rng.standard_normal((m, r)) if cplx else 0)
        piv, C, swaps = R.maxvol(A, 1.0, 100)
        assert len(set(piv)) == r and np.max(np.abs(C)) <= 1.0 + 1e-12
        assert np.allclose(C[piv - 1], np.eye(r), atol=1e-12) and np.allclose(C @ A[piv - 1], A, atol=1e-10)
    # an already dominant block: no swap
    A = np.vstack([np.eye(4), 0.1 * rng.standard_normal((20, 4))])
    assert R.maxvol(A)[2] == 0


# ---- no CPU fallback ------------------------------------------------------------------------------------------------------------
def test_cross_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    f = lambda X: X.sum(axis=1)       # noqa: E731
    with pytest.raises(T.TTNError):
        T.tt_cross(f, [np.linspace(0, 1, 4)] * 3, T.MaxVol(verbose=False))
    with pytest.raises(T.TTNError):
        T.tt_integrate(f, 3, alg=T.DMRG(verbose=False))
    with pytest.raises(T.TTNError):
        T.cross._evaluate_tt([np.ones((2, 1, 1))], np.ones((1, 1)), 1)
    L = T._lib.lib()
    assert L.ttn_cross_maxvol(0, 4, 2, None, 1.05, 10, None, None, None, None) != 0


def test_cross_kernels_have_no_spills(tmp_path):
    """The maxvol, index and evaluation kernels compile for gfx950 without VGPR or SGPR spills (the compiler's resource report)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "tensortrainnumerics.jl_amd", "csrc")
    tu = tmp_path / "cross_tu.hip"
    inst = []
    for c in ("false", "true"):
        inst += [f"template __global__ void k_cross_maxvol<{c}>(int, int, const double*, double, int, long long*, double*, double*, int*, "
                 "long long*, int);",
                 f"template __global__ void k_cross_points<{c}>(int, long long, int, int, long long, long long, long long, long long, "
                 "const long long*, const long long*, const long long*, const long long*, const double*, long long*, double*);",
                 f"template __global__ void k_cross_eval<{c}>(int, long long, const long long*, const long long*, const double*, int, double*);",
                 f"template __global__ void k_cross_relerr<{c}>(long long, const double*, const double*, double, double*);"]
    tu.write_text('#include "ttn_cross_kernels.h"\n' + "\n".join(inst) + "\n")
    out = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-c", "-Rpass-analysis=kernel-resource-usage", "-I", csrc,
                          str(tu), "-o", str(tmp_path / "cross_tu.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
    names = [b.split()[0] for b in blocks]
    assert sum("k_cross" in n for n in names) == 8, names
    for b in blocks:
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, b[:200]
        assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, b[:200]
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b[:200]
