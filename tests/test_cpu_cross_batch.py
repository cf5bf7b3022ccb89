"""tt_cross_batch without a GPU: the function families of the batched parity tests (shared with tests/test_gpu_cross_batch.py) qualify
for pivot parity by the NumPy restatement alone, the refusals that need no device, the C header against the ctypes table, and the
register report of the new kernels."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ttn_amd as T
from tests import cross_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the families ------------------------------------------------------------------------------------------------------------------
# Pivot parity holds for tie-free fibres of full numerical rank only.  A random table looked up by grid index has
# random fibre matrices, and its values are the same bits whichever side computes them.
def table_family(dims, batch, seed):
    """`batch` random tensors on the integer grid 1..n_k"""
    tabs = [np.random.default_rng(1000 * seed + b).uniform(-1.0, 1.0, dims) for b in range(batch)]

    def make(tab):
        return lambda X: tab[tuple(np.rint(X[:, k]).astype(np.int64) - 1 for k in range(len(dims)))]
    return [make(t) for t in tabs]


# (name, dims, batch, ranks, algorithm keywords, seed); the domain is the integer grid, val_size 50.  The seed is part of a family: random
# right sets and kick rows are drawn with replacement, and a repeated row makes a fibre rank deficient, so each seed here is one whose
# draws are distinct rows (the test below is the proof).
PARITY = [
    ("N2-b1", (5, 7), 1, 3, dict(tol=1e-10, maxiter=2, kickrank=None), 0),
    ("N3-b3-list-capped-kick", (4, 6, 5), 3, [9, 3], dict(tol=1e-10, maxiter=3, kickrank=2), 12),
    ("N5-b5-kick", (4, 5, 6, 7, 4), 5, 2, dict(tol=1e-10, maxiter=2, kickrank=2), 16),
    ("N5-b3-nokick", (6, 4, 7, 5, 4), 3, [3, 5, 4, 2], dict(tol=1e-10, maxiter=2, kickrank=None), 1),
]

# one rank-1 function, one that needs a kick, one that never converges within maxiter = 2
MIXED_DOMAIN = [0.05 + 3.0 * (np.arange(n) / (n - 1.0)) ** 1.3 * (1 + 0.07 * k) for k, n in enumerate((6, 5, 7))]
MIXED_ALG = dict(tol=1e-10, maxiter=2, kickrank=1)
MIXED_KW = dict(ranks=1, val_size=50, seed=0)
_MIXED_TABLE = np.random.default_rng(77).uniform(-1.0, 1.0, (6, 5, 7))


def _mixed_lookup(X):
    idx = tuple(np.argmin(np.abs(X[:, k][:, None] - MIXED_DOMAIN[k][None, :]), axis=1) for k in range(3))
    return _MIXED_TABLE[idx]


MIXED = [lambda X: np.exp(-np.sum((X - 0.13 * np.arange(1, 4)) ** 2, axis=1)), lambda X: np.sin(np.sum(X, axis=1)), _mixed_lookup]
MIXED_SWEEPS = [1, 2, 2]


def perturbed(g, domain):
    """g (1 + 1e-13 cos(a fixed hash of the grid indices))"""
    def h(X):
        idx = [np.argmin(np.abs(X[:, k][:, None] - np.asarray(domain[k])[None, :]), axis=1) for k in range(len(domain))]
        return g(X) * (1.0 + 1e-13 * np.cos(sum(7919.0 * (k + 1) * (i + 1) for k, i in enumerate(idx))))
    return h


def _same_trace(g, domain, akw, kw):
    c0, r0, t0 = R.cross_maxvol(g, domain, **akw, **kw)
    c1, r1, t1 = R.cross_maxvol(perturbed(g, domain), domain, **akw, **kw)
    assert r0 == r1 and t0["sweeps"] == t1["sweeps"]
    for k in range(2, len(domain) + 1):
        assert np.array_equal(t0["lsets"][k], t1["lsets"][k]), ("lsets", k)
    for k in range(1, len(domain)):
        assert np.array_equal(t0["rsets"][k], t1["rsets"][k]), ("rsets", k)
    return t0


@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_table_families_qualify_for_parity(case):
    name, dims, batch, ranks, akw, seed = case
    domain = [np.arange(1.0, n + 1.0) for n in dims]
    for g in table_family(dims, batch, seed):
        _same_trace(g, domain, akw, dict(ranks=ranks, val_size=50, seed=seed))


def test_mixed_family_qualifies_and_finishes_in_different_sweeps():
    sweeps, conv = [], []
    for g in MIXED:
        tr = _same_trace(g, MIXED_DOMAIN, MIXED_ALG, MIXED_KW)
        sweeps.append(tr["sweeps"])
        conv.append(tr["eps"][-1] < MIXED_ALG["tol"])
    assert sweeps == MIXED_SWEEPS and conv == [True, True, False]
    assert len({s for s, c in zip(sweeps, conv) if c}) >= 2 and not all(conv)


# ---- refusals that are known before the device is touched ----------------------------------------------------------------------------
def test_refusals_before_any_launch():
    dom = [np.linspace(0, 1, 5)] * 3
    f = lambda X, which: X.sum(axis=2)       # noqa: E731
    for alg, word in [(T.DMRG(verbose=False), "DMRG"), (T.Greedy(verbose=False), "Greedy"),
                      (T.MaxVol(verbose=False, pivot=T.RandomPivot()), "MaxVolPivot")]:
        with pytest.raises(T.TTNError, match=word):
            T.tt_cross_batch(f, dom, 2, alg)
        with pytest.raises(T.TTNError, match=word):
            T.tt_integrate_batch(f, 3, 2, alg=alg)
    for batch in (0, -3):
        with pytest.raises(T.TTNError, match="batch"):
            T.tt_cross_batch(f, dom, batch, T.MaxVol(verbose=False))
    with pytest.raises(T.TTNError, match="real domain"):
        T.tt_cross_batch(f, [np.linspace(0, 1, 4) + 0.5j] * 2, 2, T.MaxVol(verbose=False))
    assert "tt_cross_batch" in T.__all__ and "tt_integrate_batch" in T.__all__


def test_batch_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(T.TTNError):
        T.tt_cross_batch(lambda X, which: X.sum(axis=2), [np.linspace(0, 1, 4)] * 3, 2, T.MaxVol(verbose=False))
    L = T._lib.lib()
    assert L.ttn_cross_batch_site(1, 0, 2, 1, 2, 1, 2, None, 1.05, 10, None, None, None, None, None) != 0


# ---- the C ABI of include/ttn_cross_batch.h ------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_agree():
    hdr = open(os.path.join(ROOT, "include", "ttn_cross_batch.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    names = {"ttn_cross_batch_points", "ttn_cross_batch_site", "ttn_cross_batch_eval"}
    assert {n for n, _ in protos} == set(T._lib.CROSS_BATCH_SIGNATURES) == names
    L = ctypes
    table = {"int": L.c_int, "int64_t": L.c_int64, "double": L.c_double}
    lib = T._lib.lib()
    for name, args in protos:
        res, argt = T._lib.CROSS_BATCH_SIGNATURES[name]
        assert res is L.c_int and hasattr(lib, name)
        types = []
        for a in [x.strip() for x in args.split(",")]:
            t = re.sub(r"\s*[A-Za-z_][A-Za-z0-9_]*$", "", re.sub(r"\bconst\b", "", a).strip())
            types.append(re.sub(r"\s+", "", t))
        assert len(types) == len(argt), name
        for ct, at in zip(types, argt):
            if ct.endswith("*"):
                assert at is L.c_void_p or hasattr(at, "_type_"), (name, ct)
            else:
                assert at is table[ct], (name, ct)
    assert '#include "ttn_cross_batch.h"' in open(os.path.join(ROOT, "include", "ttn.h")).read()
    assert "ttn_cross_batch_site" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_batch_kernels_have_no_spills(tmp_path):
    """The four kernels compile for gfx950 without VGPR spills and without scratch memory (the compiler's resource report).  The site
    kernel, which holds the QR, the pivot search and the final solve in one body, keeps some scalar values in lanes of a vector
    register (an SGPR spill that never reaches memory: ScratchSize stays 0); the three small kernels spill nothing."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "tensortrainnumerics.jl_amd", "csrc")
    tu = tmp_path / "cross_batch_tu.hip"
    tu.write_text('#include "ttn_cross_batch_kernels.h"\n')
    out = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-c", "-Rpass-analysis=kernel-resource-usage", "-I", csrc,
                          str(tu), "-o", str(tmp_path / "cross_batch_tu.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: Function Name: ", out.stderr)[1:] if "k_cross_batch" in b.split()[0]]
    assert len(blocks) == 4, [b.split()[0] for b in blocks]
    for b in blocks:
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, b[:200]
        assert "k_cross_batch_site" in b.split()[0] or int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, b[:200]
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b[:200]
