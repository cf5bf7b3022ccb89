"""CPU-side tests (no GPU) of contract_sites: the NumPy reference against itself (two association orders and the dense tensor), the
argument checks that need no device, and the metadata arithmetic of marginal / slice_dim."""
import itertools

import numpy as np
import pytest

import ttn_amd as T
from tests import contract_reference as R
from ttn_amd import device as D
from ttn_amd import qttnd as Q


def rand_cores(rng, dims, rks):
    return [np.asfortranarray(rng.standard_normal((dims[k], rks[k], rks[k + 1]))) for k in range(len(dims))]


def test_reference_chain_equals_dense_for_every_pattern():
    """d = 5 with mixed dims: for all 30 proper non-empty contracted sets the chain reference, expanded, is the dense reference within the
    derived bound, and the ranks are those of the specification."""
    rng = np.random.default_rng(0)
    dims, rks = (3, 2, 4, 1, 5), [1, 3, 5, 4, 2, 1]
    cores = rand_cores(rng, dims, rks)
    worst = 0.0
    for ncon in range(1, 5):
        for con in itertools.combinations(range(5), ncon):
            w = {k: rng.standard_normal(dims[k]) for k in con}
            kept, start = R.kept_and_start(5, con)
            y = R.contract_chain(cores, w)
            assert [c.shape[0] for c in y] == [dims[k] for k in kept]
            assert [c.shape[1] for c in y] == [rks[s] for s in start] and y[-1].shape[2] == 1
            assert all(y[m].shape[2] == y[m + 1].shape[1] for m in range(len(y) - 1))
            ref = R.contract_dense(cores, w)
            S = R.contract_dense(*R.abs_inputs(cores, w))
            worst = max(worst, float(np.max(np.abs(R.dense(y) - ref) / S)))
    print("worst err / S = %.2e (bound %.2e)" % (worst, R.bound_factor(cores) * R.EPS))
    assert worst <= R.bound_factor(cores) * R.EPS


def test_reference_known_values():
    """all-ones weights sum an index, a unit vector picks one"""
    rng = np.random.default_rng(1)
    cores = rand_cores(rng, (2, 3, 2), [1, 2, 3, 1])
    full = R.dense(cores)
    assert np.allclose(R.contract_dense(cores, {1: np.ones(3)}), full.sum(axis=1), rtol=0, atol=1e-13)
    assert np.allclose(R.contract_dense(cores, {0: [0.0, 1.0], 2: [1.0, 0.0]}), full[1, :, 0], rtol=0, atol=1e-13)
    kept, start = R.kept_and_start(6, [0, 1, 3])
    assert kept == [2, 4, 5] and start == [0, 3, 5]


def test_kept_sites_and_capacity():
    assert D.contract_kept(6, [1, 2, 4]) == ([2, 4, 5], [0, 3, 5])
    assert D.contract_kept(4, [4]) == ([0, 1, 2], [0, 1, 2])
    assert D.contract_rank_capacity([1, 7, 8, 9, 1], [2]) == [1, 7, 9, 1]          # the bond left of the run in front of kept site 3
    assert D.contract_rank_capacity([1, 7, 8, 9, 1], [1, 4]) == [1, 8, 1]
    assert D.contract_rank_capacity([1, 7, 8, 9, 1], [3, 4]) == [1, 7, 1]


def test_weight_tables():
    sites, wbatch, tab = D._contract_tables("t", (2, 3, 2), 1, {3: [1.0, 2.0], 2: [3.0, 4.0, 5.0]})
    assert sites == [2, 3] and wbatch == 1 and tab.tolist() == [[3.0, 4.0, 5.0, 1.0, 2.0]]
    sites, wbatch, tab = D._contract_tables("t", (2, 3, 2), 2, {1: [[1.0, 2.0], [3.0, 4.0]], 2: [5.0, 6.0, 7.0]})
    assert wbatch == 2 and tab.tolist() == [[1.0, 2.0, 5.0, 6.0, 7.0], [3.0, 4.0, 5.0, 6.0, 7.0]]
    assert tab.flags["C_CONTIGUOUS"] and tab.dtype == np.float64


@pytest.mark.parametrize("weights, what", [
    ({}, "non-empty dict"),
    ([1.0, 2.0], "non-empty dict"),
    ({0: [1.0, 1.0]}, "not in 1:3"),
    ({4: [1.0, 1.0]}, "not in 1:3"),
    ({1.5: [1.0, 1.0]}, "not in 1:3"),
    ({1: [1.0, 1.0], 2: [1.0, 1.0, 1.0], 3: [1.0, 1.0]}, "no kept site"),
    ({2: [1.0, 1.0]}, "shape"),
    ({1: np.ones((3, 2))}, "shape"),
    ({1: [1.0, 1.0j]}, "complex"),
])
def test_argument_checks_without_a_device(weights, what):
    with pytest.raises(T.TTNError, match=what):
        D._contract_tables("contract_sites", (2, 3, 2), 2, weights)


def test_host_entry_refuses_before_any_upload():
    x = T.TTvector(2, [np.ones((2, 1, 1), order="F")] * 2, (2, 2), [1, 1, 1], [0, 0])
    with pytest.raises(T.TTNError, match="no kept site"):
        T.contract_sites(x, {1: [1.0, 1.0], 2: [1.0, 1.0]})
    z = T.TTvector(2, [np.ones((2, 1, 1), order="F") * 1j] * 2, (2, 2), [1, 1, 1], [0, 0])
    with pytest.raises(T.TTNError, match="Float64 only"):
        T.contract_sites(z, {1: [1.0, 1.0]})
    with pytest.raises(TypeError):
        T.contract_sites([1, 2], {1: [1.0, 1.0]})


@pytest.mark.parametrize("ordering", Q.ORDERINGS)
def test_dim_sites_follow_the_bit_rule(ordering):
    """The sites of a dimension, level 0 first, against site_dim_level and grid_strides; reduced metadata for every kept set."""
    n_dims, bits = 3, 4
    strides = Q.grid_strides(n_dims, bits, ordering)
    seen = []
    for dim in range(n_dims):
        sites = Q.dim_sites(dim, n_dims, bits, ordering)
        assert len(sites) == bits and sites == sorted(sites)
        for level, s in enumerate(sites):
            assert Q.site_dim_level(s, n_dims, bits, ordering) == (dim, level)
            assert strides[s] == 2 ** (bits - 1 - level) * (2 ** bits) ** dim
        seen += sites
    assert sorted(seen) == list(range(n_dims * bits))
    for nk in range(1, n_dims + 1):
        for keep in itertools.combinations(range(n_dims), nk):
            assert Q.reduced_meta(n_dims, bits, ordering, keep) == (nk, bits, ordering)
            # the sites that stay, renumbered, are the sites of the reduced layout: dimension keep[j] becomes dimension j, levels stay
            left = sorted(s for dim in keep for s in Q.dim_sites(dim, n_dims, bits, ordering))
            for new, s in enumerate(left):
                dim, level = Q.site_dim_level(s, n_dims, bits, ordering)
                assert Q.site_dim_level(new, nk, bits, ordering) == (keep.index(dim), level)
    assert Q.reduced_meta(n_dims, bits, ordering, 1) == (1, bits, ordering)
    for bad in ((0, 0), (3,), (-1,)):
        with pytest.raises(T.TTNError, match="keep"):
            Q.reduced_meta(n_dims, bits, ordering, bad)


@pytest.mark.parametrize("ordering", Q.ORDERINGS)
def test_site_to_grid_is_the_bit_rule(ordering):
    """the reference's own site -> grid map against an explicit loop over grid_strides"""
    n_dims, bits = 2, 3
    rng = np.random.default_rng(2)
    t = rng.standard_normal((2,) * (n_dims * bits))
    g = R.site_to_grid(t, n_dims, bits, ordering)
    strides = Q.grid_strides(n_dims, bits, ordering)
    flat = np.zeros(2 ** (n_dims * bits))
    for z in np.ndindex(*t.shape):
        flat[sum(zi * st for zi, st in zip(z, strides))] = t[z]
    assert np.array_equal(g, flat.reshape((2 ** bits,) * n_dims, order="F"))


def test_qtt_entry_points_check_their_arguments():
    q = T.QTTvector(T.TTvector(4, [np.ones((2, 1, 1), order="F")] * 4, (2,) * 4, [1] * 5, [0] * 4), 2, 2, "serial")
    with pytest.raises(T.TTNError, match="keep"):
        T.marginal(q, (2,))
    with pytest.raises(T.TTNError, match="dim must be"):
        T.slice_dim(q, 2, 0)
    with pytest.raises(T.TTNError, match="index out of"):
        T.slice_dim(q, 0, 4)
    with pytest.raises(T.TTNError, match="integer"):
        T.slice_dim(q, 0, 1.5)
    with pytest.raises(T.TTNError, match="integer"):
        T.slice_dim(q, 0, [0, 1])                    # one index per train needs a resident batch
    with pytest.raises(TypeError):
        T.marginal(q.ttvector(), (0,))
    q1 = T.QTTvector(T.TTvector(2, [np.ones((2, 1, 1), order="F")] * 2, (2,) * 2, [1] * 3, [0] * 2), 2, 1, "serial")
    with pytest.raises(T.TTNError, match="at least 2"):
        T.moments(q1, 0.0, 1.0)


# ---- header, ctypes table, exports -----------------------------------------------------------------------------------------------------
def test_contract_header_and_ctypes_table_agree():
    import ctypes
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ttn_contract.h")).read(), flags=re.S)
    protos = re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert {n for n, _ in protos} == set(T._lib.CONTRACT_SIGNATURES) == {"ttn_tt_contract_sites"}
    others = set()
    for name in dir(T._lib):
        if name.endswith("SIGNATURES") and name != "CONTRACT_SIGNATURES":
            others |= set(getattr(T._lib, name))
    assert "ttn_tt_kron" in others and not set(T._lib.CONTRACT_SIGNATURES) & others
    lib = T._lib.lib()
    for name, args in protos:
        res, argt = T._lib.CONTRACT_SIGNATURES[name]
        assert res is ctypes.c_int and hasattr(lib, name)
        assert len(args.split(",")) == len(argt) == 6
    assert '#include "ttn_contract.h"' in open(os.path.join(root, "include", "ttn.h")).read()
    api = open(os.path.join(root, "tensortrainnumerics.jl_amd", "csrc", "ttn_api.hip")).read()
    assert '#include "ttn_host_contract.h"' in api and '#include "ttn_contract_kernels.h"' in api


def test_exports():
    for name in ("contract_sites", "marginal", "slice_dim", "moments", "dim_sites", "reduced_meta"):
        assert name in T.__all__ and callable(getattr(T, name))
    assert callable(D.contract_sites) and callable(T.DeviceTT.contract_sites)
