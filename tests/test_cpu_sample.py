"""CPU tests of tt_sample (no GPU): the NumPy restatement of tests/sample_reference.py — the yardstick of tests/test_gpu_sample.py —
draws from the distribution it claims, draws no fragile sample on any case the GPU tests compare exactly, and states the exact cases;
sample_uniforms is pinned to the project's splitmix64 stream; the ctypes table agrees with include/ttn_sample.h; the argument checks
of tt_sample raise before any device call.

Bars: logp against the dense tensor 1e-12 absolute (the restatement and the dense contraction differ by a few roundings per site:
2e-14 was the worst seen); the chi-square bar is the (1 - 1e-6) quantile of chi^2 with 15 degrees of freedom, 56.493 (scipy
chi2.ppf(1 - 1e-6, 15)): a correct sampler fails it once in a million seeds, and the seed is fixed."""
import os
import re

import numpy as np
import pytest

from tests import sample_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CHI2_15_Q = 56.493            # chi2.ppf(1 - 1e-6, df=15)


@pytest.fixture(scope="module")
def T():
    import __graft_entry__ as g
    g.build()
    import ttn_amd
    return ttn_amd


def to_tt(T, cores):
    dims = tuple(c.shape[0] for c in cores)
    rks = [c.shape[1] for c in cores] + [cores[-1].shape[2]]
    return T.TTvector(len(cores), [np.asfortranarray(c) for c in cores], dims, rks, [0] * len(cores))


@pytest.mark.parametrize("born", [True, False], ids=["born", "density"])
@pytest.mark.parametrize("name,S,seed", R.GPU_RUNS, ids=[f"{n}-S{s}" for n, s, _ in R.GPU_RUNS])
def test_reference_draws_no_fragile_sample(name, S, seed, born):
    """The precondition of the 0.1 % cap of the GPU tests: on every run they compare, the reference's own fragile share is 0, nothing
    is clamped and nothing dies."""
    _, trains, _, res = R.run(name, S, seed, born)
    for b, (idx, logp, margin, clamps, dead) in enumerate(res):
        print(f"{name} train {b} {'born' if born else 'density'}: min margin {margin.min():.2e}")
        assert int((margin < R.FRAGILE).sum()) == 0
        assert clamps == 0 and dead == 0
        assert np.all(np.isfinite(logp))
        assert idx.min() >= 1 and np.all(idx <= np.array([c.shape[0] for c in trains[b]]))


@pytest.mark.parametrize("born", [True, False], ids=["born", "density"])
@pytest.mark.parametrize("name,S,seed", [r for r in R.GPU_RUNS if r[0] not in ("d480", "d4_chi2")], ids=lambda v: str(v))
def test_logp_against_dense(name, S, seed, born):
    _, trains, _, res = R.run(name, min(S, 512), seed, born)
    for t, (idx, logp, _, _, _) in zip(trains, res):
        full = R.dense(t)
        prob = full ** 2 / np.sum(full ** 2) if born else full / np.sum(full)
        want = np.log(prob[tuple((idx - 1).T)])
        err = float(np.max(np.abs(logp - want)))
        print(f"{name}: logp against the dense tensor {err:.2e}")
        assert err <= 1e-12
        assert np.max(np.abs(R.target_logp(t, idx, born) - want)) <= 1e-12


def test_chi_square_of_the_reference():
    _, trains, _, res = R.run("d4_chi2", 20000, 19, True)
    full = R.dense(trains[0])
    stat = R.chi2_stat(res[0][0], full ** 2 / np.sum(full ** 2))
    print(f"chi-square of 20000 Born samples, 15 degrees of freedom: {stat:.1f} (bar {CHI2_15_Q})")
    assert stat <= CHI2_15_Q


def test_sample_uniforms_are_the_splitmix64_stream(T):
    from ttn_amd import constructors, cross
    assert cross.DRAW_SAMPLE == R.DRAW_SAMPLE == 6
    seed, B, S, d = 2024, 3, 7, 5
    u = T.sample_uniforms(seed, B, S, d)
    assert u.shape == (B, S, d) and u.dtype == np.float64
    for b in range(B):
        sub = cross._subseed(seed, 6, b, 0)
        assert sub == R.subseed(seed, 6, b, 0)
        words = constructors._splitmix64(S * d, sub)
        want = ((words >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(S, d)
        assert np.array_equal(u[b], want)
        assert np.array_equal(u[b], R.uniforms(seed, b, S, d))
        for s, k in ((0, 0), (3, 2), (S - 1, d - 1)):                       # word j = 1 + k + d s, in Python integers
            assert u[b, s, k] == (R.splitmix64_word(sub, 1 + k + d * s) >> 11) * 2.0 ** -53
    assert np.all(u >= 0.0) and np.all(u < 1.0)
    assert np.array_equal(T.sample_uniforms(seed, B, 4, d), u[:, :4])       # the first S samples do not depend on S
    assert np.array_equal(T.sample_uniforms(-1, 1, 2, 2), T.sample_uniforms((1 << 64) - 1, 1, 2, 2))
    with pytest.raises(T.TTNError, match="at least 1"):
        T.sample_uniforms(0, 1, 0, 3)


def test_clamp_case_of_the_reference():
    _, cores = R.clamp_train()
    S = 50
    idx, logp, _, clamps, dead = R.sample(cores, R.uniforms(5, 0, S, 3), False)
    assert np.all(idx[:, 0] == 1) and clamps == S and dead == 0
    # the clamped target: site 1 certain, the other two sites their own normalised values
    want = np.log(np.array([1.0, 3.0]) / 4.0)[idx[:, 1] - 1] + np.log(np.array([0.5, 0.25]) / 0.75)[idx[:, 2] - 1]
    assert np.max(np.abs(logp - want)) <= 1e-14


def test_zero_train_of_the_reference():
    _, cores = R.zero_train()
    for born in (True, False):
        idx, logp, _, clamps, dead = R.sample(cores, R.uniforms(6, 0, 9, 3), born)
        assert dead == 9 and clamps == 0 and np.all(idx == 1) and np.all(np.isneginf(logp))


def test_ctypes_table_matches_the_header(T):
    text = open(os.path.join(INCLUDE, "ttn_sample.h")).read()
    declared = set(re.findall(r"^int (ttn_\w+)\(", text, flags=re.M))
    assert declared == set(T._lib.SAMPLE_SIGNATURES) == {"ttn_tt_sample", "ttn_tt_sample_dev", "ttn_tt_sample_last_ms"}
    from ttn_amd import device as D
    assert D.SAMPLE_MODES == {"born": 0, "density": 1}
    assert '#include "ttn_sample.h"' in open(os.path.join(INCLUDE, "ttn.h")).read()


def test_refusals_before_the_device(T):
    """Raised by the argument checks: with no GPU here, a call that reached the upload would fail with another message."""
    x = to_tt(T, R.case("d2")[1][0])
    with pytest.raises(T.TTNError, match="mode must be"):
        T.tt_sample(x, 4, mode="fermi")
    with pytest.raises(T.TTNError, match="nsamples must be"):
        T.tt_sample(x, 0)
    with pytest.raises(T.TTNError, match="nsamples must be"):
        T.tt_sample(x, 2.5)
    with pytest.raises(T.TTNError, match="u has shape"):
        T.tt_sample(x, 4, u=np.zeros((4, 3)))
    with pytest.raises(T.TTNError, match=r"\[0, 1\)"):
        T.tt_sample(x, 4, u=np.ones((4, 2)))
    with pytest.raises(T.TTNError, match="seed must be"):
        T.tt_sample(x, 4, seed="a")
    z = to_tt(T, [c.astype(np.complex128) for c in R.case("d2")[1][0]])
    with pytest.raises(T.TTNError, match="Float64 only"):
        T.tt_sample(z, 4)
    with pytest.raises(TypeError, match="TTvector"):
        T.tt_sample([1, 2], 4)
    with pytest.raises(TypeError, match="QTTvector"):
        T.qttv_sample(x, 4)
