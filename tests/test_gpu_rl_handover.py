"""The hand-over of the left factor between consecutive right-to-left route-F steps of k_compress.

With rand_tt((2,)*d, 64) and Delta(d) the right-to-left route-F steps with r_mid = 64 are the (0-based) bonds 6 ... d-8: d = 14 has one
(no hand-over), d = 15 two (the first and the last of a chain), d = 16 three (a middle step that is handed over to and hands over).
The step after the chain is the 64-row ramp step, which does not read from the staging area and has to put the core back first.

Every case: ranks exact, tensors to 1e-9 relative against the oracle (as tests/test_gpu_route_f_pairs.py), compress_status clean.
The plain chains also compare the Jacobi sweep totals compress_status returns with those of the parent commit (the build without the
hand-over) on the same seeds: a hand-over that quietly dropped to the Householder route would pass the tensor bound but not that."""
import pytest

from oracle import tt_oracle as O
from tests.helpers import to_oracle, tt_rel_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


_REF = {}


def _seed(d, b):
    return 10 * d + b


def _reference(T, d, seed, max_bond=64):
    """the rank-64 train of this seed and the oracle's Delta(d) x, rounded to max_bond (computed once per module)"""
    if (d, seed) not in _REF:
        _REF[(d, seed)] = (T.rand_tt((2,) * d, 64, seed=seed), {})
    x, rounded = _REF[(d, seed)]
    if max_bond not in rounded:
        rounded[max_bond] = O.tt_compress_(O.apply(O.Delta(d), to_oracle(x)), max_bond)      # (tt_compress_ works in place)
    return x, rounded[max_bond]


def _product(T, d, seeds):
    """dA, dx and an empty dy for A x of these seeds' trains"""
    A = T.Delta(d)
    xs = [_reference(T, d, s)[0] for s in seeds]
    dA = T.DeviceTTO(A)
    dx = T.DeviceTT((2,) * d, xs[0].ttv_rks, batch=len(seeds))
    for b, x in enumerate(xs):
        dx.upload(b, x)
    dy = T.DeviceTT((2,) * d, [a * c for a, c in zip(A.tto_rks, xs[0].ttv_rks)], batch=len(seeds))
    return dA, dx, dy


def _check(T, dy, d, seeds, which=None, max_bond=64, tag=""):
    for b in (range(len(seeds)) if which is None else which):
        ref = _reference(T, d, seeds[b], max_bond)[1]
        got = dy.download(b)
        assert got.ttv_rks == ref.ttv_rks, f"train {b} seed {seeds[b]}"
        err = tt_rel_diff(to_oracle(got), ref)
        print(f"d={d} train={b} seed={seeds[b]} {tag}: rel diff {err:.2e}")
        assert err <= 1e-9, f"train {b} seed {seeds[b]}: {err:.2e}"


def _run(T, d, seeds, fused, max_bond=64, which=None, tag=""):
    dA, dx, dy = _product(T, d, seeds)
    if fused:
        T.device.apply_compress(dA, dx, dy, max_bond, 0.0, 1)
    else:
        T.device.apply(dA, dx, dy)
        T.device.tt_compress_(dy, max_bond)
    sweeps = T.device.compress_status(dy)
    _check(T, dy, d, seeds, which, max_bond, tag)
    return sweeps


# Jacobi sweep totals per train (compress_status) of the PARENT commit, measured once on an MI355X with the seeds _seed(d, b):
# {(d, wg512, fused): [train 0, train 1, train 2]}.  The interior route-F steps go through the eigensolver and add nothing; the totals
# are those of the ramp steps, so a chain step that fell back to the merge routes shows up as a larger total.
PARENT_SWEEPS = {
    (15, 0, True): [141, 149, 144], (15, 0, False): [141, 149, 144], (15, 1, True): [141, 144, 145], (15, 1, False): [141, 144, 145],
    (16, 0, True): [146, 143, 145], (16, 0, False): [146, 143, 145], (16, 1, True): [143, 145, 147], (16, 1, False): [143, 145, 147],
}


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("wg512", [0, 1])
@pytest.mark.parametrize("d", [15, 16])
def test_plain_chains_vs_oracle_and_parent_sweep_totals(T, monkeypatch, d, wg512, B, fused):
    """the chain, its start from a core and its end at the ramp step that must put the core back; no silent fallback"""
    monkeypatch.setenv("TTN_WG512", str(wg512))
    sweeps = _run(T, d, [_seed(d, b) for b in range(B)], fused, tag=f"wg512={wg512} fused={fused}")
    print(f"sweep totals d={d} wg512={wg512} fused={fused}: {sweeps}")
    assert sweeps == PARENT_SWEEPS[(d, wg512, fused)][:B], (sweeps, PARENT_SWEEPS[(d, wg512, fused)][:B])


@pytest.mark.parametrize("wg512", [0, 1])
def test_chain_cut_by_the_launch(T, monkeypatch, wg512):
    """d = 16: apply, the left-to-right half, then the right-to-left half as two ttn_sweep launches, the first ending in the middle of
    the chain (1-based bond 8 = 0-based 7 of 6, 7, 8): the last step of a launch must not leave its left factor in the staging area"""
    monkeypatch.setenv("TTN_WG512", str(wg512))
    d, seeds = 16, [_seed(16, 0), _seed(16, 1)]
    L = T._lib
    dA, dx, dy = _product(T, d, seeds)
    T.device.apply(dA, dx, dy)
    L.check(L.lib().ttn_sweep(dy.h, 1, d - 1, 64, 0.0))
    L.check(L.lib().ttn_sweep(dy.h, d - 1, 8, 64, 0.0))
    L.check(L.lib().ttn_sweep(dy.h, 7, 1, 64, 0.0))
    T.device.compress_status(dy)
    dA1, dx1, dy1 = _product(T, d, seeds)
    T.device.apply(dA1, dx1, dy1)
    T.device.tt_compress_(dy1, 64)
    T.device.compress_status(dy1)
    for b in range(len(seeds)):
        got, one = dy.download(b), dy1.download(b)
        assert got.ttv_rks == one.ttv_rks, f"train {b}"
        err = tt_rel_diff(to_oracle(got), to_oracle(one))
        print(f"cut chain wg512={wg512} train={b}: rel diff to the one-call compress {err:.2e}")
        assert err <= 1e-9, f"train {b}: {err:.2e}"
    _check(T, dy, d, seeds, tag=f"cut chain wg512={wg512}")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("wg512", [0, 1])
def test_restore_path_after_rf_went_into_the_dead_core(T, monkeypatch, wg512, fused):
    """TTN_FAST = 33: every step that received a handed-over B' treats its a-posteriori check as failed — Rf is in core k+1 already,
    the core is put back over it and the fallback routes deliver the result"""
    monkeypatch.setenv("TTN_WG512", str(wg512))
    monkeypatch.setenv("TTN_FAST", "33")
    _run(T, 16, [_seed(16, 0), _seed(16, 1)], fused, tag=f"TTN_FAST=33 wg512={wg512} fused={fused}")


@pytest.mark.parametrize("fast", [5, 9])
@pytest.mark.parametrize("wg512", [0, 1])
def test_handed_over_step_without_eigensolver_or_diagonal_shortcut(T, monkeypatch, wg512, fast):
    """TTN_FAST = 5 / 9: no eigensolver in route F / no diagonal shortcut — the handed-over B' goes through the other products of
    route F (or out of it before any product)"""
    monkeypatch.setenv("TTN_WG512", str(wg512))
    monkeypatch.setenv("TTN_FAST", str(fast))
    _run(T, 16, [_seed(16, 0), _seed(16, 1)], False, tag=f"TTN_FAST={fast} wg512={wg512}")


@pytest.mark.parametrize("wg512", [0, 1])
def test_max_bond_48_chains(T, monkeypatch, wg512):
    """max_bond = 48: r_mid = 48, the Cholesky path of route F and chains with rk = r < 64"""
    monkeypatch.setenv("TTN_WG512", str(wg512))
    _run(T, 16, [_seed(16, 0), _seed(16, 1)], False, max_bond=48, tag=f"max_bond=48 wg512={wg512}")
    _run(T, 16, [_seed(16, 0), _seed(16, 1)], True, max_bond=48, tag=f"max_bond=48 fused wg512={wg512}")


def test_slot_reuse_clears_the_note(T, monkeypatch):
    """B = 514 in the 512-thread build: 512 slots, two of them take a second train; the trains cycle through four seeds"""
    monkeypatch.setenv("TTN_WG512", "1")
    d = 15
    seeds = [_seed(d, b % 4) for b in range(514)]
    _run(T, d, seeds, True, which=[0, 1, 512, 513], tag="B=514")
