"""The one-pass fused merge of ttn_apply_compress (csrc/ttn_dense_kernels.h, wg_fused_merge_direct) runs tile loops specialised on the
operator rank Rl = 1, 2, 3 on the left of the site it merges.  Every specialisation, under both builds of k_compress (1024 threads:
TTN_WG512=0, 512 threads: TTN_WG512=1), against
  * the unfused route on the device, compress(apply(A, x)): ranks exact, tensors to 1e-12 relative (same bond steps on a merged
    matrix that differs only by the rounding of another summation order);
  * the oracle, at the project's parity bar: ranks exact, tensors to 1e-9.
Shapes: the smallest that reach the direct form with one and with two row blocks per wave column — d = 12, rank 32 (merged matrices of
p = 64 rows: two wave columns in the 512-thread build) and d = 14, rank 64 (p = 128) — in a batch of 3 trains with different seeds.
Operators: TT rank 1; TT rank 2 (an unrounded sum of two rank-1 operators); the Laplacian (rank 3, its boundary cores have Rl = 1 and
Rr = 1); the Heisenberg XYZ chain (rank 5), which the direct form must refuse (Rl > 3) and the general path must get right."""
import numpy as np
import pytest

from oracle import tt_oracle as O
from tests.helpers import to_oracle, to_product, tt_rel_diff

pytestmark = pytest.mark.gpu

SHAPES = {"d12r32": (12, 32), "d14r64": (14, 64)}
BATCH = 3
_refs = {}


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _operator(T, kind, d):
    rng = np.random.default_rng(1234 + d)
    dims = (2,) * d
    if kind == "rank1":
        return O.rand_tto(dims, 1, rng)
    if kind == "rank2":
        return O.tto_add(O.rand_tto(dims, 1, rng), O.rand_tto(dims, 1, rng))
    if kind == "delta":
        return O.Delta(d)
    return to_oracle(T.heisenberg_xyz_tto(d, 1.0, 0.8, 0.6, 0.3, "x"))


def _case(T, shape, kind):
    """Operator, the batch's trains and the oracle's results: computed once per (shape, operator), shared by both builds."""
    key = (shape, kind)
    if key not in _refs:
        d, r = SHAPES[shape]
        A = _operator(T, kind, d)
        xs = [T.rand_tt((2,) * d, r, seed=500 + 17 * b + d) for b in range(BATCH)]
        refs = [O.tt_compress_(O.apply(A, to_oracle(x)), r) for x in xs]
        _refs[key] = (A, xs, refs)
    return _refs[key]


@pytest.mark.parametrize("wg512", [0, 1])
@pytest.mark.parametrize("kind", ["rank1", "rank2", "delta", "heisenberg"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_merge_operator_ranks(T, monkeypatch, shape, kind, wg512):
    d, r = SHAPES[shape]
    A, xs, refs = _case(T, shape, kind)
    assert max(A.tto_rks) == {"rank1": 1, "rank2": 2, "delta": 3, "heisenberg": 5}[kind]
    monkeypatch.setenv("TTN_WG512", str(wg512))
    dims = (2,) * d
    dA = T.DeviceTTO(to_product(A))
    dx = T.DeviceTT(dims, xs[0].ttv_rks, batch=BATCH)
    for b, x in enumerate(xs):
        dx.upload(b, x)
    cap = [a * c for a, c in zip(A.tto_rks, xs[0].ttv_rks)]
    need, _ = T.device.compress_rank_bound(dims, cap, r)
    cap = [max(a, b) for a, b in zip(cap, need)]
    fused, unfused = T.DeviceTT(dims, cap, batch=BATCH), T.DeviceTT(dims, cap, batch=BATCH)
    T.device.apply_compress(dA, dx, fused, r)
    T.device.compress_status(fused)
    T.device.apply(dA, dx, unfused)
    T.device.tt_compress_(unfused, r)
    T.device.compress_status(unfused)
    for b in range(BATCH):
        f, u = fused.download(b), unfused.download(b)
        e_dev = tt_rel_diff(to_oracle(f), to_oracle(u))
        e_ref = tt_rel_diff(to_oracle(f), refs[b])
        print(f"{shape} {kind} wg512={wg512} train {b}: fused vs unfused {e_dev:.3e}, fused vs oracle {e_ref:.3e}")
        assert list(f.ttv_rks) == list(u.ttv_rks)
        assert e_dev <= 1e-12
        assert list(f.ttv_rks) == list(refs[b].ttv_rks)
        assert e_ref <= 1e-9
