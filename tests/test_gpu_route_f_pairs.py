"""Route F of the bond step with its Gram products paired (wg_syrk2), against the oracle at the parity bar of test_gpu_parity.py.

The interior right-to-left steps of a rank-64 sweep take route F with a diagonal left Gram matrix: A'^T A' with B' B'^T, and the two
a-posteriori check products, each pair in one two-team call.  d = 14 is the shortest train with interior right-to-left steps of
r_mid = 64; batches of 2 and 3 trains, fused apply_compress and apply followed by a plain compress, in the 1024-thread build and in
the 512-thread build (TTN_WG512=1).  A d = 10, rank 16 train takes the non-diagonal path of the same route (Cholesky factors), whose
Gram pairs go through the same call.  Ranks exact, tensors to 1e-9 relative, compress_status clean."""
import numpy as np
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


def _reference(T, d, r, seed):
    """the train of this seed and the oracle's Delta(d) x, rounded to rank r (computed once per module)"""
    if (d, r, seed) not in _REF:
        x = T.rand_tt((2,) * d, r, seed=seed)
        _REF[(d, r, seed)] = (x, O.tt_compress_(O.apply(O.Delta(d), to_oracle(x)), r))
    return _REF[(d, r, seed)]


def _run(T, d, r, seeds, fused):
    A = T.Delta(d)
    xs = [_reference(T, d, r, s)[0] for s in seeds]
    dA = T.DeviceTTO(A)
    dx = T.DeviceTT((2,) * d, xs[0].ttv_rks, batch=len(seeds))
    for b, x in enumerate(xs):
        dx.upload(b, x)
    dy = T.DeviceTT((2,) * d, [a * c for a, c in zip(A.tto_rks, xs[0].ttv_rks)], batch=len(seeds))
    if fused:
        T.device.apply_compress(dA, dx, dy, r, 0.0, 1)
    else:
        T.device.apply(dA, dx, dy)
        T.device.tt_compress_(dy, r)
    T.device.compress_status(dy)
    for b, s in enumerate(seeds):
        ref = _reference(T, d, r, s)[1]
        got = dy.download(b)
        assert got.ttv_rks == ref.ttv_rks, f"seed {s}"
        err = tt_rel_diff(to_oracle(got), ref)
        print(f"d={d} r={r} seed={s} fused={fused}: rel diff {err:.2e}")
        assert err <= 1e-9, f"seed {s}: {err:.2e}"


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("wg512", [0, 1])
def test_rank64_interior_steps_vs_oracle(T, monkeypatch, wg512, B, fused):
    monkeypatch.setenv("TTN_WG512", str(wg512))
    _run(T, 14, 64, [140 + b for b in range(B)], fused)


@pytest.mark.parametrize("wg512", [0, 1])
def test_rank16_non_diagonal_path_vs_oracle(T, monkeypatch, wg512):
    monkeypatch.setenv("TTN_WG512", str(wg512))
    _run(T, 10, 16, [7], True)
    _run(T, 10, 16, [7], False)
