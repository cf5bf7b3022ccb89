"""The host API's library-level state: the StreamTimer and ttn_last_launch_ms keep separate events, and everything the library
keeps on the device between calls is released by finalize and rebuilt by the next init."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def test_stream_timer_spans_a_dot_inside_it(T):
    """A StreamTimer region that ends with a dot measures from its own start, not from the dot's kernel: the region holds two event
    slots around a batched apply + compress, so by stream order its time is at least theirs."""
    D = T.device
    d, r, B = 24, 16, 64
    dA = T.DeviceTTO(T.Delta(d))
    dx = T.DeviceTT.from_host(T.rand_tt((2,) * d, r, seed=11), batch=B)
    cap = D.compress_rank_bound((2,) * d, [a * b for a, b in zip(dA.rks, dx.cap)], r)[0]
    dy = T.DeviceTT((2,) * d, cap, batch=B)
    with T.StreamTimer() as t:
        D.event_record(0)
        D.apply_compress(dA, dx, dy, r)
        D.event_record(1)
        D.dot(dy, dy)
    inner = D.event_elapsed_ms(0, 1)
    assert inner > 0.0
    assert t.ms >= inner, (t.ms, inner)
    assert D.last_launch_ms() > 0.0          # the dot kernel alone, still available after the region
    D.compress_status(dy)


_CHILD = r"""
import gc, hashlib, json, os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
import ttn_amd as T
from oracle import tt_oracle as O
from tests.helpers import to_oracle, to_product

D = T.device


def digest(h, t):
    for c in t.ttv_vec:
        h.update(np.ascontiguousarray(c).tobytes())
    h.update(np.asarray(list(t.ttv_rks) + list(t.ttv_ot), dtype=np.int64).tobytes())


def one_round():
    h = hashlib.sha256()
    d = 8
    rng = np.random.default_rng(4)
    spd = O.tto_add(O.Delta(d), O.tto_scale(1.5, O.id_tto(d)))
    dA = T.DeviceTTO(to_product(spd))
    # scale_batch on trains whose gauge flags differ: a per-train table of scaled cores
    xs = [to_product(O.rand_tt((2,) * d, 3, rng)) for _ in range(3)]
    xs[1].ttv_ot = [-1, -1, 0] + [1] * (d - 3)
    xs[2].ttv_ot = [-1] * (d - 1) + [0]
    dx = T.DeviceTT((2,) * d, xs[0].ttv_rks, batch=3)
    for b in range(3):
        dx.upload(b, xs[b])
    dy = T.DeviceTT((2,) * d, xs[0].ttv_rks, batch=3)
    D.scale_batch([0.5, -2.0, 3.0], dx, dy)
    for b in range(3):
        digest(h, dy.download(b))
    # dmrg_linsolve with the matrix-free local solver (CG iteration counts kept on the device)
    b0, x0 = O.rand_tt((2,) * d, 2, rng), O.rand_tt((2,) * d, 2, rng)
    db, dx0 = T.DeviceTT.from_host(to_product(b0), batch=2), T.DeviceTT.from_host(to_product(x0), batch=2)
    dsol = T.DeviceTT((2,) * d, T.solvers.mals_capacity((2,) * d, x0.ttv_rks, 6), batch=2)
    T.solvers.dmrg_linsolve_(dA, db, dx0, dsol, 1e-9, [2, 3], [4, 6], it_solver=True)
    D.compress_status(dsol)
    digest(h, dsol.download(1))
    # dmrg_eigsolve (energy / rank history and Lanczos statistics kept on the device)
    ising = T.DeviceTTO(to_product(to_oracle(T.ising_tto(d, J=1.0, h=1.5))))
    e0 = T.DeviceTT.from_host(to_product(O.rand_tt((2,) * d, 4, rng)), batch=2)
    ev = T.DeviceTT((2,) * d, T.solvers.dmrg_capacity((2,) * d, e0.cap, 8), batch=2)
    E, rh = T.solvers.dmrg_eigsolve_(ising, e0, ev, 1e-12, [3], [8])
    h.update(np.asarray(E, dtype=np.float64).tobytes())
    h.update(np.asarray(rh, dtype=np.int64).tobytes())
    digest(h, ev.download(0))
    # als_linsolve through the grid form (k_lu_panel / k_lu_trail, the singular-pivot word)
    os.environ["TTN_ALS_GRID"] = "1"
    dals = T.DeviceTT((2,) * d, x0.ttv_rks, batch=2)
    T.solvers.als_linsolve_(dA, db, dx0, dals, 2)
    del os.environ["TTN_ALS_GRID"]
    D.compress_status(dals)
    digest(h, dals.download(0))
    # hadamard_ttm (the site-swap chain and its upload table)
    hx, hy = O.rand_tt((2,) * d, 3, rng), O.rand_tt((2,) * d, 2, rng)
    dz = T.DeviceTT((2,) * d, [1] + [16] * (d - 1) + [1])
    T.qtt.hadamard_ttm_(T.DeviceTT.from_host(to_product(hx)), T.DeviceTT.from_host(to_product(hy)), dz, tol=1e-10, work_cap=16)
    D.compress_status(dz)
    digest(h, dz.download(0))
    # site_expect and sample on one rank-3 batch of 2 (the measurement table and its event; the sample outputs and events)
    ms = [to_product(O.rand_tt((2,) * d, 3, rng)) for _ in range(2)]
    dm = T.DeviceTT((2,) * d, ms[0].ttv_rks, batch=2)
    for b in range(2):
        dm.upload(b, ms[b])
    h.update(np.ascontiguousarray(D.site_expect(dm, np.diag([1.0, -1.0]))).tobytes())
    idx, logp, _ = D.sample(dm, 64, "born", seed=7)
    h.update(np.ascontiguousarray(idx).tobytes())
    h.update(np.ascontiguousarray(logp).tobytes())
    # dot_pullback with one factor per train (the coefficient table)
    gs = [to_product(O.rand_tt((2,) * d, 3, rng)) for _ in range(2)]
    dg = T.DeviceTT((2,) * d, gs[0].ttv_rks, batch=2)
    for b in range(2):
        dg.upload(b, gs[b])
    _, abar, bbar = T.grad.dot_pullback(dm, dg, delta=[0.5, -2.0])
    for b in range(2):
        digest(h, abar.download(b))
        digest(h, bbar.download(b))
    # dmrg_eigsolve penalised against the states found above (weights, norms and overlaps kept on the device)
    e1 = T.DeviceTT.from_host(to_product(O.rand_tt((2,) * d, 4, rng)), batch=2)
    ev1 = T.DeviceTT((2,) * d, T.solvers.dmrg_capacity((2,) * d, e1.cap, 8), batch=2)
    E1, rh1, ovl = T.solvers.dmrg_eigsolve_(ising, e1, ev1, 1e-12, [3], [8], ortho_to=[ev], weight=10.0)
    h.update(np.asarray(E1, dtype=np.float64).tobytes())
    h.update(np.asarray(rh1, dtype=np.int64).tobytes())
    h.update(np.asarray(ovl, dtype=np.float64).tobytes())
    digest(h, ev1.download(0))
    D.status_all()
    return h.hexdigest()


first = one_round()
gc.collect()
T.finalize()
second = one_round()
print(json.dumps({"first": first, "second": second}))
"""


def test_finalize_then_init_repeats_bitwise():
    """In a fresh process: every path that keeps device memory between calls, run, then finalize + init, then run again.  The
    second results are bitwise the first (nothing points into a torn-down context)."""
    p = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["first"] == out["second"], out
