"""Diagnostic (not a test): tt_cross_batch against `batch` sequential tt_cross calls in the same process.  Two cases, the d = 30 QTT
sine family sin(lambda_b x) (rank 2, no kick) and the 5-D random tensors whose site-2 fibres take the workspace route (rmax 60, 24
points per axis, two sweeps), at batch 1, 16 and 256 (the 5-D case stops at the largest batch given by --max5d, default 256: its
tables are 64 MB each, drawn on the device).  Each side runs once to warm up and is then timed with a HIP event pair around the
whole call; the batched run is repeated with event pairs around the parts of every half sweep (gathers, f, site, evaluation with the
sweep's host read, and "end": the bookkeeping up to the next sweep).  f is a torch function on the device on both sides.  Prints one JSON object and writes it to profiles/diag_cross_batch.json (or the path given).
    python tools/diag_cross_batch.py [--max5d B] [out.json]"""
import json
import math
import sys

import numpy as np

sys.path.insert(0, ".")
import ttn_amd as T

args = sys.argv[1:]
max5d = 256
if "--max5d" in args:
    i = args.index("--max5d")
    max5d = int(args[i + 1])
    del args[i:i + 2]
out = args[0] if args else "profiles/diag_cross_batch.json"
torch, stream = T.tdvp._dev()
W30 = torch.tensor([2.0 ** (30 - k) / (2 ** 30 - 1) for k in range(1, 31)], dtype=torch.float64, device="cuda")


def timed(run):
    run()                                            # warm-up
    with torch.cuda.stream(stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = run()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def qtt_case(batch):
    lam = torch.tensor([math.pi ** 2 * (1.0 + 0.37 * b / max(batch, 1)) for b in range(batch)], dtype=torch.float64, device="cuda")
    dom = [np.array([0.0, 1.0])] * 30
    alg = T.MaxVol(verbose=False, tol=1e-10, maxiter=3, kickrank=None)
    fb = lambda X, which: torch.sin(lam[which][:, None] * (X @ W30))                       # noqa: E731
    one = lambda b: T.tt_cross(lambda X: torch.sin(lam[b] * (X @ W30)), dom, alg, ranks=2)  # noqa: E731
    return (lambda: T.tt_cross_batch(fb, dom, batch, alg, ranks=2)), (lambda: [one(b) for b in range(batch)])


def rand5_case(batch):
    g = torch.Generator(device="cuda")
    g.manual_seed(55)
    tabs = (torch.rand((batch * 24 ** 5,), dtype=torch.float64, device="cuda", generator=g) * 2.0 - 1.0)
    dom = [np.linspace(0, 1, 24)] * 5
    alg = T.MaxVol(verbose=False, tol=1e-10, maxiter=2, rmax=60, kickrank=None)
    kw = dict(ranks=[24, 60, 24, 6], seed=2)
    strides = torch.tensor([24 ** 4, 24 ** 3, 24 ** 2, 24, 1], dtype=torch.int64, device="cuda")

    def lin(X):
        return (torch.round(X * 23.0).to(torch.int64) * strides).sum(dim=-1)

    fb = lambda X, which: tabs[which[:, None] * 24 ** 5 + lin(X)]                          # noqa: E731
    one = lambda b: T.tt_cross(lambda X: tabs[b * 24 ** 5 + lin(X)], dom, alg, **kw)       # noqa: E731
    return (lambda: T.tt_cross_batch(fb, dom, batch, alg, **kw)), (lambda: [one(b) for b in range(batch)])


res = {"note": "ms per call, HIP events on the library stream after one warm-up; ratio = sequential / batched; split: the batched run's "
               "event pairs summed over all half sweeps (f includes the caller's function only)"}
for name, make, batches in [("qtt-sin-d30", qtt_case, [1, 16, 256]), ("global-route-5d", rand5_case, [b for b in [1, 16, 256] if b <= max5d])]:
    for batch in batches:
        run_b, run_s = make(batch)
        tb, tts = timed(run_b)
        ts, ref = timed(run_s)
        T.cross._Timer.on = True
        run_b()
        T.cross._Timer.on = False
        last = T.cross._LAST_BATCH
        same = all(a.ttv_rks == b.ttv_rks for a, b in zip(tts, ref))
        res[f"{name}-b{batch}"] = {"batched_ms": round(tb, 3), "sequential_ms": round(ts, 3), "ratio": round(ts / tb, 3), "sweeps": max(last["sweeps"]),
                                  "same_ranks": same, "split_ms": {k: round(v, 3) for k, v in sorted(last["split"].items())}}
        print(f"{name}-b{batch}", json.dumps(res[f"{name}-b{batch}"]), flush=True)
s = json.dumps(res)
print(s)
with open(out, "w") as fh:
    fh.write(s + "\n")
