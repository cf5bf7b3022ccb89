"""Diagnostic of the operator batches, written to profiles/diag_opbatch.json: what one operator per train costs.

At config C3 (d = 30, rank-64 QTT trains, Delta(30), batch 1024) the time of
  (a) device.apply with the one shared operator,
  (b) device.apply with `batch` distinct operators c_b * Delta(d) in one handle (DeviceTTO.stack),
  (c) device.sandwich the same two ways,
each between a HIP-event pair on the library stream, after one warm-up of each, the forms alternating, the median of --reps runs with
the minimum and the maximum.  On a tree without operator batches (the parent of the change that added them) only the shared forms
run, so that (a) can be compared across the two trees: the kernels gained one multiply-add per block where they form the operator
pointer, and the shared form must not have moved by more than its own spread."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                    # noqa: E402

import ttn_amd as T                                   # noqa: E402
from ttn_amd import device as D                       # noqa: E402


def timed(fn, slot):
    D.event_record(slot)
    v = fn()
    D.event_record(slot + 1)
    return D.event_elapsed_ms(slot, slot + 1), v


def summary(ts):
    return {"ms": ts, "median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def scaled(A, c):
    """c * A on the host, the factor in the first core (src/tt_operations.jl:271-281 for an operator without gauge flags)."""
    cores = [np.asfortranarray(np.array(k)) for k in A.tto_vec]
    cores[0] = np.asfortranarray(c * cores[0])
    return T.TToperator(A.N, cores, A.tto_dims, list(A.tto_rks), list(A.tto_ot))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=30)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_opbatch.json"))
    a = ap.parse_args()
    assert a.reps >= 7, "the median of at least 7 runs"
    T.ensure_init(0)
    have = hasattr(T.DeviceTTO, "stack")
    d, B = a.d, a.batch
    A = T.Delta(d)
    x = T.rand_tt((2,) * d, a.rank, seed=30)
    dx = T.DeviceTT.from_host(x, batch=B)
    dy = T.DeviceTT((2,) * d, [p * q for p, q in zip(A.tto_rks, x.ttv_rks)], batch=B)
    shared = T.DeviceTTO(A)
    forms = {"apply_shared": lambda: D.apply(shared, dx, dy), "sandwich_shared": lambda: D.sandwich(dx, shared, dx)}
    rec = {"tool": "tools/diag_opbatch.py", "operator_batches": have, "d": d, "rank": a.rank, "batch": B, "reps": a.reps, "operator": "Delta"}
    if have:
        cs = 1.0 + np.arange(B) / B                      # distinct factors in [1, 2)
        stacked = T.DeviceTTO.stack([scaled(A, float(c)) for c in cs])
        forms["apply_batch"] = lambda: D.apply(stacked, dx, dy)
        forms["sandwich_batch"] = lambda: D.sandwich(dx, stacked, dx)
    order = [n for n in ("apply_shared", "apply_batch", "sandwich_shared", "sandwich_batch") if n in forms]
    first = {}
    for n in order:                                       # the warm-up of each
        first[n] = forms[n]()
        D.sync()
    times = {n: [] for n in order}
    for _ in range(a.reps):
        for i, n in enumerate(order):
            ms, _v = timed(forms[n], 2 * i)
            times[n].append(ms)
    for n in order:
        rec[n] = summary(times[n])
    if have:
        # the same again with the batch form BEFORE the shared one of each pair: what a form inherits from its predecessor (the state of
        # the caches and of the memory channels) then changes sides, what belongs to the form stays
        swapped = ["apply_batch", "apply_shared", "sandwich_batch", "sandwich_shared"]
        times = {n: [] for n in swapped}
        for _ in range(a.reps):
            for i, n in enumerate(swapped):
                ms, _v = timed(forms[n], 2 * i)
                times[n].append(ms)
        for n in swapped:
            rec[n + "_swapped_order"] = summary(times[n])
    if have:
        # operator b is c_b * Delta: its expectation value is c_b times the shared one, to rounding
        s, b = first["sandwich_shared"], first["sandwich_batch"]
        rec["sandwich_batch_over_shared_minus_c_max"] = float(np.max(np.abs(b / s - cs)))
        sa, sb = rec["apply_shared"], rec["apply_batch"]
        rec["apply_batch_median_within_shared_min_max"] = bool(sa["min"] <= sb["median"] <= sa["max"])
        sa, sb = rec["sandwich_shared"], rec["sandwich_batch"]
        rec["sandwich_batch_median_within_shared_min_max"] = bool(sa["min"] <= sb["median"] <= sa["max"])
        stacked.free()
    print(json.dumps(rec), flush=True)
    D.status_all()
    for h in (shared, dx, dy):
        h.free()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
