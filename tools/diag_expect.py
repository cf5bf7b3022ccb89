"""Diagnostic of <x, A x> on resident batches, written to profiles/diag_expect.json.

For A = Delta(d) (R = 3) and A = heisenberg_xyz_tto(d) (R = 5) on rank-r QTT trains, at each batch size: the time of device.expect next to
the composition it replaces on the same handles — device.apply into a preallocated handle followed by device.dot.  HIP-event pairs on
the library stream around each (both end with their result on the host), one warm-up of each first, the two alternating, the median of
--reps runs and the spread (max - min) of each.  The kernel of expect alone (ttn_last_launch_ms) gives its share of the fp64 matrix
peak on its own flop count: per site 2 (r_x R) r_y (n r_y') + 2 (r_x r_y') (n R) (n R') + 2 r_x' (n r_x) (R' r_y')."""
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

PEAK_F64 = 78.6e12


def sandwich_flops(n, rx, R, ry):
    """Right to left: the incoming state carries the right ranks (index k + 1), the outgoing one the left ranks (index k)."""
    f = 0
    for k in range(len(rx) - 1):
        f += 2 * rx[k + 1] * R[k + 1] * ry[k + 1] * n * ry[k]
        f += 2 * rx[k + 1] * ry[k] * (n * R[k + 1]) * (n * R[k])
        f += 2 * rx[k] * n * rx[k + 1] * R[k] * ry[k]
    return f


def timed(fn, slot):
    D.event_record(slot)
    v = fn()
    D.event_record(slot + 1)
    return D.event_elapsed_ms(slot, slot + 1), v


def case(name, A, d, r, batch, reps):
    x = T.rand_tt((2,) * d, r, seed=30)
    dA, dx = T.DeviceTTO(A), T.DeviceTT.from_host(x, batch=batch)
    dy = T.DeviceTT((2,) * d, [p * q for p, q in zip(A.tto_rks, x.ttv_rks)], batch=batch)

    def composed():
        D.apply(dA, dx, dy)
        return D.dot(dx, dy)

    def direct():
        return D.expect(dA, dx)

    ref = composed()
    got = direct()                                     # (the warm-up of both)
    scale = float(np.max(np.abs(D.norm(dx) * D.norm(dy))))
    t_comp, t_dir, t_kern = [], [], []
    for _ in range(reps):
        t_comp.append(timed(composed, 0)[0])
        t_dir.append(timed(direct, 2)[0])
        t_kern.append(D.last_launch_ms())
    for h in (dA, dx, dy):
        h.free()
    mc, md, mk = statistics.median(t_comp), statistics.median(t_dir), statistics.median(t_kern)
    flops = batch * sandwich_flops(2, x.ttv_rks, A.tto_rks, x.ttv_rks)
    return {"operator": name, "d": d, "rank": r, "op_rank": max(A.tto_rks), "batch": batch, "reps": reps,
            "apply_dot_ms": t_comp, "apply_dot_ms_median": mc, "apply_dot_ms_spread": max(t_comp) - min(t_comp),
            "expect_ms": t_dir, "expect_ms_median": md, "expect_ms_spread": max(t_dir) - min(t_dir),
            "speedup": mc / md, "faster_by_more_than_spread": mc - md > max(max(t_comp) - min(t_comp), max(t_dir) - min(t_dir)),
            "expect_kernel_ms_median": mk, "sandwich_flops": flops, "expect_fraction_of_fp64_peak": flops / (mk * 1e-3) / PEAK_F64,
            "max_abs_diff_over_norms": float(np.max(np.abs(got - ref))) / scale}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=30)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 1])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_expect.json"))
    a = ap.parse_args()
    assert a.reps >= 7, "the median of at least 7 runs"
    T.ensure_init(0)
    rec = {"tool": "tools/diag_expect.py", "peak_fp64_flops": PEAK_F64, "cases": []}
    for name, A in (("Delta", T.Delta(a.d)), ("heisenberg_xyz", T.heisenberg_xyz_tto(a.d))):
        for B in a.batches:
            rec["cases"].append(case(name, A, a.d, a.rank, B, a.reps))
            print(json.dumps(rec["cases"][-1]), flush=True)
    D.status_all()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
