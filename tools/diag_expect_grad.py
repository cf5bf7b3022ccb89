"""Diagnostic of the pullback of <x, A y>, written to profiles/diag_expect_grad.json.

For A = Delta(d) (R = 3) and A = heisenberg_xyz_tto(d) (R = 5) on rank-r QTT trains, at each batch size, on the same handles:

* grad.rayleigh_value_and_grad composed (apply, dot_pullback on (psi, A psi), apply_pullback, dot_pullback on (psi, psi)) next to
  fused=True (sandwich_pullback, dot_pullback on (psi, psi));
* ttn_sandwich_pullback alone (both tangents, no value, no cotangent: asynchronous) next to ttn_sandwich (its `batch` doubles to the host).

HIP-event pairs on the library stream around each, one warm-up of each first, the two forms alternating, the median of --reps runs and the
spread (max - min) of each.  Flops of the pullback: two chains (the count of tools/diag_expect.py each) and per site and tangent the three
products of the gradient, 2 (r_x R) r_y (n r_y') + 2 (r_x r_y') (n R) (n R') + 2 (n r_x) (R' r_y') r_x' for xbar and the same with x and y
exchanged for ybar.  Also the workspace per train and the bytes of the handles Y = A psi and Ybar that the fused form does not allocate."""
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
from ttn_amd import grad as G                         # noqa: E402

PEAK_F64 = 78.6e12


def chain_flops(n, rx, R, ry):
    f = 0
    for k in range(len(rx) - 1):
        f += 2 * rx[k + 1] * R[k + 1] * ry[k + 1] * n * ry[k]
        f += 2 * rx[k + 1] * ry[k] * (n * R[k + 1]) * (n * R[k])
        f += 2 * rx[k] * n * rx[k + 1] * R[k] * ry[k]
    return f


def core_flops(n, rx, R, ry):
    f = 0
    for k in range(len(rx) - 1):
        for p, q in ((rx, ry), (ry, rx)):
            f += 2 * p[k] * R[k] * q[k] * n * q[k + 1]
            f += 2 * p[k] * q[k + 1] * (n * R[k]) * (n * R[k + 1])
            f += 2 * n * p[k] * R[k + 1] * q[k + 1] * p[k + 1]
    return f


def workspace_doubles(d, n, rx, R, ry):
    """The formula of include/ttn_expect_grad.h for one train of the on-chip class."""
    W = max(a * b * c for a, b, c in zip(rx, R, ry))
    W += W & 1
    S = max(rx) * max(R) * max(ry)
    return 2 * (d + 1) * W + 2 * max(2 * n * S, 4096 * max(R))


def timed(fn, slot):
    D.event_record(slot)
    v = fn()
    D.event_record(slot + 1)
    return D.event_elapsed_ms(slot, slot + 1), v


def spread(v):
    return max(v) - min(v)


def case(name, A, d, r, batch, reps):
    x = T.rand_tt((2,) * d, r, seed=30)
    dA, dx = T.DeviceTTO(A), T.DeviceTT.from_host(x, batch=batch)
    g1, g2 = G._like(dx), G._like(dx)
    xb, yb = G._like(dx), G._like(dx)

    def composed():
        return G.rayleigh_value_and_grad(dA, dx, g=g1)[0]

    def fused():
        return G.rayleigh_value_and_grad(dA, dx, g=g2, fused=True)[0]

    def pullback():
        G.sandwich_pullback(dx, dA, dx, xbar=xb, ybar=yb, want_value=False)

    def sandwich():
        D.sandwich(dx, dA, dx)

    Ec, Ef = composed(), fused()                        # (the warm-up of all four)
    pullback(), sandwich()
    D.sync()
    gdiff = 0.0
    for b in {0, batch - 1}:
        c1, c2 = g1.download(b).ttv_vec, g2.download(b).ttv_vec
        gdiff = max(gdiff, max(float(np.max(np.abs(a - c))) for a, c in zip(c1, c2)) / max(float(np.max(np.abs(a))) for a in c1))
    t = {"composed": [], "fused": [], "pullback": [], "sandwich": []}
    for _ in range(reps):
        t["composed"].append(timed(composed, 0)[0])
        t["fused"].append(timed(fused, 2)[0])
        t["pullback"].append(timed(pullback, 4)[0])
        t["sandwich"].append(timed(sandwich, 6)[0])
    for h in (dA, dx, g1, g2, xb, yb):
        h.free()
    med = {k: statistics.median(v) for k, v in t.items()}
    rk, Rk = x.ttv_rks, A.tto_rks
    flops = batch * (2 * chain_flops(2, rk, Rk, rk) + core_flops(2, rk, Rk, rk))
    ybytes = 8 * sum(2 * Rk[k] * rk[k] * Rk[k + 1] * rk[k + 1] for k in range(d))
    return {"operator": name, "d": d, "rank": r, "op_rank": max(Rk), "batch": batch, "reps": reps,
            "rayleigh_composed_ms": t["composed"], "rayleigh_composed_ms_median": med["composed"], "rayleigh_composed_ms_spread": spread(t["composed"]),
            "rayleigh_fused_ms": t["fused"], "rayleigh_fused_ms_median": med["fused"], "rayleigh_fused_ms_spread": spread(t["fused"]),
            "rayleigh_speedup": med["composed"] / med["fused"],
            "fused_faster_by_more_than_spread": med["composed"] - med["fused"] > max(spread(t["composed"]), spread(t["fused"])),
            "pullback_ms": t["pullback"], "pullback_ms_median": med["pullback"], "pullback_ms_spread": spread(t["pullback"]),
            "sandwich_ms": t["sandwich"], "sandwich_ms_median": med["sandwich"], "sandwich_ms_spread": spread(t["sandwich"]),
            "pullback_over_sandwich": med["pullback"] / med["sandwich"],
            "pullback_flops": flops, "pullback_fraction_of_fp64_peak": flops / (med["pullback"] * 1e-3) / PEAK_F64,
            "workspace_bytes_per_train": 8 * workspace_doubles(d, 2, rk, Rk, rk),
            "Y_and_Ybar_bytes_per_train_not_allocated": 2 * ybytes,
            "max_rel_diff_E": float(np.max(np.abs(Ec - Ef) / np.maximum(np.abs(Ec), 1e-300))), "max_diff_gradient_over_largest_entry": gdiff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=30)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_expect_grad.json"))
    a = ap.parse_args()
    assert a.reps >= 7, "the median of at least 7 runs"
    T.ensure_init(0)
    rec = {"tool": "tools/diag_expect_grad.py", "peak_fp64_flops": PEAK_F64, "cases": []}
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
