"""Diagnostic of ttn_apply_rect, written to profiles/diag_prolong.json.

The coarse-to-fine step d = 30 -> 31 on B rank-64 trains: the constant prolongation (ranks 1, the output is as large as the input
plus one site) and the linear prolongation (interior ranks 5: the output cores are 25 times the input's).  The yardstick is ttn_apply
(k_apply, unchanged) with a SQUARE operator of the same ranks on the same trains, measured in the same run: windows of the two calls
alternate.  Every window is timed with StreamTimer (HIP events on the library's stream) after a warm-up; reported are the median
over the windows, the bytes of the output cores per second and that as a fraction of 8 TB/s, and the ratio of the two fractions.
`--only rect_linear|rect_constant|square_linear` runs one form a few times for a kernel-trace profiler run."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ttn_amd as T                                   # noqa: E402
from ttn_amd import device as D                       # noqa: E402

PEAK_BW = 8.0e12


def window(fn, reps):
    with D.StreamTimer() as t:
        for _ in range(reps):
            fn()
    return t.ms / reps


def core_bytes(dims, rks):
    return 8 * sum(n * rks[k] * rks[k + 1] for k, n in enumerate(dims))


def square_like(P: T.TToperator, d: int) -> T.TToperator:
    """A square operator on d sites with the ranks of P's first d bonds (right end 1): random cores, the yardstick's input."""
    rks = list(P.tto_rks[:d]) + [1]
    cores = [np.asfortranarray(T.portable_randn(4 * rks[k] * rks[k + 1], 500 + k).reshape((2, 2, rks[k], rks[k + 1]), order="F")) for k in range(d)]
    return T.TToperator(d, cores, (2,) * d, rks, [0] * d)


def setup(kind, d, r, B):
    P = T.qtto_constant_prolongation(d) if kind == "constant" else T.qtto_linear_prolongation(d)
    S = square_like(P, d)
    x = D.DeviceTT.from_host(T.rand_tt((2,) * d, r, seed=30), batch=B)
    dP, dS = D.DeviceRectTTO(P), D.DeviceTTO(S)
    yr = D.rect_rank_capacity(P.tto_rks, d + 1, x.cap)
    ys = [a * b for a, b in zip(S.tto_rks, x.cap)]
    y_rect, y_sq = D.DeviceTT((2,) * (d + 1), yr, B), D.DeviceTT((2,) * d, ys, B)
    return {"rect": lambda: D.apply_rect(dP, x, y_rect), "square": lambda: D.apply(dS, x, y_sq),
            "rect_bytes": core_bytes((2,) * (d + 1), yr) * B, "square_bytes": core_bytes((2,) * d, ys) * B,
            "read_bytes": core_bytes((2,) * d, x.cap) * B, "rect_ranks": yr, "handles": (x, y_rect, y_sq, dP, dS)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_prolong.json"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--d", type=int, default=30)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--only", default=None, help="rect_linear | rect_constant | square_linear: run that call 5 times (for a profiler run)")
    a = ap.parse_args()
    T.ensure_init(0)
    if a.only:
        form, kind = a.only.split("_")
        s = setup(kind, a.d, a.rank, a.batch)
        for _ in range(5):
            s[form]()
        D.sync()
        D.status_all()
        print("ran", a.only, "5 times")
        return
    rec = {"peak_bytes_per_s": PEAK_BW, "d": a.d, "rank": a.rank, "B": a.batch, "cases": []}
    for kind in ("constant", "linear"):
        s = setup(kind, a.d, a.rank, a.batch)
        for _ in range(3):                               # warm-up of both calls
            s["rect"](), s["square"]()
        D.sync()
        per = max(window(s["rect"], 3), window(s["square"], 3), 1e-3)
        reps = int(max(3, min(500, 300.0 / per)))        # windows of about 0.3 s
        w_rect, w_sq = [], []
        for _ in range(a.windows):                       # alternate the call and its yardstick
            w_rect.append(window(s["rect"], reps))
            w_sq.append(window(s["square"], reps))
        ms_r, ms_s = statistics.median(w_rect), statistics.median(w_sq)
        fr, fs = s["rect_bytes"] / (ms_r * 1e-3) / PEAK_BW, s["square_bytes"] / (ms_s * 1e-3) / PEAK_BW
        case = {"operator": kind, "reps_per_window": reps, "out_ranks": s["rect_ranks"],
                "rect_ms_windows": w_rect, "rect_ms": ms_r, "rect_bytes_written": s["rect_bytes"], "rect_share_of_8TBps": fr,
                "square_ms_windows": w_sq, "square_ms": ms_s, "square_bytes_written": s["square_bytes"], "square_share_of_8TBps": fs,
                "bytes_read": s["read_bytes"], "rect_over_square_share": fr / fs}
        rec["cases"].append(case)
        print(json.dumps(case), flush=True)
        for h in s["handles"]:
            h.free()
    D.status_all()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
