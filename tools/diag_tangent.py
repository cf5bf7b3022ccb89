"""Diagnostic of the fixed-rank manifold calls, written to profiles/diag_tangent.json.

QTT trains of d = 30 sites at rank 64 (rand_tt: the rank ramps 1, 2, 4, ... at both ends), batch 1 and 256, the projected train z of
rank 64 and of rank 192 (Delta * x):
  * ttn_tangent_project (asynchronous form: no value) against ttn_dot_pullback with abar alone on the SAME operands (U, z) — that call runs
    the same chains and sandwiches without the gauge term — in alternating windows of the same session;
  * ttn_tangent_to_tt, with the bytes it moves as a fraction of 8 TB/s.
Every case is timed with event pairs on the library's stream after a warm-up, in windows of about 0.3 s, five windows per call,
alternating the two calls; reported: the median, the smallest and the largest window, the ratio of the medians, and the algorithmic
flops of the extra product (2 n r r rz per site) beside those of the call."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ttn_amd as T                                   # noqa: E402
from ttn_amd import _lib                              # noqa: E402
from ttn_amd import device as D                       # noqa: E402

PEAK_BW, PEAK_F64 = 8.0e12, 78.6e12


def window(fn, reps):
    D.event_record(0)
    for _ in range(reps):
        fn()
    D.event_record(1)
    D.sync()
    return D.event_elapsed_ms(0, 1) / reps


def alternate(fns, target_s=0.3, windows=5):
    """{name: [ms per call of every window]}: warm-up, then `windows` rounds, each timing every call once, in turn."""
    reps = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        D.sync()
        per = max(window(fn, 2), 1e-3)
        reps[name] = int(max(3, min(2000, target_s * 1e3 / per)))
    out = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            out[name].append(window(fn, reps[name]))
    return out, reps


def stats(ws):
    return {"median_ms": statistics.median(ws), "min_ms": min(ws), "max_ms": max(ws), "windows": len(ws)}


def case(name, M, pt, z, batch, rec):
    L = _lib.lib()
    dims, r, rz = M.dims, M.ranks, z.max_ranks()
    d = len(dims)
    xi = T.DeviceTT(dims, r, batch)
    abar = T.DeviceTT(dims, r, batch)
    y = T.DeviceTT(dims, [1] + [2 * v for v in r[1:-1]] + [1], batch)
    _lib.check(L.ttn_tangent_project(pt.U.h, pt.V.h, z.h, xi.h, None))
    fns = {
        "project": lambda: _lib.check(L.ttn_tangent_project(pt.U.h, pt.V.h, z.h, xi.h, None)),
        "dot_pullback_abar": lambda: _lib.check(L.ttn_dot_pullback(pt.U.h, z.h, None, abar.h, None, None)),
        "to_tt": lambda: _lib.check(L.ttn_tangent_to_tt(pt.U.h, pt.V.h, xi.h, None, None, y.h)),
    }
    ws, reps = alternate(fns)
    f_chain = sum(2 * dims[k] * (r[k] * rz[k] * rz[k + 1] + r[k] * r[k + 1] * rz[k + 1]) for k in range(d))
    f_sand = sum(2 * dims[k] * (r[k] * rz[k] * rz[k + 1] + r[k] * rz[k + 1] * r[k + 1]) for k in range(d))
    f_extra = sum(2 * dims[k] * r[k] * r[k + 1] * rz[k + 1] for k in range(d - 1))
    by = 8 * sum(dims[k] * (3 * r[k] * r[k + 1] + (1 if k == 0 else 2 * r[k]) * (1 if k == d - 1 else 2 * r[k + 1])) for k in range(d))
    c = {"case": name, "batch": batch, "d": d, "max_rank_x": max(r), "max_rank_z": max(rz), "reps": reps,
         "project": stats(ws["project"]), "dot_pullback_abar": stats(ws["dot_pullback_abar"]), "to_tt": stats(ws["to_tt"]),
         "ratio_project_to_dot_pullback_abar": statistics.median(ws["project"]) / statistics.median(ws["dot_pullback_abar"]),
         "flops_dot_pullback_abar": 2 * f_chain + f_sand, "flops_gauge_term": f_extra,
         "flops_ratio_expected": (2 * f_chain + f_sand + f_extra) / (2 * f_chain + f_sand),
         "project_fraction_of_fp64_peak": batch * (2 * f_chain + f_sand + f_extra) / (statistics.median(ws["project"]) * 1e-3) / PEAK_F64,
         "to_tt_bytes_per_train": by, "to_tt_fraction_of_8TBs": batch * by / (statistics.median(ws["to_tt"]) * 1e-3) / PEAK_BW}
    print(json.dumps(c), flush=True)
    rec["cases"].append(c)
    for h in (xi, abar, y):
        h.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=30)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--bench", nargs="*", default=[], help="name=json pairs: bench.py result lines recorded beside the cases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_tangent.json"))
    args = ap.parse_args()
    T.ensure_init(0)
    dims = (2,) * args.d
    dA = T.DeviceTTO(T.Delta(args.d))
    rec = {"tool": "tools/diag_tangent.py", "d": args.d, "rank": args.rank, "peak_fp64_flops": PEAK_F64, "peak_bytes_per_s": PEAK_BW, "cases": [],
           "bench": {}}
    for pair in args.bench:
        name, _, path = pair.partition("=")
        with open(path) as f:
            rec["bench"][name] = json.loads([l for l in f.read().splitlines() if l.startswith("{")][-1])
    for batch in args.batches:
        x = T.DeviceTT.from_host(T.rand_tt(dims, args.rank, seed=1), batch)
        M = T.ttvector_manifold(x)
        pt = M.gauge(x)
        z64 = T.DeviceTT.from_host(T.rand_tt(dims, args.rank, seed=2), batch)
        case("z of rank %d" % args.rank, M, pt, z64, batch, rec)
        z64.free()
        zA = D.apply(dA, x, T.DeviceTT(dims, [R * c for R, c in zip(dA.rks, M.ranks)], batch))
        case("z = Delta x", M, pt, zA, batch, rec)
        zA.free()
        pt.free()
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
