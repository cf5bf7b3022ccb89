"""Diagnostic (not a test): the 128x128 symmetric eigensolver of the Gram route against NumPy, and its stand-alone time.

    python tools/diag_eig.py [SEED]                     accuracy of a few shapes against numpy.linalg.eigh (the 1024-thread build, or
                                                        the 512-thread one with TTN_WG512_SELFTEST=1)
    python tools/diag_eig.py --timing [--json OUT]      clock counts of the routine (`ticks`: s_memtime around wg_eig_n in
                                                        k_selftest_eig128, one workgroup) at the shapes of the benchmark's Gram steps,
                                                        (n, r, nev) = (128, 64, 64) and (64, 64, 64), both builds, --reps launches each

The kernel times of the same launches come from the profiler, as in tools/diag_leaves.py:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o eig -- python tools/diag_eig.py --timing --json OUT/eig.json
    python tools/diag_eig.py --summarize OUT --json OUT/eig.json

The second command adds the median / minimum duration of the k_selftest_eig128 dispatches, in launch order, to the record.
`TTN_LIB` selects another build of the library (the parent of a change, or a throw-away build whose routine returns after the
bisection or after the eigenvectors: the differences of their clock counts are the phases' — profiles/r03l_eig*.json)."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TIMING_SHAPES = [(128, 64, 64), (64, 64, 64)]


def gram(rng, n, decades):
    M = rng.standard_normal((128, 384))
    if decades > 0:
        # shape the spectrum like the workload: smooth decay over `decades` decades
        U, s, Vt = np.linalg.svd(M, full_matrices=False)
        s = s[0] * 10.0 ** (-decades * np.arange(128) / 127)
        M = (U * s) @ Vt
    M /= np.max(np.abs(M))
    return M


def launch(T, L, G, n, r, nev):
    sig = np.zeros(128)
    X = np.zeros((128, 64), order="F")
    tk = (C.c_int64 * 2)()
    T._lib.check(L.ttn_selftest_eig128(G.ctypes.data_as(C.c_void_p), n, r, nev, sig.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p), tk))
    return sig, X, tk


def accuracy(args):
    import ttn_amd as T

    T.ensure_init(0)
    L = T._lib.lib()
    rng = np.random.default_rng(args.seed)
    for trial in range(4):
        M = gram(rng, 128, 1.5 * (trial + 1) / 3 if trial < 3 else 0.0)
        for n, r, nev in ((128, 64, 64), (128, 64, 128), (128, 17, 40), (64, 64, 64), (64, 20, 64), (64, 32, 32), (64, 5, 9)):
            G = np.asfortranarray(M[:n] @ M[:n].T)
            sig, X, tk = launch(T, L, G, n, r, nev)
            w, V = np.linalg.eigh(G)
            w, V = w[::-1], V[:, ::-1]
            sref = np.sqrt(w)
            es = np.max(np.abs(sig[:nev] - sref[:nev]) / sref[:nev])
            Ux = X[:n, :r] / sig[:r]
            orth = np.max(np.abs(Ux.T @ Ux - np.eye(r)))
            resid = np.max(np.abs(G @ Ux - Ux * w[:r]) / w[0])
            sgn = np.sign(np.sum(Ux * V[:, :r], axis=0))
            ev = np.max(np.abs(Ux * sgn - V[:, :r]))
            print(f"trial {trial} n={n} r={r} nev={nev}: rc={tk[1]} ticks={tk[0]}  sig rel err {es:.1e}  |U'U-I| {orth:.1e}  resid {resid:.1e}  vec diff {ev:.1e}")


def timing(args):
    import ttn_amd as T

    T.ensure_init(0)
    L = T._lib.lib()
    M = gram(np.random.default_rng(args.seed), 128, 1.5)
    out = {"tool": "tools/diag_eig.py --timing", "lib": args.label or ("TTN_LIB (another build of the library)" if os.environ.get("TTN_LIB") else "in-tree"),
           "reps": args.reps, "unit": "clock counts of s_memtime around wg_eig_n, one workgroup (about 2.35 per ns of kernel time)", "shapes": []}
    for wg512 in (0, 1):
        os.environ["TTN_WG512_SELFTEST"] = str(wg512)
        for n, r, nev in TIMING_SHAPES:
            G = np.asfortranarray(M[:n] @ M[:n].T)
            ticks = []
            for rep in range(args.reps):
                _, _, tk = launch(T, L, G, n, r, nev)
                if tk[1] != 0:
                    raise SystemExit(f"n={n} (wg512={wg512}): the routine reported {tk[1]}")
                ticks.append(int(tk[0]))
            t = sorted(ticks[1:]) if len(ticks) > 2 else sorted(ticks)      # the first launch of a shape loads code
            rec = {"build": 512 if wg512 else 1024, "n": n, "r": r, "nev": nev, "median_ticks": t[len(t) // 2], "min_ticks": t[0], "max_ticks": t[-1]}
            out["shapes"].append(rec)
            print(json.dumps(rec))
    os.environ.pop("TTN_WG512_SELFTEST", None)
    if args.json:
        json.dump(out, open(args.json, "w"), indent=1)


def summarize(args):
    out = json.load(open(args.json))
    traces = glob.glob(os.path.join(args.summarize, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        raise SystemExit(f"no *kernel_trace.csv under {args.summarize}")
    rows = [r for t in traces for r in csv.DictReader(open(t)) if "k_selftest_eig128" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    reps = out["reps"]
    if len(rows) != reps * len(out["shapes"]):
        raise SystemExit(f"{len(rows)} k_selftest_eig128 dispatches in the trace, {reps * len(out['shapes'])} in the record")
    for i, rec in enumerate(out["shapes"]):
        mine = rows[i * reps:(i + 1) * reps]
        if any(("wg512" in r["Kernel_Name"]) != (rec["build"] == 512) for r in mine):
            raise SystemExit("the trace and the record disagree on the build of a launch")
        d = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in (mine[1:] if reps > 2 else mine))
        rec["median_us"], rec["min_us"] = round(d[len(d) // 2], 2), round(d[0], 2)
        print(json.dumps(rec))
    json.dump(out, open(args.json, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("seed", nargs="?", type=int, default=0)
    ap.add_argument("--timing", action="store_true", help="clock counts at the benchmark's shapes instead of the accuracy table")
    ap.add_argument("--reps", type=int, default=40, help="--timing: launches per shape and build")
    ap.add_argument("--label", default=None, help="--timing: what the record calls the library it ran")
    ap.add_argument("--json", default=None, help="--timing: write the record here; --summarize: the record to extend")
    ap.add_argument("--summarize", metavar="DIR", default=None, help="add the kernel durations of the rocprofv3 trace under DIR to --json")
    args = ap.parse_args()
    if args.summarize:
        summarize(args)
    elif args.timing:
        timing(args)
    else:
        accuracy(args)


if __name__ == "__main__":
    main()
