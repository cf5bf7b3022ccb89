"""Stand-alone times of the matrix-product leaves of k_compress at the benchmark's shapes (profiles/r03j_leaves*.json).

The leaves are launched through the unit-test hook `ttn_selftest_gemm` (one workgroup, k_selftest_gemm), in the 1024-thread build and
in the 512-thread build (`TTN_WG512_SELFTEST=1`), each shape `--reps` times in a row.  The library holds no cycle counters, so the
times come from the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o leaves -- python tools/diag_leaves.py --plan OUT/plan.json
    python tools/diag_leaves.py --summarize OUT --plan OUT/plan.json --json profiles/<tag>_leaves.json

The first command writes the launch plan (which dispatch of k_selftest_gemm is which shape); the second reads the kernel trace the
profiler left under OUT, maps the dispatches to the plan in launch order and writes, per build and shape, the median / minimum kernel
duration next to the shape's MFMA floor: the v_mfma_f64_16x16x4 instructions of the busiest SIMD x 64 clk at 2.4 GHz (one SIMD issues
one fp64 MFMA per 64 clk; a workgroup's waves sit on 4 SIMDs, wave w on SIMD w mod 4, and the tiles are dealt round-robin over the waves).  `TTN_LIB` selects another
build of the library (the parent of a change).

The `syrk2` and `ra2` shapes launch k_selftest_syrk2 / k_selftest_gemm_ra2: route F's pair of 64-row Gram products (the left one stored
transposed) and its pair of 64 x 128 x 64 output products as ONE two-team call (`syrk2_...`, `ra2_...`) and as two single calls in the
same launch (`syrk2seq_...`, `ra2seq_...`): the difference of the two is what the pairing saves.  A library from before the paired
leaves has no such hooks: run its own copy of this tool for the members' times."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLOCK_GHZ = 2.4
MFMA_CLK = 64

# (name, routine, m, n, k, ta): the shapes of the benchmark's bond steps (d = 30, rank 64, Laplacian: 128 x 384 Gram steps left to right,
# 64-row factored steps right to left)
SHAPES = [
    ("syrk_128x384", "syrk", 128, 128, 384, 0),
    ("syrk_64x384", "syrk", 64, 64, 384, 0),
    ("syrk_64x128_ta0", "syrk", 64, 64, 128, 0),
    ("syrk_64x128_ta1", "syrk", 64, 64, 128, 1),
    ("ra_64x384x128", "ra", 64, 384, 128, 0),
    ("ra_64x128x64", "ra", 64, 128, 64, 0),
    ("small_64x64x128", "gemm", 64, 64, 128, 0),
    ("syrk2_64x128_ta1_ta0", "syrk2", 64, 64, 128, 1),            # ta: bit 0 = first member stored transposed, bit 1 = second
    ("syrk2seq_64x128_ta1_ta0", "syrk2seq", 64, 64, 128, 1),
    ("ra2_64x128x64", "ra2", 64, 128, 64, 0),                      # the left member with A, B, C transposed, the right one with A transposed
    ("ra2seq_64x128x64", "ra2seq", 64, 128, 64, 0),
]


def mfma_floor_us(routine, m, n, k, nwaves):
    """MFMA instructions of the busiest SIMD x 64 clk: a lower bound.  The tiles (SYRK: the lower triangle; register-A and the one-shot
    GEMM: all 16 x 16 outputs) are dealt round-robin over the waves, wave w gets tiles w, w + nwaves, ...; wave w runs on SIMD w mod 4,
    and a SIMD issues the MFMAs of all its waves one after another; k / 4 MFMAs per tile."""
    ksteps = (k + 3) // 4
    if routine in ("syrk2", "syrk2seq"):
        # two equal members: one after the other on all waves, or at once on half of the waves each (team wave w sits on SIMD w mod 4
        # in both builds: a team is 4 or 8 consecutive waves)
        tw = nwaves if routine == "syrk2seq" else nwaves // 2
        nt = (m + 15) // 16
        per_wave = [len(range(w, nt * (nt + 1) // 2, tw)) for w in range(tw)]
        return 2 * max(sum(per_wave[s::4]) for s in range(4)) * ksteps * MFMA_CLK / (CLOCK_GHZ * 1e3)
    if routine in ("ra2", "ra2seq"):
        return 2 * mfma_floor_us("ra", m, n, k, nwaves)          # two equal members; a team's wave takes both column groups of a chunk
    if routine == "syrk":
        nt = (m + 15) // 16
        tiles = nt * (nt + 1) // 2
    else:
        tiles = ((m + 15) // 16) * ((n + 15) // 16)
    per_wave = [len(range(w, tiles, nwaves)) for w in range(nwaves)]
    per_simd = max(sum(per_wave[s::4]) for s in range(4))
    return per_simd * ksteps * MFMA_CLK / (CLOCK_GHZ * 1e3)


def run(args):
    import numpy as np

    import ttn_amd as T

    T.ensure_init(0)
    lib = T._lib.lib()
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rng = np.random.default_rng(0)
    plan = []
    for wg512 in (0, 1):
        os.environ["TTN_WG512_SELFTEST"] = str(wg512)
        for name, routine, m, n, k, ta in SHAPES:
            if routine in ("syrk2", "syrk2seq"):
                A1, A2 = (rng.integers(-8, 9, size=(m, k)).astype(np.float64) for _ in range(2))
                M1, M2 = np.ascontiguousarray(A1.T if ta & 1 else A1), np.ascontiguousarray(A2.T if ta & 2 else A2)
                for rep in range(args.reps):
                    G1, G2 = np.full((m, m), np.nan), np.full((m, m), np.nan)
                    T._lib.check(lib.ttn_selftest_syrk2(m, k, p(M1), p(G1), 1.0, ta & 1, m, k, p(M2), p(G2), 1.0, (ta >> 1) & 1, int(routine == "syrk2")))
                    if rep == 0 and not (np.array_equal(G1, A1 @ A1.T) and np.array_equal(G2, A2 @ A2.T)):
                        raise SystemExit(f"{name} (wg512={wg512}): wrong result")
                    plan.append({"build": 512 if wg512 else 1024, "shape": name})
                continue
            if routine in ("ra2", "ra2seq"):
                A1, A2 = (rng.integers(-8, 9, size=(m, k)).astype(np.float64) for _ in range(2))
                B1, B2 = (rng.integers(-8, 9, size=(k, n)).astype(np.float64) for _ in range(2))
                M1, N1, M2 = np.ascontiguousarray(A1.T), np.ascontiguousarray(B1.T), np.ascontiguousarray(A2.T)
                for rep in range(args.reps):
                    C1, C2 = np.full((n, m), np.nan), np.full((m, n), np.nan)
                    T._lib.check(lib.ttn_selftest_gemm_ra2(m, n, k, p(M1), p(N1), p(C1), 1.0, 7, m, n, k, p(M2), p(B2), p(C2), 1.0, 1, int(routine == "ra2")))
                    if rep == 0 and not (np.array_equal(C1.T, A1 @ B1) and np.array_equal(C2, A2 @ B2)):
                        raise SystemExit(f"{name} (wg512={wg512}): wrong result")
                    plan.append({"build": 512 if wg512 else 1024, "shape": name})
                continue
            A = rng.integers(-8, 9, size=(k, m) if ta else (m, k)).astype(np.float64)
            B = rng.integers(-8, 9, size=(k, n)).astype(np.float64)
            flag = {"syrk": 2 | ta, "ra": 4 | ta, "gemm": ta}[routine]
            ref = (A.T @ A if ta else A @ A.T) if routine == "syrk" else (A.T if ta else A) @ B
            for rep in range(args.reps):
                Cc = np.full((m, n), np.nan)
                T._lib.check(lib.ttn_selftest_gemm(m, n, k, p(A), p(B), p(Cc), 1.0, 0.0, flag, 0))
                if rep == 0 and not np.array_equal(Cc, ref):
                    raise SystemExit(f"{name} (wg512={wg512}): wrong result")
                plan.append({"build": 512 if wg512 else 1024, "shape": name})
    os.environ.pop("TTN_WG512_SELFTEST", None)
    json.dump({"reps": args.reps, "lib": "TTN_LIB (another build of the library)" if os.environ.get("TTN_LIB") else "in-tree", "launches": plan}, open(args.plan, "w"))
    print(f"{len(plan)} launches, plan -> {args.plan}")


def summarize(args):
    plan = json.load(open(args.plan))
    traces = glob.glob(os.path.join(args.summarize, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        raise SystemExit(f"no *kernel_trace.csv under {args.summarize}")
    rows = [r for t in traces for r in csv.DictReader(open(t)) if "k_selftest_gemm" in r["Kernel_Name"] or "k_selftest_syrk2" in r["Kernel_Name"]]     # one file per process
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != len(plan["launches"]):
        raise SystemExit(f"{len(rows)} k_selftest_gemm / k_selftest_syrk2 dispatches in the trace, {len(plan['launches'])} in the plan")
    durs = {}
    for r, l in zip(rows, plan["launches"]):
        is512 = "wg512" in r["Kernel_Name"]
        if is512 != (l["build"] == 512):
            raise SystemExit("the trace and the plan disagree on the build of a launch")
        durs.setdefault((l["build"], l["shape"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    spec = {s[0]: s for s in SHAPES}
    out = {"tool": "tools/diag_leaves.py", "lib": plan["lib"], "reps": plan["reps"], "unit": "us per single-workgroup launch of k_selftest_gemm / k_selftest_syrk2",
           "floor": f"MFMAs of the busiest SIMD x {MFMA_CLK} clk at {CLOCK_GHZ} GHz", "leaves": []}
    for (build, shape), d in sorted(durs.items()):
        _, routine, m, n, k, ta = spec[shape]
        d = sorted(d[1:]) if len(d) > 2 else sorted(d)                # the first launch of a shape loads code and tables
        floor = mfma_floor_us(routine, m, n, k, build // 64)
        rec = {"build": build, "shape": shape, "median_us": round(d[len(d) // 2], 2), "min_us": round(d[0], 2), "max_us": round(d[-1], 2),
               "mfma_floor_us": round(floor, 2), "median_over_floor": round(d[len(d) // 2] / floor, 2)}
        out["leaves"].append(rec)
        print(json.dumps(rec))
    if args.json:
        json.dump(out, open(args.json, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=40, help="launches per shape and build")
    ap.add_argument("--plan", default="leaves_plan.json", help="where the launch plan is written / read")
    ap.add_argument("--summarize", metavar="DIR", default=None, help="read the rocprofv3 kernel trace under DIR instead of launching")
    ap.add_argument("--json", default=None, help="--summarize: write the per-shape record here")
    ap.add_argument("--refloor", metavar="JSON", nargs="+", default=None,
                    help="recompute mfma_floor_us and median_over_floor of existing records from their stored medians (no launch)")
    args = ap.parse_args()
    if args.refloor:
        spec = {s[0]: s for s in SHAPES}
        for path in args.refloor:
            rec = json.load(open(path))
            for l in rec["leaves"]:
                _, routine, m, n, k, ta = spec[l["shape"]]
                floor = mfma_floor_us(routine, m, n, k, l["build"] // 64)
                l["mfma_floor_us"], l["median_over_floor"] = round(floor, 2), round(l["median_us"] / floor, 2)
            json.dump(rec, open(path, "w"), indent=1)
        return
    summarize(args) if args.summarize else run(args)


if __name__ == "__main__":
    main()
