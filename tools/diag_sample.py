"""Diagnostic of tt_sample, written to profiles/diag_sample.json.

On QTT trains of d sites (n = 2) of rank r, for S samples of each of B trains, in both modes: the device time of the environments and of
the sweeps of one device.sample_dev call (the library's own event pairs, ttn_tt_sample_last_ms), after a warm-up call; the median of
--reps calls and the spread (max - min).  From the sweep time: samples per second and the share of the fp64 matrix peak, counted on
2 n r_l r_r (W = V A) + 2 n r_r^2 (T = W G, Born only) flops per sample and site.  Rank 64 runs the on-chip route at every site, rank 65
the general route at every interior site: next to each other they are the A/B of the two routes on almost the same work.

--reference-only times tests/sample_reference.py on the host for the B = 1 jobs instead (no device is touched)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                    # noqa: E402

PEAK_F64 = 78.6e12


def qtt_ranks(d, r):
    return [min(2 ** k, 2 ** (d - k), r) for k in range(d + 1)]


def train_cores(d, r, born):
    rng = np.random.default_rng(30)
    rks = qtt_ranks(d, r)
    cores = [rng.standard_normal((2, rks[k], rks[k + 1])) / np.sqrt(rks[k]) for k in range(d)]
    return cores if born else [np.abs(c) for c in cores]


def flops_per_sample(rks, born, n=2):
    return sum(2 * n * rks[k] * rks[k + 1] + (2 * n * rks[k + 1] ** 2 if born else 0) for k in range(len(rks) - 1))


def stats(ts):
    return {"ms": ts, "ms_median": statistics.median(ts), "ms_spread": max(ts) - min(ts)}


def device_cases(a, save):
    import ttn_amd as T
    from ttn_amd import device as D
    T.tdvp._dev()                                     # (asks torch for the GPU before the library binds it)
    T.ensure_init(0)
    out = []
    for r in a.ranks:
        route = "on-chip at every site" if r <= 64 else "general at every site that touches a rank above 64, on-chip on the ramps"
        for born in (True, False):
            cores = train_cores(a.d, r, born)
            rks = qtt_ranks(a.d, r)
            x = T.TTvector(a.d, [np.asfortranarray(c) for c in cores], (2,) * a.d, rks, [0] * a.d)
            for B in a.batches:
                dx = T.DeviceTT.from_host(x, batch=B)
                for S in a.samples:
                    D.sample_dev(dx, S, mode="born" if born else "density", seed=1)        # the warm-up (and the workspace)
                    D.sync()
                    env, sweep = [], []
                    info = None
                    for _ in range(a.reps):
                        _, _, info = D.sample_dev(dx, S, mode="born" if born else "density", seed=1)
                        e, s = D.sample_last_ms()
                        env.append(e)
                        sweep.append(s)
                    ms = statistics.median(sweep)
                    fl = flops_per_sample(rks, born) * B * S
                    rec = {"d": a.d, "rank": r, "mode": "born" if born else "density", "batch": B, "samples": S, "reps": a.reps, "route": route,
                           "environments": stats(env), "sweep": stats(sweep), "samples_per_second": B * S / (ms * 1e-3),
                           "flops_counted": fl, "sweep_fraction_of_fp64_peak": fl / (ms * 1e-3) / PEAK_F64,
                           "clamps_and_dead": [int(v) for v in info.sum(dim=0).cpu()]}
                    out.append(rec)
                    print(json.dumps(rec), flush=True)
                    save(out)                             # (kept after every case: a long run leaves what it has)
                dx.free()
    D.status_all()
    return out


def reference_cases(a):
    from tests import sample_reference as R
    out = []
    for r in a.ranks:
        for born in (True, False):
            cores = train_cores(a.d, r, born)
            for S in a.samples:
                u = R.uniforms(1, 0, S, a.d)
                t0 = time.perf_counter()
                R.sample(cores, u, born)
                sec = time.perf_counter() - t0
                rec = {"d": a.d, "rank": r, "mode": "born" if born else "density", "batch": 1, "samples": S, "reference_seconds": sec,
                       "samples_per_second": S / sec, "threads": os.cpu_count()}
                out.append(rec)
                print(json.dumps(rec), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=30)
    ap.add_argument("--ranks", type=int, nargs="+", default=[64, 65, 16])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--samples", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reference-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_sample.json"))
    a = ap.parse_args()
    assert a.reps >= 7, "the median of at least 7 runs"
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    rec.update({"tool": "tools/diag_sample.py", "peak_fp64_flops": PEAK_F64})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def save(cases, key="cases"):
        rec[key] = cases
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")

    if a.reference_only:
        save(reference_cases(a), "reference_on_the_host")
    else:
        device_cases(a, save)


if __name__ == "__main__":
    main()
