"""Diagnostic of ttn_tt_merge_sites / ttn_tt_split_sites, written to profiles/diag_resite.json.

Merge: d = 30 binary sites at rank 64 merged in groups of 3 (ten 8-point sites), B = 1 and B = 1024.
Split: the inverse — ten 8-point sites at rank <= 32 (largest unfolding 64 x 128) split to [2, 2, 2], B = 1 and B = 256.

Every case is timed with event pairs on the library's stream after a warm-up, medians over windows, into a preallocated output handle
(the whole call: copy kernel plus contraction steps, or the one split kernel).  Reported per merge case: time, bytes of the output cores
per second, and the fraction of a torch fill_ of a buffer of the same size on the same stream.  Reported per split case: time, and the
time of the same kernel on the same trains with one-entry split lists (copies only, no SVD): 1 - copy / split estimates the share of
the SVD steps from outside the kernel; `--only split_full|split_copy|merge` runs one form a few times for a kernel-trace profiler run.
Both also report the host route that existed before: download, the NumPy restatement (tests/resite_reference.py), upload — measured
for one train (times B is what a batch would cost)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ttn_amd as T                                   # noqa: E402
from ttn_amd import _lib                              # noqa: E402
from ttn_amd import device as D                       # noqa: E402
from ttn_amd.tdvp import _dev                         # noqa: E402
from tests import resite_reference as R               # noqa: E402

PEAK_BW = 8.0e12


def window(fn, reps):
    D.event_record(0)
    for _ in range(reps):
        fn()
    D.event_record(1)
    D.sync()
    return D.event_elapsed_ms(0, 1) / reps


def timed(fn, target_s=0.2, windows=5):
    for _ in range(3):
        fn()
    D.sync()
    per = max(window(fn, 3), 1e-3)
    reps = int(max(3, min(2000, target_s * 1e3 / per)))
    return [window(fn, reps) for _ in range(windows)], reps


def core_bytes(dims, rks):
    return 8 * sum(n * rks[k] * rks[k + 1] for k, n in enumerate(dims))


def host_route(x, fn):
    """download -> NumPy -> upload for one train, seconds"""
    t0 = time.perf_counter()
    h = x.download(0)
    out = fn(R.Train(h.ttv_vec))
    y = D.DeviceTT.from_host(T.TTvector(out.N, [c.copy(order="F") for c in out.ttv_vec], out.ttv_dims, out.ttv_rks, [0] * out.N))
    D.sync()
    dt = time.perf_counter() - t0
    y.free()
    return dt


def merge_setup(B):
    x = D.DeviceTT.from_host(T.rand_tt((2,) * 30, 64, seed=7), batch=B)
    z = D.DeviceTT((8,) * 10, [x.cap[3 * g] for g in range(11)], B)
    mn = T.tt._i64([3] * 10)
    return x, z, lambda: _lib.check(_lib.lib().ttn_tt_merge_sites(x.h, z.h, mn, 10))


def split_setup(B, copy_only=False):
    x = D.DeviceTT.from_host(T.rand_tt((8,) * 10, 32, seed=8), batch=B)
    sd = [[8]] * 10 if copy_only else [[2, 2, 2]] * 10
    flat = [f for s in sd for f in s]
    z = D.DeviceTT(flat, D.split_rank_capacity(x.dims, x.cap, sd), B)
    ns, fl = T.tt._i64([len(s) for s in sd]), T.tt._i64(flat)
    return x, z, sd, lambda: _lib.check(_lib.lib().ttn_tt_split_sites(x.h, z.h, ns, fl, 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_resite.json"))
    ap.add_argument("--only", default=None, help="merge | split_full | split_copy: run that form 5 times at the large batch (for a profiler run)")
    a = ap.parse_args()
    torch, stream = _dev()
    if a.only:
        run = merge_setup(1024)[2] if a.only == "merge" else split_setup(256, a.only == "split_copy")[3]
        for _ in range(5):
            run()
        D.sync()
        D.status_all()
        print("ran", a.only, "5 times")
        return
    rec = {"peak_bytes_per_s": PEAK_BW, "device": torch.cuda.get_device_name(0), "merge": [], "split": []}
    with torch.cuda.stream(stream):
        for B in (1, 1024):
            x, z, run = merge_setup(B)
            run()
            D.compress_status(z)
            rks = z.ranks(0)[0]
            nbytes = core_bytes(z.dims, rks) * B
            buf = torch.empty((nbytes // 8,), dtype=torch.float64, device="cuda")
            ms_w, fill_w = [], []
            for _ in range(2):                         # alternate the call and the fill yardstick
                w, reps = timed(run)
                ms_w += w
                fill_w += timed(lambda: buf.fill_(1.0))[0]
            ms, fms = statistics.median(ms_w), statistics.median(fill_w)
            host_s = statistics.median([host_route(x, lambda t: R.to_ttv(t, [3] * 10)) for _ in range(3)])
            case = {"B": B, "sites": 30, "rank": 64, "groups_of": 3, "out_ranks": rks, "reps_per_window": reps, "ms_windows": ms_w, "ms": ms,
                    "bytes_written": nbytes, "write_GBps": nbytes / (ms * 1e-3) / 1e9, "share_of_8TBps": nbytes / (ms * 1e-3) / PEAK_BW,
                    "fill_ms": fms, "fill_GBps": nbytes / (fms * 1e-3) / 1e9, "fraction_of_fill": fms / ms,
                    "host_route_ms_per_train": host_s * 1e3, "host_route_ms_times_B": host_s * 1e3 * B}
            rec["merge"].append(case)
            print(json.dumps(case), flush=True)
            del buf
            x.free(); z.free()
        for B in (1, 256):
            x, z, sd, run = split_setup(B)
            run()
            sweeps = D.compress_status(z)
            rks = z.ranks(0)[0]
            w, reps = timed(run)
            xc, zc, _, run_copy = split_setup(B, copy_only=True)
            wc, _ = timed(run_copy)
            ms, cms = statistics.median(w), statistics.median(wc)
            host_s = statistics.median([host_route(x, lambda t: R.to_qtt(t, sd)) for _ in range(3)])
            case = {"B": B, "sites": 10, "n": 8, "rank": 32, "largest_unfolding": [64, 128], "out_ranks": rks, "jacobi_sweeps_train0": sweeps[0],
                    "reps_per_window": reps, "ms_windows": w, "ms": ms, "copy_only_ms": cms, "svd_share_estimate": 1.0 - cms / ms,
                    "svd_steps_per_train": 20, "us_per_svd_step_per_train": (ms - cms) * 1e3 / 20 / B,
                    "host_route_ms_per_train": host_s * 1e3, "host_route_ms_times_B": host_s * 1e3 * B}
            rec["split"].append(case)
            print(json.dumps(case), flush=True)
            for h in (x, z, xc, zc):
                h.free()
    D.status_all()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
