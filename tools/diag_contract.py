"""Diagnostic of contract_sites, written to profiles/diag_contract.json.

On QTT trains of d = 30 sites and rank 64 (rank 65 for the general route), at each batch size, device.contract_sites into a handle
created beforehand, for the layouts of the PDE examples:
  * interleaved 2 x 15 bits, one dimension kept: 15 kept sites, each behind a run of one contracted site (14 matrix products per train on
    the on-chip route, one vector step at the left end);
  * serial 2 x 15 bits, the first dimension kept: 14 copies and one run of 15 sites behind the last kept site (a chain of matrix-vector
    products in one workgroup per train);
  * interleaved 3 x 10 bits, the last dimension kept: 10 kept sites behind runs of two;
  * the interleaved 2 x 15 case at rank 65, and at rank 64 in handles of capacity 65: the general route on the same data as the
    on-chip one.
Each against the bytes of x read once plus y written once, at the rate a torch ``fill_`` of that many bytes reaches in the same process.
At 2 x 12 bits, where the dense array still fits, qttnd.marginal on a resident batch next to the only route there was before:
DeviceTT.to_dense followed by torch.sum over one axis (both on the library's stream).
HIP-event pairs on the library stream around each call, one warm-up of each first, the median of --reps runs and the spread (max - min)."""
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
from ttn_amd import qttnd as Q                        # noqa: E402

torch, STREAM = T.tdvp._dev()                 # (asks torch for the GPU before the library binds it)
HBM_PEAK = 8.0e12


def timed(fn, slot):
    D.event_record(slot)
    v = fn()
    D.event_record(slot + 1)
    return D.event_elapsed_ms(slot, slot + 1), v


def stats(ts):
    return {"ms": ts, "ms_median": statistics.median(ts), "ms_spread": max(ts) - min(ts)}


def train_bytes(dims, rks):
    return 8 * sum(n * rks[k] * rks[k + 1] for k, n in enumerate(dims))


def fill_rate(nbytes, reps):
    """bytes per second of torch's fill_ on a buffer of nbytes, on the library's stream"""
    with torch.cuda.stream(STREAM):
        buf = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device="cuda")
        buf.fill_(1.0)
        ts = [timed(lambda: buf.fill_(2.0), 6)[0] for _ in range(reps)]
    return buf.numel() * 8 / (statistics.median(ts) * 1e-3), stats(ts)


def case(label, n_dims, bits, ordering, keep, r, batch, reps, cap=None):
    d = n_dims * bits
    x = T.rand_tt((2,) * d, r, seed=35)
    dx = T.DeviceTT.from_host(x, batch=batch, cap_rks=None if cap is None else [1] + [cap] * (d - 1) + [1])
    sites = [s + 1 for m in range(n_dims) if m not in keep for s in Q.dim_sites(m, n_dims, bits, ordering)]
    w = {s: np.ones(2) for s in sites}
    kept, start = D.contract_kept(d, sites)
    y = T.DeviceTT((2,) * len(kept), D.contract_rank_capacity(dx.cap, sites), batch)
    yr = [x.ttv_rks[s] for s in start] + [1]
    nbytes = batch * (train_bytes(x.ttv_dims, x.ttv_rks) + train_bytes((2,) * len(kept), yr))

    def run():
        return D.contract_sites(dx, w, y)

    run()
    ts = [timed(run, 0)[0] for _ in range(reps)]
    rate, fill = fill_rate(nbytes, reps)
    D.sync()
    assert y.ranks(0)[0] == yr
    med = statistics.median(ts)
    rec = {"case": label, "n_dims": n_dims, "bits": bits, "ordering": ordering, "keep": list(keep), "rank": r, "capacity": cap or r, "batch": batch,
           "route": "on-chip" if (cap or r) <= 64 else "general", "kept_sites": len(kept), "bytes_x_once_plus_y_once": nbytes,
           "contract_sites": stats(ts), "bytes_per_s": nbytes / (med * 1e-3), "fraction_of_hbm_peak": nbytes / (med * 1e-3) / HBM_PEAK,
           "fill_same_bytes": fill, "fill_bytes_per_s": rate, "fill_fraction_of_hbm_peak": rate / HBM_PEAK,
           "fraction_of_fill_rate": nbytes / (med * 1e-3) / rate}
    dx.free()
    y.free()
    return rec


def dense_case(bits, r, batch, reps):
    """2 x bits, interleaved: the marginal over the second dimension, next to to_dense + torch.sum"""
    d = 2 * bits
    x = T.rand_tt((2,) * d, r, seed=36)
    dx = T.DeviceTT.from_host(x, batch=batch)
    meta = (2, bits, "interleaved")
    strides = Q.grid_strides(*meta)
    G = 2 ** bits

    def new():
        my, _ = Q.marginal((dx, meta), (0,))
        return my

    def old():
        with torch.cuda.stream(STREAM):
            return dx.to_dense(strides).reshape(batch, G, G).sum(dim=1)       # memory order (b, g2, g1): the second dimension summed

    new().free()
    old()
    t_new, t_old = [], []
    for i in range(reps):
        t, my = timed(new, 0)
        t_new.append(t)
        t, dense_sum = timed(old, 2)
        t_old.append(t)
        if i + 1 < reps:
            my.free()
    D.sync()
    got = T.qttv_to_array(T.QTTvector(my.download(0), 1, bits, "interleaved"))
    ref = dense_sum[0].cpu().numpy()
    my.free()
    dx.free()
    mn, mo = statistics.median(t_new), statistics.median(t_old)
    return {"case": "dense-parent", "bits": bits, "rank": r, "batch": batch, "marginal": stats(t_new), "to_dense_then_sum": stats(t_old),
            "speedup": mo / mn, "faster_by_more_than_both_spreads": mo - mn > (max(t_new) - min(t_new)) + (max(t_old) - min(t_old)),
            "max_abs_diff_relative_to_max": float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dense-batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_contract.json"))
    a = ap.parse_args()
    assert a.reps >= 7, "the median of at least 7 runs"
    T.ensure_init(0)
    rec = {"tool": "tools/diag_contract.py", "hbm_peak_bytes_per_s": HBM_PEAK, "cases": []}

    def keep_(r):
        rec["cases"].append(r)
        print(json.dumps(r), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:                   # (kept after every case: a long run leaves what it has)
            json.dump(rec, f, indent=1)
            f.write("\n")

    for B in a.batches:
        keep_(case("interleaved-2d", 2, 15, "interleaved", (1,), 64, B, a.reps))
        keep_(case("serial-2d", 2, 15, "serial", (0,), 64, B, a.reps))
        keep_(case("interleaved-3d", 3, 10, "interleaved", (2,), 64, B, a.reps))
        keep_(case("interleaved-2d-rank65", 2, 15, "interleaved", (1,), 65, B, a.reps))
        keep_(case("interleaved-2d-rank64-general", 2, 15, "interleaved", (1,), 64, B, a.reps, cap=65))
    keep_(dense_case(12, 64, a.dense_batch, a.reps))
    D.status_all()


if __name__ == "__main__":
    main()
