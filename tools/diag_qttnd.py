"""Diagnostic of ttn_tt_to_dense, written to profiles/diag_qttnd.json.

Binary trains of N = 20, 24, 26 sites at ranks 4, 16, 64, with the output strides of Julia column-major, of qttv_to_array for an
interleaved 2-D QTT and for a serial 2-D QTT.  Every case is timed with event pairs on the library's stream after a warm-up, in
windows of about 0.2 s, alternating with yardstick (a); the whole call is timed (offset tables, partial products and the product
kernel), because that is what a caller waits for.

Two yardsticks, measured in the same process:
  (a) torch.Tensor.fill_ on a buffer of the same size on the same stream: the store-rate ceiling.  Reported per case: the achieved
      fraction of it.
  (b) the only device route to values before this kernel: cross._d_eval (k_cross_eval, one wave per point) at all 2^N index rows,
      for N = 20 only.  Reported: the ratio of its time to ttn_tt_to_dense's.
Per case also: bytes written (8 * total) per second, flops (2 * r_m * total) per second, and the share of the roofline
max(bytes / 8 TB/s, flops / 78.6 TFLOP/s) / time, with the bound that applies."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ttn_amd as T                                   # noqa: E402
from ttn_amd import _lib, cross                       # noqa: E402
from ttn_amd import device as D                       # noqa: E402
from ttn_amd.tdvp import _dev                         # noqa: E402

PEAK_BW, PEAK_F64 = 8.0e12, 78.6e12


def window(fn, reps):
    """ms per call of `reps` back-to-back calls between two events on the library's stream"""
    D.event_record(0)
    for _ in range(reps):
        fn()
    D.event_record(1)
    D.sync()
    return D.event_elapsed_ms(0, 1) / reps


def timed(fn, target_s=0.2, windows=3):
    for _ in range(3):                                 # warm-up: code objects, scratch growth, allocator
        fn()
    D.sync()
    per = max(window(fn, 3), 1e-3)
    reps = int(max(5, min(5000, target_s * 1e3 / per)))
    return [window(fn, reps) for _ in range(windows)], reps


def strides_for(kind, N):
    if kind == "column_major":
        return None
    return T.grid_strides(2, N // 2, "interleaved" if kind == "interleaved_2d" else "serial")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, nargs="+", default=[20, 24, 26])
    ap.add_argument("--ranks", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_qttnd.json"))
    ap.add_argument("--only", default=None, help="N,rank,kind: run that single case without the yardsticks (for a profiler run)")
    a = ap.parse_args()
    torch, stream = _dev()
    L = _lib.lib()
    if a.only:
        N, r, kind = a.only.split(",")
        N, r = int(N), int(r)
        h = D.DeviceTT.from_host(T.rand_tt((2,) * N, r, seed=N + r))
        st = strides_for(kind, N)
        with torch.cuda.stream(stream):
            out = torch.empty((1 << N,), dtype=torch.float64, device="cuda")
            for _ in range(5):
                _lib.check(L.ttn_tt_to_dense(h.h, None if st is None else T.tt._i64(st), C.c_void_p(out.data_ptr())))
        D.sync()
        print("ran", a.only, "5 times; bytes per call", 8 << N)
        return
    rec = {"peak_bytes_per_s": PEAK_BW, "peak_f64_flops": PEAK_F64, "device": torch.cuda.get_device_name(0), "cases": []}
    with torch.cuda.stream(stream):
        for N in a.sites:
            total = 1 << N
            out = torch.empty((total,), dtype=torch.float64, device="cuda")
            po = C.c_void_p(out.data_ptr())
            for r in a.ranks:
                x = T.rand_tt((2,) * N, r, seed=N + r)
                h = D.DeviceTT.from_host(x)
                r_m = x.ttv_rks[N // 2]
                eval_ms = None
                if N == 20:                            # yardstick (b)
                    cores = cross._up_cores(x.ttv_vec, np.float64)
                    e = torch.arange(total, dtype=torch.int64, device="cuda")
                    idx = torch.stack([((e >> s) & 1) + 1 for s in range(N)]).contiguous()
                    ev, ev_reps = timed(lambda: cross._d_eval(cores, idx=idx), target_s=0.1)
                    eval_ms = statistics.median(ev)
                    ref = cross._d_eval(cores, idx=idx)[0]
                    _lib.check(L.ttn_tt_to_dense(h.h, None, po))
                    D.sync()
                    scale = float(ref.abs().max())
                    assert float((out - ref).abs().max()) <= 1e-9 * scale, "the two routes disagree"
                for kind in ("column_major", "interleaved_2d", "serial_2d"):
                    st = strides_for(kind, N)
                    pst = None if st is None else T.tt._i64(st)
                    dense, fill = [], []
                    for _ in range(2):                 # alternate the kernel and yardstick (a)
                        w, reps = timed(lambda: _lib.check(L.ttn_tt_to_dense(h.h, pst, po)))
                        dense += w
                        w, freps = timed(lambda: out.fill_(1.0))
                        fill += w
                    ms, fms = statistics.median(dense), statistics.median(fill)
                    t = ms * 1e-3
                    nbytes, flops = 8 * total, 2 * r_m * total
                    t_min = max(nbytes / PEAK_BW, flops / PEAK_F64)
                    case = {"N": N, "rank": r, "rank_at_cut": r_m, "strides": kind, "reps_per_window": reps, "ms_windows": dense, "ms": ms,
                            "bytes_written": nbytes, "write_GBps": nbytes / t / 1e9, "flops": flops, "TFLOPs": flops / t / 1e12,
                            "roofline_bound": "stores" if nbytes / PEAK_BW >= flops / PEAK_F64 else "fp64", "share_of_roofline": t_min / t,
                            "fill_ms_windows": fill, "fill_ms": fms, "fill_GBps": nbytes / (fms * 1e-3) / 1e9, "fraction_of_fill": fms / ms}
                    if eval_ms is not None:
                        case["cross_eval_ms"] = eval_ms
                        case["cross_eval_over_to_dense"] = eval_ms / ms
                    rec["cases"].append(case)
                    print(json.dumps(case), flush=True)
                h.free()
            del out
    D.status_all()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
