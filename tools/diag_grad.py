"""Diagnostic of the core gradients, written to profiles/diag_grad.json.

QTT trains of d = 30 sites at rank 64 (rand_tt: the rank ramps 1, 2, 4, ... at both ends), batch 1, 256 and 1024:
  * ttn_dot_pullback with both outputs and with abar alone (asynchronous form: no cotangent array, no value), and ttn_dot on the same
    operands beside each (its kernel alone, ttn_last_launch_ms);
  * the pair (psi, Delta psi) — ranks 64 against 192, both chain routes in one call — at batch 1 and 256;
  * ttn_apply_pullback against ttn_apply on the same shapes (Delta, ranks 3).
Every case is timed with event pairs on the library's stream after a warm-up, in windows of about 0.2 s.  Reported per case: ms, the
ratio to the yardstick beside it, algorithmic flops (2 n (P S T + P T Q) per sandwich, the same per chain step) per second as a
fraction of the fp64 matrix peak, bytes moved (the streaming kernel) as a fraction of 8 TB/s, and the workspace in bytes."""
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


def timed(fn, target_s=0.2, windows=3):
    for _ in range(3):                                 # warm-up: code objects, workspace growth
        fn()
    D.sync()
    per = max(window(fn, 2), 1e-3)
    reps = int(max(3, min(2000, target_s * 1e3 / per)))
    return statistics.median(window(fn, reps) for _ in range(windows)), reps


def chain_flops(dims, ra, rb):
    """one transfer-matrix chain of dot(A, B): 2 n (ra rb rb' + ra ra' rb') per site"""
    return sum(2 * dims[k] * (ra[k] * rb[k] * rb[k + 1] + ra[k] * ra[k + 1] * rb[k + 1]) for k in range(len(dims)))


def sandwich_flops(dims, rp, rs):
    """the outputs of one operand: P = rp[k], Q = rp[k + 1], S = rs[k], T = rs[k + 1]"""
    return sum(2 * dims[k] * (rp[k] * rs[k] * rs[k + 1] + rp[k] * rs[k + 1] * rp[k + 1]) for k in range(len(dims)))


def workspace_bytes(dims, ra, rb):
    d = len(dims)
    W = (max(x * y for x, y in zip(ra, rb)) + 1) & ~1
    return 8 * (2 * (d + 1) * W + 2 * ((max(dims) * max(ra) * max(rb) + 1) & ~1))


def dot_cases(name, a, b, batch, rec):
    L = _lib.lib()
    dims, ra, rb = a.dims, a.max_ranks(), b.max_ranks()
    abar, bbar = T.DeviceTT(dims, a.cap, batch), T.DeviceTT(dims, b.cap, batch)
    out = (C.c_double * batch)()

    def dot_kernel_ms():
        _lib.check(L.ttn_dot(a.h, b.h, out))
        return D.last_launch_ms()

    for _ in range(3):
        dot_kernel_ms()
    dot_ms = statistics.median(dot_kernel_ms() for _ in range(9))
    both_ms, reps = timed(lambda: _lib.check(L.ttn_dot_pullback(a.h, b.h, None, abar.h, bbar.h, None)))
    one_ms, _ = timed(lambda: _lib.check(L.ttn_dot_pullback(a.h, b.h, None, abar.h, None, None)))
    f_chain = chain_flops(dims, ra, rb)
    f_both = 2 * f_chain + sandwich_flops(dims, ra, rb) + sandwich_flops(dims, rb, ra)
    f_one = 2 * f_chain + sandwich_flops(dims, ra, rb)
    case = {"case": name, "batch": batch, "d": len(dims), "max_rank_a": max(ra), "max_rank_b": max(rb), "reps": reps,
            "dot_kernel_ms": dot_ms, "pullback_both_ms": both_ms, "pullback_abar_ms": one_ms,
            "ratio_both_to_dot": both_ms / dot_ms, "ratio_abar_to_dot": one_ms / dot_ms,
            "flops_dot": f_chain, "flops_both": f_both, "flops_abar": f_one,
            "dot_fraction_of_fp64_peak": batch * f_chain / (dot_ms * 1e-3) / PEAK_F64,
            "both_fraction_of_fp64_peak": batch * f_both / (both_ms * 1e-3) / PEAK_F64,
            "abar_fraction_of_fp64_peak": batch * f_one / (one_ms * 1e-3) / PEAK_F64,
            "workspace_bytes_per_train": workspace_bytes(dims, ra, rb), "workspace_bytes": batch * workspace_bytes(dims, ra, rb)}
    print(json.dumps(case), flush=True)
    rec["cases"].append(case)
    for h in (abar, bbar):
        h.free()


def apply_case(A, dA, x, batch, rec):
    L = _lib.lib()
    dims, rx = x.dims, x.max_ranks()
    ry = [R * r for R, r in zip(A.tto_rks, rx)]
    y, xbar = T.DeviceTT(dims, ry, batch), T.DeviceTT(dims, x.cap, batch)
    apply_ms, reps = timed(lambda: _lib.check(L.ttn_apply(dA.h, x.h, y.h)))
    pb_ms, _ = timed(lambda: _lib.check(L.ttn_apply_pullback(dA.h, x.h, y.h, xbar.h)))          # (A x as the cotangent: any data of the right ranks)
    by = 8 * sum(dims[k] * ry[k] * ry[k + 1] for k in range(len(dims)))
    bx = 8 * sum(dims[k] * rx[k] * rx[k + 1] for k in range(len(dims)))
    case = {"case": "apply_pullback vs apply", "batch": batch, "d": len(dims), "max_rank_x": max(rx), "reps": reps,
            "apply_ms": apply_ms, "apply_pullback_ms": pb_ms, "ratio_pullback_to_apply": pb_ms / apply_ms,
            "bytes_per_train": by + bx,
            "apply_fraction_of_8TBs": batch * (by + bx) / (apply_ms * 1e-3) / PEAK_BW,
            "apply_pullback_fraction_of_8TBs": batch * (by + bx) / (pb_ms * 1e-3) / PEAK_BW}
    print(json.dumps(case), flush=True)
    rec["cases"].append(case)
    return y, xbar


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=30)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_grad.json"))
    args = ap.parse_args()
    T.ensure_init(0)
    dims = (2,) * args.d
    A = T.Delta(args.d)
    dA = T.DeviceTTO(A)
    rec = {"tool": "tools/diag_grad.py", "d": args.d, "rank": args.rank, "peak_fp64_flops": PEAK_F64, "peak_bytes_per_s": PEAK_BW, "cases": []}
    for batch in args.batches:
        a = T.DeviceTT.from_host(T.rand_tt(dims, args.rank, seed=1), batch)
        b = T.DeviceTT.from_host(T.rand_tt(dims, args.rank, seed=2), batch)
        dot_cases("rank %d against rank %d" % (args.rank, args.rank), a, b, batch, rec)
        y, xbar = apply_case(A, dA, a, batch, rec)
        if batch <= 256:
            dot_cases("(psi, Delta psi)", a, y, batch, rec)
        for h in (a, b, y, xbar):
            h.free()
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
