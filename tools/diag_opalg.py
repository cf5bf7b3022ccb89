"""Diagnostic of the TT operator algebra, written to profiles/diag_opalg.json:

1. k_tto_mul alone on a product whose output is about 1.1 GB: the raw rank-28 Ornstein2D_coupled generator at d = 30 bits per axis
   (60 sites) times itself.  HBM bytes = both operands read once + the output written once, over the kernel's HIP-event time
   (ttn_last_launch_ms), as a fraction of 8 TB/s.
2. In the same run k_apply (Δ(30) on rank-64 trains) on a batch that writes the same number of bytes: the yardstick, same access pattern.
3. The d = 8 assembly + rounding chain of the generator: device wall time next to the NumPy restatement's (tests/opalg_reference.py).

--label tags the record (the K sweep runs this tool once per build of the library with another TTN_TTOMUL_K, selected by TTN_LIB);
--skip-chain leaves part 3 out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ttn_amd as T                                   # noqa: E402
from tests import opalg_reference as R                # noqa: E402
from tests.test_gpu_opalg import DeviceOps            # noqa: E402
from ttn_amd import device as D                       # noqa: E402

PEAK = 8.0e12


def core_bytes(dims, rks):
    return 8 * sum(n * n * a * b for n, a, b in zip(dims, rks[:-1], rks[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="default")
    ap.add_argument("--bits", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-chain", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_opalg.json"))
    a = ap.parse_args()
    T.ensure_init(0)
    rec = {"label": a.label, "lib": os.path.basename(T._lib.LIB_PATH), "bits_per_axis": a.bits, "peak_bytes_per_s": PEAK}

    # 1. k_tto_mul
    G = R.ornstein2d_coupled(a.bits, DeviceOps)
    out_rks = [r * r for r in G.ranks()]
    out_bytes, in_bytes = core_bytes(G.dims, out_rks), 2 * core_bytes(G.dims, G.ranks())
    ms = []
    for i in range(a.reps + 1):                        # the first is the warm-up
        P = G.mul(G)
        if i:
            ms.append(D.last_launch_ms())
        else:
            D.sync()
        P.free()
    t = min(ms) * 1e-3
    rec["tto_mul"] = {"ranks": [G.ranks()[1], G.ranks()[len(G.dims) // 2]], "sites": len(G.dims), "out_bytes": out_bytes, "in_bytes": in_bytes,
                      "ms": ms, "ms_best": min(ms), "fraction_of_peak": (out_bytes + in_bytes) / t / PEAK}

    # 2. k_apply writing the same number of bytes
    d, r = 30, 64
    A = T.Delta(d)
    x = T.rand_tt((2,) * d, r, seed=30)
    ycap = [p * q for p, q in zip(A.tto_rks, x.ttv_rks)]
    by = 8 * sum(2 * p * q for p, q in zip(ycap[:-1], ycap[1:]))
    bx = 8 * sum(2 * p * q for p, q in zip(x.ttv_rks[:-1], x.ttv_rks[1:]))
    B = max(1, round(out_bytes / by))
    dA, dx = T.DeviceTTO(A), T.DeviceTT.from_host(x, batch=B)
    dy = T.DeviceTT((2,) * d, ycap, batch=B)
    ms = []
    for i in range(a.reps + 1):
        with D.StreamTimer() as tm:
            D.apply(dA, dx, dy)
        if i:
            ms.append(tm.ms)
    t = min(ms) * 1e-3
    rec["apply"] = {"batch": B, "out_bytes": by * B, "in_bytes": bx * B, "ms": ms, "ms_best": min(ms), "fraction_of_peak": (by + bx) * B / t / PEAK}
    rec["tto_mul_over_apply"] = rec["tto_mul"]["fraction_of_peak"] / rec["apply"]["fraction_of_peak"]
    for h in (dA, dx, dy, G):
        h.free()

    # 3. the d = 8 chain
    if not a.skip_chain:
        def device_chain():
            C = R.ornstein2d_coupled(8, DeviceOps).compress(truncerr=1e-6)
            D.sync()
            return C.ranks()
        device_chain()
        t0 = time.perf_counter()
        rk = device_chain()
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        rk_ref = R.tto_compress(R.ornstein2d_coupled(8, R.HostOps), truncerr=1e-6).tto_rks
        t_ref = time.perf_counter() - t0
        rec["chain_d8"] = {"device_wall_ms": 1e3 * t_dev, "numpy_wall_ms": 1e3 * t_ref, "ranks": rk, "ranks_equal": rk == rk_ref}
    D.status_all()
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
