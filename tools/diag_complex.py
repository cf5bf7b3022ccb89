"""Diagnostic of the ComplexF64 kernels, written to profiles/diag_complex.json.  HIP events on the library stream,
a warm-up of every shape, best of --reps:

1. k_zapply: fourier_qtto(30; K = 25) on a batch of complex rank-16 trains sized so that one launch writes at least 1 GB; achieved
   bytes/s = (operator cores + input cores read + output cores written, once each) / time, as a fraction of 8 TB/s — beside k_apply
   for Δ(30) on rank-64 trains on a batch that writes about as much, in the same run.
2. complex tt_compress_: ms per launch at B = 1 and B = 256 for the shape of examples/dft.jl (d = 10, K = 50, max_bond = 100) and for
   d = 20, K = 25, a rank-8 complex input, max_bond = 32.  Beside it (i) the same sweep driven from the host with one
   ttn_dense_svd(cplx = 1) per bond (the only complex two-site SVD the library had before: what tdvp2sweep_ does), B = 1, wall
   clock; (ii) the oracle on the host's CPUs the way bench.py's cpu_baseline measures (one train per process, one BLAS thread),
   scaled to B trains.

--section picks one part (each part of a GPU visit runs as its own process under its own time limit); --label tags a record (the K
sweep of k_zapply runs part 1 once per build of the library with another TTN_ZAPPLY_K, selected by TTN_LIB); records are merged into
the output file by label and section."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                    # noqa: E402

import ttn_amd as T                                   # noqa: E402
from ttn_amd import device as D                       # noqa: E402

PEAK = 8.0e12


def crand_tt(d, r, seed):
    rng = np.random.default_rng(seed)
    rks = T.r_and_d_to_rks([r] * (d + 1), (2,) * d)
    vec = [np.asfortranarray(rng.standard_normal((2, rks[k], rks[k + 1])) + 1j * rng.standard_normal((2, rks[k], rks[k + 1]))) for k in range(d)]
    return T.TTvector(d, vec, (2,) * d, rks, [0] * d)


def timed(fn, reps):
    ms = []
    for i in range(reps + 1):                          # the first is the warm-up
        with D.StreamTimer() as tm:
            fn()
        if i:
            ms.append(tm.ms)
    return ms


def section_zapply(a):
    rec = {}
    d = 30
    F = T.fourier_qtto(d, K=25)
    x = crand_tt(d, 16, 30)
    yr = [p * q for p, q in zip(F.tto_rks, x.ttv_rks)]
    by = 16 * sum(2 * p * q for p, q in zip(yr[:-1], yr[1:]))
    bx = 16 * sum(2 * p * q for p, q in zip(x.ttv_rks[:-1], x.ttv_rks[1:]))
    bA = 16 * sum(4 * p * q for p, q in zip(F.tto_rks[:-1], F.tto_rks[1:]))
    B = max(1, math.ceil(1.0e9 / by))
    dF, dx = D.DeviceTTO(F), D.DeviceTT.from_host(x, batch=B)
    dy = D.DeviceTT((2,) * d, yr, B, dtype=np.complex128)
    ms = timed(lambda: D.apply(dF, dx, dy), a.reps)
    D.status_all()
    rec["zapply"] = {"d": d, "K": 25, "rank": 16, "batch": B, "bytes_written": B * by, "bytes_read": B * bx + bA, "ms": ms, "ms_best": min(ms),
                     "fraction_of_peak": (B * (by + bx) + bA) / (min(ms) * 1e-3) / PEAK}
    dy.free(); dx.free(); dF.free()
    # the yardstick: k_apply, Δ(30) on rank-64 trains, about as many bytes written
    A = T.Delta(d)
    xr = T.rand_tt((2,) * d, 64, seed=30)
    yr = [p * q for p, q in zip(A.tto_rks, xr.ttv_rks)]
    by2 = 8 * sum(2 * p * q for p, q in zip(yr[:-1], yr[1:]))
    bx2 = 8 * sum(2 * p * q for p, q in zip(xr.ttv_rks[:-1], xr.ttv_rks[1:]))
    B2 = max(1, round(B * by / by2))
    dA, dx = D.DeviceTTO(A), D.DeviceTT.from_host(xr, batch=B2)
    dy = D.DeviceTT((2,) * d, yr, B2)
    ms = timed(lambda: D.apply(dA, dx, dy), a.reps)
    rec["apply_real"] = {"d": d, "rank": 64, "batch": B2, "bytes_written": B2 * by2, "bytes_read": B2 * bx2, "ms": ms, "ms_best": min(ms),
                         "fraction_of_peak": B2 * (by2 + bx2) / (min(ms) * 1e-3) / PEAK}
    rec["zapply_over_apply"] = rec["zapply"]["fraction_of_peak"] / rec["apply_real"]["fraction_of_peak"]
    return rec


def compress_shapes():
    from tests import fourier_reference as FR
    _, f = FR.spikes_problem(10, 50, 12)
    return {"dft": lambda: (T.fourier_qtto(10, K=50), T.function_to_qtt_uniform(f, 10), 100),
            "d20_r8": lambda: (T.fourier_qtto(20, K=25), crand_tt(20, 8, 20), 32)}


def section_compress(a):
    F, x, mb = compress_shapes()[a.shape]()
    y = T.apply(F, x)                                   # the raw product, formed once
    need = D.compress_rank_bound(y.ttv_dims, y.ttv_rks, mb)[0]
    out = {"d": y.N, "max_bond": mb, "raw_ranks_max": max(y.ttv_rks)}
    for B in (1, 256):
        src = D.DeviceTT.from_host(y, batch=B, cap_rks=need)
        work = D.DeviceTT(y.ttv_dims, need, B, dtype=np.complex128)
        ms = []
        for i in range(a.reps + 1):
            T._lib.check(T._lib.lib().ttn_tt_copy(work.h, src.h))       # the rounding is in place: every repetition starts from the raw product
            with D.StreamTimer() as tm:
                D.tt_compress_(work, mb)
            if i:
                ms.append(tm.ms)
        sweeps = D.compress_status(work)
        out["B%d" % B] = {"ms": ms, "ms_best": min(ms), "ranks": work.ranks(0)[0], "jacobi_sweeps_train0": sweeps[0]}
        work.free(); src.free()
    return {"compress_" + a.shape: out}


def section_host_svd(a):
    """(i) the sweep of tt_compress! with the merged matrix formed by torch and one ttn_dense_svd(cplx = 1) per bond, B = 1"""
    import torch
    from ttn_amd import tdvp as TD
    F, x, mb = compress_shapes()[a.shape]()
    y = T.apply(F, x)
    dev = torch.device("cuda:0")

    def run():
        cores = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in y.ttv_vec]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = len(cores)
        for k in list(range(d - 1)) + list(range(d - 2, -1, -1)):
            A, Bc = cores[k], cores[k + 1]
            n1, Dl, _ = A.shape
            n2, _, Dr = Bc.shape
            M = torch.einsum("sag,tgb->sabt", A, Bc).reshape(n1 * Dl, Dr * n2)          # the oracle's layout of the merged matrix
            Ut, s, Vtt = TD._svd_j(M.transpose(0, 1).contiguous())
            s = torch.as_tensor(s, device=dev)
            r = min(int(s.shape[0]), mb)
            sq = torch.sqrt(s[:r]).to(M.dtype)
            U = Ut[:r, :].transpose(0, 1) * sq[None, :]
            Vt = sq[:, None] * Vtt[:, :r].transpose(0, 1)
            cores[k] = U.reshape(n1, Dl, r).contiguous()
            cores[k + 1] = Vt.reshape(r, Dr, n2).permute(2, 0, 1).contiguous()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, [1] + [int(c.shape[2]) for c in cores]

    run()
    res = [run() for _ in range(min(a.reps, 3))]
    return {"host_svd_" + a.shape: {"ms": [r_[0] for r_ in res], "ms_best": min(r_[0] for r_ in res), "ranks": res[0][1]}}


def _cpu_worker(shape):
    from threadpoolctl import threadpool_limits
    from oracle import tt_oracle as O
    from tests.helpers import to_oracle
    with threadpool_limits(limits=1):
        F, x, mb = compress_shapes()[shape]()
        y = O.apply(to_oracle(F), to_oracle(x))
        t0 = time.perf_counter()
        O.tt_compress_(O.copy_tt(y), mb)
        return time.perf_counter() - t0


def section_cpu(a):
    """(ii) bench.py's cpu_baseline method: one train per process, one BLAS thread, as many processes as this job may use"""
    import multiprocessing as mp
    cores = max(1, len(os.sched_getaffinity(0)))
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and int(omp) > 0:
        cores = min(cores, int(omp))
    ctx = mp.get_context("spawn")
    with ctx.Pool(cores) as pool:
        pool.map(_cpu_worker, [a.shape] * cores)       # warm the workers
        t0 = time.perf_counter()
        per = pool.map(_cpu_worker, [a.shape] * cores)
        wall = time.perf_counter() - t0
    return {"cpu_" + a.shape: {"processes": cores, "s_per_train_one_thread": float(np.mean(per)), "ms_B1": 1e3 * float(np.min(per)),
                               "ms_B256": 1e3 * float(np.max(per)) * math.ceil(256 / cores), "wall_s_incl_setup": wall}}


SECTIONS = {"zapply": section_zapply, "compress": section_compress, "host_svd": section_host_svd, "cpu": section_cpu}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=sorted(SECTIONS), required=True)
    ap.add_argument("--shape", choices=["dft", "d20_r8"], default="dft")
    ap.add_argument("--label", default="default")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_complex.json"))
    a = ap.parse_args()
    if a.section == "host_svd":
        import torch
        torch.cuda.is_available()                      # (asked before the library touches the device, as tdvp._dev does)
    if a.section != "cpu":
        T.ensure_init(0)
    rec = SECTIONS[a.section](a)
    commit = ""
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        pass
    allrec = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            allrec = json.load(fh)
    allrec.setdefault(a.label, {"lib": os.path.basename(T._lib.LIB_PATH), "peak_bytes_per_s": PEAK, "parent_commit": commit}).update(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(allrec, fh, indent=1, sort_keys=True)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
