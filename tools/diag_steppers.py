"""Diagnostic of the stepper kernels, written to profiles/diag_steppers.json.

1. z = x + beta (A x) on C3-shaped trains (d = 30, rank 64, A = Delta(30)) at B = 256: the fused k_apply_axpby against, in the same
   process, the four-launch composition it replaces (ttn_apply -> ttn_scale_batch -> ttn_scale_batch -> ttn_add), and k_apply and k_add
   alone, and the three launches euler_method ran before (apply, scale with one factor, add).  HIP events on the library's stream
   around windows of back-to-back calls, every shape warmed up, the versions alternated, 5 windows each: best and median.  Fractions of 8 TB/s are on each kernel's OWN algorithmic bytes (cores read + cores written, once
   each; x counted once where x is y).
2. One Crank-Nicolson / ALS step at d = 20, rank 16, B = 256, split into operator build, right-hand side, solve and round (host clock
   around stages that end in a stream synchronise; 5 repetitions after a warm-up: best and median).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ttn_amd as T                                   # noqa: E402
from ttn_amd import device as D                       # noqa: E402
from ttn_amd import solvers as S                      # noqa: E402

HBM_PEAK = 8.0e12


def window(fn, reps):
    """ms per call of `reps` back-to-back calls between two events on the library's stream"""
    D.event_record(0)
    for _ in range(reps):
        fn()
    D.event_record(1)
    D.sync()
    return D.event_elapsed_ms(0, 1) / reps


def alternate(fns, target_s=0.15, windows=5):
    """{name: [ms per call of every window]}: warm-up of every version, then `windows` rounds over the versions in turn"""
    reps = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        D.sync()
        reps[name] = int(max(3, min(500, target_s * 1e3 / max(window(fn, 3), 1e-3))))
    out = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            out[name].append(window(fn, reps[name]))
    return out


def summary(ms, nbytes):
    best, med = min(ms), statistics.median(ms)
    return {"windows_ms": [round(v, 4) for v in ms], "best_ms": round(best, 4), "median_ms": round(med, 4), "algorithmic_bytes": nbytes,
            "frac_of_8TBs_best": round(nbytes / (best * 1e-3) / HBM_PEAK, 4), "frac_of_8TBs_median": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}


def fused_vs_composition(d, r, B, beta):
    dims = (2,) * d
    A = T.Delta(d)
    dA = T.DeviceTTO(A)
    xr = list(T.rand_tt(dims, r, seed=30).ttv_rks)
    x = T.DeviceTT(dims, xr, batch=B)
    for b in range(B):
        x.upload(b, T.rand_tt(dims, r, seed=30 + b))
    tr = [a * c for a, c in zip(A.tto_rks, xr)]
    zr = [1] + [p + q for p, q in zip(xr[1:-1], tr[1:-1])] + [1]
    t, t2, x2 = T.DeviceTT(dims, tr, B), T.DeviceTT(dims, tr, B), T.DeviceTT(dims, xr, B)
    z, zc = T.DeviceTT(dims, zr, B), T.DeviceTT(dims, zr, B)
    ones, betas = [1.0] * B, [beta] * B
    cb = lambda rk: 8.0 * sum(2 * rk[k] * rk[k + 1] for k in range(d))                    # noqa: E731
    a_bytes = 8.0 * sum(c.size for c in A.tto_vec)

    def composition():
        D.apply(dA, x, t)
        D.scale_batch(betas, t, t2)
        D.scale_batch(ones, x, x2)
        D.add(x2, t2, zc)

    def three_launches():                              # what euler_method ran before: apply, scale (one factor, no upload), add
        D.apply(dA, x, t)
        D.scale(beta, t, t2)
        D.add(x, t2, zc)

    ms = alternate({"fused": lambda: D.apply_axpby(None, x, beta, dA, x, z), "composition": composition, "three_launches": three_launches,
                    "k_apply": lambda: D.apply(dA, x, t), "k_add": lambda: D.add(x2, t2, zc)})
    same = all(z.ranks(b) == zc.ranks(b) and all((g == c).all() for g, c in zip(z.download(b).ttv_vec, zc.download(b).ttv_vec)) for b in (0, B - 1))
    nbytes = {"fused": B * (cb(xr) + cb(zr)) + a_bytes,
              "composition": B * ((cb(xr) + cb(tr)) + 2 * cb(tr) + 2 * cb(xr) + (cb(xr) + cb(tr) + cb(zr))) + a_bytes,
              "three_launches": B * ((cb(xr) + cb(tr)) + 2 * cb(tr) + (cb(xr) + cb(tr) + cb(zr))) + a_bytes,
              "k_apply": B * (cb(xr) + cb(tr)) + a_bytes, "k_add": B * (cb(xr) + cb(tr) + cb(zr))}
    res = {name: summary(v, nbytes[name]) for name, v in ms.items()}
    comp, fus = res["composition"], res["fused"]
    res["shape"] = {"d": d, "rank": r, "batch": B, "operator": "Delta(%d)" % d, "z_ranks_max": max(zr), "beta": beta}
    res["bit_identical_trains_0_and_last"] = bool(same)
    res["speedup_median"] = round(comp["median_ms"] / fus["median_ms"], 3)
    res["composition_best_to_median_spread_ms"] = round(comp["median_ms"] - comp["best_ms"], 4)
    res["accepted"] = bool(fus["median_ms"] <= comp["median_ms"] + (comp["median_ms"] - comp["best_ms"]))
    for h in (x, t, t2, x2, z, zc, dA):
        h.free()
    return res


def crank_nicholson_als_step(d, r, B, h=0.05, reps=5):
    dims = (2,) * d
    A = S._tto_scale(-(1.0 / d ** 2) ** 2, T.toeplitz_to_qtto(-2.0, 1.0, 1.0, d))
    dA, dI = T.DeviceTTO(A), T.DeviceTTO(T.id_tto(d))
    u0 = T.rand_tt(dims, r, seed=40)
    ur = list(u0.ttv_rks)
    u = T.DeviceTT(dims, ur, batch=B)
    for b in range(B):
        u.upload(b, T.rand_tt(dims, r, seed=40 + b))
    stages = {"operator_build": [], "right_hand_side": [], "solve": [], "round": [], "step": []}

    def clock(name, fn):
        D.sync()
        t0 = time.perf_counter()
        out = fn()
        D.sync()
        stages[name].append((time.perf_counter() - t0) * 1e3)
        return out

    def build():
        cA = dA.scale(h / 2)
        M = dI.sub(cA)
        cA.free()
        return M

    for it in range(reps + 1):
        if it == 1:                                    # the first pass is the warm-up
            for v in stages.values():
                v.clear()
        t0 = time.perf_counter()
        M = clock("operator_build", build)
        rhs, _ = clock("right_hand_side", lambda: S._axpby(None, u, ur, h / 2, dA, u, ur))
        nxt = clock("solve", lambda: S.als_linsolve_(M, rhs, u, T.DeviceTT(dims, ur, B), 2))
        v = clock("round", lambda: S._round(S._Vec(nxt, nxt.max_ranks()), 0))
        D.status_all()
        stages["step"].append((time.perf_counter() - t0) * 1e3)
        for hd in (M, rhs, v.h):
            hd.free()
    out = {name: {"ms": [round(x, 3) for x in v], "best_ms": round(min(v), 3), "median_ms": round(statistics.median(v), 3)} for name, v in stages.items()}
    out["shape"] = {"d": d, "rank": r, "batch": B, "step_size": h, "tt_solver": "als", "sweep_count": 2, "rhs_ranks_max": max(ur) * 4}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_steppers.json"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--kernel-only", action="store_true", help="part 1 alone (experiment builds of the kernel through TTN_LIB)")
    args = ap.parse_args()
    T.ensure_init(0)
    B = args.batch
    res = {"fused_vs_composition": fused_vs_composition(8, 4, 4, 0.025) if args.small else fused_vs_composition(30, 64, B, 0.025)}
    if not args.kernel_only:
        res["crank_nicholson_als_step"] = crank_nicholson_als_step(6, 4, 4) if args.small else crank_nicholson_als_step(20, 16, B)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
