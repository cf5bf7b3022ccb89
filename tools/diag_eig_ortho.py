"""Diagnostic (not a test): the cost of the penalty of the excited-state solvers (csrc/ttn_eig_ortho_kernels.h).  dmrg_eigsolve on
ising_tto(32; J = 1, h = 1.5), schedule [2, 3] / [16, 32] (the shape of tools/diag_eigsolve.py), B = 1 and B = 64, with n_ortho = 0
(through ttn_dmrg_eigsolve_ortho), 1 and 3 next to the plain ttn_dmrg_eigsolve.  The penalty trains are the lowest states themselves
(level j against levels 0 .. j-1), so n_ortho = 1 is the search for level 1 and n_ortho = 3 that for level 3.  HIP events on the library
stream around the call, one warm-up, best of 5; the five plain times give the run-to-run spread.  Prints one JSON object; with a path
argument it is also written there.
    python tools/diag_eig_ortho.py [out.json] [--plain-only] [--yardstick other.json]
--plain-only measures only the plain entry point, with nothing of the penalised interface touched: run from a checkout of the parent
commit it yields the yardstick, which --yardstick then folds into the report as ratios."""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import ttn_amd as T
from oracle import tt_oracle as O
from tests.helpers import to_product

args = [a for a in sys.argv[1:] if not a.startswith("--")]
plain_only = "--plain-only" in sys.argv
yard = sys.argv[sys.argv.index("--yardstick") + 1] if "--yardstick" in sys.argv else None
if yard in args:
    args.remove(yard)
out = args[0] if args else None
d, BIG, REPS = 32, 64, 5
dims = (2,) * d
sched, rmaxs = [2, 3], [16, 32]
T.ensure_init(0)
dA = T.DeviceTTO(T.ising_tto(d, J=1.0, h=1.5))
rng = np.random.default_rng(3)
x0s = [O.rand_tt(dims, 2, rng) for _ in range(BIG)]
cap = T.solvers.dmrg_capacity(dims, x0s[0].ttv_rks, max(rmaxs))
res = {"problem": "dmrg_eigsolve(ising_tto(32; J=1, h=1.5))", "sweep_schedule": sched, "rmax_schedule": rmaxs, "reps": REPS, "weight": 10.0}


def starts(batch):
    h = T.DeviceTT(dims, x0s[0].ttv_rks, batch=batch)
    for i in range(batch):
        h.upload(i, to_product(x0s[i]))
    return h


def timed(call, batch):
    """Best and all of REPS event times of `call` after one warm-up, with the Lanczos statistics of the last run."""
    call()
    ms = []
    for _ in range(REPS):
        with T.StreamTimer() as t:
            ret = call()
        ms.append(t.ms)
    it, lres = T.solvers.eigsolve_stats(batch)
    return {"ms_best": min(ms), "ms_all": ms, "spread": (max(ms) - min(ms)) / min(ms), "micro_steps": len(ret[0][0]),
            "lanczos_applies_train0": it[0], "lanczos_applies_mean": float(np.mean(it)), "max_lanczos_residual": max(lres)}


for batch in (1, BIG):
    dx0 = starts(batch)
    xs = [T.DeviceTT(dims, cap, batch=batch) for _ in range(4)]
    r = {"plain": timed(lambda: T.solvers.dmrg_eigsolve_(dA, dx0, xs[0], 1e-12, sched, rmaxs, linsolv_tol=1e-10), batch)}
    if not plain_only:
        for m in (0, 1, 2, 3):                                # level m against the levels below it (m = 2 only builds level 2)
            key = "n_ortho_%d" % m
            r[key] = timed(lambda: T.solvers.dmrg_eigsolve_(dA, dx0, xs[m], 1e-12, sched, rmaxs, linsolv_tol=1e-10, ortho_to=xs[:m],
                                                            weight=10.0 if m else None), batch)
            r[key]["energy_train0"] = float(T.device.rayleigh(dA, xs[m])[0])
            base = r["plain"]
            r[key]["ms_per_micro_step_ratio"] = r[key]["ms_best"] / base["ms_best"]
            r[key]["ms_per_lanczos_apply_ratio"] = (r[key]["ms_best"] / r[key]["lanczos_applies_mean"]) / (base["ms_best"] / base["lanczos_applies_mean"])
            r[key]["extra_lanczos_applies_mean"] = r[key]["lanczos_applies_mean"] - base["lanczos_applies_mean"]
    res["B%d" % batch] = r
    for h in [dx0] + xs:
        h.free()
if yard:
    with open(yard) as f:
        y = json.loads(f.readline())
    for batch in (1, BIG):
        p, r = y["B%d" % batch]["plain"], res["B%d" % batch]
        r["yardstick_plain"] = p
        for key in [k for k in r if k.startswith("n_ortho_") or k == "plain"]:
            r[key]["ms_ratio_to_yardstick"] = r[key]["ms_best"] / p["ms_best"]
line = json.dumps(res)
print(line)
if out:
    with open(out, "w") as f:
        f.write(line + "\n")
