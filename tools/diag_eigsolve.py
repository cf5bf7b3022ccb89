"""Diagnostic (not a test): dmrg_eigsolve on the transverse-field Ising chain ising_tto(32; J = 1, h = 1.5) with rank 32 (local problems
up to 4096 unknowns: the matrix-free Lanczos branch), one train (B = 1) and 64 different start trains in one call (B = 64), next to the
NumPy restatement (tests/eig_reference.py) for one train.  Prints one JSON object; with a path argument it is also written there.
    python tools/diag_eigsolve.py [out.json] [rmax] [batch]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import ttn_amd as T
from oracle import tt_oracle as O
from tests import eig_reference as ER
from tests.helpers import to_oracle, to_product

out = sys.argv[1] if len(sys.argv) > 1 else None
rmax = int(sys.argv[2]) if len(sys.argv) > 2 else 32
B = int(sys.argv[3]) if len(sys.argv) > 3 else 64
d = 32
sched, rmaxs = [2, 3], [rmax // 2, rmax]
T.ensure_init(0)
A = T.ising_tto(d, J=1.0, h=1.5)
exact = ER.free_fermion_ground_energy(d, 1.0, 1.5)
rng = np.random.default_rng(3)
x0s = [O.rand_tt((2,) * d, 2, rng) for _ in range(B)]
dA = T.DeviceTTO(A)
cap = T.solvers.dmrg_capacity((2,) * d, x0s[0].ttv_rks, rmax)
res = {"problem": "dmrg_eigsolve(ising_tto(32; J=1, h=1.5))", "sweep_schedule": sched, "rmax_schedule": rmaxs, "exact_E0": exact}


def run(batch):
    dx0 = T.DeviceTT((2,) * d, x0s[0].ttv_rks, batch=batch)
    for i in range(batch):
        dx0.upload(i, to_product(x0s[i]))
    dx = T.DeviceTT((2,) * d, cap, batch=batch)
    T.solvers.dmrg_eigsolve_(dA, dx0, dx, 1e-12, sched, rmaxs, linsolv_tol=1e-10)        # warm-up (allocations, code load)
    t = time.perf_counter()
    E, R = T.solvers.dmrg_eigsolve_(dA, dx0, dx, 1e-12, sched, rmaxs, linsolv_tol=1e-10)   # synchronises
    dt = time.perf_counter() - t
    it, lres = T.solvers.eigsolve_stats(batch)
    dx0.free(); dx.free()
    return dt, E, R, it, lres


for batch in (1, B):
    dt, E, R, it, lres = run(batch)
    res[f"B{batch}"] = {"seconds": dt, "seconds_per_train": dt / batch, "micro_steps": len(E[0]), "max_rank": max(R[0]),
                        "worst_rel_err_E0": max(abs(e[-1] - exact) / abs(exact) for e in E), "lanczos_applies_train0": it[0],
                        "max_lanczos_residual": max(lres)}
t = time.perf_counter()
Ec, xc, Rc = ER.dmrg_eigsolve(to_oracle(A), x0s[0], tol=1e-12, sweep_schedule=sched, rmax_schedule=rmaxs, linsolv_tol=1e-10)
res["cpu_restatement_one_train"] = {"seconds": time.perf_counter() - t, "rel_err_E0": abs(Ec[-1] - exact) / abs(exact)}
res["gpu_B%d_speedup_per_train_vs_cpu" % B] = res["cpu_restatement_one_train"]["seconds"] / res[f"B{B}"]["seconds_per_train"]
line = json.dumps(res)
print(line)
if out:
    with open(out, "w") as f:
        f.write(line + "\n")
