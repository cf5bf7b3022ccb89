"""Diagnostic (not a test): als_eigsolve on the transverse-field Ising chain ising_tto(32; J = 1, h = 1.5) at rank 16 with
sweep_schedule [3] (two full sweeps, local problems up to 2 * 16 * 16 = 512 unknowns: the dense branch), one train (B = 1) and 64
different start trains in one call (B = 64), next to the NumPy restatement (tests/als_eig_reference.py) for one train.  Prints one JSON
object; with a path argument it is also written there.
    python tools/diag_als_eig.py [out.json] [rank] [batch]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import ttn_amd as T
from oracle import tt_oracle as O
from tests import als_eig_reference as AR
from tests import eig_reference as ER
from tests.helpers import to_oracle, to_product

out = sys.argv[1] if len(sys.argv) > 1 else None
rank = int(sys.argv[2]) if len(sys.argv) > 2 else 16
B = int(sys.argv[3]) if len(sys.argv) > 3 else 64
d = 32
sched = [3]
T.ensure_init(0)
A = T.ising_tto(d, J=1.0, h=1.5)
exact = ER.free_fermion_ground_energy(d, 1.0, 1.5)
rng = np.random.default_rng(3)
x0s = [O.rand_tt((2,) * d, rank, rng) for _ in range(B)]
dA = T.DeviceTTO(A)
rks = x0s[0].ttv_rks
res = {"problem": "als_eigsolve(ising_tto(32; J=1, h=1.5))", "rank": rank, "sweep_schedule": sched, "exact_E0": exact}


def run(batch):
    dx0 = T.DeviceTT((2,) * d, rks, batch=batch)
    for i in range(batch):
        dx0.upload(i, to_product(x0s[i]))
    dx = T.DeviceTT((2,) * d, rks, batch=batch)
    T.solvers.als_eigsolve_(dA, dx0, dx, sched)                     # warm-up (allocations, code load)
    t = time.perf_counter()
    E = T.solvers.als_eigsolve_(dA, dx0, dx, sched)                 # synchronises
    dt = time.perf_counter() - t
    dx0.free(); dx.free()
    return dt, E


for batch in (1, B):
    dt, E = run(batch)
    res[f"B{batch}"] = {"seconds": dt, "seconds_per_train": dt / batch, "micro_steps": len(E[0]),
                        "worst_rel_err_E0": max(abs(e[-1] - exact) / abs(exact) for e in E)}
t = time.perf_counter()
Ec, xc = AR.als_eigsolve(to_oracle(A), x0s[0], sweep_schedule=sched)
res["cpu_restatement_one_train"] = {"seconds": time.perf_counter() - t, "rel_err_E0": abs(Ec[-1] - exact) / abs(exact)}
res["gpu_B%d_speedup_per_train_vs_cpu" % B] = res["cpu_restatement_one_train"]["seconds"] / res[f"B{B}"]["seconds_per_train"]
line = json.dumps(res)
print(line)
if out:
    with open(out, "w") as f:
        f.write(line + "\n")
