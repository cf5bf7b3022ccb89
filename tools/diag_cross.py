"""Diagnostic (not a test): where the time of a TT-cross goes.  Each case runs tt_cross once to warm up, then once with HIP event pairs
around the parts of every half sweep (f, gathers and index updates, QR / SVD, maxvol, evaluation), summed over the run, next to the
wall time and the NumPy restatement's CPU time (tests/cross_reference.py) on the same machine.  Cases: README example 2 (MaxVol and
DMRG), a 5-D random tensor whose fibres take the global-memory maxvol route (rmax 60, 24 points per axis, two sweeps), and the
d = 30 QTT of sin(pi^2 x).  Prints one JSON object; with a path argument it is also written there.
    python tools/diag_cross.py [out.json]"""
import json
import math
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import ttn_amd as T
from tests import cross_reference as R

out = sys.argv[1] if len(sys.argv) > 1 else None
torch, _ = T.tdvp._dev()                     # (asks torch for the GPU before the library binds it)

TABLE5 = np.random.default_rng(55).uniform(-1.0, 1.0, (24,) * 5)
W30 = np.array([2.0 ** (30 - k) / (2 ** 30 - 1) for k in range(1, 31)])


def gauss(X):
    return np.exp(-np.sum(np.asarray(X) ** 2, axis=1))


def rand5(X):
    i = np.rint(np.asarray(X) * 23.0).astype(np.int64)
    return TABLE5[i[:, 0], i[:, 1], i[:, 2], i[:, 3], i[:, 4]]


def sin30(X):
    return np.sin(math.pi ** 2 * (np.asarray(X) @ W30))


def sin30_t(X):
    return torch.sin(math.pi ** 2 * (X @ torch.from_numpy(W30).to(X.device)))


CASES = [
    ("readme2-maxvol", "maxvol", gauss, gauss, [np.linspace(-1, 1, 8)] * 4, dict(tol=1e-8), dict(ranks=2)),
    ("readme2-dmrg", "dmrg", gauss, gauss, [np.linspace(-1, 1, 8)] * 4, dict(tol=1e-8), dict(ranks=2)),
    ("global-route-5d-maxvol", "maxvol", rand5, rand5, [np.linspace(0, 1, 24)] * 5, dict(tol=1e-10, maxiter=2, rmax=60, kickrank=None),
     dict(ranks=[24, 60, 24, 6], seed=2)),
    ("qtt-sin-d30-maxvol", "maxvol", sin30_t, sin30, [np.array([0.0, 1.0])] * 30, dict(tol=1e-10, maxiter=3, kickrank=None), dict(ranks=2)),
]
res = {"note": "event-pair split summed over all half sweeps of one run (ms); f = the caller's function incl. its host copies"}
for name, alg, fdev, fref, domain, akw, kw in CASES:
    A = T.MaxVol if alg == "maxvol" else T.DMRG
    run = lambda: T.tt_cross(lambda X: fdev(X if fdev is sin30_t else X.cpu().numpy()), domain, A(verbose=False, **akw), **kw)  # noqa: E731
    run()
    T.cross._Timer.on = True
    torch.cuda.synchronize()
    t = time.perf_counter()
    tt = run()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t
    T.cross._Timer.on = False
    last = T.cross._LAST
    ref = R.cross_maxvol if alg == "maxvol" else R.cross_dmrg
    t = time.perf_counter()
    ref(fref, domain, **akw, **kw)
    cpu = time.perf_counter() - t
    res[name] = {"ranks": tt.ttv_rks, "sweeps": last["sweeps"], "eps": last["eps"][-1] if last["eps"] else None,
                 "split_ms": {k: round(v, 3) for k, v in sorted(last["split"].items())}, "gpu_wall_s": wall, "cpu_restatement_s": cpu}
    print(name, json.dumps(res[name]), flush=True)
s = json.dumps(res)
print(s)
if out:
    with open(out, "w") as fh:
        fh.write(s + "\n")
