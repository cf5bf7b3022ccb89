"""Diagnostic of <x| A |y> on ComplexF64 trains, written to profiles/diag_braket.json.  HIP events on the library
stream, a warm-up of every shape, best of --reps.

Shapes: d = 30, rank-64 complex trains (and one rank-65 shape, which leaves the on-chip class), B = 1 and B = 256; the operators
pauli_pair_sum_tto (rank 3, real) and heisenberg_xyz_tto (rank 5, real), pauli_sum_tto("x") (rank 2, real: the on-chip route with a
real operator) and pauli_sum_tto("y", complex128) (rank 2: the complex operator, on the on-chip route).  For each:

* ``braket``: device.braket(x, A, x) — event pair around the call (the result ends on the host), and the kernel alone
  (ttn_last_launch_ms);
* the composition it replaces, on the same handles and in the same run: device.apply into a preallocated complex handle, then
  device.dot — k_zapply and k_zdot, which this feature does not touch;
* the real twin: device.sandwich on Float64 trains of the same ranks with the real operator of the same ranks (for the complex
  sigma_y sum: the real sigma_x sum), and the ratio braket / sandwich.  Four times the real kernel's MFMA work is what the flop count
  of a complex product predicts.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                    # noqa: E402

import ttn_amd as T                                   # noqa: E402
from ttn_amd import device as D                       # noqa: E402


def crand_tt(d, r, seed):
    rng = np.random.default_rng(seed)
    rks = T.r_and_d_to_rks([r] * (d + 1), (2,) * d)
    scale = 1.0 / np.sqrt(2.0 * r)                    # keeps the chain's numbers of order one
    vec = [np.asfortranarray(scale * (rng.standard_normal((2, rks[k], rks[k + 1])) + 1j * rng.standard_normal((2, rks[k], rks[k + 1]))))
           for k in range(d)]
    return T.TTvector(d, vec, (2,) * d, rks, [0] * d)


def timed(fn, reps):
    """(best of reps in ms, all of them, the last value); one warm-up first."""
    ms, v = [], fn()
    for _ in range(reps):
        with D.StreamTimer() as tm:
            v = fn()
        ms.append(tm.ms)
    return min(ms), ms, v


def case(name, A, A_real, d, r, batch, reps):
    x = crand_tt(d, r, 30)
    xr = T.TTvector(d, [np.asfortranarray(c.real * np.sqrt(2.0)) for c in x.ttv_vec], x.ttv_dims, x.ttv_rks, x.ttv_ot)
    dA, dx = T.DeviceTTO(A), T.DeviceTT.from_host(x, batch=batch)
    dy = T.DeviceTT((2,) * d, [p * q for p, q in zip(A.tto_rks, x.ttv_rks)], batch=batch, dtype=np.complex128)

    def composed():
        D.apply(dA, dx, dy)
        return D.dot(dx, dy)

    kern = []

    def direct():
        v = D.braket(dx, dA, dx)
        kern.append(D.last_launch_ms())
        return v

    t_comp, all_comp, ref = timed(composed, reps)
    t_dir, all_dir, got = timed(direct, reps)
    scale = float(np.max(np.abs(D.norm(dx) * D.norm(dy))))
    for h in (dA, dx, dy):
        h.free()
    dAr, dxr = T.DeviceTTO(A_real), T.DeviceTT.from_host(xr, batch=batch)
    t_real, all_real, _ = timed(lambda: D.sandwich(dxr, dAr, dxr), reps)
    dAr.free(), dxr.free()
    on_chip = max(A.tto_rks) <= D.BRAKET_QTT_MAX_OP_RANK and max(x.ttv_rks) <= D.BRAKET_QTT_MAX_RANK
    return {"operator": name, "operator_dtype": "complex128" if np.iscomplexobj(A.tto_vec[0]) else "float64", "d": d, "rank": max(x.ttv_rks),
            "op_rank": max(A.tto_rks), "batch": batch, "reps": reps, "route": "on-chip" if on_chip else "general",
            "apply_dot_ms_best": t_comp, "apply_dot_ms": all_comp, "braket_ms_best": t_dir, "braket_ms": all_dir,
            "braket_kernel_ms_best": min(kern[1:]), "speedup_over_composition": t_comp / t_dir, "not_slower_than_composition": t_dir <= t_comp,
            "real_sandwich_ms_best": t_real, "real_sandwich_ms": all_real, "braket_over_real_sandwich": t_dir / t_real,
            "max_abs_diff_over_norms": float(np.max(np.abs(got - ref))) / scale}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=30)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_braket.json"))
    a = ap.parse_args()
    T.ensure_init(0)
    d = a.d
    pair, heis = T.pauli_pair_sum_tto("x", "z", d), T.heisenberg_xyz_tto(d)
    sx, sy = T.pauli_sum_tto("x", d), T.pauli_sum_tto("y", d, dtype=np.complex128)
    shapes = [("pauli_pair_sum_tto(x, z)", pair, pair, a.rank), ("heisenberg_xyz_tto", heis, heis, a.rank), ("pauli_sum_tto(x)", sx, sx, a.rank),
              ("pauli_sum_tto(y, complex128)", sy, sx, a.rank), ("pauli_pair_sum_tto(x, z)", pair, pair, a.rank + 1)]
    rec = {"tool": "tools/diag_braket.py", "timing": "HIP events on the library stream, one warm-up of every shape, best of reps",
           "on_chip_limits": {"rank": D.BRAKET_QTT_MAX_RANK, "op_rank": D.BRAKET_QTT_MAX_OP_RANK}, "cases": []}
    for name, A, A_real, r in shapes:
        for B in a.batches:
            rec["cases"].append(case(name, A, A_real, d, r, B, a.reps))
            print(json.dumps(rec["cases"][-1]), flush=True)
    rec["braket_not_slower_than_composition_at_B256"] = all(c["not_slower_than_composition"] for c in rec["cases"] if c["batch"] == 256)
    D.status_all()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
