"""Diagnostic of the site-resolved measurements on ComplexF64 trains, written to profiles/diag_zmeasure.json.

On rank-r complex QTT trains of d sites, at each batch size, for each new call — device.zsite_expect_dev with one table (sigma_y) and
device.zcorrelation_matrix_dev with complex P != Q (two passes of walks) — the time of the call next to
  * the only route without it: one rank-1 complex product operator per site (d of them) or per ordered pair (d (d - 1)), uploaded
    beforehand, each through device.braket_dev into one device tensor — only device time is compared.  The route runs in full up to
    --full-up-to trains; above that a sample of --sample operators is timed and scaled by operators / sample (reported as scaled);
  * device.site_expect_dev / device.correlation_matrix_dev on a Float64 train of the same shape with real tables: the flop yardstick (a
    complex product is four real ones, so about 4 x is the expectation, not a bar).
HIP-event pairs on the library stream around each, one warm-up of each first, the routes alternating, the median of --reps runs and the
spread (max - min) of each."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                    # noqa: E402

import ttn_amd as T                                   # noqa: E402
from ttn_amd import device as D                       # noqa: E402

torch, _ = T.tdvp._dev()                     # (asks torch for the GPU before the library binds it)
SY = np.array([[0, -1j], [1j, 0]])
I2 = np.eye(2, dtype=np.complex128)


def timed(fn, slot):
    D.event_record(slot)
    v = fn()
    D.event_record(slot + 1)
    return D.event_elapsed_ms(slot, slot + 1), v


def product_operator(d, placed):
    """The rank-1 complex operator with the matrices of `placed` = {site: matrix} and identities elsewhere."""
    mats = [placed.get(k, I2) for k in range(d)]
    return T.TToperator(d, [np.asfortranarray(np.asarray(m, dtype=np.complex128).reshape(2, 2, 1, 1)) for m in mats], (2,) * d, [1] * (d + 1), [0] * d)


def stats(ts):
    return {"ms": ts, "ms_median": statistics.median(ts), "ms_spread": max(ts) - min(ts)}


def compare(label, placements, direct, yardstick, braket_into, pick, reps, scaled_to):
    """Times `direct` (the new call), the braket route over `placements` and the Float64 `yardstick`, alternating."""
    ops = [T.DeviceTTO(A) for A in placements]

    def composed():
        for hA in ops:
            braket_into(hA)

    composed(), direct(), yardstick()                  # the warm-up of each
    t_comp, t_dir, t_real = [], [], []
    for _ in range(reps):
        t_comp.append(timed(composed, 0)[0] * (scaled_to / len(ops)))
        t_dir.append(timed(direct, 2)[0])
        t_real.append(timed(yardstick, 4)[0])
    diff = pick(ops[0])                                # the numbers agree: the first timed operator against the direct result
    for hA in ops:
        hA.free()
    mc, md, mr = statistics.median(t_comp), statistics.median(t_dir), statistics.median(t_real)
    sc, sd = max(t_comp) - min(t_comp), max(t_dir) - min(t_dir)
    return {"operators": scaled_to, "braket_operators_timed": len(ops), "braket_scaled": scaled_to != len(ops), "braket_route": stats(t_comp),
            label: stats(t_dir), "float64_call": stats(t_real), "speedup_over_braket": mc / md,
            "faster_by_more_than_both_spreads": mc - md > sc + sd, "times_the_float64_call": md / mr, "max_abs_diff_first_operator": diff}


def case(d, r, batch, reps, full_up_to, sample):
    rng = np.random.default_rng(4)
    xr = T.rand_tt((2,) * d, r, seed=30)
    xi = T.rand_tt((2,) * d, r, seed=31)
    xz = T.TTvector(d, [np.asfortranarray((np.asarray(a) + 1j * np.asarray(b)) / np.sqrt(2.0)) for a, b in zip(xr.ttv_vec, xi.ttv_vec)], xr.ttv_dims,
                    list(xr.ttv_rks), [0] * d)
    dz = T.DeviceTT.from_host(xz, batch=batch)
    dr = T.DeviceTT.from_host(xr, batch=batch)
    P = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    Q = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    Pr, Qr = rng.standard_normal((2, 2)), rng.standard_normal((2, 2))
    out_b = torch.empty(batch, dtype=torch.complex128, device="cuda")
    out_e = torch.empty((batch, 1, d), dtype=torch.complex128, device="cuda")
    out_c = torch.empty((batch, d, d), dtype=torch.complex128, device="cuda")
    out_er = torch.empty((batch, 1, d), dtype=torch.float64, device="cuda")
    out_cr = torch.empty((batch, d, d), dtype=torch.float64, device="cuda")
    rec = {"d": d, "rank": r, "batch": batch, "reps": reps}
    scaled = batch > full_up_to

    def braket_into(hA):
        D.braket_dev(dz, hA, dz, out=out_b)

    def first_value(hA):
        D.braket_dev(dz, hA, dz, out=out_b)
        D.sync()
        return out_b.cpu().numpy() / np.real(D.dot(dz, dz))

    # the profile: d operators with sigma_y at one site
    sites = list(range(d))
    used = [sites[k] for k in np.linspace(0, d - 1, min(sample, d)).astype(int)] if scaled else sites
    rec["zsite_expect"] = compare(
        "zsite_expect", [product_operator(d, {k: SY}) for k in used], lambda: D.zsite_expect_dev(dz, SY, out=out_e),
        lambda: D.site_expect_dev(dr, Pr, out=out_er), braket_into,
        lambda hA: float(np.max(np.abs(first_value(hA) - out_e.cpu().numpy()[:, 0, used[0]]))), reps, d)
    # the correlations: d (d - 1) operators with P at a and Q at b
    pairs = [(a, b) for a in range(d) for b in range(d) if a != b]
    usedp = [pairs[k] for k in np.linspace(0, len(pairs) - 1, sample).astype(int)] if scaled else pairs
    a0, b0 = usedp[0]
    rec["zcorrelation_matrix"] = compare(
        "zcorrelation_matrix", [product_operator(d, {a: P, b: Q}) for a, b in usedp], lambda: D.zcorrelation_matrix_dev(dz, P, Q, out=out_c),
        lambda: D.correlation_matrix_dev(dr, Pr, Qr, out=out_cr), braket_into,
        lambda hA: float(np.max(np.abs(first_value(hA) - out_c.cpu().numpy()[:, b0, a0]))), reps, len(pairs))      # the tensor holds C[b, j, i]
    dz.free()
    dr.free()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=30)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--full-up-to", type=int, default=256, help="largest batch at which the braket route runs every operator")
    ap.add_argument("--sample", type=int, default=16, help="operators timed above it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_zmeasure.json"))
    a = ap.parse_args()
    assert a.reps >= 7, "the median of at least 7 runs"
    T.ensure_init(0)
    rec = {"tool": "tools/diag_zmeasure.py", "cases": []}
    for B in a.batches:
        rec["cases"].append(case(a.d, a.rank, B, a.reps, a.full_up_to, a.sample))
        print(json.dumps(rec["cases"][-1]), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:                   # (kept after every batch size: a long run leaves what it has)
            json.dump(rec, f, indent=1)
            f.write("\n")
    D.status_all()


if __name__ == "__main__":
    main()
