"""Diagnostic of the site-resolved measurements, written to profiles/diag_measure.json.

On rank-r QTT trains of d sites, at each batch size:
  * device.correlation_matrix_dev with P = Q = Z (one pass of walks, mirrored) and with P != Q (two passes), next to the composed route
    it replaces through unchanged code: one rank-1 product operator per pair (d (d - 1) / 2 of them, or d (d - 1) for P != Q), uploaded
    beforehand, each through device.sandwich_dev into one device tensor — only device time is compared.  The composed route runs in full
    up to --full-up-to trains; above that a sample of --sample pairs is timed and scaled by pairs / sample (reported as scaled);
  * device.site_expect_dev(Z) next to device.sandwich_dev with pauli_sum_tto("z", d), which returns one number instead of d;
  * the walks alone: the time of correlation_matrix_dev minus the time of site_expect_dev with as many tables (the same chains and
    opening steps), as a share of the fp64 matrix peak on the walks' own flop count, sum over the steps of a walk of
    2 n (r_in^2 r_out + r_out^2 r_in) (8 r^3 per rank-r step) per pass and train.
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
PEAK_F64 = 78.6e12
Z = np.diag([1.0, -1.0])
I2 = np.eye(2)


def timed(fn, slot):
    D.event_record(slot)
    v = fn()
    D.event_record(slot + 1)
    return D.event_elapsed_ms(slot, slot + 1), v


def walk_flops(rks, n=2):
    """One pass of walks of one train: the walk that opens at site j (0-based) runs the sites j .. 1."""
    d = len(rks) - 1
    step = [2 * n * (rks[i + 1] ** 2 * rks[i] + rks[i] ** 2 * rks[i + 1]) for i in range(d)]
    return sum(sum(step[1:j + 1]) for j in range(1, d))


def product_operator(d, a, Pa, b, Qb):
    mats = [I2] * d
    mats[a], mats[b] = Pa, Qb
    return T.TToperator(d, [np.asfortranarray(m.reshape(2, 2, 1, 1)) for m in mats], (2,) * d, [1] * (d + 1), [0] * d)


def stats(ts):
    return {"ms": ts, "ms_median": statistics.median(ts), "ms_spread": max(ts) - min(ts)}


def case(d, r, batch, reps, full_up_to, sample):
    x = T.rand_tt((2,) * d, r, seed=30)
    dx = T.DeviceTT.from_host(x, batch=batch)
    rng = np.random.default_rng(4)
    P, Q = rng.standard_normal((2, 2)), rng.standard_normal((2, 2))
    out_c = torch.empty((batch, d, d), dtype=torch.float64, device="cuda")
    out_s = torch.empty(batch, dtype=torch.float64, device="cuda")
    rec = {"d": d, "rank": r, "batch": batch, "reps": reps}
    for label, (A, B_) in (("ZZ", (Z, None)), ("PQ", (P, Q))):
        pairs = [(i, j) for i in range(d) for j in range(i + 1, d)]
        if B_ is not None:
            pairs = pairs + [(j, i) for i, j in pairs]
        scaled = batch > full_up_to
        used = pairs
        if scaled:
            used = [pairs[k] for k in np.linspace(0, len(pairs) - 1, sample).astype(int)]
        ops = [T.DeviceTTO(product_operator(d, a, A, b, A if B_ is None else B_)) for a, b in used]
        ntab = 2 if B_ is None else 3                  # the tables of the correlation: P Q and P, or P Q, P and Q
        out_e = torch.empty((batch, ntab, d), dtype=torch.float64, device="cuda")

        def composed():
            for hA in ops:
                D.sandwich_dev(dx, hA, dx, out=out_s)

        def direct():
            return D.correlation_matrix_dev(dx, A, B_, out=out_c)

        def opens():
            tabs = [A] * ntab if B_ is None else [A, B_, A]
            return D.site_expect_dev(dx, *tabs, out=out_e)

        composed(), direct(), opens()                    # the warm-up of each
        t_comp, t_dir, t_open = [], [], []
        for _ in range(reps):
            t_comp.append(timed(composed, 0)[0] * (len(pairs) / len(used)))
            t_dir.append(timed(direct, 2)[0])
            t_open.append(timed(opens, 4)[0])
        # the numbers agree: the first sampled pair against the direct result
        a, b = used[0]
        D.sandwich_dev(dx, ops[0], dx, out=out_s)
        D.sync()
        nn = D.dot(dx, dx)
        diff = float(np.max(np.abs(out_s.cpu().numpy() / nn - out_c.cpu().numpy()[:, b, a])))      # the tensor holds C[b, j, i]
        for hA in ops:
            hA.free()
        mc, md, mo = statistics.median(t_comp), statistics.median(t_dir), statistics.median(t_open)
        sc, sd = max(t_comp) - min(t_comp), max(t_dir) - min(t_dir)
        passes = 1 if B_ is None else 2
        flops = batch * passes * walk_flops(x.ttv_rks)
        walks_ms = md - mo
        rec[label] = {"pairs": len(pairs), "composed_pairs_timed": len(used), "composed_scaled": scaled,
                      "composed": stats(t_comp), "correlation_matrix": stats(t_dir), "chains_and_opens": stats(t_open),
                      "speedup": mc / md, "faster_by_more_than_both_spreads": mc - md > sc + sd,
                      "walks_ms_by_difference": walks_ms, "walk_flops": flops,
                      "walks_fraction_of_fp64_peak": flops / (walks_ms * 1e-3) / PEAK_F64 if walks_ms > 0 else None,
                      "max_abs_diff_pair_%d_%d" % (a, b): diff}
    # the profile against the one number of expect(pauli_sum_tto)
    hS = T.DeviceTTO(T.pauli_sum_tto("z", d))
    out_1 = torch.empty((batch, 1, d), dtype=torch.float64, device="cuda")

    def profile():
        return D.site_expect_dev(dx, Z, out=out_1)

    def total():
        return D.sandwich_dev(dx, hS, dx, out=out_s)

    profile(), total()
    t_p, t_t = [], []
    for _ in range(reps):
        t_t.append(timed(total, 0)[0])
        t_p.append(timed(profile, 2)[0])
    D.sync()
    nn = D.dot(dx, dx)
    rec["site_expect_Z"] = {"site_expect": stats(t_p), "expect_pauli_sum": stats(t_t), "slower_by": statistics.median(t_p) / statistics.median(t_t),
                            "max_abs_diff_of_the_sum": float(np.max(np.abs(out_1.cpu().numpy()[:, 0, :].sum(axis=1) - out_s.cpu().numpy() / nn)))}
    hS.free()
    dx.free()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=30)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--full-up-to", type=int, default=256, help="largest batch at which the composed route runs every pair")
    ap.add_argument("--sample", type=int, default=16, help="pairs timed above it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_measure.json"))
    a = ap.parse_args()
    assert a.reps >= 7, "the median of at least 7 runs"
    T.ensure_init(0)
    rec = {"tool": "tools/diag_measure.py", "peak_fp64_flops": PEAK_F64, "cases": []}
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
