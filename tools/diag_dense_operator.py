"""Diagnostic of the dense bridge for operators, written to profiles/diag_dense_operator.json.

Binary operators of d = 10, 12, 13 sites at operator ranks 3 (Delta) and 16, and one mixed-dims operator, in the tensor and the matrix
layout.  Event pairs on the library's stream after a warm-up, windows of about 0.2 s, the versions alternated in one call, every window
reported.

Export.  ttn_tto_to_dense against the only route the library offered before it for the same array: ttn_tt_to_dense of the operator as
a train on n_k^2 sites (the train is made once, outside the timed region) followed by torch's permute(...).contiguous() into the
layout (two passes above d = 8: torch permutes at most 16 axes, see permute_stages); and against torch.Tensor.fill_ on a buffer of the same size (the store-rate ceiling, as in tools/diag_qttnd.py).  Per case
also the cut and the tile split (TM rows of L x TN columns of R) the library chose (ttn_debug_dense_plan): a side of 1 means MFMA
blocks with 15 of 16 rows padded.

Import.  k_dense_gather (ttn_last_launch_ms after ttn_tto_decomp_dev: its table launches and the kernel) against torch's
permute(...).contiguous() of the same tensor, and the whole ttn_tto_decomp_dev against permute + ttn_ttv_decomp_dev + ttn_tto_from_tt
(wall clock around synchronising calls: the decomposition is one workgroup and dominates both).  What the host's search for the LDS
pad is worth: the gather again with the fixed pads 0 and 8 (TTN_GATHER_PAD), with the leading dimension each run used."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ttn_amd as T                                   # noqa: E402
from ttn_amd import _lib                              # noqa: E402
from ttn_amd import device as D                       # noqa: E402
from ttn_amd.tdvp import _dev                         # noqa: E402

def window(fn, reps):
    """ms per call of `reps` back-to-back calls between two events on the library's stream"""
    D.event_record(0)
    for _ in range(reps):
        fn()
    D.event_record(1)
    D.sync()
    return D.event_elapsed_ms(0, 1) / reps


def timed(fn, target_s=0.2, windows=3):
    for _ in range(3):                                 # warm-up: code objects, scratch growth, allocator
        fn()
    D.sync()
    per = max(window(fn, 3), 1e-3)
    reps = int(max(3, min(2000, target_s * 1e3 / per)))
    return [window(fn, reps) for _ in range(windows)]


def spread(ws):
    return (max(ws) - min(ws)) / statistics.median(ws)


def random_operator(dims, r, seed):
    """a TToperator with standard-normal cores at the ranks min(left product, right product, r)"""
    rng = np.random.default_rng(seed)
    d = len(dims)
    rks = [1] + [min(int(np.prod(dims[:k], dtype=object)), int(np.prod(dims[k:], dtype=object)), r) for k in range(1, d)] + [1]
    vec = [np.asfortranarray(rng.standard_normal((dims[k], dims[k], rks[k], rks[k + 1])) / np.sqrt(dims[k] * rks[k])) for k in range(d)]
    return T.TToperator(d, vec, tuple(dims), rks, [0] * d)


def dense_plan():
    """(cut m, TM, TN) the library chose for the last to_dense launch (ttn_debug_dense_plan)"""
    out = (C.c_int64 * 3)()
    _lib.check(_lib.lib().ttn_debug_dense_plan(out))
    return [int(v) for v in out]


def gather_plan():
    """{TI, TO, ld, RO} of the gather of the last ttn_tto_decomp_dev (ttn_debug_gather_plan)"""
    out = (C.c_int64 * 4)()
    _lib.check(_lib.lib().ttn_debug_gather_plan(out))
    return dict(zip(("TI", "TO", "ld", "RO"), (int(v) for v in out)))


def inverse(perm):
    inv = [0] * len(perm)
    for i, p in enumerate(perm):
        inv[p] = i
    return inv


def permute_stages(dims, layout):
    """torch's permute(...).contiguous() takes at most 16 axes, and the bridge between the merged-site array — in C order the axes
    (y_d, x_d, ..., y_1, x_1) — and a layout has 2 d of them that do not coalesce.  So the route is one pass up to d = 8 and two passes
    above: first the lower sites are de-interleaved under one merged upper axis, then the upper sites around the merged lower Y and X.
    Returns [(shape of the view, permutation)] for merged -> layout; the inverse route runs the inverted stages backwards."""
    d = len(dims)
    dl = d if 2 * d <= 16 else d // 2
    low, up = list(range(dl)), list(range(dl, d))
    order = (lambda S: list(reversed(S))) if layout == "tensor" else (lambda S: list(S))       # a layout's C order, slowest first
    PU = int(np.prod([dims[k] ** 2 for k in up], dtype=object)) if up else 1
    NL = int(np.prod([dims[k] for k in low], dtype=object))
    y1 = lambda k: 1 + 2 * (dl - 1 - k)
    stages = [([PU] + [n for k in reversed(low) for n in (dims[k], dims[k])], [0] + [y1(k) for k in order(low)] + [y1(k) + 1 for k in order(low)])]
    if up:
        y2 = lambda k: 2 * (d - 1 - k)
        YL, XL = 2 * len(up), 2 * len(up) + 1
        shape = [n for k in reversed(up) for n in (dims[k], dims[k])] + [NL, NL]
        if layout == "tensor":
            perm = [y2(k) for k in order(up)] + [YL] + [y2(k) + 1 for k in order(up)] + [XL]
        else:
            perm = [YL] + [y2(k) for k in order(up)] + [XL] + [y2(k) + 1 for k in order(up)]
        stages.append((shape, perm))
    return stages


def merged_to_layout(t, stages):
    for shape, perm in stages:
        t = t.view(shape).permute(perm).contiguous()
    return t.reshape(-1)


def layout_to_merged(t, stages):
    for shape, perm in reversed(stages):
        t = t.view([shape[p] for p in perm]).permute(inverse(perm)).contiguous()
    return t.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, nargs="+", default=[10, 12, 13])
    ap.add_argument("--ranks", type=int, nargs="+", default=[3, 16])
    ap.add_argument("--mixed", type=int, nargs="+", default=[3, 4, 5, 6, 7])
    ap.add_argument("--import-max-sites", type=int, default=13)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_dense_operator.json"))
    a = ap.parse_args()
    torch, stream = _dev()
    L = _lib.lib()
    rec = {"device": torch.cuda.get_device_name(0), "export": [], "import": []}

    def save():
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)

    cases = [((2,) * d, r) for d in a.sites for r in a.ranks] + [(tuple(a.mixed), 8)]
    with torch.cuda.stream(stream):
        for dims, r in cases:
            d = len(dims)
            binary = all(n == 2 for n in dims)
            A = T.Delta(d) if (binary and r == 3) else random_operator(dims, r, d + r)
            total = int(np.prod([n * n for n in dims], dtype=object))
            h = D.DeviceTTO(A)
            t = h.to_tt()
            out = torch.empty((total,), dtype=torch.float64, device="cuda")
            mid = torch.empty((total,), dtype=torch.float64, device="cuda")
            po, pm = C.c_void_p(out.data_ptr()), C.c_void_p(mid.data_ptr())
            for layout in ("tensor", "matrix"):
                xs, ys = T.operator_strides(dims, layout)
                pxs, pys = T.tt._i64(xs), T.tt._i64(ys)
                stages = permute_stages(dims, layout)
                new = lambda: _lib.check(L.ttn_tto_to_dense(h.h, pxs, pys, po))

                def old():
                    _lib.check(L.ttn_tt_to_dense(t.h, None, pm))
                    return merged_to_layout(mid, stages)
                # the two routes write the same array
                new()
                m, TM, TN = dense_plan()
                ref = old()
                D.sync()
                bitwise = bool((out == ref).all())
                assert float((out - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), "the two export routes disagree"
                del ref
                w_new, w_old, w_fill, w_tt = [], [], [], []
                for _ in range(2):                     # alternate the versions
                    w_new += timed(new)
                    w_old += timed(old)
                    w_tt += timed(lambda: _lib.check(L.ttn_tt_to_dense(t.h, None, pm)))
                    w_fill += timed(lambda: out.fill_(1.0))
                ms_new, ms_old = statistics.median(w_new), statistics.median(w_old)
                case = {"dims": list(dims) if not binary else "2^%d" % d, "sites": d, "rank": max(A.tto_rks), "layout": layout, "entries": total,
                        "cut": m, "TM": TM, "TN": TN, "torch_permute_passes": len(stages), "bitwise_equal_to_train_route": bitwise,
                        "to_dense_ms": ms_new, "to_dense_ms_windows": w_new, "to_dense_spread": spread(w_new),
                        "train_route_ms": ms_old, "train_route_ms_windows": w_old, "train_route_spread": spread(w_old),
                        "train_to_dense_alone_ms": statistics.median(w_tt),
                        "fill_ms": statistics.median(w_fill), "fill_ms_windows": w_fill,
                        "new_over_old": ms_new / ms_old, "fraction_of_fill": statistics.median(w_fill) / ms_new,
                        "write_GBps": 8 * total / (ms_new * 1e-3) / 1e9}
                rec["export"].append(case)
                print(json.dumps(case), flush=True)
                save()
            # ---- import ----
            if binary and d <= a.import_max_sites:     # (the mixed case's unfoldings have short sides of 1764: minutes of one-workgroup SVD)
                dense = {"tensor": None, "matrix": None}
                for layout in ("tensor", "matrix"):
                    xs, ys = T.operator_strides(dims, layout)
                    _lib.check(L.ttn_tto_to_dense(h.h, T.tt._i64(xs), T.tt._i64(ys), po))
                    dense[layout] = out.clone()
                D.sync()
                cap = [1] + [min(int(np.prod([n * n for n in dims[:k]], dtype=object)), int(np.prod([n * n for n in dims[k:]], dtype=object)), 1024)
                             for k in range(1, d)] + [1]
                tol = 1e-10 * float(dense["tensor"].abs().max())
                for layout in ("tensor", "matrix"):
                    src = dense[layout]
                    stages = permute_stages(dims, layout)
                    perm_fn = lambda: layout_to_merged(src, stages)
                    w_perm = timed(perm_fn) + timed(perm_fn)

                    def new_import():
                        g = D.DeviceTTO.from_dense(src, dims, index=1, tol=tol, layout=layout)
                        rks = list(g.rks)
                        g.free()
                        return rks

                    def old_import():
                        z = D.DeviceTT([n * n for n in dims], cap)
                        T.qtt.ttv_decomp_dev_(z, perm_fn(), 1, tol)
                        D.compress_status(z)
                        g = D.DeviceTTO.from_tt(z)
                        rks = list(g.rks)
                        g.free(), z.free()
                        return rks
                    wall = {"new": [], "old": []}
                    gather = []
                    ranks = {}
                    for name, fn in (("new", new_import), ("old", old_import), ("new", new_import), ("old", old_import), ("new", new_import), ("old", old_import)):
                        D.sync()
                        t0 = time.perf_counter()
                        ranks[name] = fn()
                        D.sync()
                        wall[name].append((time.perf_counter() - t0) * 1e3)
                        if name == "new":
                            gather.append(D.last_launch_ms())
                    assert ranks["new"] == ranks["old"], ranks
                    plan = gather_plan()
                    pads = {}
                    for pad in ("0", "8"):             # the searched pad against fixed ones
                        os.environ["TTN_GATHER_PAD"] = pad
                        try:
                            g_ms = []
                            for _ in range(3):
                                new_import()
                                g_ms.append(D.last_launch_ms())
                            pads[pad] = {"ld": gather_plan()["ld"], "gather_ms": statistics.median(g_ms[1:]), "gather_ms_calls": g_ms}
                        finally:
                            del os.environ["TTN_GATHER_PAD"]
                    case = {"dims": list(dims) if not binary else "2^%d" % d, "sites": d, "rank": max(A.tto_rks), "layout": layout, "entries": total, "ranks_found": max(ranks["new"]),
                            "gather_plan": plan, "fixed_pads": pads,
                            "gather_ms": statistics.median(gather[1:]), "gather_ms_calls": gather,
                            "torch_permute_passes": len(stages), "torch_permute_ms": statistics.median(w_perm), "torch_permute_ms_windows": w_perm,
                            "gather_over_permute": statistics.median(gather[1:]) / statistics.median(w_perm),
                            "gather_GBps": 16 * total / (statistics.median(gather[1:]) * 1e-3) / 1e9,
                            "decomp_dev_wall_ms_calls": wall["new"], "old_route_wall_ms_calls": wall["old"],
                            "decomp_dev_wall_ms": statistics.median(wall["new"][1:]), "old_route_wall_ms": statistics.median(wall["old"][1:])}
                    rec["import"].append(case)
                    print(json.dumps(case), flush=True)
                    save()
                del dense
            t.free(), h.free()
            del out, mid
    D.status_all()
    save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
