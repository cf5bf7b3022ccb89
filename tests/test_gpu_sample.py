"""tt_sample on the GPU (csrc/ttn_sample_kernels.h, include/ttn_sample.h) against the NumPy restatement of tests/sample_reference.py.

Parity rule: on the same uniforms the indices are IDENTICAL to the reference for every sample that is not fragile (margin >= 1e-9 in
the reference; tests/test_cpu_sample.py asserts that the reference finds no fragile sample on these runs, the cap here is 0.1 %), logp
agrees to 1e-9 absolute (the project's tensor-parity bar), and independently logp equals the log of the target, log(x(z)^2 / <x, x>) or
log(x(z) / sum x), with x(z) from the device evaluation kernel of the cross module — taken as 2 log|x| - log <x, x>, the same number
without the square that underflows at d = 480.  Every test prints its worst logp error and its fragile count.

Shapes: the smallest at which each piece can go wrong — the on-chip class with full and ragged, off-tile ranks in one batch and more
than one sample tile; a rank-80 interior between ramps inside the class (V changes its home twice per sweep); mixed dims and odd ranks
on the general route; d = 1 and 2, S = 1 and one tile + 1; a batch beyond one launch chunk; 480 sites."""
import numpy as np
import pytest

import ttn_amd as T
from tests import sample_reference as R
from tests.helpers import worst_of
from ttn_amd import cross
from ttn_amd import device as D

pytestmark = pytest.mark.gpu

TOL = 1e-9
CHI2_15_Q = 56.493            # chi2.ppf(1 - 1e-6, df=15), as in tests/test_cpu_sample.py
MODES = [pytest.param(True, id="born"), pytest.param(False, id="density")]


def mode_of(born):
    return "born" if born else "density"


def to_tt(cores):
    dims = tuple(c.shape[0] for c in cores)
    rks = [c.shape[1] for c in cores] + [cores[-1].shape[2]]
    return T.TTvector(len(cores), [np.asfortranarray(c) for c in cores], dims, rks, [0] * len(cores))


def upload(trains, batch=None):
    dims = tuple(c.shape[0] for c in trains[0])
    d = len(dims)
    cap = [max(([t[k].shape[1] for k in range(d)] + [1])[m] for t in trains) for m in range(d + 1)]
    h = D.DeviceTT(dims, cap, batch=batch or len(trains))
    for b, t in enumerate(trains):
        h.upload(b, to_tt(t))
    return h


def target_logp(cores, idx, born):
    """log of the target at the device's own samples, x(z) from cross._evaluate_tt, the normalisation from the reference's environments"""
    x = cross._evaluate_tt([np.asfortranarray(c) for c in cores], idx, len(cores))
    e0 = R.envs(cores, born)[0]
    with np.errstate(all="ignore"):
        if born:
            return 2.0 * np.log(np.abs(x)) - np.log(e0[0, 0])
        return np.log(x) - np.log(e0[0])


def check_parity(tag, trains, res, got, born):
    idx, logp, info = got
    worst = worst_t = 0.0
    nfrag = 0
    for b, cores in enumerate(trains):
        ridx, rlogp, margin, clamps, dead = res[b]
        S = ridx.shape[0]
        ok = margin >= R.FRAGILE
        nfrag += int((~ok).sum())
        assert int((~ok).sum()) <= R.FRAGILE_SHARE * S
        bad = np.flatnonzero(ok & np.any(idx[b] != ridx, axis=1))
        assert bad.size == 0, f"{tag} train {b}: {bad.size} samples differ, first {bad[:5]}: {idx[b][bad[:2]]} vs {ridx[bad[:2]]}"
        worst = worst_of(worst, float(np.max(np.abs(logp[b][ok] - rlogp[ok]))))
        worst_t = worst_of(worst_t, float(np.max(np.abs(logp[b] - target_logp(cores, idx[b], born)))))
        assert tuple(info[b]) == (clamps, dead)
    print(f"{tag} {mode_of(born)}: logp against the reference {worst:.2e}, against the target {worst_t:.2e}, fragile {nfrag}")
    assert worst <= TOL and worst_t <= TOL


def run_case(name, S, seed, born):
    _, trains, u, res = R.run(name, S, seed, born)
    h = upload(trains)
    try:
        got = D.sample(h, S, mode=mode_of(born), u=u)
        assert got[0].shape == (len(trains), S, len(trains[0])) and got[1].shape == (len(trains), S) and got[2].shape == (len(trains), 2)
        check_parity(f"{name} S={S}", trains, res, got, born)
    finally:
        h.free()
    return trains, u, res, got


@pytest.mark.parametrize("born", MODES)
def test_on_chip_class(born):
    """d = 12, ranks 1, 2, .., 64, .., 2, 1; three trains, the second capped at rank 13, the third at 7; S = 300: five tiles, the last one
    partly filled."""
    trains = R.case("chip_d12", born)[1]
    assert [c.shape[2] for c in trains[0]][5] == 64 and max(c.shape[2] for c in trains[1]) == 13 and max(c.shape[2] for c in trains[2]) == 7
    assert 300 > D._header_define("ttn_sample.h", "TTN_SAMPLE_TILE") and 300 % D._header_define("ttn_sample.h", "TTN_SAMPLE_TILE") != 0
    run_case("chip_d12", 300, 11, born)


@pytest.mark.parametrize("born", MODES)
@pytest.mark.parametrize("name,S,seed", [("rank80_d10", 130, 12), ("mixed_dims", 200, 13)])
def test_general_route(name, S, seed, born):
    run_case(name, S, seed, born)


@pytest.mark.parametrize("born", MODES)
@pytest.mark.parametrize("name,S,seed", [("d1", 65, 14), ("d2", 65, 15), ("d2", 1, 16)])
def test_edge_sizes(name, S, seed, born):
    assert S in (1, D._header_define("ttn_sample.h", "TTN_SAMPLE_TILE") + 1)
    run_case(name, S, seed, born)


@pytest.mark.parametrize("born", MODES)
def test_480_sites(born):
    """the rescale of v: no dead sample over 480 sites, and parity holds"""
    _, _, _, got = run_case("d480", 100, 17, born)
    assert got[2][0, 1] == 0 and np.all(np.isfinite(got[1]))


@pytest.mark.parametrize("born", MODES)
def test_generated_uniforms(born):
    """u=None with a seed is the call with sample_uniforms(seed, ...); the same call twice gives the same non-fragile samples"""
    S, seed = 150, 4242
    _, trains = R.case("chip_d12", born)
    u = T.sample_uniforms(seed, len(trains), S, 12)
    res = [R.sample(t, u[b], born) for b, t in enumerate(trains)]
    h = upload(trains)
    try:
        a = D.sample(h, S, mode=mode_of(born), seed=seed)
        b2 = D.sample(h, S, mode=mode_of(born), seed=seed)
        c = D.sample(h, S, mode=mode_of(born), u=u)
        ok = np.stack([r[2] >= R.FRAGILE for r in res])
        print(f"generated uniforms {mode_of(born)}: fragile {int((~ok).sum())}")
        assert int((~ok).sum()) <= R.FRAGILE_SHARE * ok.size
        for other in (b2, c):
            assert np.array_equal(a[0][ok], other[0][ok])
            assert np.max(np.abs(a[1][ok] - other[1][ok])) <= TOL
        check_parity("seeded", trains, res, a, born)
        # the prefix property on the device: the first 70 samples of a shorter call
        short = D.sample(h, 70, mode=mode_of(born), seed=seed)
        assert np.array_equal(short[0][ok[:, :70]], a[0][:, :70][ok[:, :70]])
        # the device-tensor forms
        import torch
        di, dl, dn = D.sample_dev(h, S, mode=mode_of(born), u=torch.from_numpy(u).to("cuda"))
        D.sync()
        assert np.array_equal(di.cpu().numpy()[ok], a[0][ok]) and np.array_equal(dn.cpu().numpy(), a[2])
        assert np.max(np.abs(dl.cpu().numpy()[ok] - a[1][ok])) <= TOL
    finally:
        h.free()


@pytest.mark.parametrize("born", MODES)
def test_batch_beyond_one_launch_chunk(born):
    """B = 65537 trains of d = 2, rank 1, S = 2: the second chunk holds two trains.  A rank-1 train is a product distribution, so the
    target of EVERY train is a closed form; the reference runs on the trains around the chunk boundary and on every 1024th."""
    B, S, seed = 65537, 2, 7
    rng = np.random.default_rng(65537 + int(born))
    special = {b: [rng.standard_normal((2, 1, 1)) if born else np.abs(rng.standard_normal((2, 1, 1))) for _ in range(2)]
               for b in (1, 65534, 65535, 65536)}
    base = [np.array([0.6, -0.8] if born else [0.6, 0.8]).reshape(2, 1, 1), np.array([0.3, 0.9]).reshape(2, 1, 1)]
    h = D.DeviceTT((2, 2), [1, 1, 1], batch=B)
    try:
        h.upload(0, to_tt(base))
        h.replicate(0)
        for b, t in special.items():
            h.upload(b, to_tt(t))
        idx, logp, info = D.sample(h, S, mode=mode_of(born), seed=seed)
        assert idx.shape == (B, S, 2) and np.all(info == 0)
        f0 = np.tile(base[0].reshape(1, 2), (B, 1))
        f1 = np.tile(base[1].reshape(1, 2), (B, 1))
        for b, t in special.items():
            f0[b], f1[b] = t[0].reshape(2), t[1].reshape(2)
        w0, w1 = (f0 ** 2, f1 ** 2) if born else (f0, f1)
        rows = np.arange(B)[:, None]
        want = np.log(w0[rows, idx[:, :, 0] - 1] / w0.sum(1, keepdims=True)) + np.log(w1[rows, idx[:, :, 1] - 1] / w1.sum(1, keepdims=True))
        err_t = float(np.max(np.abs(logp - want)))
        worst, nfrag = 0.0, 0
        for b in sorted(set(range(0, B, 1024)) | set(special) | {0}):
            ridx, rlogp, margin, _, _ = R.sample(special.get(b, base), R.uniforms(seed, b, S, 2), born)
            ok = margin >= R.FRAGILE
            nfrag += int((~ok).sum())
            assert np.array_equal(idx[b][ok], ridx[ok]), b
            worst = worst_of(worst, float(np.max(np.abs(logp[b][ok] - rlogp[ok]), initial=0.0)))
        print(f"B = {B} {mode_of(born)}: logp against the reference {worst:.2e}, against the closed form {err_t:.2e}, fragile {nfrag}")
        assert worst <= TOL and err_t <= TOL and nfrag <= 1
    finally:
        h.free()


def test_exact_cases():
    """clamps = S and z_1 = 1 on the rank-1 density train with site-1 values (2, -1); a zero train: every sample dead, nothing raised;
    the library stays usable after each"""
    S = 70
    _, cl = R.clamp_train()
    _, zr = R.zero_train()
    probe = R.case("d2")[1][0]
    hp = upload([probe])
    try:
        want = D.sample(hp, 5, seed=1)
        h = upload([cl])
        idx, logp, info = D.sample(h, S, mode="density", seed=3)
        h.free()
        assert np.all(idx[0, :, 0] == 1) and tuple(info[0]) == (S, 0)
        ref = np.log(np.array([1.0, 3.0]) / 4.0)[idx[0, :, 1] - 1] + np.log(np.array([0.5, 0.25]) / 0.75)[idx[0, :, 2] - 1]
        print(f"clamp case: logp against the closed form {np.max(np.abs(logp[0] - ref)):.2e}")
        assert np.max(np.abs(logp[0] - ref)) <= TOL
        assert np.array_equal(D.sample(hp, 5, seed=1)[0], want[0])
        for mode in ("born", "density"):
            h = upload([zr])
            idx, logp, info = D.sample(h, S, mode=mode, seed=3)
            h.free()
            assert np.all(idx == 1) and np.all(np.isneginf(logp)) and tuple(info[0]) == (0, S)
            assert np.array_equal(D.sample(hp, 5, seed=1)[0], want[0])
    finally:
        hp.free()


def test_magnetisation_profile_ties_to_site_expect():
    """|mean_s Z(z_k) - site_expect(x, Z)[k]| <= 5 / sqrt(S) at every site of a d = 8 Born case, S = 4096 (a fixed seed: deterministic)"""
    S = 4096
    cores = R.case("d8_born")[1][0]
    x = to_tt(cores)
    idx, _, info = T.tt_sample(x, S, seed=18)
    assert idx.shape == (S, 8) and tuple(info) == (0, 0)
    got = np.mean(np.where(idx == 1, 1.0, -1.0), axis=0)
    want = T.site_expect(x, np.diag([1.0, -1.0]))
    print(f"<Z_k>: worst |sample mean - site_expect| {np.max(np.abs(got - want)):.3e} (bar {5 / np.sqrt(S):.3e})")
    assert np.max(np.abs(got - want)) <= 5.0 / np.sqrt(S)


def test_chi_square_on_device_samples():
    cores = R.case("d4_chi2")[1][0]
    idx, _, _ = T.tt_sample(to_tt(cores), 20000, seed=19)
    full = R.dense(cores)
    stat = R.chi2_stat(idx, full ** 2 / np.sum(full ** 2))
    print(f"chi-square of 20000 device samples, 15 degrees of freedom: {stat:.1f} (bar {CHI2_15_Q})")
    assert stat <= CHI2_15_Q


@pytest.mark.parametrize("ordering", ["interleaved", "serial"])
def test_qttv_sample(ordering):
    """a 2-D Gaussian with 5 bits per dimension: the decoded grid indices reproduce qttv_to_array's values, logp matches them"""
    import torch

    def f(X):
        return torch.exp(-((X[:, 0] - 0.5) ** 2 + (X[:, 1] - 0.4) ** 2) / 0.05)

    q = T.function_to_qttv(f, 2, 5, ordering)
    arr = T.qttv_to_array(q)
    assert arr.shape == (32, 32) and arr.min() > 0.0
    S = 500
    grid, logp = T.qttv_sample(q, S, seed=5)
    assert grid.shape == (S, 2) and grid.min() >= 0 and grid.max() <= 31
    vals = arr[grid[:, 0], grid[:, 1]]
    err = float(np.max(np.abs(logp - np.log(vals / arr.sum()))))
    # the same seed through tt_sample: the value of the train at the sampled bits is the array's value at the decoded point
    idx, logp2, _ = T.tt_sample(q.ttvector(), S, mode="density", seed=5)
    at_bits = R.evaluate([np.asarray(c) for c in q.ttvector().ttv_vec], idx)
    rel = float(np.max(np.abs(at_bits - vals) / vals))
    print(f"qttv_sample {ordering}: logp against the array {err:.2e}, value at the bits against the array {rel:.2e}")
    assert err <= TOL and rel <= 1e-9 and np.array_equal(logp, logp2)
    assert len(np.unique(grid, axis=0)) > 50                                # samples spread over the bump


def test_refusals():
    """every refusal leaves the library usable: the next call gives the known answer"""
    probe = R.case("d2")[1][0]
    hp = upload([probe])
    z = None
    A = None
    try:
        want = D.sample(hp, 5, seed=1)

        def still_works():
            assert np.array_equal(D.sample(hp, 5, seed=1)[0], want[0])

        z = D.DeviceTT((2, 2), [1, 2, 1], dtype=np.complex128)
        with pytest.raises(T.TTNError, match="Float64 only"):
            D.sample(z, 4)
        still_works()
        A = D.DeviceTTO(T.id_tto(2))
        with pytest.raises(TypeError, match="DeviceTT"):
            D.sample(A, 4)
        still_works()
        with pytest.raises(T.TTNError, match="nsamples"):
            D.sample(hp, 0)
        still_works()
        with pytest.raises(T.TTNError, match="mode"):
            D.sample(hp, 4, mode="fermi")
        still_works()
        with pytest.raises(T.TTNError, match="u has shape"):
            D.sample(hp, 4, u=np.zeros((1, 4, 3)))
        still_works()
        # the library's own checks, behind the Python layer's
        L = T._lib.lib()
        out_i, out_l = np.zeros(8, dtype=np.int64), np.zeros(4)
        pi, pl = out_i.ctypes.data_as(T._lib.p_i64), out_l.ctypes.data_as(T._lib.p_f64)
        assert L.ttn_tt_sample(hp.h, 2, 4, 0, None, pi, pl, None) != 0 and "mode" in T._lib.last_error()
        assert L.ttn_tt_sample(hp.h, 0, 0, 0, None, pi, pl, None) != 0 and "nsamples" in T._lib.last_error()
        assert L.ttn_tt_sample(None, 0, 4, 0, None, pi, pl, None) != 0
        assert L.ttn_tt_sample(hp.h, 0, 4, 0, None, None, pl, None) != 0
        still_works()
    finally:
        hp.free()
        if z is not None:
            z.free()
        if A is not None:
            A.free()
