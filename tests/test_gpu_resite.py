"""to_qtt / to_ttv on the device (csrc/ttn_resite_kernels.h: ttn_tt_split_sites, ttn_tt_merge_sites) against the NumPy restatement
tests/resite_reference.py (pinned by tests/test_cpu_resite.py).

Tolerances.  The split runs the SVD step of ttv_decomp, so it gets the tolerances of tests/test_gpu_ttv_decomp.py: reconstruction
1e-12 * max|tensor|, orthogonality 1e-12, sign-fixed cores 1e-9 (non-degenerate spectra only).  The merge has no SVD: a core entry is
a sum of at most 65 products per contraction and at most three chained contractions, 65 * 3 * eps = 4e-14 relative to the largest
partial sum, so cores agree entrywise to 1e-13 * max|core|."""
import numpy as np
import pytest

import ttn_amd as T
from tests import resite_reference as R
from tests.helpers import sign_fix_compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    T.ensure_init(0)


def up(x):
    """restatement Train -> product TTvector"""
    return T.TTvector(x.N, [np.asfortranarray(c) for c in x.ttv_vec], x.ttv_dims, list(x.ttv_rks), [0] * x.N)


def flat(sd):
    return [f for s in sd for f in s]


def tensor_err(got, want):
    return float(np.max(np.abs(R.dense(got) - want)))


def sin_train():
    """sin(x + y + z) on three 8-point sites, TT ranks (1, 2, 2, 1)"""
    t = np.arange(8) / 8.0
    c0 = np.stack([np.sin(t), np.cos(t)], axis=1)[:, None, :]
    c1 = np.stack([np.stack([np.cos(t), -np.sin(t)], axis=1), np.stack([np.sin(t), np.cos(t)], axis=1)], axis=1)
    c2 = np.stack([np.cos(t), np.sin(t)], axis=1)[:, :, None]
    return R.Train([c0, c1, c2])


SD = [[2, 3, 2], [3, 2], [4]]


@pytest.fixture(scope="module")
def x12():
    x = R.random_train((12, 6, 4), (1, 5, 3, 1), seed=21)
    return x, R.dense(x), R.to_qtt(x, SD)


# ---- split ----------------------------------------------------------------------------------------------------------------------
def test_split_non_palindromic_factor_lists(x12):
    """a tall unfolding (15 x 6), wide ones (2 x 30, 6 x 10) and a copy site in one train; [2, 3, 2] tells coarse from fine"""
    x, full, ref = x12
    got = T.to_qtt(up(x), SD)
    assert isinstance(got, T.TTvector) and got.ttv_dims == tuple(flat(SD)) and list(got.ttv_ot) == [0] * 6
    assert list(got.ttv_rks) == ref.ttv_rks == [1, 2, 6, 5, 6, 3, 1]
    err = tensor_err(got, full.reshape(flat(SD)))
    print("split reconstruction", err / np.max(np.abs(full)))
    assert err <= 1e-12 * np.max(np.abs(full))
    for k in (0, 1, 3):                                          # the U cores: every core but the last one of its site
        c = np.asarray(got.ttv_vec[k])
        m = c.reshape(c.shape[0] * c.shape[1], c.shape[2])
        orth = float(np.max(np.abs(m.T @ m - np.eye(c.shape[2]))))
        print("orthogonality core", k, orth)
        assert orth <= 1e-12
    diff = sign_fix_compare(got, ref)
    print("sign-fixed core difference", diff)
    assert diff <= 1e-9


@pytest.mark.parametrize("dims,sd", [((4,), [[1, 4]]), ((4,), [[4, 1]]), ((12,), [[2, 3, 2]]), ((12,), [[12]])])
def test_split_edge_lists(dims, sd):
    """a factor of 1, and trains of one site"""
    x = R.random_train(dims, (1, 1), seed=22)
    ref = R.to_qtt(x, sd)
    got = T.to_qtt(up(x), sd)
    assert got.ttv_dims == ref.ttv_dims and list(got.ttv_rks) == ref.ttv_rks
    assert tensor_err(got, R.dense(ref)) <= 1e-12 * np.max(np.abs(R.dense(x)))


def test_split_threshold():
    x = sin_train()
    full = R.dense(x).reshape((2,) * 9)
    sd = [[2, 2, 2]] * 3
    got = T.to_qtt(up(x), sd, threshold=1e-10)
    assert list(got.ttv_rks) == R.to_qtt(x, sd, 1e-10).ttv_rks == [1] + [2] * 8 + [1]
    assert tensor_err(got, full) <= 1e-12 * np.max(np.abs(full))
    got0 = T.to_qtt(up(x), sd)                                  # threshold 0 keeps min(rows, cols): two bonds are doubly degenerate
    assert list(got0.ttv_rks) == R.to_qtt(x, sd).ttv_rks == [1, 2, 4, 2, 4, 4, 2, 4, 2, 1]
    assert tensor_err(got0, full) <= 1e-12 * np.max(np.abs(full))


def test_split_batch_with_different_ranks():
    sd = [[2, 2, 2], [2, 2, 2]]
    trains = [R.random_train((8, 8), (1, r, 1), seed=30 + r) for r in (1, 3, 6)]
    dx = T.DeviceTT((8, 8), [1, 6, 1], batch=3)
    for b, x in enumerate(trains):
        dx.upload(b, up(x))
    dz = dx.split_sites(sd, threshold=1e-10)
    T.device.compress_status(dz)
    seen = []
    for b, x in enumerate(trains):
        ref = R.to_qtt(x, sd, 1e-10)
        got = dz.download(b)
        assert list(got.ttv_rks) == ref.ttv_rks
        assert tensor_err(got, R.dense(ref)) <= 1e-12 * np.max(np.abs(R.dense(x)))
        seen.append(ref.ttv_rks)
    assert seen[0] != seen[1] != seen[2]


def test_split_capacity_is_reported_and_the_handle_stays_usable(x12):
    x, full, ref = x12
    lib = T._lib.lib()
    dx = T.DeviceTT.from_host(up(x))
    dz = dx.split_sites(SD, cap_rks=[1, 2, 6, 5, 5, 3, 1])      # bond 4 needs 6
    with pytest.raises(T.TTNError):
        T.device.compress_status(dz)
    y = R.random_train((12, 6, 4), (1, 2, 2, 1), seed=23)       # needs (1, 2, 4, 2, 4, 2, 1): fits the same handles
    dx.upload(0, up(y))
    T._lib.check(lib.ttn_tt_split_sites(dx.h, dz.h, T.tt._i64([3, 2, 1]), T.tt._i64(flat(SD)), 0.0))
    T.device.compress_status(dz)
    got = dz.download(0)
    assert list(got.ttv_rks) == R.to_qtt(y, SD).ttv_rks
    assert tensor_err(got, R.dense(y).reshape(flat(SD))) <= 1e-12 * np.max(np.abs(R.dense(y)))


# ---- merge ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def x65():
    return R.random_train((3, 5, 2, 4), (1, 17, 65, 3, 1), seed=24)


@pytest.mark.parametrize("groups", [[2, 2], [1, 3], [4], [1, 1, 1, 1]], ids=str)
def test_merge_cores_match_the_restatement(x65, groups):
    """odd sizes, a rank on each side of the 16 and 64 tile edges; groups of one (copies), two, three and four cores"""
    ref = R.to_ttv(x65, groups)
    got = T.to_ttv(up(x65), groups)
    assert isinstance(got, T.TTvector) and got.ttv_dims == ref.ttv_dims and list(got.ttv_rks) == ref.ttv_rks
    assert list(got.ttv_ot) == [0] * len(groups)
    for k, (a, b) in enumerate(zip(got.ttv_vec, ref.ttv_vec)):
        err = float(np.max(np.abs(np.asarray(a) - b)))
        print("merge core", k, err / np.max(np.abs(b)))
        assert err <= 1e-13 * np.max(np.abs(b))


@pytest.mark.parametrize("dims,rks,groups", [((3, 20), (1, 17, 1), [2]), ((20, 20), (2, 5, 3), [2]), ((2, 3, 37), (1, 2, 18, 2), [3])], ids=str)
def test_merge_wide_second_operand(dims, rks, groups):
    """n2 > 16: the merged index of a workgroup is a run of i2 alone, with a tail chunk (20 = 16 + 4, 37 = 2 * 16 + 5)"""
    x = R.random_train(dims, rks, seed=25)
    ref = R.to_ttv(x, groups)
    got = T.to_ttv(up(x), groups)
    assert got.ttv_dims == ref.ttv_dims and list(got.ttv_rks) == ref.ttv_rks
    for a, b in zip(got.ttv_vec, ref.ttv_vec):
        assert np.max(np.abs(np.asarray(a) - b)) <= 1e-13 * np.max(np.abs(b))


def test_merge_batch_with_different_ranks():
    dims, cap = (2, 3, 2, 2, 3), [1, 5, 18, 7, 3, 1]
    rks = [[1, 5, 18, 7, 3, 1], [1, 1, 1, 1, 1, 1], [1, 2, 17, 3, 2, 1], [1, 4, 6, 7, 1, 1]]
    trains = [R.random_train(dims, r, seed=40 + b) for b, r in enumerate(rks)]
    dx = T.DeviceTT(dims, cap, batch=4)
    for b, x in enumerate(trains):
        dx.upload(b, up(x))
    dz = dx.merge_sites([2, 3])
    T.device.compress_status(dz)
    assert dz.dims == (6, 12) and dz.cap == [1, 18, 1]
    for b, x in enumerate(trains):
        ref = R.to_ttv(x, [2, 3])
        got = dz.download(b)
        assert list(got.ttv_rks) == ref.ttv_rks
        for a, c in zip(got.ttv_vec, ref.ttv_vec):
            assert np.max(np.abs(np.asarray(a) - c)) <= 1e-13 * np.max(np.abs(c))


# ---- both -----------------------------------------------------------------------------------------------------------------------
def test_round_trip(x12):
    x, full, _ = x12
    back = T.to_ttv(T.to_qtt(up(x), SD), [len(s) for s in SD])
    assert back.ttv_dims == (12, 6, 4) and list(back.ttv_rks) == [1, 5, 3, 1]
    assert tensor_err(back, full) <= 1e-12 * np.max(np.abs(full))
    q = T.QTTvector(T.to_qtt(T.rand_tt((4, 4), 3, seed=5), [[2, 2], [2, 2]]), 2, 2, "serial")     # a QTTvector counts as its TTvector
    assert isinstance(T.to_ttv(q, [2, 2]), T.TTvector) and T.to_ttv(q, [2, 2]).ttv_dims == (4, 4)
    assert isinstance(T.to_qtt(q, [[2]] * 4), T.TTvector)


def _refused(rc, code, name):
    assert rc == code, (rc, T._lib.last_error())
    assert name in T._lib.last_error(), T._lib.last_error()


def test_refusals_name_the_call_and_leave_the_library_usable():
    lib, i64, L = T._lib.lib(), T.tt._i64, T._lib
    x = T.DeviceTT.from_host(T.rand_tt((4, 4), 3, seed=1))
    xb = T.DeviceTT.from_host(T.rand_tt((4, 4), 3, seed=1), batch=2)
    z4 = T.DeviceTT((2, 2, 2, 2), [1, 2, 3, 6, 1])
    z3 = T.DeviceTT((2, 2, 2), [1, 2, 3, 1])
    zbad = T.DeviceTT((2, 2, 2, 3), [1, 2, 3, 6, 1])
    split = "ttn_tt_split_sites"
    _refused(lib.ttn_tt_split_sites(x.h, z3.h, i64([2, 2]), i64([2, 2, 2, 2]), 0.0), L.TTN_ERR_ARG, split)          # sum(nsplit) != z's sites
    _refused(lib.ttn_tt_split_sites(x.h, z4.h, i64([2, 2]), i64([2, 3, 2, 2]), 0.0), L.TTN_ERR_ARG, split)          # prod != the site's dimension
    _refused(lib.ttn_tt_split_sites(x.h, zbad.h, i64([2, 2]), i64([2, 2, 2, 2]), 0.0), L.TTN_ERR_ARG, split)        # z.dims != flattened lists
    _refused(lib.ttn_tt_split_sites(xb.h, z4.h, i64([2, 2]), i64([2, 2, 2, 2]), 0.0), L.TTN_ERR_ARG, split)         # batch
    _refused(lib.ttn_tt_split_sites(x.h, z4.h, None, i64([2, 2, 2, 2]), 0.0), L.TTN_ERR_ARG, split)                 # null pointer
    _refused(lib.ttn_tt_split_sites(None, z4.h, i64([2, 2]), i64([2, 2, 2, 2]), 0.0), L.TTN_ERR_ARG, split)
    xc = T.DeviceTT((4, 4), [1, 3, 1], dtype=np.complex128)
    with pytest.raises(T.TTNError, match=split):
        xc.split_sites([[2, 2], [2, 2]])
    _refused(lib.ttn_tt_split_sites(xc.h, z4.h, i64([2, 2]), i64([2, 2, 2, 2]), 0.0), L.TTN_ERR_UNSUPPORTED, split)
    # an unfolding above the limits of the SVD step: (2049 * 2) x (2 * 2049), short side 4098 > 4096
    big = T.TTvector(3, [np.zeros((2, 1, 2049), order="F"), np.zeros((4, 2049, 2049), order="F"), np.zeros((2, 2049, 1), order="F")],
                     (2, 4, 2), [1, 2049, 2049, 1], [0, 0, 0])
    xbig = T.DeviceTT.from_host(big)
    zbig = T.DeviceTT((2, 2, 2, 2), [1, 2049, 1, 2049, 1])
    _refused(lib.ttn_tt_split_sites(xbig.h, zbig.h, i64([1, 2, 1]), i64([2, 2, 2, 2]), 0.0), L.TTN_ERR_UNSUPPORTED, split)
    xbig.free(); zbig.free()
    merge = "ttn_tt_merge_sites"
    q = T.DeviceTT.from_host(T.rand_tt((2, 2, 2, 2), 3, seed=2))
    qb = T.DeviceTT.from_host(T.rand_tt((2, 2, 2, 2), 3, seed=2), batch=2)
    m2 = T.DeviceTT((4, 4), [1, 3, 1])
    _refused(lib.ttn_tt_merge_sites(q.h, m2.h, i64([2, 1]), 2), L.TTN_ERR_ARG, merge)                                # sum(merge_numbers) != x's sites
    _refused(lib.ttn_tt_merge_sites(q.h, m2.h, i64([3, 1]), 2), L.TTN_ERR_ARG, merge)                                # z.dims != merged products
    _refused(lib.ttn_tt_merge_sites(q.h, z3.h, i64([2, 2]), 2), L.TTN_ERR_ARG, merge)                                # groups != z's sites
    _refused(lib.ttn_tt_merge_sites(qb.h, m2.h, i64([2, 2]), 2), L.TTN_ERR_ARG, merge)                               # batch
    _refused(lib.ttn_tt_merge_sites(q.h, m2.h, None, 2), L.TTN_ERR_ARG, merge)
    qc = T.DeviceTT((2, 2, 2, 2), [1, 2, 3, 2, 1], dtype=np.complex128)
    with pytest.raises(T.TTNError, match=merge):
        qc.merge_sites([2, 2])
    # the reference's assertions at the host level
    tt = T.rand_tt((4, 4), 3, seed=1)
    with pytest.raises(AssertionError, match="one entry per TT core"):
        T.to_qtt(tt, [[2, 2]])
    with pytest.raises(AssertionError, match="must equal 4"):
        T.to_qtt(tt, [[2, 2], [2, 3]])
    with pytest.raises(AssertionError, match="must sum to 2"):
        T.to_ttv(tt, [1, 2])
    # valid calls on the same handles afterwards
    T._lib.check(lib.ttn_tt_split_sites(x.h, z4.h, i64([2, 2]), i64([2, 2, 2, 2]), 0.0))
    T.device.compress_status(z4)
    T._lib.check(lib.ttn_tt_merge_sites(z4.h, m2.h, i64([2, 2]), 2))
    T.device.compress_status(m2)
    want = R.dense(R.Train(x.download(0).ttv_vec))
    assert tensor_err(m2.download(0), want) <= 1e-12 * np.max(np.abs(want))


def test_interpolation_3d_chain():
    """examples/interpolation_3d.jl: a cross train on fused 8-point sites (one site per level, index 4 bx + 2 by + bz) -> to_qtt ->
    QTTvector(interleaved) -> qttv_to_array, and reorder to serial.  The split may add nothing beyond rounding to the error e0 of the
    cross train itself."""
    bits = 4
    grid = np.arange(2 ** bits) / (2 ** bits - 1.0)             # function_to_qttv's grid on [0, 1]

    def g(x, y, z):
        return 1.0 / np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2 + 0.01)

    def f(X):
        v = (X.cpu().numpy() if hasattr(X, "cpu") else np.asarray(X)).astype(np.int64) - 1      # (P, 4): the fused index per level
        gi = [sum(((v[:, l] >> (2 - dim)) & 1) << (bits - 1 - l) for l in range(bits)) for dim in range(3)]
        return g(grid[gi[0]], grid[gi[1]], grid[gi[2]])

    exact = g(grid[:, None, None], grid[None, :, None], grid[None, None, :])
    tt = T.tt_cross(f, (8,) * bits, T.MaxVol(verbose=False, tol=1e-8), ranks=4, seed=3)
    # the cross train on the grid: axes (level, dim) -> (dim, level)
    fused = R.dense(R.Train(tt.ttv_vec)).reshape((2,) * (3 * bits))
    order = [3 * l + dim for dim in range(3) for l in range(bits)]
    e0 = float(np.max(np.abs(fused.transpose(order).reshape((2 ** bits,) * 3) - exact)))
    bound = e0 + 1e-12 * np.max(np.abs(exact))
    q = T.QTTvector(T.to_qtt(tt, [[2, 2, 2]] * bits), 3, bits, "interleaved")
    e1 = float(np.max(np.abs(T.qttv_to_array(q) - exact)))
    e2 = float(np.max(np.abs(T.qttv_to_array(q.reorder("serial")) - exact)))
    print("cross error", e0, "after the split", e1, "after reorder", e2, "ranks", tt.ttv_rks)
    assert e0 < 1e-3 * np.max(np.abs(exact))                      # the chain is only worth testing on a train that interpolates g
    assert e1 <= bound and e2 <= bound
