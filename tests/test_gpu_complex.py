"""ComplexF64 trains on the device (csrc/ttn_cplx_kernels.h) against the CPU oracle on the same inputs: handles and
refusals, apply (complex x complex and the two mixed forms), + / hadamard / scalar *, dot / norm, the bond step and tt_compress_,
the QFT operator (``fourier_qtto``) against the reference's known answers and numpy.fft, and a train from the real-time TDVP driver.

The oracle computes with complex cores as it stands (``apply`` is an einsum, ``dot`` conjugates its first argument, ``svdtrunc`` is
LAPACK gesdd, ``add`` takes the result type); its ``hadamard`` allocates real cores, so that one product is restated here.

Bars (the real case): layout and ranks exact; apply elementwise 4 n eps (|A_k| * |X_k|) — the bound of an n-term sum in any
order, doubled because a complex product is a pair of two-term real sums; + bitwise; hadamard and scalar * 4 eps |x| |y|; dot 1e-12 of
||a|| ||b||; compress: ranks equal, per-bond singular values rtol 1e-10 + 1e-13 sigma_1, tensor 1e-9.  An input of the ill-posed class
(a kept singular value <= 1e-13 sigma_1 in the ORACLE's own run: LAPACK's and Jacobi's null vectors may differ) is held to the
approximation error against the unrounded input instead; the share of such cases is asserted."""
import ctypes as C
import math

import numpy as np
import pytest

import ttn_amd as T
from oracle import tt_oracle as O
from tests import fourier_reference as FR
from tests.helpers import to_oracle, to_product, worst_of
from tests.test_gpu_opalg import CASES
from ttn_amd import _lib
from ttn_amd import device as D

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
UNSUP = _lib.TTN_ERR_UNSUPPORTED


@pytest.fixture(scope="module", autouse=True)
def _init():
    T.ensure_init(0)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def crand(shape, rng):
    return np.asfortranarray(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def crand_tt(dims, rks, rng, cplx=True):
    d = len(dims)
    vec = [crand((dims[k], rks[k], rks[k + 1]), rng) if cplx else np.asfortranarray(rng.standard_normal((dims[k], rks[k], rks[k + 1])))
           for k in range(d)]
    return O.TTvector(d, vec, tuple(dims), list(rks), [0] * d)


def crand_tto(dims, rks, rng, cplx=True):
    d = len(dims)
    vec = [crand((dims[k], dims[k], rks[k], rks[k + 1]), rng) if cplx
           else np.asfortranarray(rng.standard_normal((dims[k], dims[k], rks[k], rks[k + 1]))) for k in range(d)]
    return O.TToperator(d, vec, tuple(dims), list(rks), [0] * d)


def qtt_ranks(d, r):
    return O.r_and_d_to_rks([r] * (d + 1), (2,) * d)


def dense(x):
    return FR._dense(x if isinstance(x, O.TTvector) else to_oracle(x))


def rel(a, b):
    ta, tb = dense(a), dense(b)
    return float(np.linalg.norm(ta - tb) / max(np.linalg.norm(tb), 1e-300))


def up(x, batch=1, cap=None):
    return D.DeviceTT.from_host(to_product(x), batch=batch, cap_rks=cap)


def dev_apply(A, x):
    dA, dx = D.DeviceTTO(to_product(A)), up(x)
    dy = D.DeviceTT(x.ttv_dims, [a * b for a, b in zip(A.tto_rks, x.ttv_rks)], 1, dtype=np.complex128)
    D.apply(dA, dx, dy)
    return dy.download(0)


def hadamard_ref(x, y):
    vec = [np.stack([np.kron(a[s], b[s]) for s in range(a.shape[0])]) for a, b in zip(x.ttv_vec, y.ttv_vec)]
    return O.TTvector(x.N, vec, x.ttv_dims, [p * q for p, q in zip(x.ttv_rks, y.ttv_rks)], [0] * x.N)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- handles --------------------------------------------------------------------------------------------------------------------
def test_handles_roundtrip_and_replicate():
    rng = np.random.default_rng(1)
    dims, rks = (2, 3, 2, 4), [1, 3, 5, 2, 1]
    for cplx in (True, False):
        x = crand_tt(dims, rks, rng, cplx)
        x.ttv_ot = [1, 0, -1, -1]
        h = D.DeviceTT(dims, [1, 4, 7, 3, 1], 3, dtype=np.complex128 if cplx else np.float64)       # capacity above the ranks
        h.upload(1, to_product(x))
        flag = C.c_int(-1)
        _lib.check(_lib.lib().ttn_tt_dtype(h.h, C.byref(flag)))
        assert flag.value == int(cplx)
        got = h.download(1)
        assert got.ttv_rks == rks and got.ttv_ot == x.ttv_ot
        assert all(same_bits(g, np.asfortranarray(c)) for g, c in zip(got.ttv_vec, x.ttv_vec))
        h.replicate(1)
        for b in (0, 2):
            rep = h.download(b)
            assert rep.ttv_rks == rks and all(same_bits(g, np.asfortranarray(c)) for g, c in zip(rep.ttv_vec, x.ttv_vec))
        assert h.max_ranks() == rks
        g2 = D.DeviceTT(dims, rks, 3, dtype=h.dtype)
        _lib.check(_lib.lib().ttn_tt_copy(g2.h, h.h))
        assert all(same_bits(g, np.asfortranarray(c)) for g, c in zip(g2.download(2).ttv_vec, x.ttv_vec))
    A = crand_tto((2, 3), [1, 4, 1], rng)
    dA = D.DeviceTTO(to_product(A))
    assert dA.dtype is np.complex128
    back = dA.download()
    assert all(same_bits(g, np.asfortranarray(c)) for g, c in zip(back.tto_vec, A.tto_vec))
    flag = C.c_int(-1)
    _lib.check(_lib.lib().ttn_tto_dtype(dA.h, C.byref(flag)))
    assert flag.value == 1
    D.status_all()


def test_unsupported_combinations_are_refused():
    """every Float64-only entry point that receives a complex handle, and every complex op whose operands do not fit, returns
    TTN_ERR_UNSUPPORTED with a message; the handles keep their contents and no failure is recorded"""
    L = _lib.lib()
    rng = np.random.default_rng(2)
    d, dims = 4, (2, 2, 2, 2)
    rks = qtt_ranks(d, 2)
    xc, xr = crand_tt(dims, rks, rng), crand_tt(dims, rks, rng, cplx=False)
    c, c2, r = up(xc), up(xc, cap=[1, 4, 4, 4, 1]), up(xr)
    r2 = up(xr, cap=[1, 4, 4, 4, 1])
    Ac, Ar = D.DeviceTTO(to_product(crand_tto(dims, [1, 2, 2, 2, 1], rng))), D.DeviceTTO(to_product(O.Delta(d)))
    i64 = lambda v: (C.c_int64 * len(v))(*v)
    out, buf = C.c_void_p(), (C.c_double * 64)()
    one, dd = i64([2]), (C.c_double * 16)()
    calls = {
        "orthogonalize": lambda: L.ttn_orthogonalize(c.h, 1, c2.h),
        "hadamard_ttm": lambda: L.ttn_hadamard_ttm(c.h, c.h, c2.h, 1e-12, 4, 4),
        "swap_sites": lambda: L.ttn_swap_sites(c.h, 1, i64([1]), 0.0),
        "ttv_decomp": lambda: L.ttn_ttv_decomp(c.h, buf, 1, 1e-12),
        "als_linsolve": lambda: L.ttn_als_linsolve(Ar.h, c.h, c.h, c2.h, 2),
        "als_linsolve (complex operator)": lambda: L.ttn_als_linsolve(Ac.h, r.h, r.h, r2.h, 2),
        "mals_linsolve": lambda: L.ttn_mals_linsolve(Ar.h, c.h, c.h, c2.h, 1e-8, 4),
        "dmrg_linsolve": lambda: L.ttn_dmrg_linsolve(Ar.h, c.h, c.h, c2.h, 1e-8, 1, one, i64([4])),
        "dmrg_linsolve_it": lambda: L.ttn_dmrg_linsolve_it(Ar.h, c.h, c.h, c2.h, 1e-8, 1, one, i64([4]), 1, 10, 1e-8, 16),
        "dmrg_eigsolve": lambda: L.ttn_dmrg_eigsolve(Ar.h, c.h, c2.h, 1e-8, 1, one, i64([4]), 0, 10, 1e-8, 256, 16, dd, i64([0] * 16)),
        "mals_eigsolve": lambda: L.ttn_mals_eigsolve(Ar.h, c.h, c2.h, 1e-8, 1, one, i64([4]), 0, 10, 1e-8, 256, 16, dd, i64([0] * 16)),
        "als_eigsolve": lambda: L.ttn_als_eigsolve(Ar.h, c.h, c2.h, 1, one, i64([4]), None, 0, 0, 10, 1e-8, 256, 6, dd),
        "als_gen_eigsolve": lambda: L.ttn_als_gen_eigsolve(Ar.h, Ar.h, c.h, c2.h, 1, one, i64([4]), 0, 256, 6, dd),
        "tto_mul": lambda: L.ttn_tto_mul(Ac.h, Ar.h, C.byref(out)),
        "tto_inner": lambda: L.ttn_tto_inner(Ar.h, Ac.h, C.byref(out)),
        "tto_add": lambda: L.ttn_tto_add(Ac.h, Ac.h, C.byref(out)),
        "tto_scale": lambda: L.ttn_tto_scale(2.0, Ac.h, C.byref(out)),
        "tto_kron": lambda: L.ttn_tto_kron(Ac.h, Ar.h, C.byref(out)),
        "tto_compress": lambda: L.ttn_tto_compress(Ac.h, 4, 0.0, 1, C.byref(out)),
        "tto_to_tt": lambda: L.ttn_tto_to_tt(Ac.h, r.h),
        "tto_from_tt": lambda: L.ttn_tto_from_tt(c.h, 0, C.byref(out)),
        "tt_outer": lambda: L.ttn_tt_outer(c.h, c.h, 0, C.byref(out)),
        "tt_diag_tto": lambda: L.ttn_tt_diag_tto(c.h, 0, C.byref(out)),
        "tt_kron": lambda: L.ttn_tt_kron(c.h, c.h, c2.h),
        "apply_begin": lambda: L.ttn_apply_begin(Ar.h, c.h, c2.h),
        "apply_sweep": lambda: L.ttn_apply_sweep(Ar.h, c.h, c2.h, 1, 2, 4, 0.0, 0),
        "core_extent": lambda: L.ttn_tt_core_extent(c.h, 1, None, None, None),
        "core_export": lambda: L.ttn_tt_core_export(c.h, 1, buf, buf),
        "core_import": lambda: L.ttn_tt_core_import(c.h, 1, buf, buf, 1, 2),
        "sv_capture": lambda: L.ttn_sv_capture(c.h, 1),
        "scale_batch": lambda: L.ttn_scale_batch((C.c_double * 1)(2.0), c.h, c2.h),
        # complex ops whose operands differ in element type
        "add mixed": lambda: L.ttn_add(c.h, r.h, c2.h),
        "add real output": lambda: L.ttn_add(c.h, c.h, r2.h),
        "hadamard mixed": lambda: L.ttn_hadamard(c.h, r.h, c2.h),
        "dot mixed": lambda: L.ttn_dot(c.h, r.h, dd),
        "scale mixed": lambda: L.ttn_scale(2.0, c.h, r2.h),
        "scale_c64 on real handles": lambda: L.ttn_scale_c64(1.0, 1.0, r.h, r2.h),
        "copy mixed": lambda: L.ttn_tt_copy(r2.h, c.h),
        "apply real x real into complex": lambda: L.ttn_apply(Ar.h, r.h, c2.h),
        "apply complex into real": lambda: L.ttn_apply(Ac.h, c.h, r2.h),
        "apply_compress complex into real": lambda: L.ttn_apply_compress(Ac.h, c.h, r2.h, 4, 0.0, 1),
    }
    for name, call in calls.items():
        rc = call()
        assert rc == UNSUP, (name, rc, _lib.last_error())
        assert _lib.last_error(), name
        assert not out.value, name
    D.status_all()
    # nothing was written: the operands still hold what was uploaded
    assert all(same_bits(g, np.asfortranarray(v)) for g, v in zip(c.download(0).ttv_vec, xc.ttv_vec))
    assert all(same_bits(g, np.asfortranarray(v)) for g, v in zip(c2.download(0).ttv_vec, xc.ttv_vec))
    assert all(same_bits(g, np.asfortranarray(v)) for g, v in zip(r2.download(0).ttv_vec, xr.ttv_vec))
    # the host interface raises instead of dropping an imaginary part
    with pytest.raises(TypeError, match="complex"):
        T.orthogonalize(to_product(xc))
    with pytest.raises(TypeError, match="complex"):
        r.upload(0, to_product(xc))


# ---- apply ----------------------------------------------------------------------------------------------------------------------
APPLY_SHARE = {}


@pytest.mark.parametrize("form", ["cc", "rc", "cr"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_apply_against_oracle(case, form):
    dims, Ar, xr = CASES[case]
    rng = np.random.default_rng(100 + case)
    A = crand_tto(dims, Ar, rng, cplx=form[0] == "c")
    x = crand_tt(dims, xr, rng, cplx=form[1] == "c")
    got = dev_apply(A, x)
    ref = O.apply(A, x)
    assert got.ttv_rks == ref.ttv_rks and got.ttv_ot == [0] * len(dims)
    share = 0.0
    for k, (g, r_) in enumerate(zip(got.ttv_vec, ref.ttv_vec)):
        assert g.shape == r_.shape and g.dtype == np.complex128
        n = dims[k]
        bound = 4 * n * EPS * O.apply(O.TToperator(1, [np.abs(A.tto_vec[k])], (n,), [Ar[k], Ar[k + 1]], [0]),
                                      O.TTvector(1, [np.abs(x.ttv_vec[k])], (n,), [xr[k], xr[k + 1]], [0])).ttv_vec[0]
        err = np.abs(g - r_)
        assert np.all(err <= bound), (k, float(np.max(err / bound)))
        share = worst_of(share, float(np.max(err / bound)))
    APPLY_SHARE[(case, form)] = share
    print("apply case %d %s: largest share of the bound %.3f" % (case, form, share))
    # the stateless entry point takes the same path
    if case < 2:
        got2 = T.apply(to_product(A), to_product(x))
        assert all(same_bits(a, b) for a, b in zip(got2.ttv_vec, got.ttv_vec))


def test_apply_batch():
    """a batch of different trains under one complex operator: every train is the single-train result"""
    rng = np.random.default_rng(7)
    d = 6
    rks = qtt_ranks(d, 5)
    A = crand_tto((2,) * d, [1, 3, 4, 3, 4, 3, 1], rng)
    xs = [crand_tt((2,) * d, rks, rng) for _ in range(5)]
    dx = D.DeviceTT((2,) * d, rks, 5, dtype=np.complex128)
    for b, x in enumerate(xs):
        dx.upload(b, to_product(x))
    dy = D.DeviceTT((2,) * d, [a * b for a, b in zip(A.tto_rks, rks)], 5, dtype=np.complex128)
    D.apply(D.DeviceTTO(to_product(A)), dx, dy)
    for b, x in enumerate(xs):
        assert all(same_bits(a, c) for a, c in zip(dy.download(b).ttv_vec, dev_apply(A, x).ttv_vec))


# ---- + / hadamard / scalar * ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(4))
def test_add_hadamard_scale(case):
    dims, ra, rb = CASES[case]
    rng = np.random.default_rng(200 + case)
    x, y = crand_tt(dims, ra, rng), crand_tt(dims, rb, rng)
    px, py = to_product(x), to_product(y)
    if len(dims) >= 2:
        s = T.add(px, py)
        ref = O.add(x, y)
        assert s.ttv_rks == ref.ttv_rks
        assert all(same_bits(g, np.asfortranarray(r_)) for g, r_ in zip(s.ttv_vec, ref.ttv_vec))
        assert all(same_bits(g, h) for g, h in zip((px + py).ttv_vec, s.ttv_vec))
        diff = T.sub(px, py)                                            # (-1.0) * y + x
        assert rel(diff, O.add(O.scale(-1.0, y), x)) <= 8 * EPS
    h = T.hadamard(px, py)
    href = hadamard_ref(x, y)
    assert h.ttv_rks == href.ttv_rks
    for g, r_, a, b in zip(h.ttv_vec, href.ttv_vec, x.ttv_vec, y.ttv_vec):
        bound = 4 * EPS * np.stack([np.kron(np.abs(a[s_]), np.abs(b[s_])) for s_ in range(a.shape[0])])
        assert g.shape == r_.shape and np.all(np.abs(g - r_) <= bound)
    for a_, ot in ((0.7 - 1.3j, [0] * len(dims)), (2.5, [1] + [0] * (len(dims) - 1)), (1j, [1] * len(dims)), (0.0, [1] * len(dims))):
        x.ttv_ot = list(ot)
        got = T.scale(a_, to_product(x))
        which = next((k for k, o in enumerate(ot) if o == 0), 0)
        assert got.ttv_ot == ([0] * len(dims) if a_ == 0 else list(ot))
        for k, (g, c) in enumerate(zip(got.ttv_vec, x.ttv_vec)):
            if a_ == 0:
                assert not np.any(g)
            elif k != which:
                assert same_bits(g, np.asfortranarray(c))
            else:
                assert np.all(np.abs(g - a_ * c) <= 4 * EPS * abs(a_) * np.abs(c))
    x.ttv_ot = [0] * len(dims)
    # the handle forms: one factor per train
    dx = up(x, batch=3)
    dy = D.DeviceTT(dims, ra, 3, dtype=np.complex128)
    fac = [0.5 + 0.25j, 0.0, -2.0j]
    D.scale_batch(fac, dx, dy)
    for b, f in enumerate(fac):
        g = dy.download(b)
        if f == 0:
            assert not any(np.any(c) for c in g.ttv_vec)
        else:
            assert np.all(np.abs(g.ttv_vec[0] - f * x.ttv_vec[0]) <= 4 * EPS * abs(f) * np.abs(x.ttv_vec[0]))
            assert all(same_bits(a, np.asfortranarray(c)) for a, c in zip(g.ttv_vec[1:], x.ttv_vec[1:]))
    D.status_all()


# ---- dot / norm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CASES)))
def test_dot_norm(case):
    dims, ra, rb = CASES[case]
    rng = np.random.default_rng(300 + case)
    a, b = crand_tt(dims, ra, rng), crand_tt(dims, rb, rng)
    na, nb = O.norm(a), O.norm(b)
    got, ref = T.dot(to_product(a), to_product(b)), O.dot(a, b)
    assert isinstance(got, complex)
    assert abs(got - ref) <= 1e-12 * na * nb
    assert abs(T.dot(to_product(b), to_product(a)) - np.conj(ref)) <= 1e-12 * na * nb
    assert abs(T.norm(to_product(a)) - na) <= 1e-12 * na
    # the side of the conjugation: dot(i x, x) = -i ||x||^2
    ia = O.scale(1j, a)
    assert abs(T.dot(to_product(ia), to_product(a)) - (-1j) * na ** 2) <= 1e-12 * na ** 2
    assert abs(T.euclidean_distance(to_product(a), to_product(a))) <= 1e-6 * na
    # handles, a batch with different trains
    da, db = D.DeviceTT(dims, ra, 2, dtype=np.complex128), D.DeviceTT(dims, [max(p, q) for p, q in zip(ra, rb)], 2, dtype=np.complex128)
    da.upload(0, to_product(a)); da.upload(1, to_product(ia))
    db.upload(0, to_product(b)); db.upload(1, to_product(a))
    out = D.dot(da, db)
    assert out.dtype == np.complex128 and abs(out[0] - ref) <= 1e-12 * na * nb and abs(out[1] + 1j * na ** 2) <= 1e-12 * na ** 2
    assert np.all(np.abs(D.norm(da) - na) <= 1e-12 * na)


# ---- bond step and tt_compress_ -------------------------------------------------------------------------------------------------
def ill_posed(svals):
    """a kept singular value <= 1e-13 sigma_1 in the oracle's own run"""
    return any(len(s) and s[-1] <= 1e-13 * s[0] for s in svals)


def random_case_inputs(seed, d=8):
    """a random complex train of d = 8 sites with ranks min(what the dimensions allow, rmax), rmax <= 16.  Most seeds take rmax = 16:
    then no bond is rank deficient against its neighbours and the problem is well posed for every max_bond / truncerr of the grid.  The
    seeds with a smaller rmax carry a middle bond whose merged matrix (16 x 16) has rank rmax < 16: with max_bond = 16 and truncerr = 0
    the reference GROWS it by null vectors — the ill-posed class, 4 of the 64 cases of the grid."""
    rng = np.random.default_rng(seed)
    rmax = {506: 12, 507: 9}.get(seed, 16)
    return crand_tt((2,) * d, qtt_ranks(d, rmax), rng)


COMPRESS_GRID = [(mb, te, sw) for mb in (4, 16) for te in (0.0, 1e-8) for sw in (1, 2)]
BATCH_SEEDS = list(range(500, 508))


def oracle_compress(x, mb, te, sw):
    sv = []
    y = O.tt_compress_(O.copy_tt(x), mb, truncerr=te, sweeps=sw, svals_out=sv)
    return y, sv


def check_compressed(got, x, ref, sv, tag):
    """ranks, then the tensor bar — or, for an ill-posed input, the approximation error against the unrounded input"""
    assert got.ttv_rks == ref.ttv_rks, (tag, got.ttv_rks, ref.ttv_rks)
    if ill_posed(sv):
        e_dev, e_ref = rel(got, x), rel(ref, x)
        print("%s: ill-posed, approximation error device %.3e oracle %.3e" % (tag, e_dev, e_ref))
        assert e_dev <= 1.5 * e_ref + 1e-9, (tag, e_dev, e_ref)          # the rule of test_compress_fuzz_ragged_ranks
        return True
    e = rel(got, ref)
    print("%s: ||y_gpu - y_ref|| / ||y_ref|| = %.3e" % (tag, e))
    assert e <= 1e-9, (tag, e)
    return False


def test_bond_step_singular_values():
    """every bond of a random complex train, each from the fresh input: rank, the kept singular values (the squared column norms of
    U sqrt(S), the squared row norms of sqrt(S) V^H) and the tensor"""
    x = random_case_inputs(41)
    d = x.N
    for k in range(1, d):
        for mb, te in ((4, 0.0), (16, 0.0), (16, 1e-8)):
            sv = []
            ref = O.copy_tt(x)
            O.tt_bond_truncate_(ref, k, max_bond=mb, truncerr=te, svals_out=sv)
            got = to_product(O.copy_tt(x))
            T._tt_bond_truncate_(got, k, max_bond=mb, truncerr=te)
            assert got.ttv_rks == ref.ttv_rks, (k, mb, te)
            s = sv[0]
            s_left = np.sum(np.abs(got.ttv_vec[k - 1]) ** 2, axis=(0, 1))
            s_right = np.sum(np.abs(got.ttv_vec[k]) ** 2, axis=(0, 2))
            tol = 1e-10 * s + 1e-13 * s[0]
            assert np.all(np.abs(s_left - s) <= tol) and np.all(np.abs(s_right - s) <= tol), (k, mb, te)
            assert rel(got, ref) <= 1e-9
            for j in range(d):
                if j not in (k - 1, k):
                    assert same_bits(got.ttv_vec[j], np.asfortranarray(x.ttv_vec[j]))


def test_compress_random_batches():
    """(i): d = 8, ranks <= 16, max_bond in {4, 16}, truncerr in {0, 1e-8}, one and two sweeps, 8 different trains in one launch"""
    xs = [random_case_inputs(s) for s in BATCH_SEEDS]
    d, dims = xs[0].N, xs[0].ttv_dims
    cap0 = [max(x.ttv_rks[m] for x in xs) for m in range(d + 1)]
    n_ill = n_all = 0
    for mb, te, sw in COMPRESS_GRID:
        need = [max(D.compress_rank_bound(dims, x.ttv_rks, mb, sw)[0][m] for x in xs) for m in range(d + 1)]
        h = D.DeviceTT(dims, [max(a, b) for a, b in zip(cap0, need)], len(xs), dtype=np.complex128)
        for b, x in enumerate(xs):
            h.upload(b, to_product(x))
        D.tt_compress_(h, mb, truncerr=te, sweeps=sw)
        D.compress_status(h)
        for b, x in enumerate(xs):
            ref, sv = oracle_compress(x, mb, te, sw)
            n_ill += check_compressed(h.download(b), x, ref, sv, "mb %d te %g sw %d train %d" % (mb, te, sw, b))
            n_all += 1
        # the last bond step of the call (bond 1 of the last right-to-left pass): its singular values from the cores
        ref, sv = oracle_compress(xs[0], mb, te, sw)
        if not ill_posed(sv):
            s, g = sv[-1], h.download(0)
            s_left = np.sum(np.abs(g.ttv_vec[0]) ** 2, axis=(0, 1))
            assert np.all(np.abs(s_left - s) <= 1e-10 * s + 1e-13 * s[0])
    print("ill-posed share of (i): %d / %d" % (n_ill, n_all))
    assert 4 * n_ill <= n_all
    # the stateless entry point is the same kernel
    x = xs[3]
    got = T.tt_compress_(to_product(O.copy_tt(x)), 16, truncerr=1e-8)
    ref, sv = oracle_compress(x, 16, 1e-8, 1)
    check_compressed(got, x, ref, sv, "stateless")
    D.status_all()


def qft_inputs():
    rng = np.random.default_rng(77)
    return {"qtt_sin": O.qtt_sin(8, lam=math.pi), "qtt_exp": O.qtt_exp(8), "complex rank 4": crand_tt((2,) * 8, qtt_ranks(8, 4), rng)}


@pytest.mark.parametrize("name", ["qtt_sin", "qtt_exp", "complex rank 4"])
def test_compress_qft_products(name):
    """(ii): fourier_qtto(8; K = 25) * x, max_bond = 32, truncerr = 1e-10 — complex operator on a real train for the first two; the
    merged matrices have a short side above 96, so the square factor lives in global memory; none of these may be ill-posed"""
    x = qft_inputs()[name]
    F = to_oracle(T.fourier_qtto(8, K=25))
    y = O.apply(F, x)
    ref, sv = oracle_compress(y, 32, 1e-10, 1)
    assert not ill_posed(sv)
    got = T.tt_compress_(T.apply(to_product(F), to_product(x)), 32, truncerr=1e-10)
    assert not check_compressed(got, y, ref, sv, "qft * " + name)
    # apply_compress on handles: apply, then round
    dF, dx = D.DeviceTTO(to_product(F)), up(x)
    need = D.compress_rank_bound(x.ttv_dims, y.ttv_rks, 32)[0]          # (a rank-deficient bond of the product can grow up to max_bond)
    dy = D.DeviceTT(x.ttv_dims, need, 1, dtype=np.complex128)
    D.apply_compress(dF, dx, dy, 32, truncerr=1e-10)
    D.compress_status(dy)
    g2 = dy.download(0)
    assert g2.ttv_rks == got.ttv_rks and all(same_bits(a, b) for a, b in zip(g2.ttv_vec, got.ttv_vec))
    g3 = T.apply_compress(to_product(F), to_product(x), 32, truncerr=1e-10)
    assert g3.ttv_rks == got.ttv_rks and all(same_bits(a, b) for a, b in zip(g3.ttv_vec, got.ttv_vec))
    D.status_all()


def test_compress_limits_refused():
    """a merged matrix beyond 512 x 8192 is refused before any launch"""
    rks = [1, 2, 600, 2, 1]
    h = D.DeviceTT((2, 512, 512, 2), rks, 1, dtype=np.complex128)
    x = O.TTvector(4, [np.zeros((n, rks[k], rks[k + 1]), dtype=complex) for k, n in enumerate((2, 512, 512, 2))], (2, 512, 512, 2), rks, [0] * 4)
    h.upload(0, to_product(x))
    assert _lib.lib().ttn_compress(h.h, 600, 0.0, 1) == UNSUP
    D.status_all()


# ---- the reference's known answers on the device --------------------------------------------------------------------------------
def test_spikes_on_the_device():
    """test/test_tt_transformations.jl:6-41 through DeviceTTO / DeviceTT: apply alone, downloaded and densified"""
    d, K, r = 10, 50, 12
    coeffs, f = FR.spikes_problem(d, K, r)
    F = T.fourier_qtto(d, K=K, sign=-1.0, normalize=True)
    x = T.function_to_qtt_uniform(f, d)
    y = dev_apply(to_oracle(F), to_oracle(x))
    e1, e2 = FR.spikes_errors(FR.matricize_vector(to_oracle(y)), coeffs, d)
    print("spikes (device apply): e1 = %.3e, e2 = %.3e" % (e1, e2))
    assert e1 < 1.0e-8
    assert e2 < 1.0e-10
    D.status_all()


def test_dft_example_on_the_device():
    """examples/dft.jl: tt_compress!(F * x, 100), d = 10, K = 50.  If the oracle's own (un-gauged) rounding misses one of the two
    inequalities the device is held to 10 x the oracle's own two errors instead."""
    d, K, r = 10, 50, 12
    coeffs, f = FR.spikes_problem(d, K, r)
    F = T.fourier_qtto(d, K=K, sign=-1.0, normalize=True)
    x = T.function_to_qtt_uniform(f, d)
    ref = O.tt_compress_(O.apply(to_oracle(F), to_oracle(x)), 100)
    o1, o2 = FR.spikes_errors(FR.matricize_vector(ref), coeffs, d)
    dF, dx = D.DeviceTTO(F), D.DeviceTT.from_host(x)
    dy = D.DeviceTT(x.ttv_dims, [a * b for a, b in zip(F.tto_rks, x.ttv_rks)], 1, dtype=np.complex128)
    D.apply(dF, dx, dy)
    D.tt_compress_(dy, 100)
    D.compress_status(dy)
    y = dy.download(0)
    e1, e2 = FR.spikes_errors(FR.matricize_vector(to_oracle(y)), coeffs, d)
    print("dft.jl: device e1 = %.3e, e2 = %.3e; oracle e1 = %.3e, e2 = %.3e; ranks %s" % (e1, e2, o1, o2, y.ttv_rks))
    assert max(y.ttv_rks) <= 100
    if o1 < 1.0e-8 and o2 < 1.0e-10:
        assert e1 < 1.0e-8 and e2 < 1.0e-10
    else:
        assert e1 <= 10 * o1 and e2 <= 10 * o2
    D.status_all()


@pytest.mark.parametrize("name", ["sin", "exp", "chirp"])
def test_fourier_against_numpy_fft(name):
    """F * x at d = 8, K = 25 against numpy.fft.fft of the samples (F's output is bit reversed: site 1 carries the most significant
    bit, which is how matricize reads it).  Tolerance: 10 x the error of the ORACLE's apply on the same input — the interpolation
    error of the operator is a property of K, not of this backend."""
    d = 8
    fs = {"sin": lambda t: math.sin(2 * math.pi * 3 * t) + 0.25, "exp": lambda t: math.exp(-3.0 * t),
          "chirp": lambda t: complex(math.cos(20 * t * t), math.sin(9 * t))}
    f = fs[name]
    x = T.function_to_qtt_uniform(f, d)               # real samples: decomposed on the device; complex ones on the host
    F = T.fourier_qtto(d, K=25)
    want = np.fft.fft(FR.samples(f, d)) / math.sqrt(2 ** d)
    e_ref = np.linalg.norm(FR.matricize_vector(O.apply(to_oracle(F), to_oracle(x))) - want) / np.linalg.norm(want)
    got = FR.matricize_vector(to_oracle(dev_apply(to_oracle(F), to_oracle(x))))
    e_dev = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("fft %s: device %.3e, oracle %.3e" % (name, e_dev, e_ref))
    assert e_dev <= 10 * e_ref


# ---- a train from the real-time TDVP driver -------------------------------------------------------------------------------------
def test_tdvp_state_on_a_complex_handle():
    d = 6
    H = O.tto_scale(0.2, O.Delta(d))
    x = O.rand_tt((2,) * d, 3, np.random.default_rng(9))
    psi = T.tdvp.tdvp(to_product(H), to_product(x), [0.05, 0.05], sweeps=2, normalize=True, imaginary_time=False)
    assert np.iscomplexobj(psi.ttv_vec[0])
    po = to_oracle(psi)
    x0 = O._tdvp_complex(x)
    h, h0 = D.DeviceTT.from_host(psi), up(x0, cap=[max(a, b) for a, b in zip(psi.ttv_rks, x0.ttv_rks)])
    assert h.dtype is np.complex128
    n_ref = O.norm(po)
    assert abs(D.norm(h)[0] - n_ref) <= 1e-12 * n_ref
    ref = O.dot(x0, po)
    assert abs(D.dot(h0, h)[0] - ref) <= 1e-12 * O.norm(x0) * n_ref
    # Δ * ψ: a real operator on a complex train
    Dl = O.Delta(d)
    got = dev_apply(Dl, po)
    want = O.apply(Dl, po)
    assert got.ttv_rks == want.ttv_rks
    for k, (g, w) in enumerate(zip(got.ttv_vec, want.ttv_vec)):
        bound = 4 * 2 * EPS * O.apply(O.TToperator(1, [np.abs(Dl.tto_vec[k])], (2,), Dl.tto_rks[k:k + 2], [0]),
                                      O.TTvector(1, [np.abs(po.ttv_vec[k])], (2,), po.ttv_rks[k:k + 2], [0])).ttv_vec[0]
        assert np.all(np.abs(g - w) <= bound)
    y = T.tt_compress_(T.apply(to_product(Dl), psi), 8)
    ref_y, sv = oracle_compress(want, 8, 0.0, 1)
    check_compressed(y, want, ref_y, sv, "Delta * psi")
    D.status_all()
