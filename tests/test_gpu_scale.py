"""The dense kernels under power-of-two scaling of the cores: op(2^e x) = 2^e op(x) with the same ranks, which the reference gets from
LAPACK's internal scaling and the kernels get by hand ("in units of s0 = max|M|").  Helpers, placements, ranges and the case table:
tests/scale_reference.py; what licenses the reference construction: tests/test_cpu_scale.py.

  reference    the oracle's result for the UNSCALED input, rescaled exactly (never the oracle on the scaled input: with truncerr > 0 it
               is itself not covariant outside about 2^+-500)
  moderate     e = +-200 (values, squares, fourth powers normal), truncerr 0 and 1e-8: every operation meets its ordinary bar
  far          e = +-800 (values normal, squares not), truncerr 0: tt_compress!, the fused apply + round, orthogonalize, dot, the
               complex rounding, the site swap, ttv_decomp, split_sites and the operator rounding meet the ordinary bar too — a fast
               route may decline (SCALE_SAFE, csrc/ttn_common.h), the result must be right.  norm squares the scale: it is run in the far
               range only where the square is representable (`graded`).
  bars         status clean; every output entry finite; ranks and ot flags identical; tensor 1e-9 (rounding) / 1e-12 (orthogonalize,
               ttv_decomp, split_sites) after `unscaled`; sigma_i / sigma_1 per bond step rtol 1e-10 with the floors of
               tests/test_gpu_parity.py; dot / norm 1e-12 of the size of the terms; apply, hadamard, +, scalar * bit for bit.
Every test prints its worst error per (placement, exponent)."""
import functools

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import scale_reference as SR
from tests.helpers import to_oracle, to_product, tt_rel_diff, worst_of

pytestmark = pytest.mark.gpu

RANGES = {"moderate": (SR.MODERATE, (0.0, 1e-8)), "far": (SR.FAR, (0.0,))}


@pytest.fixture(scope="module")
def T():
    import ttn_amd
    ttn_amd.ensure_init(0)
    return ttn_amd


def _report(tag, table):
    for (place, e), v in sorted(table.items()):
        print("%s  %-6s e=%+5d  worst %.3e" % (tag, place, e, v))


def _fold(table, place, e, v):
    table[(place, e)] = worst_of(table.get((place, e), 0.0), v)


# ---------------------------------------------------------------------------------------------------------------------------------
# tt_compress! and the fused apply + round
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _compress_case(name):
    return SR.compress_input(name)


@functools.lru_cache(maxsize=None)
def _compress_ref(name, mb, te):
    _, _, y = _compress_case(name)
    sv = []
    ref = O.tt_compress_(O.copy_tt(y), mb, truncerr=te, svals_out=sv)
    return ref, sv


def _check_rounded(got, ref, place, e, tensors, tag):
    assert SR.all_finite(got), (tag, "non-finite entries")
    assert list(got.ttv_rks) == list(ref.ttv_rks), (tag, got.ttv_rks, ref.ttv_rks)
    err = tt_rel_diff(SR.unscaled(to_oracle(got), SR.total_exponent(place, e)), ref)
    _fold(tensors, place, e, err)
    assert err <= 1e-9, (tag, err)


def _run_compress(T, name, rng_name):
    exps, tes = RANGES[rng_name]
    A, x, _ = _compress_case(name)
    dims = x.ttv_dims
    tensors, svs = {}, {}
    for mb in SR.COMPRESS_CASES[name][1]:
        for te in tes:
            ref, sv_ref = _compress_ref(name, mb, te)
            for e in exps:
                for place in SR.PLACEMENTS:
                    tag = (name, mb, te, place, e)
                    xs = SR.scale_input(A, x, place, e)
                    # the stateless tt_compress! on the materialised train (its status is checked by the call)
                    ys = O.apply(A, xs) if A is not None else xs
                    got = T.tt_compress_(to_product(ys), mb, truncerr=te)
                    _check_rounded(got, ref, place, e, tensors, tag + ("tt_compress_",))
                    # handles: the fused apply + round (or the resident train), singular values captured
                    if A is not None:
                        cap = [a * c for a, c in zip(A.tto_rks, xs.ttv_rks)]
                        need, _ = T.device.compress_rank_bound(dims, cap, mb)
                        dy = T.DeviceTT(dims, [max(a, b) for a, b in zip(cap, need)])
                        dy.capture_singular_values(True)
                        T.device.apply_compress(T.DeviceTTO(to_product(A)), T.DeviceTT.from_host(to_product(xs)), dy, mb, te)
                    else:
                        need, _ = T.device.compress_rank_bound(dims, xs.ttv_rks, mb)
                        dy = T.DeviceTT.from_host(to_product(xs), cap_rks=[max(a, b) for a, b in zip(xs.ttv_rks, need)])
                        dy.capture_singular_values(True)
                        T.device.tt_compress_(dy, mb, te)
                    T.device.compress_status(dy)
                    _check_rounded(dy.download(), ref, place, e, tensors, tag + ("handle",))
                    for i in range(SR.sv_steps_compared(name, mb, x.N, len(sv_ref))):
                        s0 = sv_ref[i]
                        s = np.asarray(dy.singular_values(0, i))[: len(s0)]
                        assert len(s) == len(s0) and np.all(np.isfinite(s)) and s[0] > 0, (tag, i)
                        dev = float(np.max(np.abs(SR.sv_ratios(s) - SR.sv_ratios(s0))))
                        _fold(svs, place, e, dev)
                        assert np.allclose(SR.sv_ratios(s), SR.sv_ratios(s0), rtol=1e-10, atol=SR.sv_atol(name)), (tag, "bond step", i, dev)
    _report("%s tensor" % name, tensors)
    _report("%s sigma_i/sigma_1" % name, svs)


BUILDS = ("1024", "512")            # the two builds of k_compress, selected as tests/test_gpu_wg512.py does


def _select_build(monkeypatch, build):
    if build == "512":
        monkeypatch.setenv("TTN_WG512", "1")
    else:
        monkeypatch.delenv("TTN_WG512", raising=False)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("rng_name", list(RANGES))
@pytest.mark.parametrize("name", list(SR.COMPRESS_CASES))
def test_compress(T, monkeypatch, name, rng_name, build):
    _select_build(monkeypatch, build)
    _run_compress(T, name, rng_name)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("rng_name", list(RANGES))
def test_compress_lds_routes_householder_only(T, monkeypatch, rng_name, build):
    """the in-LDS case again with TTN_FAST=0: route H for every step (test_compress runs it with TTN_FAST unset: routes G / F)"""
    _select_build(monkeypatch, build)
    monkeypatch.setenv("TTN_FAST", "0")
    _run_compress(T, "lds_routes_r24", rng_name)


# ---------------------------------------------------------------------------------------------------------------------------------
# orthogonalize
# ---------------------------------------------------------------------------------------------------------------------------------
def _gauge_error(got, center):
    worst = 0.0
    for j, G in enumerate(got.ttv_vec):
        G = np.asarray(G)
        n, rl, rr = G.shape
        if j < center - 1:
            Amat = G.transpose(1, 0, 2).reshape(rl * n, rr, order="F")
            worst = worst_of(worst, float(np.max(np.abs(Amat.T @ Amat - np.eye(rr)))))
        elif j > center - 1:
            Amat = G.transpose(1, 2, 0).reshape(rl, rr * n, order="F")
            worst = worst_of(worst, float(np.max(np.abs(Amat @ Amat.T - np.eye(rl)))))
    return worst


@pytest.mark.parametrize("rng_name", list(RANGES))
@pytest.mark.parametrize("d,r,center", SR.ORTHO_CASES)
def test_orthogonalize(T, monkeypatch, d, r, center, rng_name):
    """Both forms (the three launches of rank <= 64 QTT trains, the single 1024-thread launch), the checks of _ortho_checks of
    tests/test_gpu_parity.py on the rescaled output: ranks / gauge flags of the oracle's result for the unscaled train, tensor
    unchanged to 1e-12, every non-centre core orthonormal to 1e-12, the centre core's norm 2^e times the oracle's."""
    x = SR.ortho_input(d, r, center)
    ref = O.orthogonalize(x, i=center)
    nref = float(np.linalg.norm(ref.ttv_vec[center - 1]))
    tensors, gauges = {}, {}
    for form in ("1", "0"):
        monkeypatch.setenv("TTN_ORTHO512", form)
        for e in RANGES[rng_name][0]:
            for place in SR.PLACEMENTS:
                tag = (form, place, e)
                got = T.orthogonalize(to_product(SR.scaled(x, place, e)), i=center)
                assert SR.all_finite(got), tag
                assert got.ttv_rks == ref.ttv_rks and got.ttv_ot == ref.ttv_ot, tag
                tot = SR.total_exponent(place, e)
                err = tt_rel_diff(SR.unscaled(to_oracle(got), tot), x)
                g = _gauge_error(got, center)
                _fold(tensors, place, e, err)
                _fold(gauges, place, e, g)
                assert err < 1e-12, (tag, err)
                assert g < 1e-12, (tag, g)
                nc = float(np.linalg.norm(np.ldexp(np.asarray(got.ttv_vec[center - 1]), -tot)))      # (the centre core carries the scale)
                assert abs(nc - nref) <= 1e-12 * nref, (tag, nc, nref)
    _report("orthogonalize d=%d r=%d centre %d tensor" % (d, r, center), tensors)
    _report("orthogonalize d=%d r=%d centre %d gauge" % (d, r, center), gauges)


# ---------------------------------------------------------------------------------------------------------------------------------
# dot, norm
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ra,rb", SR.DOT_CASES)
def test_dot_norm(T, d, ra, rb):
    """1e-12 of the size of the terms (||a|| ||b||, the existing bar) against c times the oracle's value for the unscaled trains.
    dot: every placement and exponent (c dot is representable: |dot| <= ||a|| ||b|| of order one).  norm = sqrt(dot(a, a)) squares
    the scale: 2^+-1600 is not a double, so the far range runs `graded` only."""
    a, b = SR.dot_input(d, ra, rb)
    ref, na, nb = O.dot(a, b), O.norm(a), O.norm(b)
    pb = to_product(b)
    table = {}
    for e in SR.MODERATE + SR.FAR:
        for place in SR.PLACEMENTS:
            tot = SR.total_exponent(place, e)
            pa = to_product(SR.scaled(a, place, e))
            got = T.dot(pa, pb)
            assert np.isfinite(got), (place, e)
            err = abs(float(np.ldexp(got, -tot)) - ref) / (na * nb)
            got2 = T.dot(pb, pa)
            err = worst_of(err, abs(float(np.ldexp(got2, -tot)) - ref) / (na * nb))
            assert err <= 1e-12, ("dot", place, e, err, got, got2)
            if abs(2 * tot) < 1000:
                n_ = T.norm(pa)
                assert np.isfinite(n_), (place, e)
                nerr = abs(float(np.ldexp(n_, -tot)) - na) / na
                assert nerr <= 1e-12, ("norm", place, e, nerr, n_)
                err = worst_of(err, nerr)
            _fold(table, place, e, err)
    _report("dot/norm d=%d ranks (%d, %d)" % (d, ra, rb), table)


# ---------------------------------------------------------------------------------------------------------------------------------
# streaming operations: the positive control.  A power of two commutes with every rounding they do.
# ---------------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return list(a.ttv_rks) == list(b.ttv_rks) and all(np.array_equal(np.asarray(ca), np.asarray(cb)) for ca, cb in zip(a.ttv_vec, b.ttv_vec))


def test_streaming_ops_are_exactly_covariant(T):
    rng = np.random.default_rng(9)
    dims = (2, 3, 2, 4, 2, 2, 3)
    x = SR.balanced(O.rand_tt(dims, 6, rng))
    y = SR.balanced(O.rand_tt(dims, 5, rng))
    Ar = O.TToperator(len(dims), [rng.standard_normal((dims[k], dims[k], rk, rk1)) for k, (rk, rk1) in
                                  enumerate(zip([1, 2, 3, 2, 3, 2, 2], [2, 3, 2, 3, 2, 2, 1]))], dims, [1, 2, 3, 2, 3, 2, 2, 1], [0] * len(dims))
    xq = SR.balanced(O.rand_tt((2,) * 12, 16, rng))
    px, py, pA, pxq, pD = to_product(x), to_product(y), to_product(Ar), to_product(xq), T.Delta(12)
    base = {"apply Delta": T.apply(pD, pxq), "apply random": T.apply(pA, px), "hadamard": T.hadamard(px, py), "add": T.add(px, py),
            "scale": T.scale(-2.5, px)}
    for e in SR.MODERATE + SR.FAR:
        for place in SR.PLACEMENTS:
            sx, sy, sxq = to_product(SR.scaled(x, place, e)), to_product(SR.scaled(y, place, e)), to_product(SR.scaled(xq, place, e))
            got = {"apply Delta": T.apply(pD, sxq), "apply random": T.apply(pA, sx), "hadamard": T.hadamard(sx, py), "add": T.add(sx, sy),
                   "scale": T.scale(-2.5, sx)}
            for op, g in got.items():
                assert _same_bits(g, SR.scaled(base[op], place, e)), (op, place, e)
    print("apply, hadamard, +, scalar *: bit for bit 2^e times the unscaled device result, e in", SR.MODERATE + SR.FAR)


# ---------------------------------------------------------------------------------------------------------------------------------
# complex tt_compress!
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng_name", list(RANGES))
def test_complex_compress(T, rng_name):
    """the smallest case of the rounding test of tests/test_gpu_complex.py: d = 8, ranks up to 16, max_bond 4 (well posed: no kept
    singular value at the noise level in the oracle's own run)"""
    import tests.test_gpu_complex as ZC
    x = SR.balanced(ZC.random_case_inputs(500))
    exps, tes = RANGES[rng_name]
    table = {}
    for te in tes:
        ref, sv = ZC.oracle_compress(x, 4, te, 1)
        assert not ZC.ill_posed(sv)
        for e in exps:
            for place in SR.PLACEMENTS:
                got = T.tt_compress_(to_product(SR.scaled(x, place, e)), 4, truncerr=te)
                assert SR.all_finite(got), (te, place, e)
                assert got.ttv_rks == ref.ttv_rks, (te, place, e)
                err = ZC.rel(SR.unscaled(to_oracle(got), SR.total_exponent(place, e)), ref)
                _fold(table, place, e, err)
                assert err <= 1e-9, (te, place, e, err)
    _report("complex tt_compress!", table)


# ---------------------------------------------------------------------------------------------------------------------------------
# site swap (route H of the bond step in its SWAP form), ttv_decomp, split_sites, operator rounding
# ---------------------------------------------------------------------------------------------------------------------------------
def test_reorder(T):
    n_dims, bits, r = 2, 3, 3
    rng = np.random.default_rng(0)
    x = SR.balanced(O.rand_tt((2,) * (n_dims * bits), r, rng))
    ref = O.reorder(x, n_dims, bits, True)
    dref = O.ttv_to_tensor(ref)
    table = {}
    for e in SR.MODERATE + SR.FAR:
        for place in SR.PLACEMENTS:
            got = T.reorder(to_product(SR.scaled(x, place, e)), n_dims, bits, "interleaved")
            assert SR.all_finite(got), (place, e)
            assert list(got.ttv_rks) == list(ref.ttv_rks), (place, e)
            dgot = O.ttv_to_tensor(SR.unscaled(to_oracle(got), SR.total_exponent(place, e)))
            err = float(np.max(np.abs(dgot - dref)) / np.max(np.abs(dref)))
            _fold(table, place, e, err)
            assert err <= 1e-11, (place, e, err)
    _report("reorder", table)


def test_ttv_decomp(T):
    """The dense tensor scaled as a whole; tol is an ABSOLUTE threshold of the reference, so it is scaled with the tensor."""
    import tests.test_gpu_ttv_decomp as TD
    rng = np.random.default_rng(4)
    t = rng.standard_normal((3, 2, 4, 2, 3))
    ref = O.ttv_decomp(t, index=3)
    sc = float(np.max(np.abs(t)))
    table = {}
    for e in SR.MODERATE + SR.FAR:
        got = T.ttv_decomp(np.ldexp(t, e), index=3, tol=float(np.ldexp(1e-12, e)))
        assert SR.all_finite(got), e
        assert list(got.ttv_rks) == list(ref.ttv_rks) and list(got.ttv_ot) == list(ref.ttv_ot), e
        err = float(np.max(np.abs(O.ttv_to_tensor(SR.unscaled(to_oracle(got), e)) - t))) / sc
        err = worst_of(err, TD._gauge_err(got))
        _fold(table, "whole", e, err)
        assert err <= 1e-12, (e, err)
    _report("ttv_decomp", table)


def test_split_sites(T):
    from tests import resite_reference as R
    sd = [[2, 3, 2], [3, 2], [4]]
    x = R.random_train((12, 6, 4), (1, 5, 3, 1), seed=21)
    ref = R.to_qtt(x, sd)
    full = R.dense(ref)
    sc = float(np.max(np.abs(full)))
    assert np.max(np.abs(full.reshape(-1) - R.dense(x).reshape(-1))) <= 1e-13 * sc
    px = T.TTvector(x.N, [np.asfortranarray(c) for c in x.ttv_vec], x.ttv_dims, list(x.ttv_rks), [0] * x.N)
    table = {}
    for e in SR.MODERATE + SR.FAR:
        for place in SR.PLACEMENTS:
            got = T.to_qtt(SR.scaled(px, place, e), sd)
            assert SR.all_finite(got), (place, e)
            assert list(got.ttv_rks) == list(ref.ttv_rks), (place, e)
            back = SR.unscaled(got, SR.total_exponent(place, e))
            err = float(np.max(np.abs(R.dense(back) - full))) / sc
            _fold(table, place, e, err)
            assert err <= 1e-12, (place, e, err)
    _report("split_sites", table)


@pytest.mark.parametrize("rng_name", list(RANGES))
def test_tto_compress(T, rng_name):
    """the smallest ragged case of tests/test_gpu_opalg.py (dims (2,)*6, ranks up to 12), max_bond 4"""
    from tests import opalg_reference as R
    rng = np.random.default_rng(12)
    A = SR.balanced(R.rand_tto((2,) * 6, [1, 3, 12, 5, 7, 2, 1], rng))
    exps, tes = RANGES[rng_name]
    table = {}
    for te in tes:
        ref = R.tto_compress(A, 4, truncerr=te)
        mref = R.tto_matrix(ref)
        for e in exps:
            for place in SR.PLACEMENTS:
                got = T.tto_compress_(to_product(SR.scaled(A, place, e)), 4, truncerr=te)
                assert SR.all_finite(got), (te, place, e)
                assert list(got.tto_rks) == list(ref.tto_rks), (te, place, e)
                m = R.tto_matrix(SR.unscaled(to_oracle(got), SR.total_exponent(place, e)))
                err = float(np.linalg.norm(m - mref) / np.linalg.norm(mref))
                _fold(table, place, e, err)
                assert err <= 1e-9, (te, place, e, err)
    _report("tto_compress_", table)
