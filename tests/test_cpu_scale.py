"""CPU checks of the scaling helpers (tests/scale_reference.py) and of what licenses the reference construction of
tests/test_gpu_scale.py: the oracle is covariant under power-of-two scaling in the moderate range (2^+-200) at the tolerances the
device tests use, for every case those tests run — so `oracle(x)`, rescaled exactly, IS the reference for `device(2^e x)` — and it is
NOT covariant in the far range once truncerr > 0 (its rank rule squares the singular values), which is why the oracle is never run
on a scaled input there."""
import numpy as np
import pytest

from oracle import tt_oracle as O
from tests import scale_reference as SR
from tests.helpers import tt_rel_diff, worst_of


def _same_bits(a, b):
    return all(np.array_equal(ca, cb) for ca, cb in zip(SR.cores_of(a), SR.cores_of(b)))


def _complex_train(rng, dims, rks):
    x = O.rand_tt(dims, rks, rng)
    y = O.rand_tt(dims, rks, rng)
    return SR.with_cores(x, [a + 1j * b for a, b in zip(x.ttv_vec, y.ttv_vec)])


def test_helpers_round_trip_bit_for_bit():
    rng = np.random.default_rng(0)
    dims, rks = (3, 2, 5, 2, 3), [1, 3, 5, 4, 3, 1]
    trains = [O.rand_tt(dims, rks, rng), _complex_train(rng, dims, rks), O.rand_tto((2,) * 5, 3, rng)]
    for x in trains:
        for e in SR.MODERATE + SR.FAR + (1, -3):
            for place in SR.PLACEMENTS:
                y = SR.scaled(x, place, e)
                assert _same_bits(SR.scaled(y, place, -e), x), (place, e)
                if abs(e) >= 200:         # the scaled core is the largest / smallest one: unscaled finds it again, both halves
                    assert _same_bits(SR.unscaled(y, SR.total_exponent(place, e)), x) == (place != "graded"), (place, e)
                changed = [k for k, (a, b) in enumerate(zip(SR.cores_of(x), SR.cores_of(y))) if not np.array_equal(a, b)]
                m = SR.middle(x.N)
                assert changed == {"first": [0], "last": [x.N - 1], "middle": [m - 1], "graded": [m - 1, m]}[place]
                for k in changed:
                    f = e if (place != "graded" or k == m - 1) else -e
                    assert np.array_equal(SR.cores_of(y)[k], SR.cores_of(x)[k] * 2.0 ** f)
        assert SR.all_finite(SR.scaled(x, "first", 800)) and SR.all_finite(SR.scaled(x, "graded", -800))
    # the tensor itself: a power of two commutes with every rounding of the dense contraction
    x = trains[0]
    T0 = O.ttv_to_tensor(x)
    for place in SR.PLACEMENTS:
        assert np.array_equal(O.ttv_to_tensor(SR.scaled(x, place, 40)), T0 * 2.0 ** SR.total_exponent(place, 40))
    # unscaled never leaves the range on the way: a compressed far-range train has its 2^800 spread over the cores
    y = SR.with_cores(x, [SR.ldexp(c, 160) for c in x.ttv_vec])
    z = SR.unscaled(y, 800)
    assert SR.all_finite(z) and np.array_equal(O.ttv_to_tensor(z), T0)
    s = np.array([8.0, 2.0, 1.0])
    assert np.array_equal(SR.sv_ratios(s * 2.0 ** 700), SR.sv_ratios(s))


def test_balanced_keeps_partial_products_near_one():
    """d = 30, rank 64: the raw random train carries about 2^100 of its own; balanced, every left partial product stays within
    2^+-8 (measured in numpy.longdouble; by construction within 2^+-1/2 up to the rounding of the float64 pass)."""
    rng = np.random.default_rng(0)
    raw = O.rand_tt((2,) * 30, 64, rng)
    assert np.log2(float(SR.partial_norms(raw)[-1])) > 60
    x = SR.balanced(raw)
    lg = [float(np.log2(p)) for p in SR.partial_norms(x)]
    print("balanced d=30 r=64: log2 of the partial products in [%.3f, %.3f]" % (min(lg), max(lg)))
    assert max(abs(v) for v in lg) <= 8
    for a, b in zip(raw.ttv_vec, x.ttv_vec):          # exact powers of two, core by core
        q = a / b
        assert np.all(q == q.flat[0]) and np.frexp(q.flat[0])[0] == 0.5
    # the cases of the device tests: inputs within 2^+-8 as well
    for name in SR.COMPRESS_CASES:
        _, x, y = SR.compress_input(name)
        assert max(abs(float(np.log2(p))) for p in SR.partial_norms(x)) <= 1
        assert max(abs(float(np.log2(p))) for p in SR.partial_norms(y)) <= 8, name


@pytest.mark.parametrize("name", list(SR.COMPRESS_CASES))
def test_oracle_rounding_is_covariant_in_the_moderate_range(name):
    """tt_compress!(2^e y) = 2^e tt_compress!(y) for the oracle, every placement, e = +-200, truncerr 0 and 1e-8: same ranks (so the
    oracle's rank decisions do not depend on the scale for these inputs), tensor to 1e-9, sigma_i / sigma_1 per bond step to rtol
    1e-10 (atol 1e-13): the bars of the device tests."""
    A, x, y = SR.compress_input(name)
    for mb in SR.COMPRESS_CASES[name][1]:
        for te in (0.0, 1e-8):
            sv_ref = []
            ref = O.tt_compress_(O.copy_tt(y), mb, truncerr=te, svals_out=sv_ref)
            worst, worst_sv, worst_rest = 0.0, 0.0, 0.0
            for e in SR.MODERATE:
                for place in SR.PLACEMENTS:
                    xs = SR.scale_input(A, x, place, e)
                    sv = []
                    got = O.tt_compress_(O.apply(A, xs) if A is not None else xs, mb, truncerr=te, svals_out=sv)
                    assert got.ttv_rks == ref.ttv_rks, (mb, te, place, e)
                    assert SR.all_finite(got)
                    worst = worst_of(worst, tt_rel_diff(SR.unscaled(got, SR.total_exponent(place, e)), ref))
                    assert len(sv) == len(sv_ref) == 2 * (y.N - 1)
                    ncmp = SR.sv_steps_compared(name, mb, y.N, len(sv))
                    for i, (s, s0) in enumerate(zip(sv, sv_ref)):
                        assert len(s) == len(s0)
                        dev = float(np.max(np.abs(SR.sv_ratios(s) - SR.sv_ratios(s0))))
                        if i < ncmp:
                            assert np.allclose(SR.sv_ratios(s), SR.sv_ratios(s0), rtol=1e-10, atol=SR.sv_atol(name)), (mb, te, place, e, i)
                            worst_sv = worst_of(worst_sv, dev)
                        else:
                            worst_rest = worst_of(worst_rest, dev)
            print("%s max_bond %d truncerr %g: worst tensor error %.2e, worst |d(sigma_i/sigma_1)| %.2e (steps not compared: %.2e)"
                  % (name, mb, te, worst, worst_sv, worst_rest))
            assert worst <= 1e-9
            if (name, mb) in SR.SV_FIRST_SWEEP_ONLY and te == 0.0:
                # the finding that takes the returning sweep of this case out of the singular-value comparison (tests/scale_reference.py):
                # the oracle does not reproduce ITS OWN values there to the floor of 1e-13 (3e-12 measured)
                assert 1e-13 < worst_rest < 1e-10, worst_rest


def test_oracle_orthogonalize_and_dot_are_covariant_in_the_moderate_range():
    worst = 0.0
    for d, r, center in SR.ORTHO_CASES:
        x = SR.ortho_input(d, r, center)
        ref = O.orthogonalize(x, i=center)
        for e in SR.MODERATE:
            for place in SR.PLACEMENTS:
                got = O.orthogonalize(SR.scaled(x, place, e), i=center)
                assert got.ttv_rks == ref.ttv_rks and got.ttv_ot == ref.ttv_ot
                worst = worst_of(worst, tt_rel_diff(SR.unscaled(got, SR.total_exponent(place, e)), ref))
    print("orthogonalize: worst %.2e" % worst)
    assert worst <= 1e-12
    for d, ra, rb in SR.DOT_CASES:
        a, b = SR.dot_input(d, ra, rb)
        ref = O.dot(a, b)
        for e in SR.MODERATE:
            for place in SR.PLACEMENTS:
                got = O.dot(SR.scaled(a, place, e), b)
                assert abs(np.ldexp(got, -SR.total_exponent(place, e)) - ref) <= 1e-12 * O.norm(a) * O.norm(b)


def test_oracle_rank_rule_is_not_covariant_in_the_far_range():
    """Pinned facts about the REFERENCE, so that the far range is never silently compared against it: with truncerr > 0 the rank
    rule accumulates squared singular values (oracle/tt_oracle.py svdtrunc, as the package's `cum += abs2(s[i])`).  d = 10, rank 8,
    Delta * x, truncerr 1e-2: with 2^600 in the middle core the ranks still agree but the rescaled result is off by about 1e-3
    (squares overflow: the rule keeps everything at the affected bonds of one sweep direction); at 2^960 the ranks differ."""
    d = 10
    rng = np.random.default_rng(5)
    x = SR.balanced(O.rand_tt((2,) * d, 8, rng))
    A = O.Delta(d)
    ref = O.tt_compress_(O.apply(A, x), 2 ** 62, truncerr=1e-2)
    with np.errstate(all="ignore"):
        ok = O.tt_compress_(O.apply(A, SR.scaled(x, "middle", 500)), 2 ** 62, truncerr=1e-2)
        off = O.tt_compress_(O.apply(A, SR.scaled(x, "middle", 600)), 2 ** 62, truncerr=1e-2)
        bad = O.tt_compress_(O.apply(A, SR.scaled(x, "middle", 960)), 2 ** 62, truncerr=1e-2)
    assert ok.ttv_rks == ref.ttv_rks and tt_rel_diff(SR.unscaled(ok, 500), ref) <= 1e-12
    assert off.ttv_rks == ref.ttv_rks
    err = tt_rel_diff(SR.unscaled(off, 600), ref)
    print("2^600 in the middle core: rescaled oracle result off by %.2e" % err)
    assert 1e-4 <= err <= 1e-2
    assert bad.ttv_rks != ref.ttv_rks
    # truncerr = 0 has no such rule: covariant in the far range too (what the far-range device cases rely on is still the
    # unscaled oracle; this only shows that the contract itself is well defined there)
    ref0 = O.tt_compress_(O.apply(A, x), 6)
    with np.errstate(all="ignore"):
        far0 = O.tt_compress_(O.apply(A, SR.scaled(x, "middle", 800)), 6)
    assert far0.ttv_rks == ref0.ttv_rks and tt_rel_diff(SR.unscaled(far0, 800), ref0) <= 1e-9
