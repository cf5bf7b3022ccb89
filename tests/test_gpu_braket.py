"""<x| A |y> on the GPU (csrc/ttn_braket_kernels.h, include/ttn_braket.h) against the oracle's dot(x, A * y), which conjugates x.

Bar: the one dot carries, |got - ref| <= 1e-12 ||x|| ||A y||, ref and norms from the oracle's complex dot / apply.  Shapes: the smallest
at which each piece can go wrong — d = 1 and 2, mixed dims on the general route with a ragged batch and an all-zero train, QTT trains
with ranks off and on the 16 x 16 tile in the three type forms (complex trains with a complex or a real operator, real trains with a
complex operator), one case just inside and one just outside each exported limit of the on-chip route, a batch whose trains take
different routes (the on-chip kernel and the general kernel of one call)."""
import numpy as np
import pytest

import ttn_amd as T
from oracle import tt_oracle as O
from tests import braket_reference as R
from tests.helpers import to_oracle, to_product
from tests.test_cpu_braket import FORMS, crand_tt, crand_tto, reference
from ttn_amd import device as D

pytestmark = pytest.mark.gpu

RMAX, OPMAX = D.BRAKET_QTT_MAX_RANK, D.BRAKET_QTT_MAX_OP_RANK


@pytest.fixture(scope="module", autouse=True)
def _init():
    T.ensure_init(0)


def upload_batch(trains, cap=None):
    """The trains in one handle whose element type is theirs (all complex or all real)."""
    dims = trains[0].ttv_dims
    if cap is None:
        cap = [max(t.ttv_rks[m] for t in trains) for m in range(len(dims) + 1)]
    cplx = any(np.iscomplexobj(c) for t in trains for c in t.ttv_vec)
    h = T.DeviceTT(dims, cap, batch=len(trains), dtype=np.complex128 if cplx else np.float64)
    for b, t in enumerate(trains):
        h.upload(b, to_product(t))
    return h


def flat(d, r):
    """Ranks [1, r, ..., r, 1], NOT capped by the dims: crand_tt with an integer rank goes through r_and_d_to_rks, which caps rank k at
    min(2^k, 2^(d - k)) — 8 at d = 7, 32 at d = 10 — and would silently shrink the shapes below."""
    return [1] + [int(r)] * (d - 1) + [1]


def flat_tt(d, r, rng, cplx=True):
    x = crand_tt((2,) * d, flat(d, r), rng, cplx)
    assert max(x.ttv_rks) == r and x.ttv_rks[1:-1] == [r] * (d - 1)
    return x


def adjoint(A):
    return O.TToperator(A.N, [np.conj(np.swapaxes(c, 0, 1)).copy() for c in A.tto_vec], A.tto_dims, A.tto_rks, A.tto_ot)


def check(xs, A, ys, same=False, cap=None):
    """braket on a batch against the oracle, train by train; returns the device numbers."""
    hx = upload_batch(xs, cap)
    hy = hx if same else upload_batch(ys)
    hA = T.DeviceTTO(to_product(A))
    got = D.braket(hx, hA, hy)
    assert got.shape == (len(xs),) and got.dtype == np.complex128
    for b, (x, y) in enumerate(zip(xs, ys)):
        ref, scale = reference(x, A, y)
        print(f"train {b}: got {got[b]:.17e} ref {ref:.17e} err/scale {abs(got[b] - ref) / scale if scale else 0.0:.2e}")
        assert abs(got[b] - ref) <= 1e-12 * scale
    for h in {hx, hy}:
        h.free()
    hA.free()
    return got


@pytest.mark.parametrize("ca,cx", FORMS)
def test_d1_and_d2(ca, cx):
    rng = np.random.default_rng(1)
    for dims, rx, ry, Ar in [((3,), [1, 1], [1, 1], [1, 1]), ((2, 3), [1, 2, 1], [1, 3, 1], [1, 2, 1])]:
        check([crand_tt(dims, rx, rng, cx)], crand_tto(dims, Ar, rng, ca), [crand_tt(dims, ry, rng, cx)])


@pytest.mark.parametrize("ca,cx", FORMS)
def test_general_route_mixed_dims_ragged_batch_and_zero_train(ca, cx):
    rng = np.random.default_rng(21)
    dims = (2, 3, 4, 2)
    x, y = crand_tt(dims, [1, 2, 5, 3, 1], rng, cx), crand_tt(dims, [1, 3, 4, 2, 1], rng, cx)
    A = crand_tto(dims, [1, 2, 3, 2, 1], rng, ca)
    x1 = crand_tt(dims, [1, 2, 3, 2, 1], rng, cx)                    # below the handle's capacity [1, 2, 5, 3, 1]
    y1 = crand_tt(dims, [1, 2, 4, 1, 1], rng, cx)
    x2 = O.TTvector(x.N, [np.zeros_like(c) for c in x.ttv_vec], x.ttv_dims, x.ttv_rks, x.ttv_ot)
    got = check([x, x1, x2], A, [y, y1, y])
    assert got[2] == 0.0 and got[2].real == 0.0 and got[2].imag == 0.0
    # the restatement of tests/braket_reference.py sees the same number
    assert abs(got[0] - R.braket(x, A, y)) <= 1e-12 * reference(x, A, y)[1]


QTT_CASES = [(9, 5, 13), (7, 16, 17), (12, 37, 64), (14, 64, 64)]          # (d, rank of x, rank of y): every interior rank is that number


@pytest.mark.parametrize("ca,cx", FORMS)
@pytest.mark.parametrize("R_", range(1, OPMAX + 1))
@pytest.mark.parametrize("d,rx,ry", QTT_CASES)
def test_on_chip_route_dense_nonsymmetric_operator(d, rx, ry, R_, ca, cx):
    rng = np.random.default_rng(100 * d + 10 * R_ + 2 * ca + cx)
    dims = (2,) * d
    A = crand_tto(dims, R_, rng, ca)
    assert max(A.tto_rks) == R_ <= OPMAX and max(rx, ry) <= RMAX
    xs, ys = [flat_tt(d, rx, rng, cx), flat_tt(d, rx, rng, cx)], [flat_tt(d, ry, rng, cx), flat_tt(d, ry, rng, cx)]
    assert all(max(t.ttv_rks) == rx for t in xs) and all(max(t.ttv_rks) == ry for t in ys)
    check(xs, A, ys)


def test_on_chip_route_zero_train_is_exactly_zero():
    d = 7
    rng = np.random.default_rng(17)
    x, y = crand_tt((2,) * d, 9, rng), crand_tt((2,) * d, 6, rng)
    x0 = O.TTvector(d, [np.zeros_like(c) for c in x.ttv_vec], x.ttv_dims, x.ttv_rks, x.ttv_ot)
    got = check([x, x0], crand_tto((2,) * d, OPMAX, rng), [y, y])
    assert got[1].real == 0.0 and got[1].imag == 0.0


@pytest.mark.parametrize("ca,cx", FORMS)
def test_limits_of_the_on_chip_route_inside_and_outside(ca, cx):
    d = 14
    dims = (2,) * d
    rng = np.random.default_rng(3)
    inside, outside = crand_tt(dims, RMAX, rng, cx), crand_tt(dims, RMAX + 1, rng, cx)
    assert max(inside.ttv_rks) == RMAX and max(outside.ttv_rks) == RMAX + 1          # d = 14 caps the ranks at 128: these are real
    # just inside both limits at once
    check([inside], crand_tto(dims, OPMAX, rng, ca), [crand_tt(dims, RMAX, rng, cx)])
    # train rank limit + 1 on either side: the general route
    check([outside], crand_tto(dims, 2, rng, ca), [inside])
    check([inside], crand_tto(dims, 2, rng, ca), [outside])
    # operator rank limit + 1
    A = crand_tto(dims, OPMAX + 1, rng, ca)
    assert max(A.tto_rks) == OPMAX + 1
    lo, hi = crand_tt(dims, 20, rng, cx), crand_tt(dims, 33, rng, cx)
    assert max(lo.ttv_rks) == 20 and max(hi.ttv_rks) == 33
    check([lo], A, [hi])


@pytest.mark.parametrize("ca,cx", FORMS)
def test_one_batch_two_routes(ca, cx):
    """Trains 0 and 2 have a rank above the limit and take the general route, trains 1 and 3 fit the on-chip route: the decision is per
    train.  The handle's rank bound is above the limit, so the call launches the on-chip kernel, which leaves trains 0 and 2 alone, and
    then the general kernel, which leaves trains 1 and 3 alone; the over-limit rank sits on y for train 0 and on x for train 2."""
    d = 10
    dims = (2,) * d
    rng = np.random.default_rng(5)
    xs = [flat_tt(d, 32, rng, cx), flat_tt(d, 32, rng, cx), flat_tt(d, RMAX + 1, rng, cx), flat_tt(d, 17, rng, cx)]
    ys = [flat_tt(d, RMAX + 1, rng, cx), flat_tt(d, RMAX, rng, cx), flat_tt(d, 20, rng, cx), flat_tt(d, 16, rng, cx)]
    assert max(ys[0].ttv_rks) == RMAX + 1 and max(xs[2].ttv_rks) == RMAX + 1
    assert all(max(xs[b].ttv_rks) <= RMAX and max(ys[b].ttv_rks) <= RMAX for b in (1, 3))
    check(xs, crand_tto(dims, 2, rng, ca), ys)


def test_identities():
    d = 9
    dims = (2,) * d
    rng = np.random.default_rng(11)
    x, y = crand_tt(dims, 13, rng), crand_tt(dims, 20, rng)
    for A in (crand_tto(dims, 2, rng), crand_tto(dims, 3, rng)):          # the on-chip and the general route
        ref, scale = reference(x, A, y)
        hx, hy = upload_batch([x]), upload_batch([y])
        hA, hAh = T.DeviceTTO(to_product(A)), T.DeviceTTO(to_product(adjoint(A)))
        s = D.braket(hx, hA, hy)[0]
        sh = D.braket(hy, hAh, hx)[0]
        assert abs(s - ref) <= 1e-12 * scale
        assert abs(s - np.conj(sh)) <= 1e-12 * (scale + reference(y, adjoint(A), x)[1])       # <x|A|y> = conj(<y|A^H|x>)
        # a non-conjugated bra would be another number
        assert abs(R.braket(x, A, y, conj_x=False) - s) > 1e-6 * scale
        # x is y: the same handle twice against two uploads of the same train
        hx2 = upload_batch([x])
        refx, scalex = reference(x, A, x)
        e1, e2 = D.braket(hx, hA, hx)[0], D.braket(hx, hA, hx2)[0]
        assert abs(e1 - refx) <= 1e-12 * scalex and abs(e2 - refx) <= 1e-12 * scalex and abs(e1 - e2) <= 1e-12 * scalex
        for h in (hx, hy, hx2, hA, hAh):
            h.free()


@pytest.mark.parametrize("name", ["heisenberg", "pauli_y", "pauli_y_real_state"])
def test_hermitian_operators_give_real_expectations(name):
    d = 9
    rng = np.random.default_rng(13)
    A = T.heisenberg_xyz_tto(d, jx=1.0, jy=0.7, jz=-1.2, lam=0.3, field="x") if name == "heisenberg" else T.pauli_sum_tto("y", d, dtype=np.complex128)
    x = crand_tt((2,) * d, 12, rng, cplx=(name != "pauli_y_real_state"))
    ref, scale = reference(x, to_oracle(A), x)
    hx, hA = upload_batch([x]), T.DeviceTTO(A)
    got = D.braket(hx, hA, hx)[0]
    assert abs(got - ref) <= 1e-12 * scale and abs(got.imag) <= 1e-12 * scale
    e = D.energy(hA, hx)
    assert e.shape == (1,) and e.dtype == np.float64
    assert abs(e[0] - ref.real / O.dot(x, x).real) <= 2e-12 * scale / O.dot(x, x).real
    hx.free(), hA.free()


def test_all_float64_operands_are_sandwich():
    """All three operands Float64: k_expect's launch.  real(braket) is sandwich's number bit for bit and the imaginary part is +0.0 — on
    the general route (ordered GEMMs) and on k_expect's on-chip route with x ranks <= 16, where ONE wave per column block adds into the
    LDS image and the sum order is fixed.  With more waves per column block (the rank-37 case) the LDS atomics of k_expect arrive in
    any order, two runs of sandwich itself agree to rounding only, and so does the comparison."""
    rng = np.random.default_rng(19)
    q = (2,) * 9
    cases = [((2, 3, 4, 2), [1, 2, 5, 3, 1], [1, 3, 4, 2, 1], [1, 2, 3, 2, 1], True), (q, flat(9, 11), flat(9, 16), 3, True),
             (q, flat(9, 16), flat(9, 20), 5, True), (q, flat(9, 37), flat(9, 20), 2, False)]
    for dims, rx, ry, ra, ordered in cases:
        xs = [crand_tt(dims, rx, rng, False), crand_tt(dims, rx, rng, False)]
        ys = [crand_tt(dims, ry, rng, False), crand_tt(dims, ry, rng, False)]
        assert all(t.ttv_rks == rx for t in xs) and all(t.ttv_rks == ry for t in ys)          # the ranks are the ones written above
        assert ordered == (len(set(dims)) > 1 or max(rx) <= 16)
        A = crand_tto(dims, ra, rng, False)
        hx, hy, hA = upload_batch(xs), upload_batch(ys), T.DeviceTTO(to_product(A))
        assert hx.dtype is np.float64 and hA.dtype is np.float64
        b, s = D.braket(hx, hA, hy), D.sandwich(hx, hA, hy)
        assert b.dtype == np.complex128 and np.all(b.imag == 0.0) and not np.any(np.signbit(b.imag))
        if ordered:
            assert np.array_equal(b.real, s)
        for k, (x, y) in enumerate(zip(xs, ys)):
            ref, scale = reference(x, A, y)
            assert abs(b[k] - ref) <= 1e-12 * scale and abs(b[k].real - s[k]) <= 2e-12 * scale
        for h in (hx, hy, hA):
            h.free()


def test_known_answers_pauli_sums_d6():
    d = 6
    rng = np.random.default_rng(29)
    psi = crand_tt((2,) * d, 5, rng)
    v = O.ttv_to_tensor(psi).reshape(-1)
    hx = upload_batch([psi])
    for A, M in ((T.pauli_sum_tto("y", d, dtype=np.complex128), R.pauli_sum_dense("y", d)),
                 (T.pauli_pair_sum_tto("x", "y", d, dtype=np.complex128), R.pauli_pair_sum_dense("x", "y", d))):
        ref = complex(np.vdot(v, M @ v))
        scale = np.linalg.norm(v) * np.linalg.norm(M @ v)
        hA = T.DeviceTTO(A)
        got = D.braket(hx, hA, hx)[0]
        print(f"got {got:.17e} dense {ref:.17e} err/scale {abs(got - ref) / scale:.2e}")
        assert abs(got - ref) <= 1e-12 * scale
        assert abs(T.braket(to_product(psi), A, to_product(psi)) - ref) <= 1e-12 * scale      # the host-train form
        hA.free()
    hx.free()


def test_energy_of_a_real_time_tdvp_state():
    d = 6
    H = O.tto_scale(0.2, O.Delta(d))
    x = O.rand_tt((2,) * d, 3, np.random.default_rng(9))
    psi = T.tdvp.tdvp(to_product(H), to_product(x), [0.05, 0.05], sweeps=2, normalize=True, imaginary_time=False)
    assert np.iscomplexobj(psi.ttv_vec[0])
    po = to_oracle(psi)
    Hp = O.apply(H, po)
    ref = O.dot(po, Hp).real / O.dot(po, po).real
    bar = 2e-12 * O.norm(po) * O.norm(Hp) / O.dot(po, po).real
    e = T.energy(to_product(H), psi)
    print(f"energy {e:.17e} oracle {ref:.17e} err/bar {abs(e - ref) / bar:.2e}")
    assert isinstance(e, float) and abs(e - ref) <= bar
    h, hH = D.DeviceTT.from_host(psi, batch=2), T.DeviceTTO(to_product(H))
    assert h.dtype is np.complex128 and hH.dtype is np.float64
    assert np.all(np.abs(D.energy(hH, h) - ref) <= bar)
    h.free(), hH.free()


def test_braket_dev_equals_braket():
    import torch
    rng = np.random.default_rng(31)
    for dims, rx, ry, ra in [((2, 3, 4, 2), [1, 2, 5, 3, 1], [1, 3, 4, 2, 1], [1, 2, 3, 2, 1]), ((2,) * 8, 9, 20, 2)]:
        xs, ys = [crand_tt(dims, rx, rng), crand_tt(dims, rx, rng)], [crand_tt(dims, ry, rng), crand_tt(dims, ry, rng)]
        A = crand_tto(dims, ra, rng)
        hx, hy, hA = upload_batch(xs), upload_batch(ys), T.DeviceTTO(to_product(A))
        host = D.braket(hx, hA, hy)
        dev = D.braket_dev(hx, hA, hy)
        buf = torch.full((2,), -1.0 - 1.0j, dtype=torch.complex128, device="cuda")
        assert D.braket_dev(hx, hA, hy, out=buf) is buf
        D.sync()
        assert dev.dtype == torch.complex128 and dev.shape == (2,)
        scale = max(reference(x, A, y)[1] for x, y in zip(xs, ys))
        if len(set(dims)) > 1:                                      # GEMMs in a fixed order: the same bits
            assert np.array_equal(dev.cpu().numpy(), host) and np.array_equal(buf.cpu().numpy(), host)
        assert np.all(np.abs(dev.cpu().numpy() - host) <= 1e-12 * scale) and np.all(np.abs(buf.cpu().numpy() - host) <= 1e-12 * scale)
        with pytest.raises(TypeError, match="complex128"):
            D.braket_dev(hx, hA, hy, out=torch.empty(2, dtype=torch.float64, device="cuda"))
        for h in (hx, hy, hA):
            h.free()


def test_refusals_leave_the_library_usable():
    d = 5
    dims = (2,) * d
    rng = np.random.default_rng(9)
    x, y = crand_tt(dims, 4, rng), crand_tt(dims, 6, rng)
    A = crand_tto(dims, 2, rng)
    ref, scale = reference(x, A, y)
    hx, hy, hA = upload_batch([x]), upload_batch([y]), T.DeviceTTO(to_product(A))

    def ok():
        assert abs(D.braket(hx, hA, hy)[0] - ref) <= 1e-12 * scale

    ok()
    # x and y of different element types
    hr = upload_batch([crand_tt(dims, 4, rng, False)])
    with pytest.raises(T.TTNError, match="ttn_braket.*element types"):
        D.braket(hr, hA, hy)
    with pytest.raises(T.TTNError, match="ttn_braket_dev.*element types"):
        D.braket_dev(hx, hA, hr)
    ok()
    # an operator batch
    hB = T.DeviceTTO.stack([T.Delta(d), T.Delta(d)])
    hr2 = upload_batch([crand_tt(dims, 4, rng, False), crand_tt(dims, 4, rng, False)])
    with pytest.raises(T.TTNError, match="operator batch"):
        D.braket(hr2, hB, hr2)
    ok()
    h3 = upload_batch([crand_tt((2,) * (d - 1) + (3,), 4, rng)])
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        D.braket(h3, hA, hy)
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        D.braket(hx, hA, h3)
    ok()
    hb = upload_batch([y, y])
    with pytest.raises(AssertionError, match="batch sizes differ"):
        D.braket(hx, hA, hb)
    ok()
    with pytest.raises(TypeError, match="DeviceTTO"):
        D.braket(hx, hx, hy)
    # sandwich keeps refusing complex handles
    with pytest.raises(T.TTNError, match="Float64 only"):
        D.sandwich(hx, hA, hy)
    ok()
    for h in (hx, hy, hA, hr, hB, hr2, h3, hb):
        h.free()


def test_status_is_clean():
    D.status_all()
