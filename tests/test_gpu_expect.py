"""<x, A y> on the GPU (csrc/ttn_expect_kernels.h, include/ttn_expect.h) against the oracle's dot(x, A * y).

Bar: the one dot carries in test_gpu_parity.py, |got - ref| <= 1e-12 ||x|| ||A y||, norms from the oracle.  Shapes: the smallest at which
each piece can go wrong — d = 1 and 2, mixed dims on the general route with a ragged batch and an all-zero train, QTT trains with ranks off
the 16 x 16 tile, different ranks on the two sides, ramps and full interior sites, one case just inside and one just outside each
exported limit of the on-chip route (a train takes ONE route for its whole chain, so there is no per-site hand-over to cross; a batch
whose trains take different routes is the hand-over that exists)."""
import numpy as np
import pytest

import ttn_amd as T
from oracle import tt_oracle as O
from tests import expect_reference as R
from tests.helpers import to_oracle, to_product
from tests.test_cpu_expect import mixed_case, periodic_ising
from ttn_amd import device as D

pytestmark = pytest.mark.gpu

RMAX, OPMAX = D.EXPECT_QTT_MAX_RANK, D.EXPECT_QTT_MAX_OP_RANK


def upload_batch(trains, cap=None):
    dims = trains[0].ttv_dims
    if cap is None:
        cap = [max(t.ttv_rks[m] for t in trains) for m in range(len(dims) + 1)]
    h = T.DeviceTT(dims, cap, batch=len(trains))
    for b, t in enumerate(trains):
        h.upload(b, to_product(t))
    return h


def reference(x, A, y):
    """(ref, scale) = (dot(x, A y), ||x|| ||A y||) from the oracle."""
    Ay = O.apply(A, y)
    return O.dot(x, Ay), O.norm(x) * O.norm(Ay)


def transpose(A):
    return O.TToperator(A.N, [np.swapaxes(c, 0, 1).copy() for c in A.tto_vec], A.tto_dims, A.tto_rks, A.tto_ot)


def check(xs, A, ys, same=False):
    """sandwich on a batch against the oracle, train by train; returns the device numbers."""
    hx = upload_batch(xs)
    hy = hx if same else upload_batch(ys)
    hA = T.DeviceTTO(to_product(A))
    got = D.sandwich(hx, hA, hy)
    assert got.shape == (len(xs),)
    for b, (x, y) in enumerate(zip(xs, ys)):
        ref, scale = reference(x, A, y)
        print(f"train {b}: got {got[b]:.17e} ref {ref:.17e} err/scale {abs(got[b] - ref) / scale if scale else 0.0:.2e}")
        assert abs(got[b] - ref) <= 1e-12 * scale
    for h in {hx, hy}:
        h.free()
    hA.free()
    return got


def test_d1_and_d2():
    rng = np.random.default_rng(1)
    for dims, rx, ry, Ar in [((3,), [1, 1], [1, 1], [1, 1]), ((2, 3), [1, 2], [1, 3], [1, 2])]:
        d = len(dims)
        rx, ry, Ar = rx + [1] * (d + 1 - len(rx)), ry + [1] * (d + 1 - len(ry)), Ar + [1] * (d + 1 - len(Ar))
        x, y = O.rand_tt(dims, rx, rng), O.rand_tt(dims, ry, rng)
        A = O.TToperator(d, [rng.standard_normal((dims[k], dims[k], Ar[k], Ar[k + 1])) for k in range(d)], dims, Ar, [0] * d)
        check([x], A, [y])


def test_general_route_mixed_dims_ragged_batch_and_zero_train():
    x, A, y = mixed_case()
    rng = np.random.default_rng(21)
    x1 = O.rand_tt(x.ttv_dims, [1, 2, 3, 2, 1], rng)                 # below the handle's capacity [1, 2, 5, 3, 1]
    y1 = O.rand_tt(y.ttv_dims, [1, 2, 4, 1, 1], rng)
    x2 = O.TTvector(x.N, [np.zeros_like(c) for c in x.ttv_vec], x.ttv_dims, x.ttv_rks, x.ttv_ot)
    got = check([x, x1, x2], A, [y, y1, y])
    assert got[2] == 0.0
    # the restatement of tests/expect_reference.py sees the same number
    assert abs(got[0] - R.sandwich(x, A, y)) <= 1e-12 * reference(x, A, y)[1]


QTT_CASES = [(9, 5, 13, 3), (7, 16, 17, 1), (12, 37, 64, 2), (14, 64, 21, 5), (14, 64, 64, 3)]


@pytest.mark.parametrize("d,rx,ry,R_", QTT_CASES)
def test_qtt_route_dense_nonsymmetric_operator(d, rx, ry, R_):
    rng = np.random.default_rng(100 * d + R_)
    dims = (2,) * d
    A = O.rand_tto(dims, R_, rng)
    assert max(A.tto_rks) == R_ <= OPMAX and max(rx, ry) <= RMAX
    check([O.rand_tt(dims, rx, rng), O.rand_tt(dims, rx, rng)], A, [O.rand_tt(dims, ry, rng), O.rand_tt(dims, ry, rng)])


@pytest.mark.parametrize("name", ["shift", "Nabla", "Delta", "heisenberg"])
def test_named_operators(name):
    d = 9
    rng = np.random.default_rng(7)
    A = {"shift": lambda: O.shift(d), "Nabla": lambda: to_oracle(T.Nabla(d)), "Delta": lambda: O.Delta(d),
         "heisenberg": lambda: to_oracle(T.heisenberg_xyz_tto(d, jx=1.0, jy=0.7, jz=-1.2, lam=0.3, field="x"))}[name]()
    assert max(A.tto_rks) == (5 if name == "heisenberg" else 3)
    check([O.rand_tt((2,) * d, 11, rng)], A, [O.rand_tt((2,) * d, 16, rng)])


def test_limits_of_the_qtt_route_inside_and_outside():
    d = 14
    dims = (2,) * d
    rng = np.random.default_rng(3)
    # just inside both limits at once
    check([O.rand_tt(dims, RMAX, rng)], O.rand_tto(dims, OPMAX, rng), [O.rand_tt(dims, RMAX, rng)])
    # train rank limit + 1 on either side: the general route
    check([O.rand_tt(dims, RMAX + 1, rng)], O.rand_tto(dims, 2, rng), [O.rand_tt(dims, RMAX, rng)])
    check([O.rand_tt(dims, RMAX, rng)], O.rand_tto(dims, 2, rng), [O.rand_tt(dims, RMAX + 1, rng)])
    # operator rank limit + 1
    A = O.rand_tto(dims, OPMAX + 1, rng)
    assert max(A.tto_rks) == OPMAX + 1
    check([O.rand_tt(dims, 20, rng)], A, [O.rand_tt(dims, 33, rng)])


def test_one_batch_two_routes():
    """Train 0 has a rank above the limit and takes the general route, train 1 fits the on-chip route: the decision is per train."""
    d = 10
    dims = (2,) * d
    rng = np.random.default_rng(5)
    xs = [O.rand_tt(dims, 32, rng), O.rand_tt(dims, 32, rng)]
    ys = [O.rand_tt(dims, RMAX + 1, rng), O.rand_tt(dims, RMAX, rng)]
    check(xs, O.Delta(d), ys)


def test_identities():
    d = 9
    dims = (2,) * d
    rng = np.random.default_rng(11)
    x, y = O.rand_tt(dims, 13, rng), O.rand_tt(dims, 20, rng)
    A = O.rand_tto(dims, 3, rng)
    ref, scale = reference(x, A, y)
    hx, hy = upload_batch([x]), upload_batch([y])
    hA, hAt, hI = T.DeviceTTO(to_product(A)), T.DeviceTTO(to_product(transpose(A))), T.DeviceTTO(to_product(O.id_tto(d)))
    s = D.sandwich(hx, hA, hy)[0]
    st = D.sandwich(hy, hAt, hx)[0]
    assert abs(s - ref) <= 1e-12 * scale and abs(st - ref) <= 1e-12 * scale
    # a transposed read is a different number (the operator is dense and non-symmetric)
    assert abs(D.sandwich(hx, hAt, hy)[0] - ref) > 1e-6 * scale
    # expect: the same handle twice
    refx, scalex = reference(x, A, x)
    e = D.expect(hA, hx)[0]
    assert abs(e - refx) <= 1e-12 * scalex and abs(D.sandwich(hx, hA, hx)[0] - refx) <= 1e-12 * scalex
    # the identity operator gives dot
    sxy = O.norm(x) * O.norm(y)
    assert abs(D.sandwich(hx, hI, hy)[0] - O.dot(x, y)) <= 1e-12 * sxy
    assert abs(D.sandwich(hx, hI, hy)[0] - D.dot(hx, hy)[0]) <= 2e-12 * sxy
    # rayleigh
    assert abs(D.rayleigh(hA, hx)[0] - refx / O.dot(x, x)) <= 2e-12 * scalex / O.dot(x, x)
    # the device-resident result
    out = D.sandwich_dev(hx, hA, hy)
    D.sync()
    assert out.shape == (1,) and abs(float(out.cpu()[0]) - ref) <= 1e-12 * scale
    import torch
    buf = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    assert D.sandwich_dev(hx, hA, hy, out=buf) is buf
    D.sync()
    assert abs(float(buf.cpu()[0]) - s) <= 1e-12 * scale
    for h in (hx, hy, hA, hAt, hI):
        h.free()


def test_sandwich_dev_equals_sandwich_on_the_general_route():
    x, A, y = mixed_case()
    hx, hy, hA = upload_batch([x, x]), upload_batch([y, y]), T.DeviceTTO(to_product(A))
    host = D.sandwich(hx, hA, hy)
    dev = D.sandwich_dev(hx, hA, hy)
    D.sync()
    assert np.array_equal(dev.cpu().numpy(), host)          # three GEMMs per site in a fixed order: the same bits
    for h in (hx, hy, hA):
        h.free()


@pytest.mark.parametrize("g", [0.5, 1.5])
def test_ising_model_energy_and_magnetisation(g):
    """examples/ising_model.jl at d = 6: the ground state from dmrg_eigsolve (rmax 8: no truncation), its Rayleigh quotient and its
    z-magnetisation from one sweep each against the dense 64-vector."""
    d = 6
    H = to_product(periodic_ising(T, d, g))
    _, psi, _ = T.dmrg_eigsolve(H, T.qtt_basis_vector(d, 1), sweep_schedule=[2, 4], rmax_schedule=[8, 8], tol=1.0e-10)
    po, Ho, Zo = to_oracle(psi), to_oracle(H), to_oracle(T.pauli_sum_tto("z", d))
    v = O.ttv_to_tensor(po).reshape(-1)
    Hd = R.periodic_ising_dense(d, g)
    nrm = O.norm(po)
    scaleH, scaleZ = nrm * O.norm(O.apply(Ho, po)), nrm * O.norm(O.apply(Zo, po))
    ray = T.rayleigh(H, psi)
    ref = float(v @ Hd @ v) / float(v @ v)
    print(f"g {g}: rayleigh {ray:.17e} dense {ref:.17e} err/scale {abs(ray - ref) / scaleH:.2e}")
    assert abs(ray - ref) <= 1e-12 * scaleH
    assert ref <= np.linalg.eigvalsh(Hd)[0] + 1e-6 * abs(ref)          # it is the ground state
    mag = abs(T.expect(T.pauli_sum_tto("z", d), psi)) / (d * T.dot(psi, psi))
    mref = R.z_magnetization(v)
    print(f"g {g}: magnetisation {mag:.17e} dense {mref:.17e} err/scale {abs(mag - mref) / scaleZ:.2e}")
    assert abs(mag - mref) <= 1e-12 * scaleZ
    # on resident handles, a batch of two
    hp, hH = T.DeviceTT.from_host(psi, batch=2), T.DeviceTTO(H)
    assert np.all(np.abs(D.rayleigh(hH, hp) - ref) <= 1e-12 * scaleH)
    hp.free(), hH.free()


def test_refusals_leave_the_library_usable():
    d = 5
    dims = (2,) * d
    rng = np.random.default_rng(9)
    x, y = O.rand_tt(dims, 4, rng), O.rand_tt(dims, 6, rng)
    A = O.Delta(d)
    ref, scale = reference(x, A, y)
    hx, hy, hA = upload_batch([x]), upload_batch([y]), T.DeviceTTO(to_product(A))

    def ok():
        assert abs(D.sandwich(hx, hA, hy)[0] - ref) <= 1e-12 * scale

    ok()
    h3 = upload_batch([O.rand_tt((2,) * (d - 1) + (3,), 4, rng)])
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        D.sandwich(h3, hA, hy)
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        D.sandwich(hx, hA, h3)
    ok()
    hb = upload_batch([y, y])
    with pytest.raises(AssertionError, match="batch sizes differ"):
        D.sandwich(hx, hA, hb)
    ok()
    hc = T.DeviceTT(dims, [1, 2, 2, 2, 2, 1], batch=1, dtype=np.complex128)
    with pytest.raises(T.TTNError, match="Float64 only"):
        D.sandwich(hc, hA, hy)
    with pytest.raises(T.TTNError, match="Float64 only"):
        D.sandwich_dev(hx, hA, hc)
    ok()
    for h in (hx, hy, hA, h3, hb, hc):
        h.free()
