"""Site-resolved measurements on ComplexF64 trains on the GPU (csrc/ttn_zmeasure_kernels.h, include/ttn_zmeasure.h) against the NumPy
restatements of tests/zmeasure_reference.py.

Bar: |got - ref| <= 1e-12 ||P_i||_2 ||Q_j||_2 on normalised values, complex modulus — the project's rule for dot (1e-12 ||a|| ||b||,
DESIGN 4.19) divided by <x|x>, as in tests/test_gpu_measure.py; a complex128 chain in another sum order shows 3.5e-16 / 5.8e-16
(tests/test_cpu_zmeasure.py).  Every test prints its worst err / scale.  Shapes: the on-chip class with full and ragged, off-tile ranks
in one batch; rank 80, mixed dims and n = 3 on the general route; a rank-64 and a rank-80 train in one handle (both routes in one call);
d = 1 and 2; analytic states that fix the side of the conjugate and the orientation of the output; a batch beyond one workspace chunk;
poisoned workspace; five pairs tied to device.braket."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ttn_amd as T
from tests import measure_reference as RR
from tests import zmeasure_reference as R
from tests.helpers import worst_of
from ttn_amd import device as D

pytestmark = pytest.mark.gpu

TOL = 1e-12


def to_tt(cores):
    dims = tuple(c.shape[0] for c in cores)
    rks = [c.shape[1] for c in cores] + [cores[-1].shape[2]]
    return T.TTvector(len(cores), [np.asfortranarray(c) for c in cores], dims, rks, [0] * len(cores))


def upload(trains, batch=None, dtype=np.complex128):
    dims = tuple(c.shape[0] for c in trains[0])
    d = len(dims)
    cap = [max(([t[k].shape[1] for k in range(d)] + [1])[m] for t in trains) for m in range(d + 1)]
    h = T.DeviceTT(dims, cap, batch=batch or len(trains), dtype=dtype)
    for b, t in enumerate(trains):
        h.upload(b, to_tt(t))
    return h


def worst_profile(what, got, ref, norms, quiet=False):
    err = float(np.max(np.abs(got - ref) / norms))
    if not quiet:
        print(f"{what}: worst err/scale {err:.2e}")
    return err


def worst_corr(what, got, ref, pn, qn, quiet=False):
    err = float(np.max(np.abs(got - ref) / np.outer(pn, qn)))
    if not quiet:
        print(f"{what}: worst err/scale {err:.2e}")
    return err


@pytest.fixture(scope="module")
def class_case():
    """Case 1: d = 12, n = 2, full ranks 1, 2, .., 64, .., 2, 1; train 1 capped at rank 13, train 2 at rank 7.  The dense references are
    computed once and left unchanged."""
    dims, trains, P, Q = R.case("class_d12")
    assert [c.shape[2] for c in trains[0]][5] == 64 and max(c.shape[2] for c in trains[1]) == 13 and max(c.shape[2] for c in trains[2]) == 7
    h = upload(trains)
    Pd = P.conj().T
    ref = {"EP": [R.dense_site_expect(t, P) for t in trains], "EQ": [R.dense_site_expect(t, Q) for t in trains],
           "EPd": [R.dense_site_expect(t, Pd) for t in trains], "C": [R.dense_correlation(t, P, Q) for t in trains]}
    yield dims, trains, P, Q, h, ref
    h.free()


@pytest.fixture(scope="module")
def general_cases():
    """Case 2: the general route's shapes with their dense references, computed once."""
    out = {}
    for name in ("rank80_d14", "mixed_dims", "n3_d6"):
        dims, trains, P, Q = R.case(name)
        out[name] = (dims, trains, P, Q, [R.dense_site_expect(t, P) for t in trains], [R.dense_site_expect(t, Q) for t in trains],
                     [R.dense_correlation(t, P, Q) for t in trains])
    return out


def check_class(class_case, tag=""):
    dims, trains, P, Q, h, ref = class_case
    Pd = P.conj().T
    got = D.zsite_expect(h, P, Q, Pd)
    assert got.shape == (3, 3, 12) and got.dtype == np.complex128
    singles = [D.zsite_expect(h, op) for op in (P, Q, Pd)]
    assert all(s.shape == (3, 12) for s in singles)
    norms = [R.op_norms(op, dims) for op in (P, Q, Pd)]
    for b in range(3):
        dense = [ref["EP"][b], ref["EQ"][b], ref["EPd"][b]]
        for j in range(3):
            assert worst_profile(f"{tag}train {b} table {j} vs dense", got[b, j], dense[j], norms[j]) <= TOL
            assert worst_profile(f"{tag}train {b} table {j} vs single call", got[b, j], singles[j][b], norms[j]) <= TOL
    Cm = D.zcorrelation_matrix(h, P, Q)
    assert Cm.shape == (3, 12, 12) and Cm.dtype == np.complex128
    for b in range(3):
        assert worst_corr(f"{tag}train {b} C", Cm[b], ref["C"][b], norms[0], norms[1]) <= TOL
    return Cm


def check_general(general_cases, name, tag=""):
    dims, trains, P, Q, refEP, refEQ, refC = general_cases[name]
    h = upload(trains)
    try:
        pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
        E = D.zsite_expect(h, P, Q)
        Cm = D.zcorrelation_matrix(h, P, Q)
        assert E.shape == (len(trains), 2, len(dims)) and Cm.shape == (len(trains), len(dims), len(dims))
        for b in range(len(trains)):
            assert worst_profile(f"{tag}{name} train {b} E_P", E[b, 0], refEP[b], pn) <= TOL
            assert worst_profile(f"{tag}{name} train {b} E_Q", E[b, 1], refEQ[b], qn) <= TOL
            assert worst_corr(f"{tag}{name} train {b} C", Cm[b], refC[b], pn, qn) <= TOL
    finally:
        h.free()


# ---- 1. the on-chip class --------------------------------------------------------------------------------------------------------------
def test_class_profiles_and_correlations(class_case):
    Cm = check_class(class_case)
    assert np.max(np.abs(Cm[0] - Cm[0].T)) > 1e-3 and np.max(np.abs(Cm[0] - Cm[0].conj().T)) > 1e-3      # P != Q: neither symmetric nor Hermitian


def test_class_p_equals_q_mirrors_the_triangle(class_case):
    dims, trains, P, Q, h, ref = class_case
    pn = R.op_norms(P, dims)
    mirrored, two_pass = D.zcorrelation_matrix(h, P), D.zcorrelation_matrix(h, P, P.copy() + 0.0)
    for b, t in enumerate(trains):
        assert np.array_equal(mirrored[b], mirrored[b].T)                # the plain copy: no conjugate
        assert worst_corr(f"P = Q train {b} vs dense", mirrored[b], R.dense_correlation(t, P, P), pn, pn) <= TOL
        assert worst_corr(f"P = Q train {b}, equal copies", mirrored[b], two_pass[b], pn, pn) <= TOL


# ---- 2. the general route --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rank80_d14", "mixed_dims", "n3_d6"])
def test_general_route(general_cases, name):
    check_general(general_cases, name)


# ---- 3. one batch, two routes ----------------------------------------------------------------------------------------------------------
def test_one_batch_two_routes():
    dims = (2,) * 14
    rng = np.random.default_rng(1464)
    trains = [R.crand_train(dims, RR.full_ranks(dims, cap), rng) for cap in (64, 80)]
    P, Q = R.crand_matrix(2, rng), R.crand_matrix(2, rng)
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    h = upload(trains)
    E, Cm = D.zsite_expect(h, P), D.zcorrelation_matrix(h, P, Q)
    for b, t in enumerate(trains):
        assert worst_profile(f"rank {(64, 80)[b]} in one handle: E", E[b], R.dense_site_expect(t, P), pn) <= TOL
        assert worst_corr(f"rank {(64, 80)[b]} in one handle: C", Cm[b], R.dense_correlation(t, P, Q), pn, qn) <= TOL
    h.free()


# ---- 4. edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(2,), (3,), (2, 2), (3, 2)])
def test_edges_d1_d2_single_train(dims):
    rng = np.random.default_rng(len(dims) * 10 + dims[0])
    cores = R.crand_train(dims, RR.full_ranks(dims, 8), rng)
    P, Q = [R.crand_matrix(n, rng) for n in dims], [R.crand_matrix(n, rng) for n in dims]
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    h = upload([cores])
    Cm = D.zcorrelation_matrix(h, P, Q)
    assert Cm.shape == (1, len(dims), len(dims))
    assert worst_corr(f"dims {dims}", Cm[0], R.dense_correlation(cores, P, Q), pn, qn) <= TOL
    E = D.zsite_expect(h, P)
    assert E.shape == (1, len(dims))
    assert worst_profile(f"dims {dims}", E[0], R.dense_site_expect(cores, P), pn) <= TOL
    if len(dims) == 1:                                              # d = 1: the 1 x 1 result is E_{PQ}
        assert abs(Cm[0, 0, 0] - D.zsite_expect(h, [P[0] @ Q[0]])[0, 0]) <= TOL * pn[0] * qn[0]
    h.free()


# ---- 5. conjugation and orientation ----------------------------------------------------------------------------------------------------
def test_plus_y_product_state():
    """|+y>^(x)6: <sigma_y> = +1.  A conjugate on the wrong side gives -1; a Float64-only library cannot give the number at all."""
    h = upload([R.plus_y_train(6)])
    E = D.zsite_expect(h, R.SX, R.SY, R.SZ)[0]
    one = np.ones(6)
    assert worst_profile("|+y> sigma_x", E[0], np.zeros(6), one) <= TOL
    assert worst_profile("|+y> sigma_y", E[1], np.ones(6), one) <= TOL
    assert worst_profile("|+y> sigma_z", E[2], np.zeros(6), one) <= TOL
    h.free()


def test_precessing_product_state():
    th = 0.1 + 0.37 * np.arange(7)
    h = upload([R.precessing_train(th)])
    one = np.ones(7)
    E = D.zsite_expect(h, R.SZ, R.SY)[0]
    assert worst_profile("precessing sigma_z", E[0], np.cos(2 * th), one) <= TOL
    assert worst_profile("precessing sigma_y", E[1], -np.sin(2 * th), one) <= TOL
    Cm = D.zcorrelation_matrix(h, R.SZ, R.SY)[0]
    off = ~np.eye(7, dtype=bool)
    want = -np.outer(np.cos(2 * th), np.sin(2 * th))
    err = float(np.max(np.abs(Cm - want)[off]))
    print(f"precessing <sigma_z,i sigma_y,j>: worst err {err:.2e}")
    assert err <= TOL
    assert np.max(np.abs(want - want.T)[off]) > 0.1                   # a transposed output would show
    h.free()


def test_complex_ghz_state():
    h = upload([R.complex_ghz_train(8, 0.7)])
    one = np.ones(8)
    assert worst_profile("GHZ <Z_k>", D.zsite_expect(h, R.SZ)[0], np.zeros(8), one) <= TOL
    assert worst_corr("GHZ <Z_i Z_j>", D.zcorrelation_matrix(h, R.SZ)[0], np.ones((8, 8)), one, one) <= TOL
    Cm = D.zcorrelation_matrix(h, R.SPLUS, R.SMINUS)[0]
    err = float(np.max(np.abs(Cm[~np.eye(8, dtype=bool)])))
    print(f"GHZ <s+_i s-_j>, i != j: worst {err:.2e}")
    assert err <= TOL
    h.free()


def test_output_is_not_transposed(class_case):
    dims, trains, P, Q, h, ref = class_case
    Cm = D.zcorrelation_matrix(h, P, Q)
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    for b in range(3):
        assert worst_corr(f"train {b} C[i, j] vs dense[i, j]", Cm[b], ref["C"][b], pn, qn) <= TOL
        wrong = float(np.max(np.abs(Cm[b] - ref["C"][b].T) / np.outer(pn, qn)))
        print(f"train {b} C[i, j] vs dense[j, i]: {wrong:.2e}")
        assert wrong > 1e-3


# ---- 6. identities on the class case ---------------------------------------------------------------------------------------------------
def test_identities(class_case):
    dims, trains, P, Q, h, ref = class_case
    one = np.ones(12)
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    Pd, Qd = P.conj().T, Q.conj().T
    assert worst_profile("E_I", D.zsite_expect(h, R.I2), np.ones((3, 12)), one) <= TOL
    Hm = P + Pd
    EH = D.zsite_expect(h, Hm)
    assert worst_profile("Hermitian table: Im E", EH.imag, np.zeros((3, 12)), np.linalg.norm(Hm, 2) * one) <= TOL
    EP, EPd = D.zsite_expect(h, P), D.zsite_expect(h, Pd)
    assert worst_profile("E_{P^+} = conj E_P", EPd, EP.conj(), pn) <= TOL
    Cm, Cd = D.zcorrelation_matrix(h, P, Q), D.zcorrelation_matrix(h, Qd, Pd)
    for b in range(3):
        assert worst_corr(f"C_PQ[i, j] = conj C_(Q^+ P^+)[j, i] train {b}", Cm[b], Cd[b].conj().T, pn, qn) <= TOL
    # x -> (0.3 - 2i) x changes nothing: two device numbers, 2 TOL
    scaled = [[c * (0.3 - 2.0j) if k == 0 else c for k, c in enumerate(t)] for t in trains]
    hs = upload(scaled)
    Es, Cs = D.zsite_expect(hs, P), D.zcorrelation_matrix(hs, P, Q)
    hs.free()
    assert worst_profile("scaled train E", Es, EP, pn) <= 2 * TOL
    for b in range(3):
        assert worst_corr(f"scaled train C, train {b}", Cs[b], Cm[b], pn, qn) <= 2 * TOL
    nn = np.real(D.dot(h, h))
    Eu, Cu = D.zsite_expect(h, P, normalize=False), D.zcorrelation_matrix(h, P, Q, normalize=False)
    for b in range(3):
        assert worst_profile(f"normalize=False train {b}", Eu[b] / nn[b], EP[b], pn) <= TOL
        assert worst_corr(f"normalize=False train {b}", Cu[b] / nn[b], Cm[b], pn, qn) <= TOL


def test_profiles_sum_to_braket_of_the_pauli_sums(class_case):
    dims, trains, P, Q, h, ref = class_case
    d = 12
    E = D.zsite_expect(h, R.SX, R.SY, R.SZ)
    nn = D.dot(h, h)
    for j, mu in enumerate("xyz"):
        hA = T.DeviceTTO(T.pauli_sum_tto(mu, d, dtype=np.complex128))
        want = D.braket(h, hA, h) / nn
        hA.free()
        err = float(np.max(np.abs(E[:, j, :].sum(axis=1) - want)))
        print(f"sum_k E_sigma_{mu}[k] vs braket / dot: worst {err:.2e}")
        assert err <= d * TOL


# ---- 7. real data ----------------------------------------------------------------------------------------------------------------------
def test_real_data_against_the_float64_calls():
    dims, trains, P, Q = RR.case("class_d12")
    hr = upload(trains, dtype=np.float64)
    hz = upload(trains, dtype=np.complex128)                          # imaginary parts zero
    pn, qn = RR.op_norms(P, dims), RR.op_norms(Q, dims)
    Ez, Cz = D.zsite_expect(hz, P, Q), D.zcorrelation_matrix(hz, P, Q)
    Er, Cr = D.site_expect(hr, P, Q), D.correlation_matrix(hr, P, Q)
    for b in range(3):                                                # two device numbers: 2 TOL
        assert worst_profile(f"real data train {b} E_P", Ez[b, 0], Er[b, 0], pn) <= 2 * TOL
        assert worst_profile(f"real data train {b} E_Q", Ez[b, 1], Er[b, 1], qn) <= 2 * TOL
        assert worst_corr(f"real data train {b} C", Cz[b], Cr[b], pn, qn) <= 2 * TOL
    hr.free()
    hz.free()


# ---- 8. the tie to braket --------------------------------------------------------------------------------------------------------------
def test_tie_to_braket_d30():
    rng = np.random.default_rng(30)
    d = 30
    dims = (2,) * d
    cores = R.crand_train(dims, RR.full_ranks(dims, 8), rng)
    P, Q = R.crand_matrix(2, rng), R.crand_matrix(2, rng)
    scale = np.linalg.norm(P, 2) * np.linalg.norm(Q, 2)
    h = upload([cores])
    Cm = D.zcorrelation_matrix(h, P, Q)[0]
    nn = D.dot(h, h)[0]
    worst = 0.0
    for i, j in [(0, 29), (3, 4), (14, 15), (7, 22), (28, 29)]:
        for a, b in ((i, j), (j, i)):                               # C[a, b] = <P_a Q_b>: the product operator with P at a and Q at b
            mats = [R.I2] * d
            mats[a], mats[b] = P, Q
            A = T.TToperator(d, [np.asfortranarray(m.reshape(2, 2, 1, 1)) for m in mats], dims, [1] * (d + 1), [0] * d)
            hA = T.DeviceTTO(A)
            want = D.braket(h, hA, h)[0] / nn
            hA.free()
            worst = worst_of(worst, abs(Cm[a, b] - want) / scale)
    print(f"five pairs, both orders, against braket / dot: worst err/scale {worst:.2e}")
    assert worst <= TOL
    h.free()


# ---- 9. chunking -----------------------------------------------------------------------------------------------------------------------
def test_batch_beyond_one_workspace_chunk(general_cases):
    """More trains than TTN_ZMEASURE_CHUNK_BYTES of workspace hold: the entry point splits the batch, every train gets the same numbers."""
    dims, trains, P, Q, refEP, refEQ, refC = general_cases["rank80_d14"]
    d, B = len(dims), 40
    hdr = open(os.path.join(T._lib.INCLUDE, "ttn_zmeasure.h")).read()
    chunk_bytes = int(re.search(r"#define\s+TTN_ZMEASURE_CHUNK_BYTES\s+(\d+)", hdr).group(1))
    W, N = max(8192, 2 * 80 * 80), 2 * 2 * 80 * 80
    per_train = 2 * (d + 1) * W + 3 * d * W + 2 * 2 * (d - 1) * W + 2 * N + max(3 * d, 2 * (d - 1)) * 2 * N      # the formula of the header
    assert 1 <= chunk_bytes // (8 * per_train) < B
    h = upload(trains[:1], batch=B)
    h.replicate(0)
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    Cm = D.zcorrelation_matrix(h, P, Q)
    E = D.zsite_expect(h, P)
    assert Cm.shape == (B, d, d) and E.shape == (B, d)
    errC = worst_of(*(worst_corr("", Cm[b], refC[0], pn, qn, quiet=True) for b in range(B)))
    errE = worst_of(*(worst_profile("", E[b], refEP[0], pn, quiet=True) for b in range(B)))
    print(f"{B} trains in chunks: worst err/scale C {errC:.2e} E {errE:.2e}")
    assert errC <= TOL and errE <= TOL
    h.free()


# ---- 10. poisoned workspace ------------------------------------------------------------------------------------------------------------
QNAN = 0x7FF8000000000000
BIG = int(np.float64(1e300).view(np.uint64))


@pytest.fixture(params=[pytest.param(QNAN, id="qnan"), pytest.param(BIG, id="1e300")])
def poison(request):
    """ttn_selftest_poison fills the workspace at every acquisition with the pattern: a read of an unwritten state or image shows."""
    T.ensure_init(0)
    assert T._lib.lib().ttn_selftest_poison(1, C.c_uint64(request.param)) == 0
    try:
        yield request.param
    finally:
        assert T._lib.lib().ttn_selftest_poison(0, C.c_uint64(0)) == 0


def test_class_on_poisoned_workspace(class_case, poison):
    check_class(class_case, tag="poisoned ")


@pytest.mark.parametrize("name", ["rank80_d14", "mixed_dims", "n3_d6"])
def test_general_route_on_poisoned_workspace(general_cases, name, poison):
    check_general(general_cases, name, tag="poisoned ")


# ---- 11. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_library_usable():
    rng = np.random.default_rng(8)
    dims = (2, 2, 2)
    hr = T.DeviceTT(dims, [1, 2, 2, 1], batch=1)
    with pytest.raises(T.TTNError, match="site_expect"):
        D.zsite_expect(hr, R.SZ)
    with pytest.raises(T.TTNError, match="site_expect"):
        D.zcorrelation_matrix(hr, R.SZ)
    # the library's own refusal, under the Python layer's
    out = np.zeros(2 * 3)
    tab = np.ascontiguousarray(np.tile(R.SZ.flatten(order="F"), 3)).view(np.float64)
    rc = T._lib.lib().ttn_zsite_expect(hr.h, 1, tab.ctypes.data_as(T._lib.p_f64), 1, out.ctypes.data_as(T._lib.p_f64))
    with pytest.raises(T.TTNError, match="ttn_site_expect"):
        T._lib.check(rc)
    hr.free()
    cores = R.crand_train(dims, [1, 2, 2, 1], rng)
    h = upload([cores])
    assert D.ZMEASURE_MAX_OPS == 16
    with pytest.raises(T.TTNError):
        D.zsite_expect(h, *([R.SZ] * 17))
    tab17 = np.ascontiguousarray(np.tile(R.SZ.flatten(order="F"), 3 * 17)).view(np.float64)
    out17 = np.zeros(2 * 3 * 17)
    rc = T._lib.lib().ttn_zsite_expect(h.h, 17, tab17.ctypes.data_as(T._lib.p_f64), 1, out17.ctypes.data_as(T._lib.p_f64))
    with pytest.raises(T.TTNError, match="nops"):
        T._lib.check(rc)
    got = D.zsite_expect(h, *([R.SZ] * 16))                          # the limit itself is fine
    assert got.shape == (1, 16, 3)
    one = np.ones(3)
    assert worst_profile("after the refusals", got[0, 15], R.dense_site_expect(cores, R.SZ), one) <= TOL
    assert worst_corr("after the refusals", D.zcorrelation_matrix(h, R.SY)[0], R.dense_correlation(cores, R.SY), one, one) <= TOL
    with pytest.raises(T.TTNError, match="Float64 only"):             # the Float64 names still refuse the complex handle
        D.site_expect(h, np.diag([1.0, -1.0]))
    h.free()


# ---- 12. host forms, device forms ------------------------------------------------------------------------------------------------------
def test_host_and_device_forms():
    import torch
    dims, trains, P, Q = R.case("n3_d6")
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    x = to_tt(trains[0])
    h = upload(trains[:1])
    E1, E2 = T.zsite_expect(x, P), T.zsite_expect(x, P, Q)
    C1 = T.zcorrelation_matrix(x, P, Q)
    assert E1.shape == (6,) and E2.shape == (2, 6) and C1.shape == (6, 6) and C1.dtype == np.complex128
    assert worst_profile("host zsite_expect", E1, D.zsite_expect(h, P)[0], pn) <= TOL
    assert worst_profile("host zsite_expect, two tables", E2[1], D.zsite_expect(h, Q)[0], qn) <= TOL
    assert worst_corr("host zcorrelation_matrix", C1, D.zcorrelation_matrix(h, P, Q)[0], pn, qn) <= TOL
    Cc = T.zcorrelation_matrix(x, P, Q, connected=True)
    # three device numbers per entry on either side (C, E_P, E_Q), each reproducible to TOL: 3 TOL
    assert worst_corr("host connected", Cc, C1 - np.outer(E2[0], E2[1]), pn, qn) <= 3 * TOL
    Ed = D.zsite_expect_dev(h, P, Q)
    Cd = D.zcorrelation_matrix_dev(h, P, Q)
    D.sync()
    torch.cuda.synchronize()
    assert Ed.dtype == torch.complex128 and Cd.dtype == torch.complex128
    assert worst_profile("zsite_expect_dev", Ed.cpu().numpy()[0], E2, np.stack([pn, qn])) <= TOL
    assert worst_corr("zcorrelation_matrix_dev", Cd.cpu().numpy()[0], C1, pn, qn) <= TOL
    h.free()
    # a real host train gets its sigma_y numbers: it is uploaded as complex128, and equals the promoted train
    rdims, rtrains, _, _ = RR.case("class_d12")
    xr = to_tt(rtrains[1])
    xz = to_tt([c.astype(np.complex128) for c in rtrains[1]])
    one = np.ones(12)
    Ey, Eyz = T.zsite_expect(xr, R.SY), T.zsite_expect(xz, R.SY)
    assert worst_profile("real host train, sigma_y, vs promoted", Ey, Eyz, one) <= TOL
    assert worst_profile("real host train, sigma_y, vs dense", Ey, R.dense_site_expect(rtrains[1], R.SY), one) <= TOL
    Cy = T.zcorrelation_matrix(xr, R.SY, R.SZ)
    assert worst_corr("real host train, <sigma_y sigma_z>", Cy, R.dense_correlation(rtrains[1], R.SY, R.SZ), one, one) <= TOL
    assert np.max(np.abs(Cy)) > 1e-3
