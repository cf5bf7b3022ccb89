"""Site-resolved measurements on the GPU (csrc/ttn_measure_kernels.h, include/ttn_measure.h) against the NumPy restatements of
tests/measure_reference.py.

Bar: |got - ref| <= 1e-12 ||P_i||_2 ||Q_j||_2 on normalised values — the project's rule for dot (1e-12 ||a|| ||b||) divided
by <x, x>; it leaves about 500x over what a float64 chain in another sum order shows (tests/test_cpu_measure.py).  Every test prints its
worst err / scale.  Shapes: the smallest at which each piece can go wrong — the LDS-resident class with full and ragged, off-tile ranks
in one batch; a rank-80 interior between ramps inside the class (the state changes its home twice per walk); mixed dims and n = 3 on the
general route; d = 1 and 2; a batch beyond one workspace chunk; a long thin chain; five pairs tied to device.sandwich."""
import os
import re

import numpy as np
import pytest

import ttn_amd as T
from tests import measure_reference as R
from tests.helpers import worst_of
from ttn_amd import device as D

pytestmark = pytest.mark.gpu

TOL = 1e-12
IY = np.array([[0.0, 1.0], [-1.0, 0.0]])       # i sigma_y
Z = np.diag([1.0, -1.0])
I2 = np.eye(2)


def to_tt(cores):
    dims = tuple(c.shape[0] for c in cores)
    rks = [c.shape[1] for c in cores] + [cores[-1].shape[2]]
    return T.TTvector(len(cores), [np.asfortranarray(c) for c in cores], dims, rks, [0] * len(cores))


def upload(trains, batch=None):
    dims = tuple(c.shape[0] for c in trains[0])
    d = len(dims)
    cap = [max(([t[k].shape[1] for k in range(d)] + [1])[m] for t in trains) for m in range(d + 1)]
    h = T.DeviceTT(dims, cap, batch=batch or len(trains))
    for b, t in enumerate(trains):
        h.upload(b, to_tt(t))
    return h


def worst_profile(what, got, ref, norms):
    err = float(np.max(np.abs(got - ref) / norms))
    print(f"{what}: worst err/scale {err:.2e}")
    return err


def worst_corr(what, got, ref, pn, qn):
    err = float(np.max(np.abs(got - ref) / np.outer(pn, qn)))
    print(f"{what}: worst err/scale {err:.2e}")
    return err


@pytest.fixture(scope="module")
def class_case():
    """Case 1: d = 12, n = 2, full ranks 1, 2, .., 64, .., 2, 1; train 1 capped at rank 13, train 2 at rank 7.  The dense references
    are computed once and left unchanged."""
    dims, trains, P, Q = R.case("class_d12")
    assert [c.shape[2] for c in trains[0]][5] == 64 and max(c.shape[2] for c in trains[1]) == 13 and max(c.shape[2] for c in trains[2]) == 7
    h = upload(trains)
    ref = {"EP": [R.dense_site_expect(t, P) for t in trains], "EQ": [R.dense_site_expect(t, Q) for t in trains],
           "C": [R.dense_correlation(t, P, Q) for t in trains]}
    yield dims, trains, P, Q, h, ref
    h.free()


# ---- 1. the LDS-resident class ---------------------------------------------------------------------------------------------------------
def test_class_site_expect_three_tables_at_once(class_case):
    dims, trains, P, Q, h, ref = class_case
    rng = np.random.default_rng(77)
    S = [rng.standard_normal((2, 2)) for _ in dims]                  # a per-site table
    got = D.site_expect(h, P, Q, S)
    assert got.shape == (3, 3, 12)
    singles = [D.site_expect(h, op) for op in (P, Q, S)]
    assert all(s.shape == (3, 12) for s in singles)
    norms = [R.op_norms(op, dims) for op in (P, Q, S)]
    for b, t in enumerate(trains):
        dense = [ref["EP"][b], ref["EQ"][b], R.dense_site_expect(t, S)]
        for j in range(3):
            assert worst_profile(f"train {b} table {j} vs dense", got[b, j], dense[j], norms[j]) <= TOL
            assert worst_profile(f"train {b} table {j} vs single call", got[b, j], singles[j][b], norms[j]) <= TOL


def test_class_correlation_matrix(class_case):
    dims, trains, P, Q, h, ref = class_case
    got = D.correlation_matrix(h, P, Q)
    assert got.shape == (3, 12, 12)
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    for b in range(3):
        assert worst_corr(f"train {b}", got[b], ref["C"][b], pn, qn) <= TOL
    assert np.max(np.abs(got[0] - got[0].T)) > 1e-3                  # P != Q: not symmetric


# ---- 2. the general route --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rank80_d14", "mixed_dims", "n3_d6"])
def test_general_route(name):
    dims, trains, P, Q = R.case(name)
    h = upload(trains)
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    E = D.site_expect(h, P, Q)
    C = D.correlation_matrix(h, P, Q)
    assert E.shape == (len(trains), 2, len(dims)) and C.shape == (len(trains), len(dims), len(dims))
    for b, t in enumerate(trains):
        assert worst_profile(f"{name} train {b} E_P", E[b, 0], R.dense_site_expect(t, P), pn) <= TOL
        assert worst_profile(f"{name} train {b} E_Q", E[b, 1], R.dense_site_expect(t, Q), qn) <= TOL
        assert worst_corr(f"{name} train {b} C", C[b], R.dense_correlation(t, P, Q), pn, qn) <= TOL
    h.free()


def test_batch_beyond_one_workspace_chunk():
    """More trains than TTN_MEASURE_CHUNK_BYTES of workspace hold: the entry point splits the batch, every train gets the same numbers."""
    dims, trains, P, Q = R.case("rank80_d14")
    d, B = len(dims), 70
    hdr = open(os.path.join(T._lib.INCLUDE, "ttn_measure.h")).read()
    chunk_bytes = int(re.search(r"#define\s+TTN_MEASURE_CHUNK_BYTES\s+(\d+)", hdr).group(1))
    W, N = 80 * 80, 2 * 80 * 80
    per_train = 2 * (d + 1) * W + 2 * N + 3 * d * W + max(3 * d, 2 * (d - 1)) * (2 * N + 2 * W)      # the formula of the header
    assert chunk_bytes // (8 * per_train) < B
    h = upload(trains[:1], batch=B)
    h.replicate(0)
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    C = D.correlation_matrix(h, P, Q)
    E = D.site_expect(h, P)
    refC, refE = R.dense_correlation(trains[0], P, Q), R.dense_site_expect(trains[0], P)
    assert C.shape == (B, d, d) and E.shape == (B, d)
    errC = worst_of(*(float(np.max(np.abs(C[b] - refC) / np.outer(pn, qn))) for b in range(B)))
    errE = worst_of(*(float(np.max(np.abs(E[b] - refE) / pn)) for b in range(B)))
    print(f"{B} trains in chunks: worst err/scale C {errC:.2e} E {errE:.2e}")
    assert errC <= TOL and errE <= TOL
    h.free()


# ---- 3. orientation --------------------------------------------------------------------------------------------------------------------
def test_orientation(class_case):
    dims, trains, P, Q, h, ref = class_case
    one = np.ones(12)
    # P = Q = i sigma_y: minus <sigma_y sigma_y>; a one-sided transposition flips the sign of every off-diagonal entry
    got = D.correlation_matrix(h, IY, IY)
    for b, t in enumerate(trains):
        dense = R.dense_correlation(t, IY, IY)
        assert worst_corr(f"i sigma_y train {b}", got[b], dense, one, one) <= TOL
        off = ~np.eye(12, dtype=bool)
        assert np.max(np.abs(dense[off])) > 1e-3 and np.max(np.abs(got[b][off] + dense[off])) > 1e-3
    assert np.max(np.abs(D.site_expect(h, IY))) <= TOL                 # a real train sees only the symmetric part
    # P antisymmetric, Q symmetric and != P: the lower-triangle pass runs
    Qs = np.array([[0.3, -1.1], [-1.1, 0.8]])
    got = D.correlation_matrix(h, IY, Qs)
    for b, t in enumerate(trains):
        assert worst_corr(f"antisym x sym train {b}", got[b], R.dense_correlation(t, IY, Qs), one, one * np.linalg.norm(Qs, 2)) <= TOL
    # `P is Q` mirrors the upper triangle; tables that differ only in the sign of a zero take both passes
    Pz = IY.copy()
    Qz = np.where(Pz == 0.0, -0.0, Pz)
    assert not np.array_equal(Pz.view(np.uint64), Qz.view(np.uint64)) and np.array_equal(Pz, Qz)
    mirrored, two_pass = D.correlation_matrix(h, Pz), D.correlation_matrix(h, Pz, Qz)
    for b in range(3):
        assert np.array_equal(mirrored[b], mirrored[b].T)
        assert worst_corr(f"mirrored vs two passes train {b}", mirrored[b], two_pass[b], one, one) <= TOL


# ---- 4. identities ---------------------------------------------------------------------------------------------------------------------
def test_identities(class_case):
    dims, trains, P, Q, h, ref = class_case
    one = np.ones(12)
    qn = R.op_norms(Q, dims)
    assert worst_corr("P = Q = I", D.correlation_matrix(h, I2), np.ones((3, 12, 12)), one, one) <= TOL
    C = D.correlation_matrix(h, I2, Q)
    EQ = D.site_expect(h, Q)
    for b in range(3):
        assert worst_corr(f"P = I train {b}", C[b], np.tile(EQ[b], (12, 1)), one, qn) <= TOL
    nn = D.dot(h, h)
    Cn, Cu = D.correlation_matrix(h, P, Q), D.correlation_matrix(h, P, Q, normalize=False)
    En, Eu = D.site_expect(h, P), D.site_expect(h, P, normalize=False)
    pn = R.op_norms(P, dims)
    for b in range(3):
        assert worst_corr(f"normalize=False train {b}", Cu[b] / nn[b], Cn[b], pn, qn) <= TOL
        assert worst_profile(f"normalize=False train {b}", Eu[b] / nn[b], En[b], pn) <= TOL


def test_product_state_and_ghz():
    rng = np.random.default_rng(31)
    dims = (2,) * 9
    prod = R.product_train(dims, rng)
    P, Q = rng.standard_normal((2, 2)), rng.standard_normal((2, 2))
    P, Q = P / np.linalg.norm(P, 2), Q / np.linalg.norm(Q, 2)        # spectral norm 1: the bar is 1e-12 as a number
    h = upload([prod])
    conn = D.correlation_matrix(h, P, Q, connected=True)[0]
    off = conn[~np.eye(9, dtype=bool)]
    print(f"product state: worst connected correlator {np.max(np.abs(off)):.2e}")
    assert np.max(np.abs(off)) <= TOL
    # the diagonal is E_{PQ}[i] - E_P[i] E_Q[i]; recomputed from three more calls, each within TOL of the first ones: 3 TOL
    EP, EQ, EPQ = D.site_expect(h, P)[0], D.site_expect(h, Q)[0], D.site_expect(h, P @ Q)[0]
    assert np.max(np.abs(np.diag(conn) - (EPQ - EP * EQ))) <= 3 * TOL
    h.free()
    g = upload([R.ghz_train(9)])
    assert worst_corr("GHZ <Z_i Z_j>", D.correlation_matrix(g, Z)[0], np.ones((9, 9)), np.ones(9), np.ones(9)) <= TOL
    assert worst_profile("GHZ <Z_k>", D.site_expect(g, Z)[0], np.zeros(9), np.ones(9)) <= TOL
    g.free()


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(2,), (3,), (2, 2), (3, 2)])
def test_edges_d1_d2_single_train(dims):
    rng = np.random.default_rng(len(dims) * 10 + dims[0])
    cores = R.rand_train(dims, R.full_ranks(dims, 8), rng)
    P, Q = [rng.standard_normal((n, n)) for n in dims], [rng.standard_normal((n, n)) for n in dims]
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    h = upload([cores])
    C = D.correlation_matrix(h, P, Q)
    assert C.shape == (1, len(dims), len(dims))
    assert worst_corr(f"dims {dims}", C[0], R.dense_correlation(cores, P, Q), pn, qn) <= TOL
    E = D.site_expect(h, P)
    assert E.shape == (1, len(dims))
    assert worst_profile(f"dims {dims}", E[0], R.dense_site_expect(cores, P), pn) <= TOL
    if len(dims) == 1:                                              # d = 1: the 1 x 1 result is E_{PQ}
        assert abs(C[0, 0, 0] - D.site_expect(h, [P[0] @ Q[0]])[0, 0]) <= TOL * pn[0] * qn[0]
    h.free()


# ---- 6. a long chain, and the tie to the existing API ----------------------------------------------------------------------------------
def test_long_thin_chain_d40():
    rng = np.random.default_rng(40)
    dims = (2,) * 40
    cores = R.rand_train(dims, R.full_ranks(dims, 6), rng)
    P, Q = rng.standard_normal((2, 2)), rng.standard_normal((2, 2))
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    h = upload([cores])
    assert worst_corr("d = 40", D.correlation_matrix(h, P, Q)[0], R.chain_correlation(cores, P, Q), pn, qn) <= TOL
    assert worst_profile("d = 40", D.site_expect(h, Q)[0], R.chain_site_expect(cores, Q), qn) <= TOL
    h.free()


def test_tie_to_sandwich_d30():
    rng = np.random.default_rng(30)
    d = 30
    dims = (2,) * d
    cores = R.rand_train(dims, R.full_ranks(dims, 8), rng)
    P, Q = rng.standard_normal((2, 2)), rng.standard_normal((2, 2))
    scale = np.linalg.norm(P, 2) * np.linalg.norm(Q, 2)
    h = upload([cores])
    C = D.correlation_matrix(h, P, Q)[0]
    nn = D.dot(h, h)[0]
    worst = 0.0
    for i, j in [(0, 29), (3, 4), (14, 15), (7, 22), (28, 29)]:
        for a, b in ((i, j), (j, i)):                               # C[a, b] = <P_a Q_b>: the product operator with P at a and Q at b
            mats = [I2] * d
            mats[a], mats[b] = P, Q
            A = T.TToperator(d, [np.asfortranarray(m.reshape(2, 2, 1, 1)) for m in mats], dims, [1] * (d + 1), [0] * d)
            hA = T.DeviceTTO(A)
            ref = D.sandwich(h, hA, h)[0] / nn
            hA.free()
            worst = worst_of(worst, abs(C[a, b] - ref) / scale)
    print(f"five pairs, both orders, against sandwich / dot: worst err/scale {worst:.2e}")
    assert worst <= TOL
    h.free()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_library_usable():
    hz = T.DeviceTT((2, 2, 2), [1, 2, 2, 1], batch=1, dtype=np.complex128)
    with pytest.raises(T.TTNError, match="Float64 only"):
        D.site_expect(hz, Z)
    with pytest.raises(T.TTNError, match="Float64 only"):
        D.correlation_matrix(hz, Z)
    hz.free()
    rng = np.random.default_rng(8)
    dims = (2, 2, 2)
    cores = R.rand_train(dims, [1, 2, 2, 1], rng)
    h = upload([cores])
    assert D.MEASURE_MAX_OPS == 16
    with pytest.raises(T.TTNError, match="nops"):
        D.site_expect(h, *([Z] * 17))
    got = D.site_expect(h, *([Z] * 16))                              # the limit itself is fine
    assert got.shape == (1, 16, 3)
    assert worst_profile("after the refusals", got[0, 15], R.dense_site_expect(cores, Z), np.ones(3)) <= TOL
    assert worst_corr("after the refusals", D.correlation_matrix(h, Z)[0], R.dense_correlation(cores, Z), np.ones(3), np.ones(3)) <= TOL
    h.free()


# ---- 8. host forms, device forms -------------------------------------------------------------------------------------------------------
def test_host_and_device_forms():
    import torch
    dims, trains, P, Q = R.case("n3_d6")
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    x = to_tt(trains[0])
    h = upload(trains[:1])
    E1, E2 = T.site_expect(x, P), T.site_expect(x, P, Q)
    C1 = T.correlation_matrix(x, P, Q)
    assert E1.shape == (6,) and E2.shape == (2, 6) and C1.shape == (6, 6)
    assert worst_profile("host site_expect", E1, D.site_expect(h, P)[0], pn) <= TOL
    assert worst_profile("host site_expect, two tables", E2[1], D.site_expect(h, Q)[0], qn) <= TOL
    assert worst_corr("host correlation_matrix", C1, D.correlation_matrix(h, P, Q)[0], pn, qn) <= TOL
    Cc = T.correlation_matrix(x, P, Q, connected=True)
    # three device numbers per entry on either side (C, E_P, E_Q), each reproducible to TOL: 3 TOL
    assert worst_corr("host connected", Cc, C1 - np.outer(E2[0], E2[1]), pn, qn) <= 3 * TOL
    Ed = D.site_expect_dev(h, P, Q)
    Cd = D.correlation_matrix_dev(h, P, Q)
    D.sync()
    torch.cuda.synchronize()
    assert worst_profile("site_expect_dev", Ed.cpu().numpy()[0], E2, np.stack([pn, qn])) <= TOL
    assert worst_corr("correlation_matrix_dev", Cd.cpu().numpy()[0], C1, pn, qn) <= TOL
    h.free()
