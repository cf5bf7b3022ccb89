"""CPU tests of the site-resolved measurements (no GPU): the two NumPy restatements of tests/measure_reference.py — the yardsticks of
tests/test_gpu_measure.py — agree with each other and with analytic states, include/ttn_measure.h stands alone for a C compiler and
agrees with the ctypes table, and the argument checks of the Python layer raise before any device call.

Bar between the restatements: 1e-13 ||P_i||_2 ||Q_j||_2 on normalised values — the condition that the inputs are well posed (the worst
case on these shapes is 5.4e-16, and the float64 chain stays as close to a longdouble dense run)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import measure_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = {"ttn_site_expect", "ttn_site_expect_dev", "ttn_correlation", "ttn_correlation_dev"}
IY = np.array([[0.0, 1.0], [-1.0, 0.0]])       # i sigma_y
Z = np.diag([1.0, -1.0])


@pytest.fixture(scope="module")
def T():
    import __graft_entry__ as g
    g.build()
    import ttn_amd
    return ttn_amd


def _agree(cores, P, Q):
    dims = [c.shape[0] for c in cores]
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    worst = 0.0
    for op, nrm in ((P, pn), (Q, qn)):
        err = np.abs(R.dense_site_expect(cores, op) - R.chain_site_expect(cores, op)) / nrm
        worst = max(worst, float(err.max()))
    err = np.abs(R.dense_correlation(cores, P, Q) - R.chain_correlation(cores, P, Q)) / np.outer(pn, qn)
    return max(worst, float(err.max()))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatements_agree(name):
    dims, trains, P, Q = R.case(name)
    for b, cores in enumerate(trains):
        worst = _agree(cores, P, Q)
        print(f"{name} train {b}: ranks {[c.shape[1] for c in cores] + [1]} worst err/scale {worst:.2e}")
        assert worst <= 1e-13


def test_restatements_agree_on_edges_and_unnormalised():
    rng = np.random.default_rng(5)
    for dims in ((2,), (3,), (2, 2), (2, 3)):
        cores = R.rand_train(dims, R.full_ranks(dims, 4), rng)
        P, Q = [rng.standard_normal((n, n)) for n in dims], [rng.standard_normal((n, n)) for n in dims]
        assert _agree(cores, P, Q) <= 1e-13
        nn = R.chain_norm2(cores)
        assert np.allclose(R.chain_correlation(cores, P, Q, normalize=False), nn * R.chain_correlation(cores, P, Q), rtol=1e-13, atol=0)
        assert np.allclose(R.dense_site_expect(cores, P, normalize=False), nn * R.dense_site_expect(cores, P), rtol=1e-13, atol=0)
    # d = 1: the 1 x 1 correlation is E_{PQ}
    cores = R.rand_train((3,), [1, 1], rng)
    P, Q = rng.standard_normal((3, 3)), rng.standard_normal((3, 3))
    assert abs(R.chain_correlation(cores, P, Q)[0, 0] - R.dense_site_expect(cores, P @ Q)[0]) <= 1e-13 * np.linalg.norm(P, 2) * np.linalg.norm(Q, 2)


def test_chain_against_longdouble_dense():
    dims, trains, P, Q = R.case("n3_d6")
    ref = R.dense_correlation(trains[0], P, Q, dtype=np.longdouble)
    got = R.chain_correlation(trains[0], P, Q)
    scale = np.outer(R.op_norms(P, dims), R.op_norms(Q, dims))
    assert float(np.max(np.abs(got - ref) / scale)) <= 1e-13


def test_orientation_of_the_restatements():
    """The first index of a matrix meets the bra: a lowering matrix moves weight one way only, and i sigma_y in both slots is -<YY>."""
    up_down = [np.array([1.0, 0.0]).reshape(2, 1, 1), np.array([0.0, 1.0]).reshape(2, 1, 1)]
    bell = R.ghz_train(2)
    for f in (R.dense_correlation, R.chain_correlation):
        assert np.allclose(f(bell, IY)[0, 1], 1.0) and np.allclose(f(bell, IY)[1, 0], 1.0)       # <YY> = -1 on (|00> + |11>) / sqrt 2
        assert np.allclose(np.diag(f(bell, IY)), -1.0)                                            # (i sigma_y)^2 = -1
    # <x| P_0 Q_1 |x> with P = |0><1| (bra 0, ket 1) and Q = |1><0| on x = (|01> + |10>) / sqrt 2: picks bra |01>, ket |10>
    x = [np.zeros((2, 1, 2)), np.zeros((2, 2, 1))]
    x[0][0, 0, 0] = x[0][1, 0, 1] = 1.0
    x[1][1, 0, 0] = x[1][0, 1, 0] = 1.0
    P, Q = np.array([[0.0, 1.0], [0.0, 0.0]]), np.array([[0.0, 0.0], [1.0, 0.0]])
    for f in (R.dense_correlation, R.chain_correlation):
        C = f(x, P, Q)
        assert np.allclose(C[0, 1], 0.5) and np.allclose(C[1, 0], 0.5)      # <P_1 Q_0>: bra |10>, ket |01>
        assert np.allclose(f(x, P.T, Q)[0, 1], 0.0)                          # a one-sided transposition is another number: bra |11>
    assert np.allclose(R.dense_site_expect(up_down, Z), [1.0, -1.0])


def test_analytic_states():
    rng = np.random.default_rng(9)
    dims = (2, 3, 2, 4)
    prod = R.product_train(dims, rng)
    P, Q = [rng.standard_normal((n, n)) for n in dims], [rng.standard_normal((n, n)) for n in dims]
    for corr, prof in ((R.dense_correlation, R.dense_site_expect), (R.chain_correlation, R.chain_site_expect)):
        C = corr(prod, P, Q)
        conn = C - np.outer(prof(prod, P), prof(prod, Q))
        off = conn - np.diag(np.diag(conn))
        assert np.max(np.abs(off) / np.outer(R.op_norms(P, dims), R.op_norms(Q, dims))) <= 1e-13       # a product state has no connected correlations
        ghz = R.ghz_train(7)
        assert np.allclose(corr(ghz, Z), 1.0, rtol=0, atol=1e-14)
        assert np.allclose(prof(ghz, Z), 0.0, rtol=0, atol=1e-14)


def test_header_stands_alone_for_a_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "probe.c"
    src.write_text('#include "ttn_measure.h"\nint main(void) { ttn_tt_t x = 0; double o[4] = {0}, out[1]; '
                   'return ttn_site_expect(x, 1, o, 1, out) == TTN_OK && TTN_MEASURE_MAX_OPS == 16; }\n')
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_measure_header_and_ctypes_table_agree(T):
    hdr_raw = open(os.path.join(INCLUDE, "ttn_measure.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_raw, flags=re.S)
    protos = re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert {n for n, _ in protos} == set(T._lib.MEASURE_SIGNATURES) == NAMES
    others = set(T._lib.SIGNATURES) | set(T._lib.RECT_SIGNATURES) | set(T._lib.DENSE_SIGNATURES) | set(T._lib.STEP_SIGNATURES)\
        | set(T._lib.CROSS_BATCH_SIGNATURES) | set(T._lib.EXPECT_SIGNATURES) | set(T._lib.EXPECT_GRAD_SIGNATURES) | set(T._lib.OPBATCH_SIGNATURES)
    assert not NAMES & others
    table = {"ttn_tt_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "double*": ctypes.POINTER(ctypes.c_double)}
    lib = T._lib.lib()
    for name, args in protos:
        res, argt = T._lib.MEASURE_SIGNATURES[name]
        assert res is ctypes.c_int and hasattr(lib, name)
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argt) == 5
        for a, at in zip(params, argt):
            typ = re.sub(r"\s+", "", re.sub(r"\bconst\b", "", re.match(r"(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a).group(1)))
            want = table[typ]
            pname = re.match(r"(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a).group(2)
            if pname == "d_out":
                assert at is ctypes.c_void_p, (name, a)           # device memory travels as an address
            else:
                assert at is want or (hasattr(at, "_type_") and hasattr(want, "_type_") and at._type_ is want._type_), (name, a, at)
    assert '#include "ttn_measure.h"' in open(os.path.join(INCLUDE, "ttn.h")).read()
    defs = dict(re.findall(r"#define\s+(TTN_MEASURE_[A-Z_]+)\s+(\d+)", hdr))
    assert int(defs["TTN_MEASURE_MAX_OPS"]) == T.device.MEASURE_MAX_OPS == 16
    binary = open(T._lib.LIB_PATH, "rb").read()
    assert b"k_measure_open" in binary and b"k_measure_walk" in binary


def test_exports(T):
    for name in ("site_expect", "correlation_matrix"):
        assert name in T.__all__ and callable(getattr(T, name))
    for name in ("site_expect", "site_expect_dev", "correlation_matrix", "correlation_matrix_dev"):
        assert callable(getattr(T.device, name))


def _fake_train(T, dims=(2, 2, 2), dtype=np.float64):
    """A DeviceTT that owns no handle: enough for the checks that run before any device call."""
    x = T.DeviceTT.__new__(T.DeviceTT)
    x.h, x.dims, x.cap, x.N, x.batch, x.dtype = None, tuple(dims), [1, 2, 2, 1], len(dims), 1, dtype
    return x


def test_argument_checks_raise_before_any_device_call(T, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(T._lib, "ensure_init", no_device)
    monkeypatch.setattr(T._lib, "lib", no_device)
    E = T.TTNError
    D = T.device
    x = _fake_train(T)
    y = _fake_train(T, dims=(2, 3, 2))
    with pytest.raises(E, match="no operator"):
        D.site_expect(x)
    with pytest.raises(E, match=r"operator 0 at site 0 has shape \(3, 3\)"):
        D.site_expect(x, np.eye(3))
    with pytest.raises(E, match=r"operator 1 at site 1 has shape \(2, 2\), expected \(3, 3\)"):
        D.site_expect(y, [np.eye(2), np.eye(3), np.eye(2)], np.eye(2))
    with pytest.raises(E, match="holds 2 matrices for 3 sites"):
        D.site_expect(x, [np.eye(2), np.eye(2)])
    with pytest.raises(E, match="P at site 0 is complex"):
        D.correlation_matrix(x, 1j * np.eye(2))
    with pytest.raises(E, match="Q at site 2 is complex"):
        D.correlation_matrix(x, np.eye(2), [np.eye(2), np.eye(2), np.eye(2) * (1 + 0j)])
    with pytest.raises(E, match="Q at site 1 has shape"):
        D.correlation_matrix(y, [np.eye(2), np.eye(3), np.eye(2)], np.eye(2))
    with pytest.raises(E, match="must be an"):
        D.site_expect(x, np.zeros(4))
    with pytest.raises(E, match="dtype"):
        D.site_expect(x, np.array([["a", "b"], ["c", "d"]]))
    with pytest.raises(TypeError, match="expected a DeviceTT"):
        D.site_expect("x", np.eye(2))
    with pytest.raises(TypeError, match="expected a DeviceTT"):
        D.correlation_matrix(None, np.eye(2))
    # the host forms check their tables before the upload
    xh = T.TTvector(2, [np.ones((2, 1, 1), order="F"), np.ones((2, 1, 1), order="F")], (2, 2), [1, 1, 1], [0, 0])
    with pytest.raises(E, match="operator 0 at site 0"):
        T.site_expect(xh, np.eye(3))
    with pytest.raises(E, match="Q at site 0 is complex"):
        T.correlation_matrix(xh, np.eye(2), 1j * np.eye(2))


def test_loud_failure_without_gpu(T):
    import torch
    x = T.rand_tt((2,) * 4, 3, seed=1)
    if torch.cuda.is_available():               # with a device the same calls answer
        cores = [np.array(c) for c in x.ttv_vec]
        assert np.max(np.abs(T.site_expect(x, Z) - R.chain_site_expect(cores, Z))) <= 1e-12
        assert np.max(np.abs(T.correlation_matrix(x, Z) - R.chain_correlation(cores, Z))) <= 1e-12
        return
    for call in (lambda: T.site_expect(x, Z), lambda: T.correlation_matrix(x, Z)):
        with pytest.raises(T.TTNError):
            call()
