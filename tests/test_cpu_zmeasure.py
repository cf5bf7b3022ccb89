"""CPU tests of the site-resolved measurements on ComplexF64 trains (no GPU): the two NumPy restatements of
tests/zmeasure_reference.py — the yardsticks of tests/test_gpu_zmeasure.py — agree with each other and with analytic states,
include/ttn_zmeasure.h stands alone for a C compiler and agrees with the ctypes table, and the argument checks of the Python layer raise
before any device call.

Bar between the restatements: 1e-14 ||P_i||_2 ||Q_j||_2 on normalised values.  The chain form in another sum order differs from the dense
one by 3.5e-16 (E) and 5.8e-16 (C) on class_d12 with caps 64 / 13 / 7: that is what the margin of the GPU bar (1e-12) rests on."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import zmeasure_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = {"ttn_zsite_expect", "ttn_zsite_expect_dev", "ttn_zcorrelation", "ttn_zcorrelation_dev"}


@pytest.fixture(scope="module")
def T():
    import __graft_entry__ as g
    g.build()
    import ttn_amd
    return ttn_amd


@pytest.mark.parametrize("name", ["class_d12", "mixed_dims", "n3_d6"])
def test_chain_against_dense(name):
    dims, trains, P, Q = R.case(name)
    pn, qn = R.op_norms(P, dims), R.op_norms(Q, dims)
    for b, cores in enumerate(trains):
        eE = 0.0
        for op, nrm in ((P, pn), (Q, qn)):
            eE = max(eE, float(np.max(np.abs(R.dense_site_expect(cores, op) - R.chain_site_expect(cores, op)) / nrm)))
        eC = float(np.max(np.abs(R.dense_correlation(cores, P, Q) - R.chain_correlation(cores, P, Q)) / np.outer(pn, qn)))
        print(f"{name} train {b}: ranks {[c.shape[1] for c in cores] + [1]} worst err/scale E {eE:.2e} C {eC:.2e}")
        assert eE <= 1e-14 and eC <= 1e-14
    # the cases are complex and the tables neither Hermitian nor equal
    assert np.max(np.abs(np.imag(trains[0][0]))) > 0.1
    Pm, Qm = R.per_site(P, dims), R.per_site(Q, dims)
    assert np.max(np.abs(Pm[0] - Pm[0].conj().T)) > 0.1 and np.max(np.abs(Pm[0] - Qm[0])) > 0.1


def test_restatements_on_edges_and_unnormalised():
    rng = np.random.default_rng(5)
    for dims in ((2,), (3,), (2, 2), (3, 2)):
        cores = R.crand_train(dims, R.full_ranks(dims, 4), rng)
        P, Q = [R.crand_matrix(n, rng) for n in dims], [R.crand_matrix(n, rng) for n in dims]
        scale = np.outer(R.op_norms(P, dims), R.op_norms(Q, dims))
        assert np.max(np.abs(R.dense_correlation(cores, P, Q) - R.chain_correlation(cores, P, Q)) / scale) <= 1e-14
        nn = R.chain_norm2(cores)
        assert np.allclose(R.chain_correlation(cores, P, Q, normalize=False), nn * R.chain_correlation(cores, P, Q), rtol=1e-13, atol=0)
        assert np.allclose(R.dense_site_expect(cores, P, normalize=False), nn * R.dense_site_expect(cores, P), rtol=1e-13, atol=0)


def test_analytic_states_and_orientation():
    """Conjugation and orientation of both restatements: |+y> has <sigma_y> = +1 (a conjugate on the wrong side gives -1), the precessing
    product state and the complex GHZ state have the values of the issue, and sigma+ at the earlier site is not sigma+ at the later."""
    for prof, corr in ((R.dense_site_expect, R.dense_correlation), (R.chain_site_expect, R.chain_correlation)):
        py = R.plus_y_train(6)
        assert np.allclose(prof(py, R.SY), 1.0, atol=1e-14) and np.allclose(prof(py, R.SX), 0.0, atol=1e-14) and np.allclose(prof(py, R.SZ), 0.0, atol=1e-14)
        th = 0.1 + 0.37 * np.arange(5)
        pr = R.precessing_train(th)
        assert np.allclose(prof(pr, R.SZ), np.cos(2 * th), atol=1e-14) and np.allclose(prof(pr, R.SY), -np.sin(2 * th), atol=1e-14)
        C = corr(pr, R.SZ, R.SY)
        off = ~np.eye(5, dtype=bool)
        assert np.allclose(C[off], (-np.outer(np.cos(2 * th), np.sin(2 * th)))[off], atol=1e-14)
        g = R.complex_ghz_train(8, 0.7)
        assert np.allclose(prof(g, R.SZ), 0.0, atol=1e-14) and np.allclose(corr(g, R.SZ), 1.0, atol=1e-14)
        assert np.allclose(corr(g, R.SPLUS, R.SMINUS)[~np.eye(8, dtype=bool)], 0.0, atol=1e-14)
        # x = (|01> + i |10>) / sqrt 2: <x| (|0><1|)_0 (|1><0|)_1 |x> picks bra |01> (amplitude 1, conjugated) and ket |10> (amplitude i)
        x = [np.zeros((2, 1, 2), dtype=complex), np.zeros((2, 2, 1), dtype=complex)]
        x[0][0, 0, 0] = x[0][1, 0, 1] = 1.0
        x[1][1, 0, 0] = 1.0
        x[1][0, 1, 0] = 1.0j
        C = corr(x, R.SPLUS, R.SMINUS)
        assert np.allclose(C[0, 1], 0.5j) and np.allclose(C[1, 0], -0.5j)


def test_header_stands_alone_for_a_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "probe.c"
    src.write_text('#include "ttn_zmeasure.h"\nint main(void) { ttn_tt_t x = 0; double o[8] = {0}, out[2]; '
                   'return ttn_zsite_expect(x, 1, o, 1, out) == TTN_OK && TTN_ZMEASURE_MAX_OPS == 16; }\n')
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_zmeasure_header_and_ctypes_table_agree(T):
    hdr_raw = open(os.path.join(INCLUDE, "ttn_zmeasure.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_raw, flags=re.S)
    protos = re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert {n for n, _ in protos} == set(T._lib.ZMEASURE_SIGNATURES) == NAMES
    others = set()
    for name in dir(T._lib):
        if name.endswith("SIGNATURES") and name != "ZMEASURE_SIGNATURES":
            others |= set(getattr(T._lib, name))
    assert "ttn_site_expect" in others and not NAMES & others
    table = {"ttn_tt_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "double*": ctypes.POINTER(ctypes.c_double)}
    lib = T._lib.lib()
    for name, args in protos:
        res, argt = T._lib.ZMEASURE_SIGNATURES[name]
        assert res is ctypes.c_int and hasattr(lib, name)
        params = [a.strip() for a in args.split(",")]
        assert len(params) == len(argt) == 5
        for a, at in zip(params, argt):
            m = re.match(r"(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a)
            want = table[re.sub(r"\s+", "", re.sub(r"\bconst\b", "", m.group(1)))]
            if m.group(2) == "d_out":
                assert at is ctypes.c_void_p, (name, a)           # device memory travels as an address
            else:
                assert at is want or (hasattr(at, "_type_") and hasattr(want, "_type_") and at._type_ is want._type_), (name, a, at)
    assert '#include "ttn_zmeasure.h"' in open(os.path.join(INCLUDE, "ttn.h")).read()
    defs = dict(re.findall(r"#define\s+(TTN_ZMEASURE_[A-Z_]+)\s+(\d+)", hdr))
    assert int(defs["TTN_ZMEASURE_MAX_OPS"]) == T.device.ZMEASURE_MAX_OPS == 16
    assert "bitwise" in hdr_raw and "LDS atomics" in hdr_raw                     # the header states what reproducible means here
    binary = open(T._lib.LIB_PATH, "rb").read()
    for k in (b"k_zmeasure_chain", b"k_zmeasure_open", b"k_zmeasure_walk"):
        assert k in binary
    assert "ttn_zsite_expect" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_exports(T):
    for name in ("zsite_expect", "zcorrelation_matrix"):
        assert name in T.__all__ and callable(getattr(T, name))
    for name in ("zsite_expect", "zsite_expect_dev", "zcorrelation_matrix", "zcorrelation_matrix_dev", "_zmeasure_table"):
        assert callable(getattr(T.device, name))


def _fake_train(T, dims=(2, 2, 2), dtype=np.complex128):
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
    xr = _fake_train(T, dtype=np.float64)
    with pytest.raises(E, match="no operator"):
        D.zsite_expect(x)
    with pytest.raises(E, match=r"operator 0 at site 0 has shape \(3, 3\)"):
        D.zsite_expect(x, np.eye(3))
    with pytest.raises(E, match=r"operator 1 at site 1 has shape \(2, 2\), expected \(3, 3\)"):
        D.zsite_expect(y, [np.eye(2), 1j * np.eye(3), np.eye(2)], np.eye(2))
    with pytest.raises(E, match="holds 2 matrices for 3 sites"):
        D.zsite_expect(x, [np.eye(2), np.eye(2)])
    with pytest.raises(E, match="Q at site 1 has shape"):
        D.zcorrelation_matrix(y, [np.eye(2), np.eye(3), np.eye(2)], R.SY)
    with pytest.raises(E, match="must be an"):
        D.zsite_expect(x, np.zeros(4))
    with pytest.raises(E, match="dtype"):
        D.zsite_expect(x, np.array([["a", "b"], ["c", "d"]]))
    with pytest.raises(E, match="must be an"):
        D.zcorrelation_matrix(x, np.array([[None, 1], [2, 3]], dtype=object))
    with pytest.raises(E, match="at most 16"):
        D.zsite_expect(x, *([R.SZ] * 17))
    for call in (lambda: D.zsite_expect(xr, R.SY), lambda: D.zsite_expect_dev(xr, R.SY), lambda: D.zcorrelation_matrix(xr, R.SY),
                 lambda: D.zcorrelation_matrix_dev(xr, R.SY)):
        with pytest.raises(E, match="site_expect"):                      # a Float64 handle: the message names the call that takes it
            call()
    with pytest.raises(TypeError, match="expected a DeviceTT"):
        D.zsite_expect("x", np.eye(2))
    with pytest.raises(TypeError, match="expected a DeviceTT"):
        D.zcorrelation_matrix(None, np.eye(2))
    # the tables are promoted, real or complex, column-major per site
    t = D._zmeasure_table("w", "P", [R.SY, np.array([[1, 2], [3, 4]])], (2, 2))
    assert t.dtype == np.complex128 and np.array_equal(t, np.array([0, 1j, -1j, 0, 1, 3, 2, 4], dtype=np.complex128))
    # the host forms check their tables before the upload
    xh = T.TTvector(2, [np.ones((2, 1, 1), order="F"), np.ones((2, 1, 1), order="F")], (2, 2), [1, 1, 1], [0, 0])
    with pytest.raises(E, match="operator 0 at site 0"):
        T.zsite_expect(xh, np.eye(3))
    with pytest.raises(E, match="Q at site 0 has shape"):
        T.zcorrelation_matrix(xh, np.eye(2), 1j * np.eye(3))
    with pytest.raises(TypeError, match="expected a TTvector"):
        T.zsite_expect([1, 2], np.eye(2))


def test_loud_failure_without_gpu(T):
    import torch
    x = T.rand_tt((2,) * 4, 3, seed=1)
    if torch.cuda.is_available():               # with a device the same calls answer: a real train gets its sigma_y numbers
        cores = [np.array(c) for c in x.ttv_vec]
        assert np.max(np.abs(T.zsite_expect(x, R.SY) - R.chain_site_expect(cores, R.SY))) <= 1e-12
        assert np.max(np.abs(T.zcorrelation_matrix(x, R.SY, R.SZ) - R.chain_correlation(cores, R.SY, R.SZ))) <= 1e-12
        return
    for call in (lambda: T.zsite_expect(x, R.SY), lambda: T.zcorrelation_matrix(x, R.SY)):
        with pytest.raises(T.TTNError):
            call()
