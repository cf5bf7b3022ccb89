"""CPU-side tests (no GPU) of the operator batches (include/ttn_opbatch.h): every entry point with a ttn_tto_t operand either takes a batch
or refuses it through single_op before anything else can happen (a source check of the host API, csrc/ttn_api.hip with the csrc/ttn_host_*.h
it includes, against the headers), the new header
stands alone for a C compiler and agrees with the ctypes table, and the argument checks of DeviceTTO.lincomb / stack raise before any
device call."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "tensortrainnumerics.jl_amd", "csrc")
HOST_HEADERS = sorted(f for f in os.listdir(CSRC) if f.startswith("ttn_host_") and f.endswith(".h"))
# the source of the host API: ttn_api.hip and every host header, found by listing so that a new one is covered as it appears
API = "".join(open(os.path.join(CSRC, f)).read() for f in ["ttn_api.hip"] + HOST_HEADERS)

# entry points that accept an operator batch: the consumers (they check the batch against the trains) and the handle's own calls
CONSUMERS = {"ttn_apply", "ttn_apply_axpby", "ttn_sandwich", "ttn_sandwich_dev", "ttn_sandwich_pullback", "ttn_dmrg_eigsolve", "ttn_mals_eigsolve"}
HANDLE_CALLS = {"ttn_tto_free", "ttn_tto_ranks", "ttn_tto_dtype", "ttn_tto_batch", "ttn_tto_select", "ttn_tto_download_b"}


@pytest.fixture(scope="module")
def T():
    import __graft_entry__ as g
    g.build()
    import ttn_amd
    return ttn_amd


def _prototypes(header):
    """(name, [(type, parameter name)]) of every function a header declares, comments stripped."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    out = []
    for name, args in re.findall(r"\bint\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr):
        params = []
        for a in [x.strip() for x in args.split(",")]:
            if a == "void":
                continue
            m = re.match(r"(.*?)([A-Za-z_][A-Za-z0-9_]*)$", a)
            params.append((re.sub(r"\s+", "", re.sub(r"\bconst\b", "", m.group(1))), m.group(2)))
        out.append((name, params))
    return out


def _body(src, name):
    """The body of function `name` in the host API (brace matching from its definition)."""
    m = re.search(r"^(?:static )?int %s\(" % re.escape(name), src, flags=re.M)
    assert m, f"{name} is not defined in the host API"
    i = src.index("{", m.end())
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        j += 1
        if depth == 0:
            return src[i:j]


def _operator_entry_points():
    found = []
    for header in sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h")):
        for name, params in _prototypes(header):
            ops = [p for t, p in params if t == "ttn_tto_t"]           # inputs only: ttn_tto_t* is a result
            if ops:
                found.append((name, ops))
    return found


def test_every_operator_entry_point_takes_a_batch_or_refuses_it():
    assert HOST_HEADERS, "no csrc/ttn_host_*.h found"
    src = API
    entries = _operator_entry_points()
    names = {n for n, _ in entries}
    assert len(entries) >= 30 and CONSUMERS <= names and HANDLE_CALLS <= names, sorted(names)
    for name, ops in entries:
        if name in CONSUMERS or name in HANDLE_CALLS:
            continue
        body = _body(src, name)
        for p in ops:
            assert re.search(r"single_op\(\s*%s\s*," % re.escape(p), body), f"{name} does not call single_op on its operand `{p}`"
    # the consumers hold the operator batch against the trains' batch where their checks live
    for fn in ("ttn_apply", "ttn_apply_axpby", "sandwich_launch", "ttn_sandwich_pullback", "two_site_eigsolve"):
        assert "op_batch_fits(A" in _body(src, fn), fn
    helper = _body(src, "single_op")
    assert "operator batch" in helper and "TTN_ERR_UNSUPPORTED" in helper


def test_kernels_add_the_stride_where_they_form_the_operator_pointer():
    """Every kernel on the list reads the operator at data + train * stride; k_compress's fused merge (refused on the host) does not."""
    csrc = CSRC

    def text(f):
        return open(os.path.join(csrc, f)).read()
    assert "A.data + (long long)b * A.stride + A.off[k]" in text("ttn_stream_kernels.h")
    assert "A.data + (long long)b * A.stride + A.off[k]" in text("ttn_step_kernels.h")
    assert "(long long)t * A.stride" in text("ttn_expect_kernels.h")
    assert text("ttn_expect_grad_kernels.h").count("(long long)t * A.stride") + text("ttn_expect_grad_kernels.h").count("(long long)t * P.A.stride") == 3
    for f in ("ttn_als_kernels.h", "ttn_eigsolve_kernels.h"):
        assert "#define AC(i) (E.A.data + (long long)E.tb * E.A.stride + E.A.off[i])" in text(f)
        # no operator read of the two-site kernels goes around AC: the macro is the one place that names the operator's data
        assert len(re.findall(r"\bA\.data\b", text(f))) == 1, f
    assert "op.stride" not in text("ttn_dense_kernels.h")


def test_header_stands_alone_for_a_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = tmp_path / "probe.c"
    src.write_text('#include "ttn_opbatch.h"\nint main(void) { int64_t n = 0; ttn_tto_t A = 0; return ttn_tto_batch(A, &n) == TTN_OK; }\n')
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_ctypes_table_matches_the_header(T):
    protos = dict(_prototypes("ttn_opbatch.h"))
    assert set(protos) == set(T._lib.OPBATCH_SIGNATURES) == {"ttn_tto_create_batch", "ttn_tto_from_tt_batch", "ttn_tto_batch", "ttn_tto_select",
                                                             "ttn_tto_download_b"}
    L = ctypes
    table = {"int64_t": L.c_int64, "int64_t*": L.POINTER(L.c_int64), "double**": L.POINTER(L.POINTER(L.c_double)), "ttn_tt_t": L.c_void_p,
             "ttn_tto_t": L.c_void_p, "ttn_tto_t*": L.POINTER(L.c_void_p)}
    lib = ctypes.CDLL(T._lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(lib, name), name
        res, args = T._lib.OPBATCH_SIGNATURES[name]
        assert res is L.c_int and len(args) == len(params), name
        for (t, p), at in zip(params, args):
            want = table[t.replace("*const*", "**")]
            assert at is want or (hasattr(at, "_type_") and hasattr(want, "_type_") and at._type_ is want._type_), (name, p, t, at)
    assert b"k_tto_pack" in open(T._lib.LIB_PATH, "rb").read()


def _fake_op(T, dims=(2, 2), rks=(1, 2, 1), dtype=np.float64):
    """A DeviceTTO that owns no handle: enough for the checks that run before any device call."""
    A = T.DeviceTTO.__new__(T.DeviceTTO)
    A.h, A.dims, A.rks, A.N, A.dtype, A.batch, A.ot = None, tuple(dims), list(rks), len(dims), dtype, 1, [0] * len(dims)
    return A


def test_lincomb_and_stack_check_their_arguments_before_any_device_call(T, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(T._lib, "ensure_init", no_device)
    monkeypatch.setattr(T._lib, "lib", no_device)
    E = T._lib.TTNError
    A, B = _fake_op(T), _fake_op(T)
    with pytest.raises(E, match="no terms"):
        T.DeviceTTO.lincomb([], np.zeros((2, 0)))
    for bad in (np.zeros(2), np.zeros((3, 1)), np.zeros((0, 2)), np.zeros((2, 2, 2))):
        with pytest.raises(E, match="coeffs of shape"):
            T.DeviceTTO.lincomb([A, B], bad)
    with pytest.raises(TypeError, match="term 1"):
        T.DeviceTTO.lincomb([A, "B"], np.zeros((2, 2)))
    with pytest.raises(E, match="dims of term 1"):
        T.DeviceTTO.lincomb([A, _fake_op(T, dims=(2, 3))], np.zeros((2, 2)))
    with pytest.raises(E, match="complex"):
        T.DeviceTTO.lincomb([A, _fake_op(T, dtype=np.complex128)], np.zeros((2, 2)))
    rng = np.random.default_rng(0)

    def op(rks, dims=(2, 2), cplx=False):
        cores = [np.asfortranarray(rng.standard_normal((dims[k], dims[k], rks[k], rks[k + 1])) * (1j if cplx else 1.0)) for k in range(2)]
        return T.TToperator(2, cores, dims, list(rks), [0, 0])
    with pytest.raises(E, match="at least one"):
        T.DeviceTTO.stack([])
    with pytest.raises(E, match="Float64 only"):
        T.DeviceTTO.stack([op([1, 2, 1]), op([1, 2, 1], cplx=True)])
    with pytest.raises(E, match="ranks of operator 1"):
        T.DeviceTTO.stack([op([1, 2, 1]), op([1, 3, 1])])
    with pytest.raises(E, match="dims of operator 1"):
        T.DeviceTTO.stack([op([1, 2, 1]), op([1, 2, 1], dims=(2, 3))])
