"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol of include/ttn.h,
the product-side input generators agree bit-for-bit with the oracle's restatement of the reference
constructors, the golden fixtures are consistent with the oracle, and host-side argument checks raise
the reference's exception types before anything touches a device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from oracle import tt_oracle as O
from tests.helpers import load_golden, tt_from_golden, tto_from_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import __graft_entry__ as g
    g.build()
    import ttn_amd
    return ttn_amd


def _header_prototypes():
    """(return type, name, [argument types]) of every function include/ttn.h declares, comments stripped."""
    hdr = open(os.path.join(ROOT, "include", "ttn.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = []
    for ret, name, args in re.findall(r"\b(int|const char\*)\s+(ttn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr):
        types = []
        for a in [x.strip() for x in args.split(",")]:
            if a == "void":
                continue
            t = re.sub(r"\bconst\b", "", a)
            t = re.sub(r"\s*[A-Za-z_][A-Za-z0-9_]*$", "", t.strip())        # drop the parameter name
            types.append(re.sub(r"\s+", "", t))
        out.append((ret, name, types))
    return out


def _ctypes_of(ctype: str):
    """ctypes types a C parameter type of ttn.h may be bound as (device pointers travel as c_void_p)."""
    L = ctypes
    table = {
        "int": [L.c_int], "int64_t": [L.c_int64], "double": [L.c_double], "uint64_t": [L.c_uint64], "uint64_t*": [L.POINTER(L.c_uint64)],
        "int*": [L.POINTER(L.c_int), L.c_void_p], "int64_t*": [L.POINTER(L.c_int64), L.c_void_p],
        "double*": [L.POINTER(L.c_double), L.c_void_p], "float*": [L.POINTER(L.c_float)],
        "double**": [L.POINTER(L.POINTER(L.c_double))], "void**": [L.POINTER(L.c_void_p)],
        "ttn_tt_t": [L.c_void_p], "ttn_tto_t": [L.c_void_p], "ttn_tt_t*": [L.POINTER(L.c_void_p)], "ttn_tto_t*": [L.POINTER(L.c_void_p)],
    }
    return table[ctype]


def test_library_exports_every_declared_symbol(T):
    protos = _header_prototypes()
    declared = {name for _, name, _ in protos}
    assert len(declared) >= 35
    lib = ctypes.CDLL(T._lib.LIB_PATH)
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, f"libttn_hip.so does not export: {missing}"
    assert declared == set(T._lib.SIGNATURES), "ctypes signature table out of sync with ttn.h"
    assert b"gfx950" in T._lib.lib().ttn_version()


def test_ctypes_signatures_match_header_argument_types(T):
    """Not only the names: return type, arity and every argument type of the ctypes table against the prototypes of ttn.h."""
    for ret, name, types in _header_prototypes():
        res, args = T._lib.SIGNATURES[name]
        assert res is (ctypes.c_char_p if ret == "const char*" else ctypes.c_int), name
        assert len(args) == len(types), f"{name}: header has {len(types)} arguments, ctypes table {len(args)}"
        for i, (ct, at) in enumerate(zip(types, args)):
            ok = any(at is c or (hasattr(at, "_type_") and hasattr(c, "_type_") and at._type_ is c._type_) for c in _ctypes_of(ct))
            assert ok, f"{name}: argument {i} is `{ct}` in ttn.h but {at} in _lib.SIGNATURES"
    hdr = open(os.path.join(ROOT, "include", "ttn.h")).read()
    for code, val in re.findall(r"#define\s+(TTN_(?:OK|ERR_[A-Z_]+))\s+(-?\d+)", hdr):
        assert getattr(T._lib, code) == int(val), f"{code} differs between ttn.h and _lib.py"


def test_header_is_usable_from_plain_c(T, tmp_path):
    """include/ttn.h compiled as C99 and linked against the .so the way a `ccall` binds it: the program calls two entry
    points that need no GPU (tests/c_abi_probe.c)."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe = str(tmp_path / "c_abi_probe")
    libdir = os.path.dirname(T._lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi_probe.c"), "-o", exe, "-L", libdir, "-l:libttn_hip.so",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in out and "rks = 1 2 1" in out and "rks = 1 4 1" in out and "not-init rc = -7" in out, out


def test_library_contains_gfx950_code_object(T):
    blob = open(T._lib.LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    for k in (b"k_apply", b"k_compress", b"k_dot", b"k_hadamard", b"k_orthogonalize"):
        assert k in blob


def test_r_and_d_to_rks_matches_oracle_and_reference_vectors(T):
    assert T.r_and_d_to_rks([5, 5, 5], (0, 2), rmax=4) == [1, 2, 1]          # test/test_tt_tools.jl:945
    assert T.r_and_d_to_rks([5, 5, 5], (0, 0), rmax=4) == [1, 4, 1]          # :946
    rng = np.random.default_rng(0)
    for _ in range(200):
        d = int(rng.integers(1, 9))
        dims = [int(v) for v in rng.integers(0, 5, size=d)]
        rks = [int(v) for v in rng.integers(1, 40, size=d + 1)]
        rmax = int(rng.integers(1, 50))
        assert T.r_and_d_to_rks(rks, dims, rmax=rmax) == O.r_and_d_to_rks(rks, dims, rmax=rmax)
    # Julia's Int64 products wrap: 64 sites of dimension 2 give prod = 2^64 = 0
    dims = [2] * 64
    out = T.r_and_d_to_rks([7] * 65, dims, rmax=1024)
    assert out[0] == 1 and out[1] == 2 and out[-1] == 1


def _same_tt(a, b):
    assert list(a.ttv_rks) == list(b.ttv_rks) and tuple(a.ttv_dims) == tuple(b.ttv_dims)
    for ca, cb in zip(a.ttv_vec, b.ttv_vec):
        assert np.array_equal(np.asarray(ca), np.asarray(cb))


def test_constructors_bit_exact_vs_oracle(T):
    for d in (2, 3, 6, 12, 30):
        A, B = T.Delta(d), O.Delta(d)
        assert A.tto_rks == B.tto_rks
        for ca, cb in zip(A.tto_vec, B.tto_vec):
            assert np.array_equal(ca, cb)
        for ca, cb in zip(T.toeplitz_to_qtto(0.5, 3.0, -7.0, d).tto_vec, O.toeplitz_to_qtto(0.5, 3.0, -7.0, d).tto_vec):
            assert np.array_equal(ca, cb)
        for ca, cb in zip(T.id_tto(d).tto_vec, O.id_tto(d).tto_vec):
            assert np.array_equal(ca, cb)
        if d >= 3:
            _same_tt(T.qtt_sin(d, lam=math.pi), O.qtt_sin(d, lam=math.pi))
            _same_tt(T.qtt_cos(d, a=0.1, b=2.0, lam=0.3), O.qtt_cos(d, a=0.1, b=2.0, lam=0.3))
            _same_tt(T.qtt_exp(d, alpha=-1.5, beta=0.2), O.qtt_exp(d, alpha=-1.5, beta=0.2))
    v = T.qtt_sin(8, lam=math.pi)
    assert np.allclose(T.qtt_to_vector(v), O.qtt_to_vector(O.qtt_sin(8, lam=math.pi)), rtol=0, atol=1e-15)


def test_rand_tt_profile_and_determinism(T):
    x = T.rand_tt((2,) * 30, 64, seed=30)
    assert x.ttv_rks == [1, 2, 4, 8, 16, 32] + [64] * 19 + [32, 16, 8, 4, 2, 1]
    y = T.rand_tt((2,) * 30, 64, seed=30)
    assert all(np.array_equal(a, b) for a, b in zip(x.ttv_vec, y.ttv_vec))
    z = T.portable_randn(200000, 7)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01
    assert all(c.flags["F_CONTIGUOUS"] for c in x.ttv_vec)


def test_golden_fixtures_consistent_with_oracle():
    g = load_golden("closed_forms.npz")
    for d in (4, 6):
        n = 2 ** d
        assert np.array_equal(g[f"delta{d}_dense"], 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1))
        for k, c in enumerate(O.Delta(d).tto_vec):
            assert np.array_equal(g[f"delta{d}_core{k}"], c)
    x = np.linspace(0, 1, 64)
    assert np.allclose(g["sin6_dense"], np.sin(math.pi ** 2 * x), atol=1e-12)
    assert np.allclose(g["c1_dense"], np.sin(math.pi ** 2 * x), atol=1e-12)
    assert list(g["c1_compressed_rks"]) == [1, 2, 2, 2, 2, 2, 1]
    r = load_golden("random_small.npz")
    for name in "abce":
        xs, ys, A = tt_from_golden(r, f"{name}_x"), tt_from_golden(r, f"{name}_y"), tto_from_golden(r, f"{name}_A")
        assert math.isclose(float(r[f"{name}_dot"]), O.dot(xs, ys), rel_tol=1e-13)
        ax = O.apply(A, xs)
        assert list(r[f"{name}_apply_rks"]) == ax.ttv_rks
        z = O.copy_tt(ax)
        O.tt_compress_(z, int(r[f"{name}_max_bond"]), truncerr=float(r[f"{name}_truncerr"]))
        assert list(r[f"{name}_compress_rks"]) == z.ttv_rks
        assert np.allclose(r[f"{name}_compress_dense"], O.ttv_to_tensor(z), atol=1e-12)


def test_host_side_assertions_need_no_device(T):
    x = T.rand_tt((2, 2, 2), [1, 2, 2, 1], seed=1)
    with pytest.raises(AssertionError, match="sweeps must be >= 1"):
        T.tt_compress_(x, 2, sweeps=0)                      # test/test_tt_tools.jl:548
    with pytest.raises(AssertionError, match=r"k must be in 1:\(N-1\)"):
        T._tt_bond_truncate_(x, 0)                          # :495
    with pytest.raises(AssertionError):
        T._tt_bond_truncate_(x, x.N)                        # :496
    with pytest.raises(AssertionError, match="Impossible orthogonalization"):
        T.orthogonalize(x, i=4)
    y = T.rand_tt((2, 3, 2), [1, 2, 2, 1], seed=2)
    with pytest.raises(AssertionError, match="Incompatible dimensions"):
        T.add(x, y)
    with pytest.raises(AssertionError):
        T.dot(x, y)
    with pytest.raises(AssertionError):
        T.hadamard(x, y)
    with pytest.raises(AssertionError):
        T.apply(T.Delta(4), x)


def test_c_abi_argument_errors_without_gpu(T):
    L = T._lib.lib()
    assert L.ttn_sync() == T._lib.TTN_ERR_NOT_INIT or L.ttn_sync() == 0
    out = (ctypes.c_int64 * 3)()
    assert L.ttn_r_and_d_to_rks(2, None, 3, None, 4, out) == T._lib.TTN_ERR_ARG
    assert b"bad argument" in L.ttn_last_error_string()
    # the Float64 / ComplexF64 twins of a stateless call refuse alike, before anything needs a device or reads a pointer
    d = 3

    def refusal(fn, *args):
        return fn(d, None, None, None, *args), L.ttn_last_error_string()

    got = refusal(L.ttn_compress_f64, 4, 0.0, 0)                        # sweeps = 0
    assert got == (T._lib.TTN_ERR_SWEEPS, b"sweeps must be >= 1")
    assert refusal(L.ttn_compress_c64, 4, 0.0, 0) == got
    for k in (0, d):
        got = refusal(L.ttn_bond_truncate_f64, k, 4, 0.0)
        assert got == (T._lib.TTN_ERR_BOND_INDEX, b"k must be in 1:(N-1)")
        assert refusal(L.ttn_bond_truncate_c64, k, 4, 0.0) == got


def test_tdvp_drivers_and_dense_kernels_fail_loudly_without_gpu(T):
    """No CPU fallback behind the TDVP drivers or the stateless fused op: without a device they raise (this suite runs where
    torch.cuda.is_available() is False); on a GPU box the test has nothing to say."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    x = T.rand_tt((2,) * 4, 2, seed=1)
    with pytest.raises(T._lib.TTNError):
        T.tdvp.tdvp(T.Delta(4), x, [0.1])
    with pytest.raises(T._lib.TTNError):
        T.apply_compress(T.Delta(4), x, 2)
    L = T._lib.lib()
    assert L.ttn_dense_qr(0, 4, 4, None, None, None) != 0 and L.ttn_dense_svd(1, 4, 4, None, None, None, None) != 0


# ---- site-swap chains: integer work of reorder is bit-exact with the oracle ----------------------------------
def test_reorder_swap_lists_match_oracle():
    import ttn_amd as T
    from oracle import tt_oracle as O
    for n_dims in range(1, 5):
        for bits in range(1, 7):
            for name, flag in (("interleaved", True), ("serial", False)):
                perm = T.reorder_perm(n_dims, bits, name)
                assert perm == O.reorder_perm(n_dims, bits, flag)
                assert sorted(perm) == list(range(n_dims * bits))
                sw = T.bubble_sort_swaps(perm)
                assert sw == O.bubble_sort_swaps(perm)
                # applying the swaps sorts the permutation
                p = list(perm)
                for k in sw:
                    p[k - 1], p[k] = p[k], p[k - 1]
                assert p == sorted(perm)
    # the two orderings are inverse site maps
    a, b = T.reorder_perm(3, 4, "interleaved"), T.reorder_perm(3, 4, "serial")
    assert [b[a[i]] for i in range(12)] == list(range(12))


def test_compress_kernel_register_budget(tmp_path):
    """k_compress (512-thread build, the one the benchmark times) runs at the 128-VGPR limit with its bond step force-inlined; one more
    call site with live views in that function once cost it 280 more spilled VGPRs and 7 % of the benchmark without any test noticing
    (round 2: the runtime A/B switch compared two arms of the same, slower binary).  The compiler's own report is the guard."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "tensortrainnumerics.jl_amd", "csrc", "ttn_wg512.hip")
    out = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed", "-c",
                          "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "wg512.o")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = out.stderr
    i = rep.find("k_compress")
    assert i >= 0, "no resource report for k_compress"
    blk = rep[i:i + 4000]
    spill = int(re.search(r"VGPRs Spill: (\d+)", blk).group(1))
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
    occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1))
    assert occ == 4, occ                                   # two 512-thread workgroups per CU
    assert spill <= 260 and scratch <= 1700, (spill, scratch)
