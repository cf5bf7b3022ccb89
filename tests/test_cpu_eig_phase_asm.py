"""The eigenvector phase of the symmetric eigensolver (wg_twisted, csrc/ttn_eig_kernels.h) stays in LDS and registers.

Before r03l the 512-thread build kept the D- pivots of a 128-row matrix, and the lower half of every eigenvector, in global memory
(the dead Gram matrix): `wg_eig_n<128>` held 276 global_load and 255 global_store instructions, about 40 dependent global round trips
per Gram step.  Now D- lives in the registers of four holder waves until the twist is known and shares the one LDS array with D+
afterwards.  The compiler's own assembly is the guard, as in test_cpu_leaf_lds_batches.py: csrc/ttn_wg512.hip is compiled to
assembly once, and `wg_eig_n<128>` may hold at most 64 global_load and 16 global_store instructions, `wg_eig_n<64>` no more than it
did (9 and 0): what remains is the staging of the reflectors for the back-transformation and sig[].  A listing in which the function
or its reflector loads are not found fails.

(The issue behind r03l also asked for bounds on the LDS waits of the z chains and of the back-transformation loop.  Those two parts
did not pay on the headline and are not in the tree — DESIGN §4.2 has the numbers — so their bounds are not here either.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EIG = {
    "wg_eig_n<128>": r"^_ZN\w*8wg_eig_nILi128EEE\w*:",
    "wg_eig_n<64>": r"^_ZN\w*8wg_eig_nILi64EEE\w*:",
}
# (global_load, global_store) a function may hold
BOUND = {"wg_eig_n<128>": (64, 16), "wg_eig_n<64>": (9, 0)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "tensortrainnumerics.jl_amd", "csrc", "ttn_wg512.hip")
    out = tmp_path_factory.mktemp("eig_phase_asm") / "wg512.s"
    run = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed", "-S",
                          "--cuda-device-only", src, "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    return open(out).read().splitlines()


def global_traffic(lines, entry_pattern):
    """(global_load, global_store) instructions between the entry label matching entry_pattern and the function's end"""
    entry = re.compile(entry_pattern)
    start = [i for i, ln in enumerate(lines) if entry.match(ln)]
    assert len(start) == 1, f"{entry_pattern}: {len(start)} entry labels"
    loads = stores = 0
    for ln in lines[start[0] + 1:]:
        if ln.startswith(".Lfunc_end"):
            return loads, stores
        ins = ln.split(";")[0].strip()
        loads += ins.startswith("global_load")
        stores += ins.startswith("global_store")
    raise AssertionError(f"{entry_pattern}: no .Lfunc_end")


@pytest.mark.parametrize("fn", list(EIG))
def test_no_global_memory_in_eigenvector_phase(asm, fn):
    loads, stores = global_traffic(asm, EIG[fn])
    print(fn, "global_load", loads, "global_store", stores)
    assert loads > 0, f"{fn}: the reflectors are staged from global memory — no load found means the parser is off"
    assert loads <= BOUND[fn][0], f"{fn}: {loads} global_load"
    assert stores <= BOUND[fn][1], f"{fn}: {stores} global_store"


PARENT_STYLE = """_ZN3foo8wg_eig_nILi128EEEiPKdiPdiiS3_S3_PiS3_:
; %bb.0:
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tglobal_load_dwordx2 v[2:3], v[0:1], off
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\tv_rcp_f64_e32 v[8:9], v[4:5]
\tglobal_store_dwordx2 v[0:1], v[8:9], off      ; a comment that names global_load
\tglobal_load_dwordx2 v[4:5], v[0:1], off offset:512
\ts_cbranch_scc1 .LBB0_1
; %bb.2:
\ts_setpc_b64 s[30:31]
.Lfunc_end0:
_ZN3foo8wg_eig_nILi64EEEiPKdiPdiiS3_S3_PiS3_:
; %bb.0:
\tglobal_load_dwordx4 v[2:5], v[0:1], off
\tds_write_b64 v10, v[2:3]
\ts_setpc_b64 s[30:31]
.Lfunc_end1:
"""


def test_parser_on_a_hand_written_listing():
    lines = PARENT_STYLE.splitlines()
    assert global_traffic(lines, EIG["wg_eig_n<128>"]) == (2, 1)          # stops at the function's end; comments do not count
    assert global_traffic(lines, EIG["wg_eig_n<64>"]) == (1, 0)
    with pytest.raises(AssertionError):
        global_traffic(lines, r"^_ZN\w*8wg_eig_nILi32EEE\w*:")
