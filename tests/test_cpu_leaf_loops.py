"""The out-of-line matrix-product leaves of k_compress keep nothing on the stack inside their loops.

k_compress (512-thread build) runs at the 128-VGPR limit, and so do the leaves it calls.  A leaf whose loop-invariant per-lane values
(addresses, staging indices, masks) do not fit next to its accumulators gets them spilled, and reloads them inside its loops — each
reload a `scratch_load` behind a full `s_waitcnt vmcnt(0)` that also drains the global loads in flight (wg_fused_merge_direct once ran
the twelve operand loads of a prefetch group as twelve serial memory round trips this way).  The compiler's own assembly is the guard:
csrc/ttn_wg512.hip is compiled to assembly once, and no basic block that the compiler marks `in Loop` of
  wg_fused_merge_direct, wg_gemm_impl<2>, wg_gemm_impl<4>
may contain a scratch_load (prologue / epilogue saves of callee-saved registers lie outside the loops and are not counted)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEAVES = {
    "wg_fused_merge_direct": r"^_ZN\w*21wg_fused_merge_directE\w*:",
    "wg_gemm_impl<2>": r"^_ZN\w*12wg_gemm_implILi2EE\w*:",
    "wg_gemm_impl<4>": r"^_ZN\w*12wg_gemm_implILi4EE\w*:",
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "tensortrainnumerics.jl_amd", "csrc", "ttn_wg512.hip")
    out = tmp_path_factory.mktemp("leaf_loops") / "wg512.s"
    run = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed", "-S",
                          "--cuda-device-only", src, "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    return open(out).read().splitlines()


def loop_reloads(lines, entry_pattern):
    """(number of `in Loop` blocks, [(block label, instruction)] of the scratch_load instructions in them) of the function whose
    entry label matches entry_pattern.  A block starts at a `.LBBn_m:` label or at a `; %bb.n:` fall-through comment; the compiler
    appends `in Loop: Header=...` to either when the block belongs to a loop, and `This (Inner) Loop Header` / `Parent Loop` to the
    header block of a loop itself."""
    entry = re.compile(entry_pattern)
    start = [i for i, ln in enumerate(lines) if entry.match(ln)]
    assert len(start) == 1, f"{entry_pattern}: {len(start)} entry labels"
    in_loop, label, nblocks, found = False, None, 0, []
    for ln in lines[start[0] + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", ln):
            in_loop = any(mark in ln for mark in ("in Loop:", "Loop Header", "Parent Loop"))
            label = ln.split()[0] if ln.startswith(".LBB") else ln.split()[1]
            nblocks += in_loop
            continue
        ins = ln.strip()
        if in_loop and ins.startswith("scratch_load"):
            found.append((label, ins.split(";")[0].strip()))
    return nblocks, found


@pytest.mark.parametrize("leaf", list(LEAVES))
def test_leaf_has_no_stack_reload_in_loops(asm, leaf):
    nblocks, found = loop_reloads(asm, LEAVES[leaf])
    assert nblocks > 0, f"{leaf}: no loop blocks found (the parser no longer matches the compiler's comments)"
    assert not found, f"{leaf}: {len(found)} scratch_load in loop blocks, first: {found[:4]}"


def test_parser_sees_reloads_where_they_are():
    """The parser on a hand-written listing: a reload in a loop block is reported, the same reload outside a loop is not."""
    listing = """_ZN3foo12wg_gemm_implILi2EEEvPKNS_8GemmDescEPd:
; %bb.0:
\tscratch_load_dword v1, off, s32 offset:4 ; 4-byte Folded Reload
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\tscratch_load_dword v4, off, s32 offset:16 ; 4-byte Folded Reload
; %bb.2:                                ;   in Loop: Header=BB0_1 Depth=1
\tscratch_load_dword v2, off, s32 offset:8 ; 4-byte Folded Reload
.LBB0_3:                                ;   in Loop: Header=BB0_1 Depth=1
\ts_cbranch_scc1 .LBB0_1
.LBB0_4:
\tscratch_load_dword v3, off, s32 offset:12 ; 4-byte Folded Reload
.Lfunc_end0:
""".splitlines()
    nblocks, found = loop_reloads(listing, LEAVES["wg_gemm_impl<2>"])
    assert nblocks == 3
    assert found == [(".LBB0_1:", "scratch_load_dword v4, off, s32 offset:16"), ("%bb.2:", "scratch_load_dword v2, off, s32 offset:8")]
