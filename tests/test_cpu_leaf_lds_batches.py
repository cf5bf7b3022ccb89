"""The SYRK and register-A leaves of k_compress read their LDS fragments in batches, ahead of the MFMAs that use them.

Written with one register pair per operand, every MFMA of wg_syrk_impl and wg_gemm_ra_impl sat behind its own `ds_read_b64` and a full
`s_waitcnt lgkmcnt(0)`, with a wave-uniform branch in between (a tile that may be absent, a k-step that may be past the end): 5 drains
for 5 MFMAs, 32 for 32.  The leaves now keep their fragments in a ring of registers — each one refilled right behind the MFMA that
consumed it, for a later k-step, with no test in between — so the waits in front of the MFMAs are counted ones.
The compiler's own assembly is the guard, as in
test_cpu_leaf_loops.py: csrc/ttn_wg512.hip is compiled to assembly once, and over the loop blocks of each leaf that contain an MFMA
  * the full drains `s_waitcnt lgkmcnt(0)` number at most a quarter of the MFMAs,
  * no conditional branch lies between two MFMAs of a k-step group: the compiler ends a basic block at every conditional branch, so
    this is measured as the shortest run of MFMAs in one block — at least a whole round of the fragment ring (SYRK) or a whole
    group of eight k-steps (register-A), where the parent had ONE MFMA per block,
and no loop block of the leaf, with or without MFMAs, contains a scratch_load."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEAVES = {
    "wg_syrk_impl<3,4,5>": r"^_ZN\w*12wg_syrk_implILi3ELi4ELi5EEE\w*:",
    "wg_syrk_impl<6,2,2>": r"^_ZN\w*12wg_syrk_implILi6ELi2ELi2EEE\w*:",
    "wg_gemm_ra_impl": r"^_ZN\w*15wg_gemm_ra_implE\w*:",
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "tensortrainnumerics.jl_amd", "csrc", "ttn_wg512.hip")
    out = tmp_path_factory.mktemp("leaf_lds_batches") / "wg512.s"
    run = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed", "-S",
                          "--cuda-device-only", src, "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    return open(out).read().splitlines()


def _is_full_lgkm_drain(ins):
    """`s_waitcnt lgkmcnt(0)`, alone or combined with other counters (`s_waitcnt vmcnt(2) lgkmcnt(0)`)."""
    return ins.startswith("s_waitcnt") and "lgkmcnt(0)" in ins


def leaf_loop_stats(lines, entry_pattern):
    """Over the function whose entry label matches entry_pattern, a dict:
      loop_blocks     blocks the compiler marks as part of a loop (see test_cpu_leaf_loops.py for the marks)
      mfma            MFMAs in loop blocks
      drains          full lgkmcnt(0) waits in the loop blocks that contain an MFMA
      min_group       the fewest MFMAs any MFMA-containing loop block holds (the compiler ends a block at every conditional branch, so
                      this is the shortest run of MFMAs that no branch interrupts)
      reloads         [(block label, instruction)]: scratch_load instructions in loop blocks
    A block starts at a `.LBBn_m:` label or at a `; %bb.m:` fall-through comment; it belongs to a loop if that line, or the comment
    line that continues it (`.LBB5_39: ; Parent Loop ...` / `; => This Inner Loop Header`), carries one of the compiler's loop marks.
    (The listing order of the blocks is not their execution order — a loop that runs at most once is laid out as a branch around a
    block placed behind the loop's other blocks — so "between" is only judged inside a block.)"""
    entry = re.compile(entry_pattern)
    start = [i for i, ln in enumerate(lines) if entry.match(ln)]
    assert len(start) == 1, f"{entry_pattern}: {len(start)} entry labels"
    body_lines = []
    for ln in lines[start[0] + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        body_lines.append(ln)
    blocks = []                                  # [label, in a loop, [instructions]]
    for i, ln in enumerate(body_lines):
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", ln):
            marks = ln
            if i + 1 < len(body_lines) and re.match(r"^\s+;", body_lines[i + 1]):
                marks += body_lines[i + 1]
            in_loop = any(mark in marks for mark in ("in Loop:", "Loop Header", "Parent Loop"))
            label = ln.split()[0] if ln.startswith(".LBB") else ln.split()[1]
            blocks.append([label, in_loop, []])
            continue
        ins = ln.split(";")[0].strip()
        if blocks and ins and not ins.startswith("."):
            blocks[-1][2].append(ins)
    st = {"loop_blocks": 0, "mfma": 0, "drains": 0, "min_group": None, "reloads": []}
    for label, in_loop, body in blocks:
        if not in_loop:
            continue
        st["loop_blocks"] += 1
        st["reloads"] += [(label, i) for i in body if i.startswith("scratch_load")]
        at = [n for n, i in enumerate(body) if i.startswith("v_mfma")]
        if at:
            assert not any(i.startswith("s_cbranch") for i in body[at[0]:at[-1]]), f"{label}: a conditional branch inside a block"
            st["mfma"] += len(at)
            st["drains"] += sum(_is_full_lgkm_drain(i) for i in body)
            st["min_group"] = len(at) if st["min_group"] is None else min(st["min_group"], len(at))
    return st


# The shortest run of MFMAs a loop block may hold.  wg_syrk_impl: a wave with NT live tiles runs rounds of D k-steps x NT tiles (D = 1 for
# NT >= 4, else 2, 3, 6 for NT = 3, 2, 1: syrk_ksteps), each round and each tail one block: 5, 4, 6, 6, 6 MFMAs for the copies of <3,4,5>,
# 6 and 6 for those of <6,2,2>.  wg_gemm_ra_impl: straight-line groups of 8, 16, 24 or 32 k-steps.
MIN_GROUP = {"wg_syrk_impl<3,4,5>": 4, "wg_syrk_impl<6,2,2>": 6, "wg_gemm_ra_impl": 8}


@pytest.mark.parametrize("leaf", list(LEAVES))
def test_leaf_reads_lds_in_batches(asm, leaf):
    st = leaf_loop_stats(asm, LEAVES[leaf])
    print(leaf, {k: (v if not isinstance(v, list) else len(v)) for k, v in st.items()})
    assert st["loop_blocks"] > 0 and st["mfma"] > 0, f"{leaf}: no MFMA in loop blocks (the parser no longer matches the compiler's output)"
    assert 4 * st["drains"] <= st["mfma"], f"{leaf}: {st['drains']} full lgkmcnt(0) drains for {st['mfma']} MFMAs"
    assert st["min_group"] >= MIN_GROUP[leaf], f"{leaf}: a run of only {st['min_group']} MFMAs between two conditional branches"
    assert not st["reloads"], f"{leaf}: {len(st['reloads'])} scratch_load in loop blocks, first: {st['reloads'][:4]}"


PARENT_STYLE = """_ZN3foo15wg_gemm_ra_implEPKNS_8GemmDescEPd:
; %bb.0:
\ts_waitcnt lgkmcnt(0)
\tscratch_load_dword v1, off, s32 offset:4 ; 4-byte Folded Reload
\tv_mfma_f64_16x16x4_f64 v[0:7], v[8:9], v[10:11], v[0:7]
.LBB0_1:                                ; =>This Loop Header: Depth=1
\ts_barrier
\ts_cbranch_scc1 .LBB0_8
.LBB0_2:                                ;   Parent Loop BB0_1 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
\ts_andn2_b64 vcc, exec, s[26:27]
\ts_cbranch_vccnz .LBB0_4
; %bb.3:                                ;   in Loop: Header=BB0_2 Depth=2
\tds_read_b64 v[8:9], v20
\ts_waitcnt lgkmcnt(0)
\tv_mfma_f64_16x16x4_f64 v[0:7], v[8:9], v[10:11], v[0:7]
.LBB0_4:                                ;   in Loop: Header=BB0_2 Depth=2
\ts_andn2_b64 vcc, exec, s[28:29]
\ts_cbranch_vccnz .LBB0_6
; %bb.5:                                ;   in Loop: Header=BB0_2 Depth=2
\tds_read_b64 v[8:9], v20 offset:8
\ts_waitcnt vmcnt(1) lgkmcnt(0)
\tv_mfma_f64_16x16x4_f64 v[12:19], v[8:9], v[10:11], v[12:19]
.LBB0_6:                                ;   in Loop: Header=BB0_2 Depth=2
\ts_cmp_lg_u32 s4, 0
\ts_cbranch_scc1 .LBB0_2
; %bb.7:                                ;   in Loop: Header=BB0_1 Depth=1
\ts_waitcnt lgkmcnt(0)
\tscratch_load_dword v2, off, s32 offset:8 ; 4-byte Folded Reload
\ts_branch .LBB0_1
.LBB0_8:
\ts_waitcnt lgkmcnt(0)
.Lfunc_end0:
"""

RING_STYLE = """_ZN3foo15wg_gemm_ra_implEPKNS_8GemmDescEPd:
; %bb.0:
\ts_waitcnt lgkmcnt(0)
.LBB0_1:                                ; =>This Loop Header: Depth=1
\tds_read_b64 v[8:9], v20
\tds_read_b64 v[20:21], v20 offset:8
\ts_cmp_lt_i32 s26, 2
\ts_cbranch_scc1 .LBB0_3
.LBB0_2:                                ;   Parent Loop BB0_1 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
\ts_waitcnt lgkmcnt(1)
\tv_mfma_f64_16x16x4_f64 v[0:7], v[8:9], v[10:11], v[0:7]
\tds_read_b64 v[8:9], v20 offset:16
\ts_waitcnt lgkmcnt(1)
\tv_mfma_f64_16x16x4_f64 v[12:19], v[20:21], v[10:11], v[12:19]
\tds_read_b64 v[20:21], v20 offset:24
\ts_cmp_lg_u32 s4, 0
\ts_cbranch_scc1 .LBB0_2
.LBB0_3:                                ;   in Loop: Header=BB0_1 Depth=1
\ts_waitcnt lgkmcnt(1)
\tv_mfma_f64_16x16x4_f64 v[0:7], v[8:9], v[10:11], v[0:7]
\ts_waitcnt lgkmcnt(0)
\tv_mfma_f64_16x16x4_f64 v[12:19], v[20:21], v[10:11], v[12:19]
\ts_barrier
\ts_cbranch_scc1 .LBB0_1
; %bb.4:
\ts_waitcnt lgkmcnt(0)
.Lfunc_end0:
"""


def test_parser_on_hand_written_listings():
    """Two listings in the compiler's block style (every conditional branch ends its block; a fall-through block is `; %bb.n:`; an
    inner loop's header carries its mark on a comment line of its own).  PARENT_STYLE is the shape the leaves had: each MFMA alone in a
    block behind a skip branch, a drain in front of it.  RING_STYLE is the shape they have now: the k loop is one block, its tail another.
    What lies outside the loops (a drain, a reload, an MFMA) is not counted."""
    st = leaf_loop_stats(PARENT_STYLE.splitlines(), LEAVES["wg_gemm_ra_impl"])
    assert st["loop_blocks"] == 7
    assert st["mfma"] == 2 and st["drains"] == 2 and st["min_group"] == 1
    assert st["reloads"] == [("%bb.7:", "scratch_load_dword v2, off, s32 offset:8")]
    st = leaf_loop_stats(RING_STYLE.splitlines(), LEAVES["wg_gemm_ra_impl"])
    assert st["loop_blocks"] == 3
    assert st["mfma"] == 4 and st["drains"] == 1 and st["min_group"] == 2
    assert st["reloads"] == []
