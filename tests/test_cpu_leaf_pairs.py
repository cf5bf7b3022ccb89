"""wg_syrk2_impl and wg_gemm_ra2_impl, the two-team products of route F, keep the loop shapes of the single leaves.

Each team of wg_syrk2 runs the single leaf's chunk loop on half of the waves: the fragments of a k-step come through the same ring of
registers, one copy of the loop per number of live tiles of a wave.  Two things can undo that silently: a wave now owns up to three
tiles next to twelve staged doubles, and if the compiler runs out of registers it reloads accumulators or fragments from the stack
between the MFMAs (each reload behind a wait that drains the prefetch); and a test of "is this team done" placed per k-step would
put a branch between every read and its MFMA again.  The compiler's assembly of csrc/ttn_wg512.hip is the guard, read by the parser
of test_cpu_leaf_lds_batches.py: over the loop blocks of wg_syrk2_impl
  * no scratch_load, in blocks with or without an MFMA,
  * the shortest run of MFMAs in one block is a whole round of the fragment ring (6: rounds of 2 k-steps x 3 tiles, 3 x 2, 6 x 1),
  * the full `s_waitcnt lgkmcnt(0)` drains number at most a quarter of the MFMAs."""
import os
import shutil
import subprocess

import pytest

from tests.test_cpu_leaf_lds_batches import leaf_loop_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYRK2 = r"^_ZN\w*13wg_syrk2_implE\w*:"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "tensortrainnumerics.jl_amd", "csrc", "ttn_wg512.hip")
    out = tmp_path_factory.mktemp("leaf_pairs") / "wg512.s"
    run = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed", "-S",
                          "--cuda-device-only", src, "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    return open(out).read().splitlines()


def test_gemm_ra2_loops_have_no_stack_reloads_and_whole_groups(asm):
    """wg_gemm_ra2_impl: the single register-A leaf's straight-line groups of eight k-steps, two column groups per chunk and wave"""
    st = leaf_loop_stats(asm, r"^_ZN\w*16wg_gemm_ra2_implE\w*:")
    print("wg_gemm_ra2_impl", {k: (v if not isinstance(v, list) else len(v)) for k, v in st.items()})
    assert st["loop_blocks"] > 0 and st["mfma"] > 0, "no MFMA in loop blocks (the parser no longer matches the compiler's output)"
    assert not st["reloads"], f"{len(st['reloads'])} scratch_load in loop blocks, first: {st['reloads'][:4]}"
    assert st["min_group"] >= 8, f"a run of only {st['min_group']} MFMAs between two conditional branches"
    assert 4 * st["drains"] <= st["mfma"], f"{st['drains']} full lgkmcnt(0) drains for {st['mfma']} MFMAs"


def test_syrk2_loops_have_no_stack_reloads_and_whole_rounds(asm):
    st = leaf_loop_stats(asm, SYRK2)
    print("wg_syrk2_impl", {k: (v if not isinstance(v, list) else len(v)) for k, v in st.items()})
    assert st["loop_blocks"] > 0 and st["mfma"] > 0, "no MFMA in loop blocks (the parser no longer matches the compiler's output)"
    assert not st["reloads"], f"{len(st['reloads'])} scratch_load in loop blocks, first: {st['reloads'][:4]}"
    assert st["min_group"] >= 6, f"a run of only {st['min_group']} MFMAs between two conditional branches"
    assert 4 * st["drains"] <= st["mfma"], f"{st['drains']} full lgkmcnt(0) drains for {st['mfma']} MFMAs"
