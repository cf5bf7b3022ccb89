"""bench.py: a plain run measures the headline alone; `--full` adds every other measurement and check, each one skipped by its
--no-* option."""
import json
import os
import subprocess
import sys

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = ("verify", "single", "ops", "c2", "core_sharded", "cpu")


def test_plain_run_measures_the_headline_alone():
    plain = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "1"])
    assert not plain.full
    assert [p for p in PARTS if bench.wants(plain, p)] == []
    assert [p for p in PARTS if bench.wants(bench.parse_args(["--no-c2"]), p)] == []


def test_full_runs_every_part_unless_skipped():
    assert [p for p in PARTS if bench.wants(bench.parse_args(["--full"]), p)] == list(PARTS)
    for skipped in PARTS:
        args = bench.parse_args(["--full", "--no-" + skipped.replace("_", "-")])
        assert [p for p in PARTS if bench.wants(args, p)] == [p for p in PARTS if p != skipped]


def _bench_line(*argv, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return lines[0]


@pytest.mark.gpu
def test_bench_plain_and_full_lines():
    common = ("--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8")
    plain = _bench_line(*common)
    assert plain["unit"] == "TT cores/s" and plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 2 and plain["warmup"] == 1
    assert plain["roofline"]["kernel"] == "k_compress"
    for key in ("verified", "c2", "other_kernels", "batch_sweep", "drop_in", "cpu_baseline"):
        assert key not in plain, key
    full = _bench_line(*common, "--full", "--no-cpu", "--no-single", "--no-ops")
    assert full["metric"] == plain["metric"] and full["config"] == plain["config"]
    assert full["verified"] == 3 and full["verified_max_rel_diff"] <= 1e-9
    assert full["c2"]["verified"] == 3
    for key in ("other_kernels", "batch_sweep", "drop_in", "cpu_baseline"):
        assert key not in full, key
