"""CPU-side test (no GPU): every header of csrc/ compiles as a translation unit of its own, i.e. it includes what it uses.
The translation units list their headers in an order; a header that leans on that order instead of its own includes hides what a
change to a lower layer can reach.  The headers are discovered by listing the directory, so a new one is covered as it appears."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensortrainnumerics.jl_amd", "csrc")
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))


def test_headers_discovered():
    assert "ttn_common.h" in HEADERS           # an empty list would make the parametrised test vanish silently


def test_host_headers_belong_to_ttn_api_alone():
    """The host API (csrc/ttn_host_*.h) has internal linkage and one copy of the library state: ttn_api.hip includes every host header,
    and ttn_wg512.hip sees none of them."""
    host = [h for h in HEADERS if h.startswith("ttn_host_")]
    assert host
    api = open(os.path.join(CSRC, "ttn_api.hip")).read()
    assert {l.split('"')[1] for l in api.splitlines() if l.startswith("#include ") and "ttn_host_" in l} == set(host)
    assert "ttn_host_" not in "".join(l for l in open(os.path.join(CSRC, "ttn_wg512.hip")).read().splitlines() if l.lstrip().startswith("#include"))


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = tmp_path / "one_header.hip"
    src.write_text('#include "%s"\n' % header)
    out = subprocess.run([hipcc, "-fsyntax-only", "--cuda-device-only", "--offload-arch=gfx950", "-std=c++17", "-Wno-unused-value",
                          "-Wno-pass-failed", "-I", CSRC, str(src)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
