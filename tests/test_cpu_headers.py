"""CPU-side test (no GPU): every header of csrc/ compiles as a translation unit of its own, i.e. it includes what it uses.
The translation units list their headers in an order; a header that leans on that order instead of its own includes hides what a
change to a lower layer can reach.  The headers are discovered by listing the directory, so a new one is covered as it appears.
The host API's headers (csrc/ttn_host_*.h) are layered besides: no cycles, ttn_api.hip lists them lowest first, and the
launchers of the second translation unit are declared in one header that both units include."""
import os
import re
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


def _host_includes(fname):
    """The csrc/ttn_host_*.h that `fname` includes, in the order it lists them."""
    return re.findall(r'^#include "(ttn_host_\w+\.h)"', open(os.path.join(CSRC, fname)).read(), re.M)


def test_host_headers_are_layered():
    """The includes among the host headers form no cycle, ttn_api.hip lists every host header after the ones it includes, and the
    dynamic-LDS table comes first (it fixes the order of the kernel templates' instantiations)."""
    host = [h for h in HEADERS if h.startswith("ttn_host_")]
    deps = {h: _host_includes(h) for h in host}
    for h, ds in deps.items():
        assert h not in ds and set(ds) <= set(host), (h, ds)
    left = dict(deps)                                   # peel off the headers whose includes have all been peeled off already
    while left:
        free = [h for h, ds in left.items() if not any(d in left for d in ds)]
        assert free, "cycle among " + ", ".join(sorted(left))
        for h in free:
            del left[h]
    order = _host_includes("ttn_api.hip")
    assert len(order) == len(set(order))
    assert order[0] == "ttn_host_lds.h"
    for h in order:
        for dep in deps[h]:
            assert order.index(dep) < order.index(h), f"ttn_api.hip lists {h} before {dep}, which it includes"


def test_wg512_seam_is_declared_once():
    """Both translation units include ttn_wg512.h, so the compiler checks each ttn_wg512_* definition and each call against the same
    prototype; nobody writes one out again (both sides are extern "C": a second, different prototype would link silently)."""
    for tu in ("ttn_api.hip", "ttn_wg512.hip"):
        assert re.search(r'^#include "ttn_wg512\.h"', open(os.path.join(CSRC, tu)).read(), re.M), tu
    # a declaration: a type, the name, the parameters and no body (a call has no type in front, or `return` / `else`)
    proto = re.compile(r'^[ \t]*(?:extern\s+"C"\s+)?(?!return\b|else\b)\w+(?:\s*\*+\s*|\s+)ttn_wg512_\w+\s*\([^;{}]*\)\s*;', re.M)
    with_protos = [f for f in sorted(os.listdir(CSRC)) if proto.search(re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read()))]
    assert with_protos == ["ttn_wg512.h"]
    # ... and it declares every launcher that ttn_wg512.hip defines (eight today), no more and no fewer
    defined = set(re.findall(r"^\w+ (ttn_wg512_\w+)\([^;{}]*\)\s*\{", open(os.path.join(CSRC, "ttn_wg512.hip")).read(), re.M))
    declared = set(re.findall(r"\b(ttn_wg512_\w+)\s*\(", "".join(proto.findall(open(os.path.join(CSRC, "ttn_wg512.h")).read()))))
    assert defined and declared == defined


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
