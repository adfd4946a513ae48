"""What the native libraries are built from (no GPU): every csrc header a source
includes is a rebuild dependency in _build.py -- the .so files travel with the
tree, and a stale one is a silent wrong test -- and every stage header of
mpc_kernels.hip (mpc_k_*.h) includes what it uses."""
import glob
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

INCLUDE_RE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def csrc_includes(b, roots):
    """The csrc files reachable from ``roots`` through quoted includes, roots excluded."""
    seen, todo = set(), list(roots)
    while todo:
        name = todo.pop()
        for inc in INCLUDE_RE.findall(open(os.path.join(b.CSRC, name)).read()):
            if inc not in seen and os.path.exists(os.path.join(b.CSRC, inc)):  # (else: include/, a system header)
                seen.add(inc)
                todo.append(inc)
    return seen - set(roots)


def test_every_included_header_is_a_dependency(pkg):
    b = pkg._build
    hip = csrc_includes(b, b.HIP_SOURCES + b.HOST_SOURCES)
    assert {"mpc_k_common.h", "mpc_k_parse.h", "mpc_plan.h"} <= hip  # the walk found the stage headers
    assert hip <= set(b.HIP_HEADERS), sorted(hip - set(b.HIP_HEADERS))
    ingest = csrc_includes(b, b.INGEST_SOURCES)
    assert "host_threads.h" in ingest
    assert ingest <= set(b.INGEST_HEADERS), sorted(ingest - set(b.INGEST_HEADERS))


def test_stage_headers_compile_alone(pkg):
    """Each mpc_k_*.h as the main file of a device-side syntax check."""
    b = pkg._build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    headers = sorted(glob.glob(os.path.join(b.CSRC, "mpc_k_*.h")))
    assert len(headers) >= 8 and {os.path.basename(h) for h in headers} <= set(b.HIP_HEADERS)

    def check(h):
        return subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", "-std=c++17",
                               "-Wno-pragma-once-outside-header", "-I", b.INCLUDE, "-I", b.CSRC, "-x", "hip", h],
                              capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=min(16, len(headers))) as pool:
        for h, r in zip(headers, pool.map(check, headers)):
            assert r.returncode == 0, "%s\n%s" % (os.path.basename(h), r.stderr[-4000:])
