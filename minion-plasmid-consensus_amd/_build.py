"""In-tree builds of the native libraries (no JIT cache: the .so files travel with
the repo snapshot to the GPU box).

  libmpc.so        HIP kernels + C-ABI (include/mpc.h, mpc_verify.h: K_vscan, mpc_coverage.h: K_covparse, mpc_linkage.h: K_lnkparse,
                   mpc_align.h: K_arevcomp, K_atrace, K_acslen, K_acswrite, mpc_draft.h: K_dvote, K_dcall), hipcc --offload-arch=gfx950;
                   its host planner (csrc/mpc_plan.cpp) with g++
  libmpc_synth.so  host-only synthetic data generator (g++)
  libmpc_ingest.so native host I/O: ingest (Steps 1-3) and writers (Step 7) (include/mpc_ingest.h, g++ -pthread)
                   and the host halves of verify_consensus (include/mpc_verify.h), coverage_qc (mpc_coverage.h)
                   linkage_qc (mpc_linkage.h), align_reads and the handoff of reads_consensus (mpc_align.h) and draft_assembly (mpc_draft.h)

Shared glue, listed below so that a change to it makes its library stale:
csrc/mpc_launch.h (the launchers of the tool .hip files) in HIP_HEADERS,
csrc/host_file.h (the host parsers' file mapping, line cuts, digit loop and
last-error message) in INGEST_HEADERS, csrc/mpc_draftrule.h (the vote's table
rule and the call of one column, host and device) in both.  The ctypes prototypes of both
libraries are in _native.py.
"""
import os
import subprocess
import tempfile

PKG = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(REPO, "include")
LIBMPC = os.path.join(PKG, "libmpc.so")
LIBSYNTH = os.path.join(PKG, "libmpc_synth.so")
LIBINGEST = os.path.join(PKG, "libmpc_ingest.so")

HIP_SOURCES = ["mpc_kernels.hip", "mpc_verify.hip", "mpc_cov.hip", "mpc_link.hip", "mpc_align.hip", "mpc_draft.hip"]
HOST_SOURCES = ["mpc_plan.cpp"]  # libmpc.so's host planner (g++, no HIP)
HIP_HEADERS = ["mpc_device.h", "mpc_geometry.h", "mpc_plan.h", "mpc_cswalk.h", "mpc_cstables.h", "mpc_bandtrace.h",
               "mpc_draftrule.h",
               "mpc_launch.h",  # the launchers' host glue of the tool .hip files
               # the stages of mpc_kernels.hip (one translation unit), in pipeline order
               "mpc_k_common.h", "mpc_k_parse.h", "mpc_k_index.h", "mpc_k_left.h", "mpc_k_wrap.h", "mpc_k_layout.h",
               "mpc_k_rows.h", "mpc_k_call.h"]
INGEST_SOURCES = ["ingest.cpp", "writers.cpp", "pseudopair.cpp", "verify.cpp", "coverage.cpp", "linkage.cpp", "align.cpp", "draft.cpp"]
INGEST_HEADERS = ["host_threads.h", "host_file.h", "mpc_cswalk_host.h", "mpc_cstables.h", "mpc_bandtrace.h", "mpc_draftrule.h"]  # csrc headers of libmpc_ingest.so


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.exists(s) and os.path.getmtime(s) > t for s in sources)


def build_synth(force=False):
    src = os.path.join(CSRC, "synth.cpp")
    if force or _stale(LIBSYNTH, [src, os.path.join(CSRC, "host_threads.h")]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", LIBSYNTH, src], check=True)
    return LIBSYNTH


def ensure_synth():
    return build_synth()


def build_ingest(force=False):
    srcs = [os.path.join(CSRC, f) for f in INGEST_SOURCES]
    hdrs = [os.path.join(INCLUDE, h) for h in ("mpc_ingest.h", "mpc_verify.h", "mpc_coverage.h", "mpc_linkage.h", "mpc_align.h", "mpc_draft.h")]
    if force or _stale(LIBINGEST, srcs + hdrs + [os.path.join(CSRC, h) for h in INGEST_HEADERS]):
        subprocess.run(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", INCLUDE, "-o", LIBINGEST] + srcs,
                       check=True)
    return LIBINGEST


def build_hip(force=False, extra=(), out=None):
    """libmpc.so (``out``/``extra``: experiment variants, e.g. -DMPC_TUNING_OVERRIDES)."""
    out = out or LIBMPC
    srcs = [os.path.join(CSRC, s) for s in HIP_SOURCES]
    host = [os.path.join(CSRC, s) for s in HOST_SOURCES]
    deps = srcs + host + [os.path.join(CSRC, h) for h in HIP_HEADERS] + [os.path.join(INCLUDE, h) for h in ("mpc.h", "mpc_verify.h", "mpc_coverage.h", "mpc_linkage.h", "mpc_align.h", "mpc_draft.h")]
    if force or extra or _stale(out, deps):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        flags = ["-O3", "-std=c++17", "-fPIC", "-I", INCLUDE, "-I", CSRC] + list(extra)
        with tempfile.TemporaryDirectory() as tmp:
            objs = []
            for s in host:  # the host planner: plain C++, same -D switches as the kernels
                objs.append(os.path.join(tmp, os.path.splitext(os.path.basename(s))[0] + ".o"))
                subprocess.run(["g++", "-c"] + flags + ["-o", objs[-1], s], check=True)
            # (objects before the .hip sources: hipcc reads everything after one as HIP)
            subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-o", out] + flags + objs + srcs, check=True)
    return out


def build_all(force=False):
    build_synth(force)
    build_ingest(force)
    build_hip(force)
