"""The stand-alone sanitizer recipe of the host-code tests: a driver with its
own main is built with ASan + UBSan and no recovery, then run; any report, a
leak included, fails the run (non-zero exit).  CPU only, no HIP; nothing is
loaded into Python under a sanitizer."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "minion-plasmid-consensus_amd", "csrc")
NATIVE = os.path.join(REPO, "tests", "native")


def build(name, sources, extra=()):
    """build/<name> from ``sources`` (a bare file name: of csrc/)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    binary = os.path.join(REPO, "build", name)
    os.makedirs(os.path.dirname(binary), exist_ok=True)
    # build under a per-process name, then rename: pytest-xdist workers each
    # build it, and one must never exec a file another is still writing
    tmp = "%s.%d" % (binary, os.getpid())
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", *extra, "-I", os.path.join(REPO, "include"), "-I", CSRC, "-o", tmp] +
                   [os.path.join(CSRC, str(s)) for s in sources], check=True)
    os.replace(tmp, binary)
    return binary


def run(binary, args, text=True, timeout=300):
    """The program's stdout; it must exit 0."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    p = subprocess.run([binary] + [str(a) for a in args], capture_output=True, text=text, env=env, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout
