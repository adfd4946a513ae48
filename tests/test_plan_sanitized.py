"""ASan + UBSan build of the host planner (csrc/mpc_plan.cpp): a driver
executable (tests/native/plan_driver.cpp) built with
-fsanitize=address,undefined and no recovery plans and destroys every shape
and every error case of tests/plan_shapes.py.  Any sanitizer report, a leak
included, fails the run (non-zero exit); what it prints must equal the fixture
tests/golden/plan_shapes.json (CPU only, no HIP)."""
import os
import subprocess

import pytest

import plan_shapes as ps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "build", "plan_asan")


@pytest.fixture(scope="module")
def asan_bin():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    csrc = os.path.join(REPO, "minion-plasmid-consensus_amd", "csrc")
    src = [os.path.join(csrc, "mpc_plan.cpp"), os.path.join(REPO, "tests", "native", "plan_driver.cpp")]
    # build under a per-process name, then rename: pytest-xdist workers each
    # build it, and one must never exec a file another is still writing
    tmp = "%s.%d" % (BIN, os.getpid())
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "include"), "-I", csrc, "-o", tmp] + src,
                   check=True)
    os.replace(tmp, BIN)
    return BIN


def _run(asan_bin, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    p = subprocess.run([asan_bin, path], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    return ps.parse_driver_output(p.stdout)


def test_plan_shapes_sanitized(asan_bin, tmp_path):
    fx = ps.load_fixture()
    path = str(tmp_path / "cases.txt")
    ps.write_case_file(path, ps.cases(fx["lds_limit"]))
    assert _run(asan_bin, path) == fx["cases"]


def test_plan_errors_sanitized(asan_bin, tmp_path):
    fx = ps.load_fixture()
    path = str(tmp_path / "errors.txt")
    ps.write_case_file(path, ps.error_cases())
    assert _run(asan_bin, path) == fx["errors"]
