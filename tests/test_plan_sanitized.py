"""ASan + UBSan build of the host planner (csrc/mpc_plan.cpp): a driver
executable (tests/native/plan_driver.cpp) built with
-fsanitize=address,undefined and no recovery plans and destroys every shape
and every error case of tests/plan_shapes.py.  Any sanitizer report, a leak
included, fails the run (non-zero exit); what it prints must equal the fixture
tests/golden/plan_shapes.json (CPU only, no HIP)."""
import os

import pytest

import native_util as nu
import plan_shapes as ps


@pytest.fixture(scope="module")
def asan_bin():
    return nu.build("plan_asan", ["mpc_plan.cpp", os.path.join(nu.NATIVE, "plan_driver.cpp")])


def _run(asan_bin, path):
    return ps.parse_driver_output(nu.run(asan_bin, [path]))


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
