"""The host planner (csrc/mpc_plan.cpp) answers exactly what the fixture
tests/golden/plan_shapes.json recorded (scripts/make_plan_golden.py) for every
shape of tests/plan_shapes.py: plan info, parse tables, workspace bytes, offset
and count of every MPC_BUF_*; and every error case returns the recorded code
and message.  Host-only (no GPU)."""
import plan_shapes as ps


def test_plan_shapes_match_golden(pkg):
    fx = ps.load_fixture()
    assert ps.bisect_lds_limit(pkg.engine) == fx["lds_limit"]
    cases = ps.cases(fx["lds_limit"])
    assert sorted(c["name"] for c in cases) == sorted(fx["cases"])
    for c in cases:
        assert ps.record(pkg.engine, c) == fx["cases"][c["name"]], c["name"]


def test_plan_errors_match_golden(pkg):
    fx = ps.load_fixture()
    cases = ps.error_cases()
    assert sorted(c["name"] for c in cases) == sorted(fx["errors"])
    for c in cases:
        got = ps.record(pkg.engine, c)
        assert got["rc"] < 0 and got == fx["errors"][c["name"]], c["name"]
