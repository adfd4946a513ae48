"""The command-line front of the seven tools (_cli.py) against transcripts of
the commit before it existed (tests/cli_cases.py says how they were recorded):
exit status, stdout, stderr and every file left behind, compared exactly once
the time stamps and the banner's values are masked.  Every case runs the tool by
file path in a process of its own; one case per tool runs again through
main(argv) of the imported module, the other way a tool finds _cli.  CPU only."""
import pytest

import cli_cases as cc


@pytest.mark.parametrize("name", sorted(cc.CPU_CASES))
def test_by_path_matches_the_transcript(name, tmp_path):
    tool, build = cc.CPU_CASES[name]
    assert cc.run_by_path(cc.PKGDIR, tool, build, tmp_path, "cpu") == cc.load(name)


@pytest.mark.parametrize("name", cc.IMPORTED)
def test_imported_matches_the_transcript(name, tmp_path, monkeypatch, capfd, pkg):
    tool, build = cc.CPU_CASES[name]
    monkeypatch.chdir(tmp_path)
    assert cc.run_imported(pkg.__name__, tool, build, tmp_path, "cpu", capfd) == cc.load(name)


@pytest.mark.parametrize("tool, argv", cc.USAGE, ids=lambda v: v if isinstance(v, str) else " ".join(v))
def test_argparse_refusals(tool, argv, tmp_path):
    want = cc.load("usage")["lines"][tool + " " + " ".join(argv)]
    assert want["exit"] == 2
    assert cc.usage_line(cc.PKGDIR, tool, argv, tmp_path) == want


def test_the_cases_end_as_intended():
    """What each recorded case is there for: its exit status and the files it leaves."""
    want = {"verify_fail": (2, ["edits.tsv", "verify.tsv"]), "verify_missing": (1, []),
            "coverage_region": (0, ["cov.tsv", "depth.tsv"]), "coverage_expected": (0, ["cov.tsv", "depth.tsv"]),
            "coverage_strict_fail": (2, ["cov.tsv"]), "coverage_bad_cs": (1, []), "coverage_min_depth": (1, []),
            "coverage_region_outside": (1, []), "coverage_unwritable": (1, ["cov.tsv"]),
            "linkage_planted": (2, ["hap.tsv", "linkage.tsv", "pairs.tsv"]), "linkage_clean": (0, ["hap.tsv", "linkage.tsv", "pairs.tsv"]),
            "linkage_sites_missing": (1, []), "linkage_fraction": (1, []),
            "align_four": (0, ["out.paf", "summary.tsv"]), "align_two_records": (1, []),
            "pseudopair_thrice": (0, ["pairs.txt"]), "pseudopair_short_line": (1, []), "dropin_missing_read": (1, [])}
    assert sorted(want) == sorted(cc.CPU_CASES)
    for name, (status, files) in want.items():
        t = cc.load(name)
        assert (t["exit"], sorted(t["files"])) == (status, files), name
        assert (t["stderr"].startswith("Error: ") and t["stderr"].count("\n") == 1) == (status == 1), name
    assert "region\t5:35\n" in cc.load("coverage_expected")["files"]["cov.tsv"]  # the core, on the target of the adapted length
    assert "region\t0:30\n" in cc.load("coverage_expected")["files"]["cov.tsv"]
    assert cc.load("align_four")["files"]["summary.tsv"].split() == [
        "reads", "4", "mapped", "2", "plus", "1", "minus", "1", "unmapped_by_distance", "1", "unmapped_no_match", "0",
        "skipped_length", "1"]
    assert cc.load("pseudopair_thrice")["files"]["pairs.txt"] == "f1 r1\n"
