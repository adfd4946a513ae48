"""ASan + UBSan build of the host half of draft_assembly (csrc/draft.cpp, with
csrc/align.cpp and csrc/verify.cpp for scan, plan and trace): a driver
executable (tests/native/draft_driver.cpp) built with
-fsanitize=address,undefined and no recovery runs one round over the planted
reads -- in one launch and cut into many -- and the call on the injected
tallies.  Any sanitizer report, a leak included, fails the run (non-zero exit);
what it prints must equal what the checker of tests/draft_util.py says (CPU
only, no HIP; nothing is loaded into Python under a sanitizer)."""
import os

import numpy as np
import pytest

import draft_util as du
import native_util as nu


@pytest.fixture(scope="module")
def asan_bin():
    return nu.build("draft_asan", ["draft.cpp", "align.cpp", "verify.cpp", os.path.join(nu.NATIVE, "draft_driver.cpp")],
                    ["-pthread"])


def _run(asan_bin, path):
    return nu.run(asan_bin, [path])


def _call_line(tally, draft):
    new, info = du.call(tally, draft)
    rc = {0: 0, 1: -7, 2: -8}[info[0]]
    return "call %d info %s draft %s\n" % (rc, " ".join(str(v) for v in info), new.decode() if new else "-")


@pytest.fixture(scope="module")
def planted(pkg):
    target, noted = du.vote_reads()
    reads = [r for _, r in noted]
    launches, pl = du.traced(pkg, target, reads, "cpu")
    tally = du.vote(len(target), du.checker_reads(launches[0]))
    lines = ["w %d %d %d\n" % (j, w, tally[j, w]) for j, w in zip(*np.nonzero(tally))]
    return target, reads, len(launches[0][1]), "".join(lines) + _call_line(tally, target)


@pytest.mark.parametrize("budget, launches", [(1 << 40, "1"), (0, "many")])
def test_round_sanitized(asan_bin, planted, tmp_path, budget, launches):
    target, reads, voted, want = planted
    path = str(tmp_path / "cases.txt")
    with open(path, "wb") as f:
        f.write(b"T %s\n" % target + b"".join(b"R %s\n" % r for r in reads) + b"E %d\n" % budget)
    head, rest = _run(asan_bin, path).split("\n", 1)
    words = head.split()
    assert words[:2] == ["round", "launches"] and words[3:] == ["voted", str(voted)]
    assert words[2] == "1" if launches == "1" else int(words[2]) >= 3
    assert rest == want


def test_calls_sanitized(asan_bin, tmp_path):
    cases = du.call_cases()
    path = str(tmp_path / "cases.txt")
    with open(path, "wb") as f:
        for note, draft, tally, _ in cases:
            rows, words = np.nonzero(tally)
            f.write(b"C %s %d\n" % (draft, len(rows)))
            f.write(b"".join(b"%d %d %d\n" % (j, w, tally[j, w]) for j, w in zip(rows, words)))
    assert _run(asan_bin, path) == "".join(_call_line(t, d) for _, d, t, _ in cases)
