"""ASan + UBSan build of the host half of align_reads (csrc/align.cpp, with
csrc/verify.cpp for the host scan): a driver executable
(tests/native/align_driver.cpp) built with -fsanitize=address,undefined and no
recovery runs the CPU grid's reverse complements, scan, plan, traces and
render, under the default budget and under one that cuts every batch into many
launches.  Any sanitizer report, a leak included, fails the run (non-zero
exit); what it prints must equal what the checker of tests/align_util.py says
(CPU only, no HIP; nothing is loaded into Python under a sanitizer)."""
import os

import pytest

import align_util as au
import native_util as nu


@pytest.fixture(scope="module")
def asan_bin():
    return nu.build("align_asan", ["align.cpp", "verify.cpp", os.path.join(nu.NATIVE, "align_driver.cpp")], ["-pthread"])


def _run(asan_bin, path):
    return nu.run(asan_bin, [path], text=False)


def _case_file(path, batches, budget):
    with open(path, "wb") as f:
        for target, max_error, records in batches:
            f.write(b"T tgt %s\nB %r %d\n" % (target, max_error, budget))
            for name, read in records:
                f.write(b"R %s %s\n" % (name, read))
            f.write(b"E\n")


def _expected(batches, launches):
    out = []
    for k, (target, max_error, records) in enumerate(batches):
        paf, _, per = au.expected_batch(target, b"tgt", records, max_error)
        mapped = sum(1 for e in per if e["mapped"])
        out.append("batch %d launches %d\n" % (k, launches(mapped)))
        for r, e in enumerate(per):
            line = "read %d scan %d %d %d %d plan %d %d %d %d %d" % ((r,) + e["scan"] + (
                e["strand"], int(e["mapped"]), e["d"], e["end"], 2 * e["d"] + 1))
            if e["mapped"]:
                start, cnt, runs = e["trace"]
                line += " out " + " ".join(str(v) for v in [0, start] + cnt + [len(runs), 0])
                line += " runs" + "".join(" %d" % v for v in runs)
            out.append(line + "\n")
        out.append("paf %d\n" % len(paf))
        out.append(paf.decode())
    return "".join(out).encode()


BATCHES = au.batches(au.grid())


def test_grid_sanitized_one_launch(asan_bin, tmp_path):
    path = str(tmp_path / "cases.txt")
    _case_file(path, BATCHES, 1 << 40)
    assert _run(asan_bin, path) == _expected(BATCHES, lambda mapped: 1)


def test_grid_sanitized_many_launches(asan_bin, tmp_path):
    """The budget is the largest single read's need: reads of equal pitch share no launch."""
    # every read of a grid batch has the same length and d <= 31 (one 64-byte pitch) ...
    small = [b for b in BATCHES if all(e is None or e["d"] <= 31 for e in au.expected_batch(b[0], b"tgt", b[2], b[1])[2])]
    assert len(small) >= len(BATCHES) // 2
    path = str(tmp_path / "cases.txt")
    _case_file(path, small, 0)
    # ... so every mapped read is a launch of its own (a batch with none still has its one empty launch)
    assert _run(asan_bin, path) == _expected(small, lambda mapped: max(mapped, 1))


def test_refused_plan_sanitized(asan_bin, tmp_path):
    target, max_error, records = max(BATCHES, key=lambda b: len(b[2]))
    path = str(tmp_path / "cases.txt")
    _case_file(path, [(target, max_error, records)], 63)
    out = _run(asan_bin, path).decode()
    assert out.startswith("batch 0 error mpc_align_plan: read ") and "the workspace budget is 63" in out
