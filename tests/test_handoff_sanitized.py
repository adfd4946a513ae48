"""ASan + UBSan build of the handoff's host twins (csrc/align.cpp): a driver
executable (tests/native/handoff_driver.cpp) built with
-fsanitize=address,undefined and no recovery sizes, places and writes every
launch of the CPU tests' case batches into buffers of exactly the bytes needed,
and asks again with each buffer one byte short.  Any sanitizer report, a leak
included, fails the run (non-zero exit); what it prints must equal what the
library gives in tests/test_handoff_cpu.py (CPU only, no HIP; nothing is
loaded into Python under a sanitizer)."""
import os

import numpy as np
import pytest

import handoff_util as hu
import native_util as nu


@pytest.fixture(scope="module")
def asan_bin():
    return nu.build("handoff_asan", ["align.cpp", os.path.join(nu.NATIVE, "handoff_driver.cpp")], ["-pthread"])


def _ints(a):
    return " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))


def test_case_batches_sanitized(pkg, asan_bin, tmp_path):
    lns = [ln for _, group in hu.all_launches() for ln in group if len(ln.jobs)]
    assert len(lns) >= 15
    path = str(tmp_path / "cases.txt")
    want = []
    with open(path, "w") as f:
        for k, ln in enumerate(lns):
            f.write("L %d %d %d\n%s\n%s\n%s\n%s\n" % (ln.seq.nbytes, len(ln.jobs), len(ln.runs), bytes(ln.seq).hex(),
                                                  _ints(ln.jobs), _ints(ln.out), _ints(ln.runs)))
            z = pkg.handoff.cs_sizes(ln.jobs, ln.out, ln.runs, ln.seq.nbytes, "cpu")
            place, ends = pkg.handoff.places(z)
            bufs = [np.zeros(e, np.uint8) for e in ends]
            pkg.handoff.cs_write(ln.seq, ln.jobs, ln.out, ln.runs, z, place, *bufs, device="cpu")
            want.append("launch %d sizes %s\n" % (k, _ints(z)) +
                        "".join("%s %s\n" % (name, bytes(b).hex()) for name, b in zip(("cs", "up", "down"), bufs)))
    assert nu.run(asan_bin, [path]) == "".join(want)


def test_refused_tables_sanitized(asan_bin, tmp_path):
    """Runs that do not walk the read, and a run span past the run buffer: refused by name, nothing read past an end."""
    (ln,) = dict(hu.all_launches())["end rule"]
    path = str(tmp_path / "cases.txt")
    bad_runs = ln.runs.copy()
    bad_runs[ln.jobs[2, 7]] += 1 << 2
    bad_jobs = ln.jobs.copy()
    bad_jobs[4, 7] = len(ln.runs)
    with open(path, "w") as f:
        for jobs, runs in ((ln.jobs, bad_runs), (bad_jobs, ln.runs)):
            f.write("L %d %d %d\n%s\n%s\n%s\n%s\n" % (ln.seq.nbytes, len(jobs), len(runs), bytes(ln.seq).hex(), _ints(jobs),
                                                  _ints(ln.out), _ints(runs)))
    assert nu.run(asan_bin, [path]).splitlines() == [
        "launch 0 error mpc_align_cs_sizes_host: read 2: runs do not span the read",
        "launch 1 error mpc_align_cs_sizes_host: read 4: runs outside the run buffer"]
