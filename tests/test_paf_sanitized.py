"""ASan + UBSan build of the PAF readers that share csrc/host_file.h with the
ingest (csrc/coverage.cpp, csrc/pseudopair.cpp): a driver executable
(tests/native/paf_driver.cpp) built with -fsanitize=address,undefined and no
recovery runs mpc_coverage_ingest / _free and mpc_pseudopair with 1 and with 16
threads on the files of tests/glue_cases.py (empty, one line with and without
its newline, fewer lines than threads, one line that spans several thread
cuts) and on a missing file.  Any sanitizer report, a leak included, fails the
run (non-zero exit); what it prints must equal what the Python restatement and
the files' own text say (CPU only, no HIP; nothing is loaded into Python under
a sanitizer)."""
import importlib
import os

import pytest

import glue_cases as gc
import native_util as nu


@pytest.fixture(scope="module")
def asan_bin():
    return nu.build("paf_asan", ["coverage.cpp", "pseudopair.cpp", os.path.join(nu.NATIVE, "paf_driver.cpp")], ["-pthread"])


def test_paf_readers_sanitized(asan_bin, tmp_path):
    pp = importlib.import_module("minion-plasmid-consensus_amd.pseudopair_reads")
    paths = gc.write_paf_files(tmp_path)
    names = sorted(paths)
    missing = str(tmp_path / "missing.paf")
    got = nu.run(asan_bin, [tmp_path / "pairs.txt"] + [paths[n] for n in names] + [missing])
    want = []
    for i, name in enumerate(names):
        lines = [ln.split("\t") for ln in gc.PAF_FILES[name].split("\n") if ln]
        pairs, nf, nr, nfk, nrk = pp.pseudopair_python(paths[name], 7)
        for threads in (1, 16):
            want.append("cov %d threads %d rc 0 records %d lines %d targets %d cs_sum %d message " % (
                i, threads, len(lines), len(lines), 1 if lines else 0, sum(sum(c[13][3:].encode()) for c in lines)))
            want.append("pp %d threads %d rc 0 fwd %d rev %d kept %d %d pairs %d message " % (i, threads, nf, nr, nfk, nrk,
                                                                                             len(pairs)))
    for threads in (1, 16):
        want.append("cov %d threads %d rc 1 records 0 lines 0 targets 0 cs_sum 0 message %s: cannot be read" % (
            len(names), threads, missing))
        want.append("pp %d threads %d rc 1 fwd 0 rev 0 kept 0 0 pairs 0 message cannot open %s" % (len(names), threads, missing))
    assert got.splitlines() == want
