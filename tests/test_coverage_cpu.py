"""coverage_qc on the host: mpc_coverage_host against the independent checker
(tests/cov_util.py) on Synth samples and hand-written records, one malformed
batch per grammar rule, the PAF ingest and its errors, the CLI with --device
cpu, and an ASan + UBSan build of coverage.cpp behind a stand-alone driver."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cov_util as cu
import glue_cases as gc
import native_util as nu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "minion-plasmid-consensus_amd", "coverage_qc.py")


@pytest.fixture(scope="module")
def synth(pkg):
    records, lengths, regions, samples = cu.synth_batch(pkg)
    return records, lengths, regions, samples, cu.check(records, lengths, regions, min_depth=295)


def test_synth_batch_is_inside_the_contract(synth):
    records, lengths, _, _, (status, rows, _, _) = synth
    assert status == (cu.OK, 0) and len(records) == 1200 and len(lengths) == 4
    assert all(cu.tokens(cs) is not None and ts >= 0 for _, ts, cs in records)
    assert max(len(cs) for _, _, cs in records) > 256  # longer than a kernel tile
    assert rows[:, 1].any() and rows[:, 2].any() and rows[:, 3].any()


def test_host_equals_checker_on_synth(pkg, synth):
    records, lengths, regions, _, (_, rows, stats, _) = synth
    for threads in (1, 5):
        cs, off, ts, rs = cu.pack(records)
        res = pkg.coverage.run(cs, off, ts, rs, lengths, regions, 295, device="cpu", threads=threads)
        assert np.array_equal(res["rows"], rows)
        assert np.array_equal(res["stats"], stats)
    assert (stats[:, 13:] == 0).all() and (stats[:, 11] > 0).any()
    for s, L in enumerate(lengths):  # row L: insertions only
        assert not rows[sum(lengths[:s]) + s + L, :3].any()


def test_walk_end_and_aligned_per_record(pkg, synth):
    records, lengths, regions, samples, (_, _, _, ends) = synth
    cs, off, ts, rs = cu.pack(records)
    tend = np.concatenate([s["tend"] for s in samples])
    aligned = np.concatenate([s["aligned"] for s in samples])
    res = pkg.coverage.run(cs, off, ts, rs, lengths, regions, 0, device="cpu", tend=tend)
    assert np.array_equal(res["rec_out"][:, 0], tend) and list(tend) == ends
    assert np.array_equal(res["rec_out"][:, 1], aligned)
    wrong = tend.copy()
    wrong[77] += 1
    with pytest.raises(pkg.coverage.CoverageError, match="record 77"):
        pkg.coverage.run(cs, off, ts, rs, lengths, regions, 0, device="cpu", tend=wrong)


HAND = [  # (sample, tstart, cs) on lengths (20, 7)
    (0, 3, b""), (0, 0, b"Z:"), (1, 7, b"Z:"), (0, 5, b":0"), (0, 0, b"Z::0:0+a:0"),
    (0, 2, b":3+ac+g+ttt:2"),            # consecutive insertions: three events at one p
    (1, 0, b"Z::7+acg"),                 # an insertion at p = L
    (1, 1, b":1*ag-ctga"),               # a deletion ending at L
    (0, 0, b":000000020"),               # nine digits
    (0, 19, b"*tc"), (0, 0, b"-a+c*gt"), (1, 6, b"+A-C"), (0, 0, b"Z::19*ac+t"),
]


def test_hand_written_records(pkg):
    lengths, regions = [20, 7], [(1, 19), (0, 7)]
    status, rows, stats, ends = cu.check(HAND, lengths, regions, min_depth=2)
    assert status == (cu.OK, 0)
    got_rows, got_stats = cu.run(pkg, HAND, lengths, regions, min_depth=2)
    assert np.array_equal(got_rows, rows) and np.array_equal(got_stats, stats)
    assert rows[2 + 3, 3] == 3 and stats[0, 3] >= 3      # the consecutive insertions
    assert rows[21 + 7, 3] == 1 and rows[21 + 7, :3].sum() == 0  # the insertion at L of sample 1
    for k, rec in enumerate(HAND):  # every record alone, too
        s = rec[0]
        _, r1, s1, _ = cu.check([(0,) + rec[1:]], [lengths[s]], [regions[s]])
        g1, gs1 = cu.run(pkg, [(0,) + rec[1:]], [lengths[s]], [regions[s]])
        assert np.array_equal(g1, r1) and np.array_equal(gs1, s1), k


BAD, GOOD = cu.BAD, cu.GOOD


@pytest.mark.parametrize("name,rec,code", BAD, ids=[b[0] for b in BAD])
def test_one_bad_record_per_rule(pkg, name, rec, code):
    batch = GOOD + [rec] + GOOD
    assert cu.check(batch, [20], [(0, 20)])[0] == (code, 3)
    assert cu.status_of(pkg, batch, [20]) == (code, 3)


def test_smaller_bad_index_wins(pkg):
    batch = GOOD * 3 + [(0, 10, b":11")] + GOOD * 5 + [(0, 0, b"=A")] + GOOD
    assert cu.status_of(pkg, batch, [20]) == (cu.RANGE, 9)
    batch[4] = (0, 0, b":1_0")
    assert cu.status_of(pkg, batch, [20]) == (cu.MALFORMED, 4)


def test_sample_index_outside_the_targets(pkg):
    cu.case_bad_sample(pkg, "cpu")


def test_abi_argument_checks(pkg):
    L = pkg.coverage.host_lib()
    z = np.zeros(64, np.int64)
    p = z.ctypes.data
    assert L.mpc_coverage_host(p, p, p, p, -1, p, p, 1, 0, p, p, p, 1, None) == -1
    assert b"n_records" in L.mpc_coverage_last_error()
    assert L.mpc_coverage_host(p, p, p, p, 0, p, p, 0, 0, p, p, p, 1, None) == -1
    assert b"n_samples" in L.mpc_coverage_last_error()
    with pytest.raises(pkg.coverage.CoverageError, match="region"):
        cu.run(pkg, GOOD, [20], [(3, 21)])


# ---------------------------------------------------------------- ingest

@pytest.fixture(scope="module")
def paf_files(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("cov")
    syn = pkg.synth.Synth(n=600, n_reads=300, profile="indel", seed=4)
    paths = [str(d / "sense.paf"), str(d / "antisense.paf")]
    syn.write_files(paf0=paths[0], paf1=paths[1])
    return paths, [syn.sample(0), syn.sample(1)]


def test_ingest_reads_synth_pafs(pkg, paf_files):
    paths, samples = paf_files
    for path, smp, name in zip(paths, samples, ("tig00000001", "tig00000001_revcomp")):
        for threads in (1, 3):
            d = pkg.coverage.read_paf(path, threads=threads)
            assert d["names"] == [name] and d["lengths"] == [600] and d["n_lines"] == 300
            for k in ("tstart", "tend", "cs_off"):
                assert np.array_equal(d[k], smp[k]), k
            assert np.array_equal(d["cs"], smp["cs"]) and not d["target"].any()
            assert set(d["strand"].tolist()) == {ord("+"), ord("-")} and (d["mapq"] == 60).all() and (d["qlen"] > 0).all()


def _lines(path):
    with open(path, "rb") as f:
        return f.read().split(b"\n")[:-1]


def test_ingest_duplicate_read_name(pkg, paf_files, tmp_path):
    lines = _lines(paf_files[0][0])[:6]
    dup = tmp_path / "dup.paf"
    dup.write_bytes(b"\n".join(lines[:3] + [lines[1]] + lines[3:]) + b"\n")
    first, every = pkg.coverage.read_paf(str(dup), 0), pkg.coverage.read_paf(str(dup), 1)
    assert len(first["tstart"]) == 6 and len(every["tstart"]) == 7 and first["n_lines"] == every["n_lines"] == 7
    assert np.array_equal(every["tstart"][[0, 1, 2, 4, 5, 6]], first["tstart"]) and every["tstart"][3] == every["tstart"][1]


def test_ingest_errors_name_the_line(pkg, paf_files, tmp_path):
    lines = _lines(paf_files[0][0])[:5]
    col = lines[2].split(b"\t")
    cases = {
        "fewer than 12 columns": b"\t".join(col[:11]),
        "no cs: field": b"\t".join(col[:13]),
        "not plain digits": b"\t".join(col[:7] + [b"+" + col[7]] + col[8:]),
        "has lengths 600 and 601": b"\t".join(col[:6] + [b"601"] + col[7:]),
        "strand": b"\t".join(col[:4] + [b"*"] + col[5:]),
    }
    for why, line in cases.items():
        bad = tmp_path / "bad.paf"
        bad.write_bytes(b"\n".join(lines[:2] + [line] + lines[3:]) + b"\n")
        with pytest.raises(pkg.coverage.CoverageError, match="line 3: .*" + why):
            pkg.coverage.read_paf(str(bad))
    with pytest.raises(pkg.coverage.CoverageError, match="cannot be read"):
        pkg.coverage.read_paf(str(tmp_path / "missing.paf"))
    empty = tmp_path / "empty.paf"
    empty.write_bytes(b"")
    assert pkg.coverage.read_paf(str(empty))["names"] == []


@pytest.mark.parametrize("name", sorted(gc.PAF_FILES))
def test_ingest_thread_cuts(pkg, name, tmp_path):
    """1 thread and 16 threads (cuts at other line starts, several of them inside
    one long line) read the same records."""
    text = gc.PAF_FILES[name]
    path = tmp_path / "in.paf"
    path.write_text(text)
    lines = [ln.split("\t") for ln in text.split("\n") if ln]
    one, many = (pkg.coverage.read_paf(str(path), 1, threads=t) for t in (1, 16))
    for d in (one, many):
        assert d["n_lines"] == len(lines) and d["tstart"].tolist() == [int(c[7]) for c in lines]
        assert d["cs"].tobytes()[:int(d["cs_off"][-1])].decode() == "".join(c[13][3:] for c in lines)
        assert d["cs_off"].tolist() == np.cumsum([0] + [len(c[13]) - 3 for c in lines]).tolist()
        assert d["names"] == (["ref"] if lines else []) and bytes(d["strand"]).decode() == "".join(c[4] for c in lines)
    for k in ("target", "tend", "qlen", "mapq", "lengths"):
        assert np.array_equal(one[k], many[k]), k


@pytest.mark.parametrize("field", sorted(gc.PLAIN_INT))
def test_plain_int_policy(pkg, field, tmp_path):
    """An integer column is 1-18 digits and nothing else."""
    path = tmp_path / "in.paf"
    path.write_text(gc.paf_line("a", 12, 1, 11, "+", field, ":10"))
    if gc.PLAIN_INT[field][1]:
        assert pkg.coverage.read_paf(str(path))["tstart"].tolist() == [int(field)]
    else:
        with pytest.raises(pkg.coverage.CoverageError, match="line 1: an integer column is not plain digits"):
            pkg.coverage.read_paf(str(path))


# ---------------------------------------------------------------- CLI

def _cli(*args):
    return subprocess.run([sys.executable, CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_cpu_report_and_verdict(pkg, paf_files, tmp_path):
    paths, samples = paf_files
    records = [(s, int(smp["tstart"][r]), smp["cs"].tobytes()[smp["cs_off"][r]:smp["cs_off"][r + 1]])
               for s, smp in enumerate(samples) for r in range(300)]
    _, rows, stats, _ = cu.check(records, [600, 600], [(50, 550)] * 2, min_depth=0)
    means = [int(stats[s, 7]) / 500 for s in (0, 1)]
    rep, per = tmp_path / "cov.tsv", tmp_path / "depth.tsv"
    common = ["--paf"] + paths + ["--region", "50:550", "--device", "cpu", "--report", rep]
    p = _cli(*common, "--per-base", per, "--min-mean-coverage", repr(min(means) - 0.001))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = rep.read_text().splitlines()
    keys = importlib.import_module(pkg.__name__ + ".coverage_qc").REPORT_KEYS
    assert len(keys) == 23 and [ln.split("\t")[0] for ln in lines[:-1]] == list(keys) * 2
    assert lines[-1] == "verdict\tPASS" and len(lines) == 2 * 23 + 1
    for s in (0, 1):
        blk = dict(ln.split("\t") for ln in lines[23 * s:23 * (s + 1)])
        assert list(blk)[:5] == ["paf", "target", "length", "records", "region"]
        assert blk["paf"] == paths[s] and blk["records"] == "300" and blk["region"] == "50:550" and blk["length"] == "600"
        assert blk["mean_depth"] == repr(means[s])
        n, sm, sq = 500, int(stats[s, 7]), int(stats[s, 8])
        assert blk["sd_depth"] == repr(((n * sq - sm * sm) / (n * n)) ** 0.5)
        d = rows[601 * s + 50:601 * s + 550, 0]
        assert blk["min_depth"] == str(d.min()) and blk["min_depth_position"] == str(50 + int(np.argmin(d)) + 1)
        assert blk["max_depth"] == str(d.max()) and blk["positions_below_min_depth"] == "0"
        err = int(stats[s, 2]) + int(stats[s, 4]) + int(stats[s, 6])
        assert blk["error_rate"] == repr(err / (int(stats[s, 1]) + err))
        assert [blk[k] for k in ("match_bases", "mismatch_bases", "inserted_bases", "deleted_bases", "insertion_events",
                                 "deletion_events")] == [str(int(stats[s, k])) for k in (1, 2, 4, 6, 3, 5)]
        assert blk["mean_mapq"] == "60.0" and int(blk["plus_strand_records"]) + int(blk["minus_strand_records"]) == 300
    pb = per.read_text().splitlines()
    assert pb[0].split("\t") == ["paf", "target", "pos", "depth", "deleted", "mismatch", "insertion"] and len(pb) == 1 + 2 * 601
    assert pb[1 + 601 + 10].split("\t") == [paths[1], "tig00000001_revcomp", "11"] + [str(x) for x in rows[601 + 10]]
    first = rep.read_bytes()
    # just above the smaller mean: FAIL, exit 0 without --strict, 2 with it
    p = _cli(*common, "--min-mean-coverage", repr(min(means) + 0.001))
    assert p.returncode == 0 and rep.read_text().splitlines()[-1] == "verdict\tFAIL"
    assert rep.read_bytes()[:-5] == first[:-5]
    assert _cli(*common, "--min-mean-coverage", repr(min(means) + 0.001), "--strict").returncode == 2
    # a position below --min-depth fails the verdict whatever the mean
    p = _cli(*common, "--min-mean-coverage", "1", "--min-depth", int(rows[50:550, 0].min()) + 1)
    assert p.returncode == 0 and rep.read_text().splitlines()[-1] == "verdict\tFAIL"


def test_cli_invalid_input_writes_nothing(paf_files, tmp_path):
    rep = tmp_path / "none.tsv"
    p = _cli("--paf", tmp_path / "missing.paf", "--device", "cpu", "--report", rep)
    assert p.returncode == 1 and not rep.exists() and "cannot be read" in p.stderr
    lines = _lines(paf_files[0][0])[:4]
    bad = tmp_path / "badcs.paf"
    bad.write_bytes(b"\n".join(lines[:3] + [lines[3].replace(b"cs:Z::", b"cs:Z:=")]) + b"\n")
    p = _cli("--paf", bad, "--device", "cpu", "--report", rep)
    assert p.returncode == 1 and not rep.exists() and "record 3: malformed cs" in p.stderr


def test_cli_expected_restricts_to_the_core(pkg, paf_files, tmp_path):
    exp = tmp_path / "x_adapted.fasta"
    exp.write_bytes(b">x\n" + b"acgt" * 10 + b"ACGT" * 130 + b"tgca" * 10 + b"\n")  # 40 + 520 + 40 = 600
    rep = tmp_path / "cov.tsv"
    p = _cli("--paf", paf_files[0][0], "--expected", exp, "--device", "cpu", "--report", rep, "--min-mean-coverage", 1)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "region\t40:560" in rep.read_text().splitlines()


# ---------------------------------------------------------------- the region rule of coverage.qc and linkage.qc

@pytest.mark.parametrize("err", ["coverage.CoverageError", "linkage.LinkageError"])
def test_target_regions(pkg, err, tmp_path):
    mod, cls = err.split(".")
    err = getattr(getattr(pkg, mod), cls)
    names, lengths = ["a", "b", "c"], [600, 599, 601]
    regions = lambda core, region: pkg.coverage.target_regions("x.paf", names, lengths, core, region, err)
    assert regions(None, None) == [(0, 600), (0, 599), (0, 601)]              # the whole target by default
    assert regions(None, (5, 90)) == [(5, 90)] * 3                            # --region, for every target
    assert regions((600, 40, 560), None) == [(40, 560), (0, 599), (0, 601)]   # the core only at equal length
    assert regions((600, 40, 560), (5, 90)) == [(40, 560), (5, 90), (5, 90)]  # (the CLI excludes the two; the API does not)
    assert regions((7, 1, 2), (0, 599)) == [(0, 599)] * 3 and regions(None, (599, 599)) == [(599, 599)] * 3
    for region, name, L in (((-1, 5), "a", 600), ((7, 6), "a", 600), ((5, 600), "b", 599)):  # lo < 0, lo > hi, hi > L
        with pytest.raises(err) as e:
            regions(None, region)
        assert str(e.value) == "x.paf: target {}: region {}:{} is outside 0:{}".format(name, region[0], region[1], L)
    with pytest.raises(err) as e:  # a core outside a target of its length is refused like a region
        regions((601, 5, 602), None)
    assert str(e.value) == "x.paf: target c: region 5:602 is outside 0:601"
    # expected_core: None without a file, (adapted length, c0, c1), and verify's refusal under the caller's class
    exp = tmp_path / "x.fasta"
    exp.write_bytes(b">x\nacgtGGTTACac\n")
    assert pkg.coverage.expected_core(None, err) is None and pkg.coverage.expected_core(str(exp), err) == (12, 4, 10)
    exp.write_bytes(b">x\nacgt\n")
    with pytest.raises(pkg.verify.VerifyError) as plain:
        pkg.verify.read_expected(str(exp))
    with pytest.raises(err) as e:
        pkg.coverage.expected_core(str(exp), err)
    assert str(e.value) == str(plain.value) and type(e.value) is err


# ---------------------------------------------------------------- sanitizers

DRIVER = r"""
// Stand-alone driver: PAF ingest (both modes) + mpc_coverage_host on what it read,
// then a malformed and an out-of-range record.  Prints the figures the test compares.
#include <cstdio>
#include <cstring>
#include <vector>
#include "mpc_coverage.h"
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  for (int mode = 0; mode < 2; ++mode) {
    mpc_coverage_paf paf;
    if (mpc_coverage_ingest(argv[1], mode, 3, &paf) != 0) { printf("ingest: %s\n", paf.message); return 3; }
    std::vector<int64_t> pos_off(1, 0), region;
    for (int64_t t = 0; t < paf.n_targets; ++t) {
      pos_off.push_back(pos_off.back() + paf.target_len[t] + 1);
      region.push_back(0);
      region.push_back(paf.target_len[t]);
    }
    std::vector<uint32_t> rows((size_t)pos_off.back() * 4);
    std::vector<uint64_t> stats((size_t)paf.n_targets * MPC_COV_STATS);
    std::vector<int64_t> rec((size_t)paf.n_records * 2);
    int32_t status[2];
    for (int threads = 1; threads <= 4; threads += 3) {
      if (mpc_coverage_host(paf.cs, paf.cs_off, paf.tstart, paf.target, paf.n_records, pos_off.data(), region.data(),
                            (int32_t)paf.n_targets, 5, rows.data(), stats.data(), status, threads, rec.data()) != 0) {
        printf("host: %s\n", mpc_coverage_last_error());
        return 4;
      }
      int64_t ends_ok = 0;
      for (int64_t r = 0; r < paf.n_records; ++r) ends_ok += rec[2 * r] == paf.tend[r];
      printf("mode %d threads %d records %lld lines %lld status %d ends_ok %lld stats", mode, threads,
             (long long)paf.n_records, (long long)paf.n_lines, status[0], (long long)ends_ok);
      for (int k = 0; k < 13; ++k) printf(" %llu", (unsigned long long)stats[k]);
      printf("\n");
    }
    mpc_coverage_ingest_free(&paf);
  }
  mpc_coverage_paf paf;
  printf("bad paf %d\n", mpc_coverage_ingest(argv[2], 0, 2, &paf));
  mpc_coverage_ingest_free(&paf);
  const char* cs[] = {":3*ag-c+tt:2", ":4=A", ":9", "", ":1234567890", "*a", ":5-"};
  for (const char* c : cs) {
    const int64_t off[2] = {0, (int64_t)strlen(c)}, ts = 1, pos_off[2] = {0, 9}, region[2] = {0, 8};
    const int32_t smp = 0;
    uint32_t rows[36];
    uint64_t stats[MPC_COV_STATS];
    int32_t status[2];
    mpc_coverage_host((const uint8_t*)c, off, &ts, &smp, 1, pos_off, region, 1, 0, rows, stats, status, 1, nullptr);
    printf("cs %s status %d\n", c, status[0]);
  }
  return 0;
}
"""


def test_host_code_sanitized(pkg, paf_files, tmp_path):
    """ASan + UBSan, no recovery: any report, a leak included, fails the run."""
    drv = tmp_path / "cov_driver.cpp"
    drv.write_text(DRIVER)
    exe = nu.build("cov_asan", ["coverage.cpp", drv], ["-pthread"])
    lines = _lines(paf_files[0][0])
    dup = tmp_path / "dup.paf"
    dup.write_bytes(b"\n".join(lines + [lines[5]]) + b"\n")
    bad = tmp_path / "bad.paf"
    bad.write_bytes(lines[0] + b"\n" + b"\t".join(lines[1].split(b"\t")[:9]))
    out = nu.run(exe, [dup, bad]).splitlines()
    smp = paf_files[1][0]
    records = [(0, int(smp["tstart"][r]), smp["cs"].tobytes()[smp["cs_off"][r]:smp["cs_off"][r + 1]]) for r in range(300)]
    for mode, recs in ((0, records), (1, records + [records[5]])):
        _, _, stats, _ = cu.check(recs, [600], [(0, 600)], min_depth=5)
        want = "records %d lines 301 status 0 ends_ok %d stats %s" % (len(recs), len(recs), " ".join(str(int(x)) for x in stats[0, :13]))
        assert out[2 * mode] == "mode %d threads 1 %s" % (mode, want)
        assert out[2 * mode + 1] == "mode %d threads 4 %s" % (mode, want)
    assert out[4:] == ["bad paf 1", "cs :3*ag-c+tt:2 status 0", "cs :4=A status 1", "cs :9 status 2", "cs  status 0",
                       "cs :1234567890 status 1", "cs *a status 1", "cs :5- status 1"]
