"""draft_assembly on the host: mpc_draft_vote_host and mpc_draft_call_host equal
the plain-Python checker of tests/draft_util.py on the planted reads of one
target and on injected tallies, and the CLI on --device cpu: usage errors, input
it refuses (exit 1, no file), --sample below --candidates, --orient-to.  No GPU."""
import importlib
import os

import numpy as np
import pytest

import align_util as au
import draft_util as du
import verify_util as vu


@pytest.fixture(scope="module")
def dr(pkg):
    return pkg.draft


@pytest.fixture(scope="module")
def planted(pkg):
    target, noted = du.vote_reads()
    launches, pl = du.traced(pkg, target, [r for _, r in noted], "cpu")
    assert len(launches) == 1
    return target, noted, launches[0], pl


def _host_vote(dr, n, launch, threads=3, out=None):
    pk, jobs, o, runs, _, _ = launch
    tally = dr.new_tally(n, "cpu")
    rc, status = dr.vote(tally, n, pk.seq, jobs, o if out is None else out, runs, "cpu", threads)
    return rc, status, tally


def test_the_planted_reads_are_what_they_are_meant_to_be(planted):
    target, noted, (pk, jobs, out, runs, _, rd), pl = planted
    notes = [noted[r][0] for r in rd]
    assert [n for n, _ in noted if n not in notes] == ["unmapped"]
    assert sorted(set(pl[rd, 0].tolist())) == [0, 1]  # both strands
    by = {n: k for k, n in enumerate(notes)}
    assert out[by["subs 70"], 6] > 128 and out[by["subs 70"], 3] == 70
    for ln in (1, 8, 9, 20):
        k = by["insertion %d" % ln]
        assert (ln << 2 | 3) in runs[jobs[k, 7]: jobs[k, 7] + out[k, 6]].tolist()
    k = by["ends not '='"]
    own = runs[jobs[k, 7]: jobs[k, 7] + out[k, 6]]
    assert own[0] & 3 != 0 and own[-1] & 3 != 0
    assert out[by["from column 0"], 1] == 0 and jobs[by["to column n"], 5] == len(target)
    assert out[by["deletions"], 4] == 16 and jobs[by["one base"], 1] == 1


def test_host_vote_equals_the_checker(dr, planted):
    target, noted, launch, _ = planted
    n = len(target)
    want = du.vote(n, du.checker_reads(launch))
    assert want[:, du.STARTS].sum() == len(launch[1]) == want[:, du.ENDS].sum()
    for threads in (1, 3):
        rc, status, tally = _host_vote(dr, n, launch, threads)
        assert rc == 0 and not status.any()
        assert np.array_equal(tally, want)
    unused = [w for w in range(du.ROW) if w not in (0, 1, 2, 3, 4, 5) and not 8 <= w < 12 and not 16 <= w < 48]
    assert not want[:, unused].any()


def test_host_vote_of_runs_that_leave_the_target(dr, planted):
    target, noted, launch, _ = planted
    pk, jobs, out, runs, _, rd = launch
    n = len(target)
    k = [noted[r][0] for r in rd].index("to column n")
    wrong = out.copy()
    wrong[k, 1] += 1  # the runs now walk to column n + 1
    rc, status, tally = _host_vote(dr, n, launch, out=wrong)
    assert rc == dr.E_RUNS and status.tolist() == [int(x == k) for x in range(len(jobs))]
    assert np.array_equal(tally, du.vote(n, du.checker_reads(launch, skip=(k,))))
    wrong[k, 6] = 2 * jobs[k, 4] + 2  # more runs than the read's capacity: refused before anything is added
    with pytest.raises(dr.DraftError, match="mpc_draft_vote_host: read %d" % k):
        _host_vote(dr, n, launch, out=wrong)


def test_host_call_equals_the_checker_on_the_votes(dr, planted):
    target, _, launch, _ = planted
    rc, _, tally = _host_vote(dr, len(target), launch)
    new, info = dr.call(tally, target, "cpu")
    want, winfo = du.call(tally, target)
    assert (new, [info[k] for k in dr.INFO_FIELDS]) == (want, winfo)
    assert new == target[info["lo"]:info["hi"]] and info["changed"] == info["dropped"] == info["inserted"] == 0


@pytest.mark.parametrize("case", du.call_cases(), ids=lambda c: c[0])
def test_host_call_on_injected_tallies(dr, case):
    note, draft, tally, expected = case
    want, winfo = du.call(tally, draft)
    if expected is not None or want is None:
        assert want == expected
    if want is None:
        with pytest.raises(dr.DraftError, match="no read mapped"):
            dr.call(tally, draft, "cpu")
        return
    new, info = dr.call(tally, draft, "cpu")
    assert (new, [info[k] for k in dr.INFO_FIELDS]) == (want, winfo)


def test_the_seeded_call_cases_move_the_offsets():
    cases = {c[0]: c for c in du.call_cases()}
    _, draft, tally, _ = cases["offsets move"]
    new, info = du.call(tally, draft)
    assert info[6] > 100 and info[7] > 8 * 100 and info[5] > 10
    _, draft, tally, _ = cases["random n 2049"]
    assert du.call(tally, draft)[1][2] > 0 and du.call(tally, draft)[1][3] < 2049  # trimmed at both ends


def test_a_draft_too_long_is_refused(dr):
    n = 20000
    draft = b"A" * n
    t = du.tallies_of(np.full(n, 2), np.full(n, 2), np.zeros(n, np.int64))
    for s in range(du.SLOTS):
        t[:, du.INS + 4 * s + 1] = 2
    with pytest.raises(dr.DraftError, match="at most 131072"):
        dr.call(t.astype(np.uint32), draft, "cpu")


# ---- the CLI ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module(pkg.__name__ + ".draft_assembly")


@pytest.fixture(scope="module")
def small(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("draft")
    syn = pkg.synth.Synth(n=300, n_reads=40, seed=3)
    ref_fa, reads_fa = str(d / "ref.fa"), str(d / "reads.fa")
    syn.write_files(ref_fa, reads_fa)
    return ref_fa, reads_fa, pkg.verify.read_consensus(ref_fa)


def _run(cli, tmp_path, reads, *more):
    sense, anti, rep = (str(tmp_path / x) for x in ("s.fa", "a.fa", "rep.tsv"))
    rc = cli.main(["--reads", reads, "--sense", sense, "--antisense", anti, "--report", rep, "--device", "cpu"] + list(more))
    return rc, sense, anti, rep


def _seq(path, header):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[0] == header and lines[2:] == [b""]
    return lines[1]


@pytest.mark.parametrize("argv", [[], ["--reads", "x", "--sense", "s"], ["--sample", "-1"], ["--candidates", "0"],
                                  ["--rounds", "x"], ["--max-error", "-0.1"], ["--device", "gpu"], ["--threads", "-2"]])
def test_cli_usage_errors(cli, argv, tmp_path, capsys):
    full = argv if len(argv) != 2 else ["--reads", "r.fa", "--sense", str(tmp_path / "s"), "--antisense", str(tmp_path / "a")] + argv
    with pytest.raises(SystemExit) as e:
        cli.main(full)
    assert e.value.code == 2 and "usage:" in capsys.readouterr().err
    assert os.listdir(tmp_path) == []


def test_cli_refuses_input_without_a_usable_read(cli, tmp_path, capsys):
    empty, skipped, bad = (str(tmp_path / x) for x in ("empty.fa", "skipped.fa", "bad.fa"))
    open(empty, "w").close()
    with open(skipped, "w") as f:
        f.write(">none\n>long\n%s\n" % ("ACGT" * 16385))
    with open(bad, "w") as f:
        f.write(">r\nAC-GT\n")
    before = sorted(os.listdir(tmp_path))
    for path, text in ((empty, "no read of 1 .. 65536 bases (0 skipped"), (skipped, "(2 skipped by length)"),
                       (bad, "ASCII letters only"), (str(tmp_path / "missing.fa"), "missing.fa")):
        rc, _, _, _ = _run(cli, tmp_path, path)
        err = capsys.readouterr().err
        assert rc == 1 and err.startswith("Error: ") and text in err and err.count("\n") == 1
        assert sorted(os.listdir(tmp_path)) == before


def test_cli_draft_holds_the_plasmid(cli, small, tmp_path):
    ref_fa, reads_fa, ref = small
    rc, sense, anti, rep = _run(cli, tmp_path, reads_fa, "--candidates", "4")
    assert rc == 0
    s, a = _seq(sense, b">draft_sense"), _seq(anti, b">draft_antisense")
    assert a == au.revcomp(s) and len(s) <= len(ref) + 80
    core = ref[50:-50].upper()
    assert min(vu.score(core, s)[0], vu.score(core, a)[0]) == 0
    report = dict(ln.split("\t") for ln in open(rep).read().splitlines())
    assert report["sample_reads"] == "40" and report["skipped_length"] == "0" and report["candidates"] == "4"
    assert report["round1_mapped"] == "40" and int(report["seed_length"]) >= 300 and report["converged"] in ("yes", "no")
    last = max(int(k[5]) for k in report if k.startswith("round"))
    assert int(report["round%d_length" % last]) == len(s)
    assert (report["converged"] == "yes") == all(
        report["round%d_%s" % (last, k)] == "0" for k in ("trim_head", "trim_tail", "changed", "dropped", "inserted"))


def test_cli_sample_below_candidates(cli, small, tmp_path):
    ref_fa, reads_fa, ref = small
    rc, sense, anti, rep = _run(cli, tmp_path, reads_fa, "--sample", "3", "--rounds", "1")
    assert rc == 0
    report = dict(ln.split("\t") for ln in open(rep).read().splitlines())
    assert report["sample_reads"] == "3" and report["candidates"] == "3" and "round2_mapped" not in report
    assert len(_seq(sense, b">draft_sense")) >= 250


def test_cli_orient_to(cli, small, tmp_path):
    ref_fa, reads_fa, ref = small
    rc_fa = str(tmp_path / "ref_rc.fa")
    with open(rc_fa, "wb") as f:
        f.write(b">rc\n" + au.revcomp(ref).lower() + b"\n")
    got = {}
    for name, fa in (("fwd", ref_fa), ("rev", rc_fa)):
        d = tmp_path / name
        d.mkdir()
        rc, sense, anti, _ = _run(cli, d, reads_fa, "--candidates", "4", "--orient-to", fa)
        assert rc == 0
        got[name] = (_seq(sense, b">draft_sense"), _seq(anti, b">draft_antisense"))
    assert got["fwd"] == got["rev"][::-1]
    core = ref[50:-50].upper()
    assert vu.score(core, got["fwd"][0])[0] == 0 and vu.score(au.revcomp(core), got["rev"][0])[0] == 0
    two = str(tmp_path / "two.fa")
    with open(two, "w") as f:
        f.write(">a\nACGT\n>b\nACGT\n")
    assert _run(cli, tmp_path, reads_fa, "--orient-to", two)[0] == 1
    assert not os.path.exists(str(tmp_path / "s.fa"))
