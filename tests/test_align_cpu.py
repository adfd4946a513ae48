"""align_reads on the host (no GPU): mpc_align_plan, mpc_align_trace_host and
mpc_align_render against the checker of tests/align_util.py (the definition of
include/mpc_align.h over a numpy full matrix), the plan's launch cuts, the CLI's
rejected inputs, and the whole chain reads -> PAF -> consensus on synthetic
sets.  Every comparison is exact equality."""
import importlib
import os

import numpy as np
import pytest

import align_util as au
import oracle
import verify_util as vu


@pytest.fixture(scope="module")
def al(pkg):
    return pkg.align


@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module(pkg.__name__ + ".align_reads")


GRID = au.grid()
BATCHES = au.batches(GRID)


def check_batch(al, target, max_error, records, device, **kw):
    """One batch through align_records on ``device`` against the checker: scan,
    plan, trace rows, runs, PAF bytes, counts; every line also passes the
    DP-free check."""
    res = al.align_records(target, b"tgt", records, device=device, max_error=max_error, detail=True, **kw)
    paf, counts, per = au.expected_batch(target, b"tgt", records, max_error)
    det = res["detail"]
    for r, k in enumerate(det["kept"]):
        e, name = per[k], records[k][0]
        assert tuple(int(v) for v in det["scan"][r]) == e["scan"], name
        assert [int(v) for v in det["plan"][r][:5]] == [e["strand"], int(e["mapped"]), e["d"], e["end"], 2 * e["d"] + 1], name
        if e["mapped"]:
            start, cnt, runs = e["trace"]
            assert [int(v) for v in det["out"][r]] == [0, start] + cnt + [len(runs), 0], name
            assert [int(v) for v in det["runs"][r]] == runs, name
        else:
            assert r not in det["out"], name
        if e["line"] is not None:
            au.check_line(e["line"], target, records[k][1])
    assert res["paf"] == paf
    assert res["counts"] == counts
    return res


def test_grid_covers_the_kinds():
    kinds = {c["kind"] for c in GRID}
    assert kinds == {"inside", "flush0", "flushn", "minus", "tie", "exact", "nonacgt", "indel", "at_limit", "above_limit",
                     "longer", "mismatch_only"}
    assert {c["m"] for c in GRID} == set(au.GRID_M)
    got = {}
    for c in GRID:
        e = au.expect(c["read"], c["target"], c["max_error"])
        got.setdefault(c["kind"], []).append(e)
        if c["kind"] == "tie":
            assert e["scan"][0] == e["scan"][2] and e["strand"] == 0
        if c["kind"] == "at_limit":
            assert e["mapped"] and e["d"] == int(c["max_error"] * c["m"])
        if c["kind"] == "above_limit":
            assert e["why"] == "distance" and e["d"] == int(c["max_error"] * c["m"]) + 1
        if c["kind"] == "longer":
            assert c["m"] > len(c["target"]) or c["m"] == 1
    # the kinds meet what they are there for at least once
    assert any(e["strand"] == 1 and e["line"] for e in got["minus"])
    assert any(e["why"] == "no_match" for e in got["mismatch_only"]) and any(e["why"] == "distance" for e in got["mismatch_only"])
    assert any(e["why"] == "no_match" for e in got["tie"])  # m = 1: the read 'N' matches nothing
    assert any(e["line"] and e["trace"][2][0] & 3 != 0 for e in got["longer"])  # trailing ops the end rule drops
    assert any(e["line"] and e["trace"][0] == 0 for e in got["flush0"])
    assert any(e["line"] and e["end"] == len(c["target"]) for c, e in zip([c for c in GRID if c["kind"] == "flushn"], got["flushn"]))
    assert any(e["line"] and e["trace"][1][2] and e["trace"][1][3] for e in got["indel"])
    assert any(e["line"] and b"r" in e["line"].split(b"cs:Z:")[1] for e in got["nonacgt"])  # the read's 'R' as a substitution


@pytest.mark.parametrize("k", range(len(BATCHES)))
def test_trace_and_render_against_the_checker(al, k):
    target, max_error, records = BATCHES[k]
    check_batch(al, target, max_error, records, "cpu", threads=3)


def test_render_is_order_preserving_over_threads(al):
    target, max_error, records = max(BATCHES, key=lambda b: len(b[2]))
    assert len(records) >= 5
    one = al.align_records(target, b"tgt", records, device="cpu", max_error=max_error, threads=1)
    many = al.align_records(target, b"tgt", records, device="cpu", max_error=max_error, threads=7)
    assert one["paf"] == many["paf"] and one["paf"].count(b"\n") >= 4


# ---- mpc_align_plan ----------------------------------------------------------------

def _plan_inputs():
    # reads of 100 bases: d = 3 (+), 20 (-), 21 (unmapped at 0.2), 0 (a tie: +), 10 (a tie: +), 7 (+)
    scan = np.array([[3, 150, 9, 140], [60, 99, 20, 130], [21, 120, 30, 100], [0, 100, 0, 100], [10, 170, 10, 171],
                     [7, 130, 50, 90]], np.int32)
    return scan, np.full(len(scan), 100, np.int32)


def test_plan_strand_mapped_and_sizes(al):
    scan, lens = _plan_inputs()
    pl, cuts = al.plan(scan, lens, 0.2)
    assert cuts == [0, len(scan)]
    assert pl[:, 0].tolist() == [0, 1, 0, 0, 0, 0]
    assert pl[:, 1].tolist() == [1, 1, 0, 1, 1, 1]
    assert pl[:, 2].tolist() == [3, 20, 21, 0, 10, 7] and pl[:, 3].tolist() == [150, 130, 120, 100, 170, 130]
    assert pl[:, 4].tolist() == [7, 41, 43, 1, 21, 15]
    need = [100 * 64, 100 * 64, 0, 100 * 64, 100 * 64, 100 * 64]
    assert pl[:, 5].tolist() == need
    assert pl[:, 6].tolist() == [0, 6400, 0, 12800, 19200, 25600]
    assert pl[:, 7].tolist() == [0, 7, 0, 48, 49, 70]


@pytest.mark.parametrize("budget, cuts", [(5 * 6400, [0, 6]), (2 * 6400, [0, 3, 5, 6]), (6400, [0, 1, 3, 4, 5, 6]),
                                          (6400 + 6399, [0, 1, 3, 4, 5, 6])])
def test_plan_cuts_under_a_budget(al, budget, cuts):
    scan, lens = _plan_inputs()
    pl, got = al.plan(scan, lens, 0.2, budget)
    assert got == cuts
    for a, b in zip(got[:-1], got[1:]):
        rows = [r for r in range(a, b) if pl[r, 1]]
        assert rows and pl[rows[0], 6] == 0 and pl[rows[0], 7] == 0  # offsets restart in every launch
        assert int(pl[rows[-1], 6] + pl[rows[-1], 5]) <= budget
        for x, y in zip(rows[:-1], rows[1:]):
            assert pl[y, 6] == pl[x, 6] + pl[x, 5] and pl[y, 7] == pl[x, 7] + pl[x, 4]


def test_plan_refuses_a_budget_below_one_read(al):
    scan, lens = _plan_inputs()
    with pytest.raises(al.AlignError, match="needs 6400 flag bytes"):
        al.plan(scan, lens, 0.2, 6399)
    with pytest.raises(al.AlignError):
        al.plan(scan, np.array([100, 100, 100, 0, 100, 100], np.int32), 0.2)
    big = np.array([[4096, 9000, 4097, 9000], [4097, 9000, 5000, 9000]], np.int32)  # MPC_ALIGN_MAX_EDITS caps the rule
    pl, _ = al.plan(big, np.array([65536, 65536], np.int32), 0.5, 1 << 40)
    assert pl[:, 1].tolist() == [1, 0] and pl[0, 5] == 65536 * 8256


def test_budgets_give_identical_bytes(al):
    target, max_error, records = max(BATCHES, key=lambda b: len(b[2]))
    one = al.align_records(target, b"tgt", records, device="cpu", max_error=max_error, detail=True)
    need = int(one["detail"]["plan"][:, 5].max())
    each = al.align_records(target, b"tgt", records, device="cpu", max_error=max_error, workspace_bytes=need)
    assert one["launches"] == 1 and each["launches"] >= 3
    assert each["paf"] == one["paf"] and each["counts"] == one["counts"]


# ---- trace: argument checks, a wrong scan result -------------------------------------

def test_trace_host_flags_a_wrong_scan_result(al):
    rng = np.random.default_rng(5)
    t = vu.rand_seq(rng, 150)
    records = [(b"a", au.plant_subs(rng, t[10:110], 3)), (b"b", t[30:140]), (b"c", au.plant_subs(rng, t[5:95], 2))]
    pk = al.Packed(t, [s for _, s in records])
    scan = al.orient_and_scan(pk, "cpu")
    pl, _ = al.plan(scan, pk.lens, 0.2)
    jobs = al.jobs_of(pk, pl, [0, 1, 2])
    rc, good, good_runs = al.trace(pk.seq, jobs, "cpu")
    assert rc == 0 and good[:, 0].tolist() == [0, 0, 0]
    for d, end in ((pl[1, 2] + 1, pl[1, 3]), (pl[1, 2], pl[1, 3] - 1)):  # a distance too large; an end with another value
        wrong = jobs.copy()
        wrong[1, 4], wrong[1, 5] = d, end
        wrong[2, 7] = wrong[1, 7] + 2 * d + 1
        rc, out, runs = al.trace(pk.seq, wrong, "cpu")
        assert rc == al.E_SCAN and out[:, 0].tolist() == [0, 1, 0]
        assert out[1].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
        for r in (0, 2):
            assert out[r].tolist() == good[r].tolist()
            assert runs[wrong[r, 7]: wrong[r, 7] + out[r, 6]].tolist() == good_runs[jobs[r, 7]: jobs[r, 7] + good[r, 6]].tolist()
    for col, val in ((1, 0), (1, 65537), (4, 4097), (4, -1), (5, 151), (0, -1), (0, pk.seq.nbytes), (7, -1)):
        wrong = jobs.copy()
        wrong[0, col] = val
        with pytest.raises(al.AlignError):
            al.trace(pk.seq, wrong, "cpu")


# ---- one band trace and one table rule (csrc/mpc_bandtrace.h) ------------------------

def test_host_trace_equals_verify_script(al):
    """mpc_align_trace_host and mpc_verify_script are one band trace: on the
    verify grid (n >= 1) the runs as a CIGAR, the start and the counts of the
    one equal the cigar, start and counts of the other."""
    pairs = [(q, t) for q, t in vu.small_pairs() if len(t) >= 1]
    scan = vu.scan_host(pairs)
    assert len(pairs) == 45 and max(d for d, _ in scan) <= vu.MAX_EDITS
    seq, tab = vu.pack(pairs)
    jobs = au.job_table(tab, scan)
    rc, out, runs = al.trace(seq, jobs, "cpu", threads=3)
    assert rc == 0
    for k, ((q, t), (d, end)) in enumerate(zip(pairs, scan)):
        src, start, counts, cigar = vu.script(q, t, d, end)
        assert src == 0
        got = runs[jobs[k, 7]: jobs[k, 7] + out[k, 6]].tolist()
        assert (au.cigar_of(got), int(out[k, 1]), out[k, 2:6].tolist()) == (cigar, start, counts), (len(q), len(t))


@pytest.fixture(scope="module")
def traced(al):
    """The GPU suite's launch traced on the host: blob, job table, out rows, runs."""
    pairs = [(q, t) for _, q, t, _ in au.trace_shapes()]
    seq, tab = vu.pack(pairs)
    jobs = au.job_table(tab, vu.scan_host(pairs, 4))
    rc, out, runs = al.trace(seq, jobs, "cpu")
    assert rc == 0
    return seq, jobs, out, runs


def test_job_rule_refuses_and_names_the_row(al, traced):
    """The rows the device entry point refuses before its launch: the host trace
    and the renderer refuse the same ones and name the row; flag_off (column 6)
    alone is the device's, the host keeps no workspace."""
    seq, jobs, out, runs = traced
    J = len(jobs)
    render = lambda tab: al.render(seq, tab, np.zeros(J, np.uint8), out, runs, [b"r%d" % k for k in range(J)], b"tgt")
    rows = au.refused_jobs(seq)
    assert {col for _, col, _ in rows} == {0, 1, 4, 5, 6, 7}
    for row, col, val in rows:
        wrong = jobs.copy()
        wrong[row, col] = val
        if col == 6:
            assert al.trace(seq, wrong, "cpu")[0] == 0
            continue
        with pytest.raises(al.AlignError, match="mpc_align_trace_host: read %d: " % row):
            al.trace(seq, wrong, "cpu")
        with pytest.raises(al.AlignError, match="mpc_align_render: read %d: " % row):
            render(wrong)
    assert len(render(jobs)[0]) > 0


def test_revcomp_rule_refuses_and_names_the_row(al):
    L = al.host_lib()
    seq = np.frombuffer(b"ACGTACGTACGTACGT", np.uint8).copy()
    good = [[0, 4, 8], [4, 4, 12], [0, 0, 0]]
    tab = np.array(good, np.int64)
    assert L.mpc_align_revcomp_host(seq.ctypes.data, seq.nbytes, tab.ctypes.data, 3, 1) == 0
    assert bytes(seq) == b"ACGTACGTACGTACGT"  # (ACGT is its own reverse complement)
    # a span outside the blob on either side, a negative length, source and destination overlapping
    for row, bad in ((0, [-1, 4, 8]), (1, [4, 4, 13]), (2, [14, 4, 0]), (1, [4, -1, 12]), (2, [0, 4, 3]), (0, [2, 4, 0])):
        tab = np.array(good, np.int64)
        tab[row] = bad
        assert L.mpc_align_revcomp_host(seq.ctypes.data, seq.nbytes, tab.ctypes.data, 3, 1) != 0, bad
        assert b"mpc_align_revcomp_host: read %d: " % row in L.mpc_align_last_error()
    assert bytes(seq) == b"ACGTACGTACGTACGT"  # refused before any byte is written


# ---- the CLI ---------------------------------------------------------------------------

def _write(path, text):
    with open(path, "wb") as f:
        f.write(text)
    return str(path)


def _run_cli(cli, tmp_path, ref, reads, *more):
    paf, summary = str(tmp_path / "out.paf"), str(tmp_path / "summary.tsv")
    rc = cli.main(["--ref", _write(tmp_path / "ref.fa", ref), "--reads", _write(tmp_path / "reads.fa", reads),
                   "--paf", paf, "--summary", summary, "--device", "cpu"] + list(more))
    return rc, paf, summary


T40 = b"ACGTTGCAAGGCTTACGATCGGATCCTAGGCATGCAAGTC"


@pytest.mark.parametrize("ref, reads", [
    (b">a\n" + T40 + b"\n>b\n" + T40 + b"\n", b">r\nACGTTGCAAG\n"),  # two target records
    (b">a\n\n", b">r\nACGTTGCAAG\n"),                                   # an empty target
    (b"", b">r\nACGTTGCAAG\n"),                                         # no target at all
    (b">a\n" + T40 + b"\n", b">r\nACGT1GCAAG\n"),                       # a digit in a sequence line
    (b">a\nACGT-ACGT\n", b">r\nACGTTGCAAG\n"),
    (b">a\n" + T40 + b"\n", b"ACGT\n>r\nACGTTGCAAG\n"),                 # sequence before a header
])
def test_cli_rejects(cli, tmp_path, capsys, ref, reads):
    rc, paf, summary = _run_cli(cli, tmp_path, ref, reads)
    assert rc == 1 and "Error:" in capsys.readouterr().err
    assert sorted(os.listdir(tmp_path)) == ["reads.fa", "ref.fa"]  # no PAF, no summary, nothing left behind


def test_cli_skips_reads_by_length_and_names_by_first_word(cli, tmp_path):
    rng = np.random.default_rng(3)
    long_read = vu.rand_seq(rng, 65537)
    reads = (b">r1 extra words\n" + T40[5:20] + b"\n" + T40[20:35].lower() + b"\r\n>empty\n>toolong\n" + long_read +
             b"\n>r2\tx\n" + au.revcomp(T40[2:38]) + b"\n>far\n" + b"T" * 30 + b"\n")
    rc, paf, summary = _run_cli(cli, tmp_path, b">plasmid 1 circular\n" + T40[:25] + b"\n" + T40[25:] + b"\n", reads)
    assert rc == 0
    assert open(paf, "rb").read() == (b"r1\t30\t0\t30\t+\tplasmid\t40\t5\t35\t30\t30\t255\tNM:i:0\tcs:Z::30\n"
                                      b"r2\t36\t0\t36\t-\tplasmid\t40\t2\t38\t36\t36\t255\tNM:i:0\tcs:Z::36\n")
    assert open(summary).read() == ("reads\t5\nmapped\t2\nplus\t1\nminus\t1\nunmapped_by_distance\t1\n"
                                    "unmapped_no_match\t0\nskipped_length\t2\n")


def test_cli_batches_give_the_same_bytes(al, tmp_path):
    target, max_error, records = max(BATCHES, key=lambda b: len(b[2]))
    ref = _write(tmp_path / "ref.fa", b">tgt\n" + target + b"\n")
    reads = _write(tmp_path / "reads.fa", b"".join(b">" + n + b"\n" + s + b"\n" for n, s in records))
    whole = al.align(ref, reads, device="cpu", max_error=max_error)
    small = al.align(ref, reads, device="cpu", max_error=max_error, batch_bases=150)
    assert whole == small and whole["paf"] == au.expected_batch(target, b"tgt", records, max_error)[0]
    chunks = []
    streamed = al.align(ref, reads, device="cpu", max_error=max_error, batch_bases=150, write=chunks.append)
    assert streamed["paf"] is None and len(chunks) >= 3 and b"".join(chunks) == whole["paf"]


# ---- reads -> PAF -> consensus ----------------------------------------------------------

def _consensus(ref_fa, paf, reads_fa):
    s = oracle.ingest_files(ref_fa, paf, reads_fa)
    res = oracle.run_packed(s["ref"], s["cs"], s["cs_off"], s["tstart"], s["up"], s["up_off"], s["down"], s["down_off"],
                            0.1, 5.0)
    return bytes(res["base"])


@pytest.mark.parametrize("n, n_reads, profile, seed, max_error", [(600, 120, "default", 5, None), (600, 120, "indel", 7, "0.35")])
def test_end_to_end_consensus_on_the_cpu(pkg, cli, tmp_path, n, n_reads, profile, seed, max_error):
    syn = pkg.synth.Synth(n=n, n_reads=n_reads, profile=profile, seed=seed)
    ref_fa, reads_fa, paf0 = (str(tmp_path / x) for x in ("ref.fa", "reads.fa", "planted.paf"))
    syn.write_files(ref_fa, reads_fa, paf0)
    ref = pkg.verify.read_consensus(ref_fa)
    assert len(ref) == n
    core = ref[50:-50]
    # the condition is one the input meets without this code: the planted alignments give it
    assert vu.score(core, _consensus(ref_fa, paf0, reads_fa))[0] == 0
    paf = str(tmp_path / "aligned.paf")
    summary = str(tmp_path / "summary.tsv")
    rc = cli.main(["--ref", ref_fa, "--reads", reads_fa, "--paf", paf, "--summary", summary, "--device", "cpu"] +
                  (["--max-error", max_error] if max_error else []))
    assert rc == 0
    counts = dict(ln.split("\t") for ln in open(summary).read().splitlines())
    assert int(counts["reads"]) == n_reads and int(counts["mapped"]) == n_reads  # no read is lost
    assert int(counts["plus"]) > 0 and int(counts["minus"]) > 0
    reads = dict(pkg.align.fasta_records(reads_fa))
    for line in open(paf, "rb"):
        au.check_line(line, ref, reads[line.split(b"\t", 1)[0]])
    assert vu.score(core, _consensus(ref_fa, paf, reads_fa))[0] == 0
