"""align_reads on the GPU: K_atrace (mpc_align_trace) equals the host band DP
(mpc_align_trace_host) field by field, K_arevcomp equals Python, and the CLI
writes the same bytes on the device and on the host; that PAF gives the
expected consensus through the GPU drop-in CLI.  Every comparison is exact
equality; the host side is checked against the numpy checker in
tests/test_align_cpu.py."""
import importlib

import numpy as np
import pytest

import align_util as au
import verify_util as vu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def al(pkg):
    return pkg.align


@pytest.fixture(scope="module")
def launch(al):
    """The shapes as ONE launch: blob, job table, and the host's results."""
    shapes = au.trace_shapes()
    pairs = [(q, t) for _, q, t, _ in shapes]
    seq, tab = vu.pack(pairs)
    scan = vu.scan_host(pairs, 4)
    for (note, q, t, d), (got, end) in zip(shapes, scan):
        if d is not None:
            assert got == d, note  # d is what was planted ...
        if len(q) <= 1000:
            assert (got, end) == vu.score(q, t), note  # ... and what the numpy checker finds
    jobs = au.job_table(tab, scan)
    rc, out, runs = al.trace(seq, jobs, "cpu")
    assert rc == 0
    return shapes, seq, jobs, out, runs


def _runs_of(jobs, out, runs, k):
    return runs[jobs[k, 7]: jobs[k, 7] + out[k, 6]].tolist()


def test_trace_equals_host_in_one_launch(al, launch):
    shapes, seq, jobs, host_out, host_runs = launch
    rc, out, runs = al.trace(seq, jobs, 0)
    assert rc == 0
    for k, (note, q, t, d) in enumerate(shapes):
        assert out[k].tolist() == host_out[k].tolist(), note
        assert _runs_of(jobs, out, runs, k) == _runs_of(jobs, host_out, host_runs, k), note
        if d is not None and note.startswith("subs"):  # the script holds exactly the planted substitutions
            assert out[k].tolist() == [0, 17, len(q) - d, d, 0, 0, out[k, 6], 0] and out[k, 6] <= 2 * d + 1
    assert np.array_equal(runs, host_runs)  # nothing outside a read's own runs either


def test_trace_equals_verify_script(al, launch):
    """K_atrace against verify's definition directly: its runs as a CIGAR, its
    start and its counts are mpc_verify_script's for the same (d, end)."""
    shapes, seq, jobs, _, _ = launch
    rc, out, runs = al.trace(seq, jobs, 0)
    assert rc == 0
    for k, (note, q, t, _) in enumerate(shapes):
        src, start, counts, cigar = vu.script(q, t, int(jobs[k, 4]), int(jobs[k, 5]))
        assert src == 0, note
        assert (au.cigar_of(_runs_of(jobs, out, runs, k)), int(out[k, 1]), out[k, 2:6].tolist()) == (cigar, start, counts), note


def test_single_read_launch_equals_the_batch(al, launch):
    shapes, seq, jobs, host_out, host_runs = launch
    for k in (4, 7, len(shapes) - 4):  # d = 63 (pitch 128), the indel set, n < m
        one = jobs[k: k + 1].copy()
        one[0, 6] = one[0, 7] = 0
        rc, out, runs = al.trace(seq, one, 0)
        assert rc == 0 and out[0].tolist() == host_out[k].tolist(), shapes[k][0]
        assert runs[: out[0, 6]].tolist() == _runs_of(jobs, host_out, host_runs, k)


def test_wrong_scan_result_sets_only_that_status(al, launch):
    shapes, seq, jobs, host_out, host_runs = launch
    k = 2  # subs d = 31
    for d, end in ((jobs[k, 4] + 1, jobs[k, 5]), (jobs[k, 4], jobs[k, 5] - 1), (jobs[k, 4] - 5, jobs[k, 5])):
        wrong = jobs.copy()
        wrong[k, 4], wrong[k, 5] = d, end
        # the plan of the wrong d: rows and runs stay disjoint and inside the buffers
        pitch = (2 * wrong[:, 4] + 1 + 63) // 64 * 64
        wrong[:, 6] = np.concatenate([[0], np.cumsum(wrong[:, 1] * pitch)[:-1]])
        wrong[:, 7] = np.concatenate([[0], np.cumsum(2 * wrong[:, 4] + 1)[:-1]])
        rc, out, runs = al.trace(seq, wrong, 0)
        assert rc == al.E_SCAN
        assert out[:, 0].tolist() == [int(x == k) for x in range(len(shapes))]
        assert out[k].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
        for x in range(len(shapes)):
            if x != k:
                assert out[x].tolist() == host_out[x].tolist()
                assert _runs_of(wrong, out, runs, x) == _runs_of(jobs, host_out, host_runs, x)
        hrc, hout, _ = al.trace(seq, wrong, "cpu")
        assert hrc == al.E_SCAN and np.array_equal(hout, out)


def test_trace_refuses_bad_jobs_before_the_launch(al, pkg, launch):
    shapes, seq, jobs, _, _ = launch
    for row, col, val in au.refused_jobs(seq):
        wrong = jobs.copy()
        wrong[row, col] = val
        with pytest.raises(pkg.engine.MpcError, match="mpc_align_trace: read"):
            al.trace(seq, wrong, 0)


@pytest.fixture(scope="module")
def one_target():
    """Reads of one target with d from 0 to 70 on both strands: (target, records)."""
    rng = np.random.default_rng(12)
    t = vu.rand_seq(rng, 900)
    recs = []
    for k, d in enumerate((0, 3, 31, 32, 70, 5, 64, 12, 1, 40)):
        a = int(rng.integers(0, 60))
        s = au.plant_subs(rng, t[a: a + 800], d)
        recs.append((b"read%d" % k, au.revcomp(s) if k % 2 else s))
    recs.insert(3, (b"none", vu.rand_seq(rng, 400)))  # unmapped by distance
    recs.insert(6, (b"empty", b""))
    return t, recs


def test_launch_cuts_give_identical_bytes(al, one_target):
    t, recs = one_target
    host = al.align_records(t, b"tgt", recs, device="cpu", detail=True)
    one = al.align_records(t, b"tgt", recs, device=0, detail=True)
    need = int(one["detail"]["plan"][:, 5].max())
    cut = al.align_records(t, b"tgt", recs, device=0, workspace_bytes=2 * need, detail=True)
    assert one["launches"] == 1 and cut["launches"] >= 3
    assert host["counts"] == dict(reads=12, mapped=10, plus=5, minus=5, unmapped_by_distance=1, unmapped_no_match=0, skipped_length=1)
    for res in (one, cut):
        assert res["paf"] == host["paf"] and res["counts"] == host["counts"]
        assert np.array_equal(res["detail"]["scan"], host["detail"]["scan"])
        assert sorted(res["detail"]["out"]) == sorted(host["detail"]["out"])
        for r in host["detail"]["out"]:
            assert res["detail"]["out"][r].tolist() == host["detail"]["out"][r].tolist()
            assert res["detail"]["runs"][r].tolist() == host["detail"]["runs"][r].tolist()
    for line, (name, s) in zip(host["paf"].splitlines(True), [r for r in recs if r[0].startswith(b"read")]):
        assert line.startswith(name + b"\t")
        au.check_line(line, t, s)


def test_revcomp_kernel_against_python(al):
    rng = np.random.default_rng(8)
    t = vu.rand_seq(rng, 100)
    reads = []
    for m in (1, 63, 64, 65, 4097):
        s = bytearray(vu.rand_seq(rng, m))
        s[::3] = bytes(s[::3]).lower()
        s[m // 2] = ord("N")
        if m > 10:
            s[7], s[m - 2] = ord("n"), ord("R")
        reads.append(bytes(s))
    pk = al.Packed(t, reads)
    al.orient_and_scan(pk, 0)
    for s, a, b in zip(reads, pk.plus, pk.minus):
        assert bytes(pk.seq[a: a + len(s)]) == s
        assert bytes(pk.seq[b: b + len(s)]) == au.revcomp(s)
    assert bytes(pk.seq[:100]) == t and not pk.seq[pk.minus_span[1]:].any()


def test_cli_device_equals_cpu_and_gives_the_consensus(pkg, al, tmp_path):
    cli = importlib.import_module(pkg.__name__ + ".align_reads")
    dropin = importlib.import_module(pkg.__name__ + ".mapped_paf_read_parser")
    syn = pkg.synth.Synth(n=1500, n_reads=300, seed=9)
    ref_fa, reads_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    syn.write_files(ref_fa, reads_fa)
    outs = {}
    for dev in ("0", "cpu"):
        paf, summary = str(tmp_path / ("%s.paf" % dev)), str(tmp_path / ("%s.tsv" % dev))
        assert cli.main(["--ref", ref_fa, "--reads", reads_fa, "--paf", paf, "--summary", summary, "--device", dev]) == 0
        outs[dev] = (open(paf, "rb").read(), open(summary, "rb").read())
    assert outs["0"] == outs["cpu"]
    assert outs["0"][0].count(b"\n") == 300 and b"mapped\t300\n" in outs["0"][1]
    cons = [str(tmp_path / x) for x in ("c.fa", "ch.tsv", "acc.tsv")]
    assert dropin.main(["--ref", ref_fa, "--reads", reads_fa, "--paf", str(tmp_path / "0.paf"), "--consensus", cons[0],
                        "--chromat", cons[1], "--accuracies", cons[2], "--min_depth_factor", "0.1",
                        "--global_threshold_factor", "5"]) == 0
    ref = pkg.verify.read_consensus(ref_fa)
    assert len(ref) == 1500
    (d, end), = pkg.verify.scan([(ref[50:-50], pkg.verify.read_consensus(cons[0]))], device=0)
    assert d == 0 and end >= 1400
