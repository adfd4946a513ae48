"""draft_assembly on the GPU: K_dvote (mpc_draft_vote) equals the host vote and
the plain-Python checker on the planted reads of one target, in one launch and
in several; K_dcall (mpc_draft_call) equals host and checker on injected
tallies; and the CLI writes the same bytes on the device and on the host, with
the plasmid in the draft.  Every comparison is exact equality."""
import importlib

import numpy as np
import pytest

import align_util as au
import draft_util as du

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dr(pkg):
    return pkg.draft


@pytest.fixture(scope="module")
def planted(pkg, dr):
    """The planted reads traced once on the device: the launch, and the tallies of host and checker."""
    target, noted = du.vote_reads()
    reads = [r for _, r in noted]
    launches, pl = du.traced(pkg, target, reads, 0)
    assert len(launches) == 1
    host, _ = du.traced(pkg, target, reads, "cpu")
    pk, jobs, out, runs, _, rd = host[0]
    assert np.array_equal(launches[0][2], out) and np.array_equal(launches[0][3], runs)  # (the trace: tests/test_align_gpu.py)
    n = len(target)
    tally = dr.new_tally(n, "cpu")
    rc, status = dr.vote(tally, n, pk.seq, jobs, out, runs, "cpu")
    assert rc == 0 and not status.any()
    want = du.vote(n, du.checker_reads(host[0]))
    assert np.array_equal(tally, want) and out[:, 6].max() > 128
    return target, noted, launches[0], pl, want


def test_vote_equals_host_and_checker(dr, planted):
    target, noted, (pk, jobs, out, runs, kept, rd), _, want = planted
    n = len(target)
    tally = dr.new_tally(n, 0)
    rc, status = dr.vote(tally, n, pk.seq, jobs, out, runs, 0, device_tensors=kept)  # what the trace left on the device
    assert rc == 0 and not status.any()
    assert np.array_equal(dr.tally_to_host(tally), want)
    again = dr.new_tally(n, 0)
    rc, status = dr.vote(again, n, pk.seq, jobs, out, runs, 0)  # the same tables copied from the host
    assert rc == 0 and np.array_equal(dr.tally_to_host(again), want)


def test_vote_in_three_launches_gives_the_same_tallies(pkg, dr, planted):
    target, noted, launch, pl, want = planted
    n = len(target)
    need = int(pl[:, 5].max())
    launches, _ = du.traced(pkg, target, [r for _, r in noted], 0, workspace_bytes=2 * need)
    assert len(launches) >= 3
    tally = dr.new_tally(n, 0)
    for pk, jobs, out, runs, kept, rd in launches:
        rc, status = dr.vote(tally, n, pk.seq, jobs, out, runs, 0, device_tensors=kept)
        assert rc == 0 and not status.any()
    assert np.array_equal(dr.tally_to_host(tally), want)


def test_runs_that_leave_the_target_set_only_that_status(pkg, dr, planted):
    target, noted, launch, _, _ = planted
    pk, jobs, out, runs, kept, rd = launch
    n = len(target)
    k = [noted[r][0] for r in rd].index("to column n")
    wrong = out.copy()
    wrong[k, 1] += 1  # the runs now walk to column n + 1
    tally = dr.new_tally(n, 0)
    rc, status = dr.vote(tally, n, pk.seq, jobs, wrong, runs, 0)
    assert rc == dr.E_RUNS and status.tolist() == [int(x == k) for x in range(len(jobs))]
    assert np.array_equal(dr.tally_to_host(tally), du.vote(n, du.checker_reads(launch, skip=(k,))))
    host = dr.new_tally(n, "cpu")
    hrc, hstatus = dr.vote(host, n, pk.seq, jobs, wrong, runs, "cpu")
    assert hrc == rc and np.array_equal(hstatus, status) and np.array_equal(host, dr.tally_to_host(tally))
    # a table the host rule refuses never reaches the kernel
    for row, col, val in ((k, 6, 2 * int(jobs[k, 4]) + 2), (k, 1, -1), (0, 1, int(jobs[0, 5]) + 1)):
        worse = out.copy()
        worse[row, col] = val
        with pytest.raises(pkg.engine.MpcError, match="mpc_draft_vote: read %d" % row):
            dr.vote(tally, n, pk.seq, jobs, worse, runs, 0)
    short = jobs.copy()
    short[2, 3] = n - 1
    with pytest.raises(pkg.engine.MpcError, match="mpc_draft_vote: read 2: target length"):
        dr.vote(tally, n, pk.seq, short, out, runs, 0)


def test_call_equals_host_on_the_votes(dr, planted):
    target, _, (pk, jobs, out, runs, kept, rd), _, want = planted
    tally = dr.new_tally(len(target), 0)
    dr.vote(tally, len(target), pk.seq, jobs, out, runs, 0, device_tensors=kept)
    new, info = dr.call(tally, target, 0, d_draft=kept["seq"])  # the target opens the blob
    assert (new, info) == dr.call(want, target, "cpu")
    assert (new, [info[k] for k in dr.INFO_FIELDS]) == du.call(want, target)


@pytest.mark.parametrize("case", du.call_cases(), ids=lambda c: c[0])
def test_call_on_injected_tallies(pkg, dr, case):
    import torch
    note, draft, tally, expected = case
    want, winfo = du.call(tally, draft)
    d_tally = torch.from_numpy(tally.view(np.int32).reshape(-1).copy()).to("cuda:0")
    if want is None:
        with pytest.raises(dr.DraftError, match="no read mapped"):
            dr.call(d_tally, draft, 0)
        with pytest.raises(dr.DraftError, match="no read mapped"):
            dr.call(tally, draft, "cpu")
        return
    new, info = dr.call(d_tally, draft, 0)
    assert (new, [info[k] for k in dr.INFO_FIELDS]) == (want, winfo)
    assert (new, info) == dr.call(tally, draft, "cpu")
    if expected is not None:
        assert new == expected


@pytest.mark.parametrize("spec, more", [(dict(n=1500, n_reads=300, seed=9), []),
                                        (dict(n=600, n_reads=300, seed=5, frac_partial=0.3), ["--candidates", "4"])],
                         ids=["n1500", "n600_partial"])
def test_cli_device_equals_cpu_and_holds_the_plasmid(pkg, spec, more, tmp_path):
    cli = importlib.import_module(pkg.__name__ + ".draft_assembly")
    syn = pkg.synth.Synth(**spec)
    ref_fa, reads_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    syn.write_files(ref_fa, reads_fa)
    outs = {}
    for dev in ("0", "cpu"):
        paths = [str(tmp_path / ("%s.%s" % (dev, x))) for x in ("sense.fa", "anti.fa", "report.tsv")]
        assert cli.main(["--reads", reads_fa, "--sense", paths[0], "--antisense", paths[1], "--report", paths[2],
                         "--device", dev] + more) == 0
        outs[dev] = [open(p, "rb").read() for p in paths]
    assert outs["0"] == outs["cpu"]
    sense, anti = (o.split(b"\n")[1] for o in outs["0"][:2])
    assert outs["0"][0] == b">draft_sense\n" + sense + b"\n" and outs["0"][1] == b">draft_antisense\n" + au.revcomp(sense) + b"\n"
    ref = pkg.verify.read_consensus(ref_fa)
    assert len(ref) == spec["n"] and len(sense) <= spec["n"] + 80
    core = ref[50:-50]
    assert min(d for d, _ in pkg.verify.scan([(core, sense), (core, anti)], device=0)) == 0
