"""align.Launches on the GPU: over the planted reads of tests/draft_util.py (a
900-base target, run lists above 128 entries), in one launch and cut into
several, every launch's jobs, out and runs equal the host loop's, the device
tensors it hands on hold the host arrays, and a draft.vote fed by them gives
the checker's tallies.  Every comparison is exact equality."""
import numpy as np
import pytest

import draft_util as du

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planted(pkg):
    """(target, reads, the host loop's launches at the default budget, the
    largest single read's need, the checker's tallies)."""
    target, noted = du.vote_reads()
    reads = [r for _, r in noted]
    loop = pkg.align.Launches(target, reads, "cpu", du.MAX_ERROR, threads=2)
    host = list(loop)
    assert len(host) == 1 and host[0][2][:, 6].max() > 128
    rd, jobs, out, runs, _ = host[0]
    want = du.vote(len(target), du.checker_reads((loop.pk, jobs, out, runs, None, rd)))
    return target, reads, host, int(loop.plan[:, 5].max()), want


@pytest.mark.parametrize("several", [False, True], ids=["one launch", "several launches"])
def test_device_launches_equal_the_host_loop(pkg, planted, several):
    al, dr = pkg.align, pkg.draft
    target, reads, host, need, want = planted
    budget = need if several else al.DEFAULT_WORKSPACE
    if several:
        host = list(al.Launches(target, reads, "cpu", du.MAX_ERROR, budget, threads=2))
    loop = al.Launches(target, reads, 0, du.MAX_ERROR, budget, keep_device=True)
    n = len(target)
    tally = dr.new_tally(n, 0)
    launches = 0
    for (rd, jobs, out, runs, kept), (hrd, hjobs, hout, hruns, _) in zip(loop, host):
        assert rd == hrd and np.array_equal(jobs, hjobs) and np.array_equal(out, hout) and np.array_equal(runs, hruns)
        assert len(rd) >= 1 and sorted(kept) == ["jobs", "out", "runs", "seq"]
        assert kept["seq"] is loop.pk.d_seq and np.array_equal(kept["seq"].cpu().numpy(), loop.pk.seq)
        assert np.array_equal(kept["jobs"].cpu().numpy().view(np.int64).reshape(-1, 8), jobs)
        assert np.array_equal(kept["out"].cpu().numpy().reshape(-1, 8), out)
        assert np.array_equal(kept["runs"].cpu().numpy(), runs)
        rc, status = dr.vote(tally, n, loop.pk.seq, jobs, out, runs, 0, device_tensors=kept)
        assert rc == 0 and not status.any()
        launches += 1
    assert launches == len(host) == len(loop.cuts) - 1
    assert launches >= 3 if several else launches == 1
    assert np.array_equal(dr.tally_to_host(tally), want)
