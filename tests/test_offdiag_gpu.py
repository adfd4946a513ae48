"""K_atrace and K_vscan off the diagonal on the GPU: exact equality with the
numpy full-matrix DP and canonical traceback of tests/verify_util.py on the
cases of tests/offdiag_cases.py -- contiguous indel runs of 31 to 200 bases,
both directions in one read, runs at the read's ends, dense divergence up to
d = 4096 (W = 8193), low complexity; query lengths whose last row sits in an
interior block of its lane, and texts shorter than the lanes in use.
tests/test_offdiag_cpu.py shows from the checker alone that these paths leave
the traceback window, cross 64-slot chunks by left moves, touch both band edges
and cross tile rows inside a D run.  No comparison here is against the host
band trace."""
import numpy as np
import pytest

import align_util as au
import offdiag_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def al(pkg):
    return pkg.align


@pytest.fixture(scope="module")
def launch(al):
    """ONE K_atrace launch over every trace case, the jobs from the CHECKER's
    (d, end): a wrong scan cannot mask a wrong trace."""
    cases, tbs = oc.traced()
    seq, jobs = oc.job_launch(cases, tbs)
    rc, out, runs = al.trace(seq, jobs, 0)
    return cases, tbs, seq, jobs, rc, out, runs


def test_trace_off_diagonal_equals_checker(launch):
    cases, tbs, seq, jobs, rc, out, runs = launch
    want_out, want_runs = oc.expected_trace(jobs, tbs)
    assert rc == 0, [(c[0], o.tolist()) for c, o in zip(cases, out) if o[0]]
    for k, ((note, q, t), tb) in enumerate(zip(cases, tbs)):
        # {status, start, n_eq, n_x, n_i, n_d, n_runs, 0}, then the runs end -> start
        assert out[k].tolist() == want_out[k].tolist(), note
        a = int(jobs[k, 7])
        assert runs[a: a + out[k, 6]].tolist() == au.runs_of(tb["ops"][::-1]), note
    assert np.array_equal(runs, want_runs)  # runs outside each read's own span stay zero


def test_trace_single_launches_agree(al, launch):
    """A read traced alone, its flag rows and runs at offset 0, gives what it gave in the batch."""
    cases, tbs, seq, jobs, rc, out, runs = launch
    notes = [c[0] for c in cases]
    for note in ("I200 at 300", "D70 then I90", "unrelated 4000 x 4200"):
        k = notes.index(note)
        one = jobs[k: k + 1].copy()
        one[0, 6] = one[0, 7] = 0
        rc1, out1, runs1 = al.trace(seq, one, 0)
        want_out, want_runs = oc.expected_trace(one, tbs[k: k + 1])
        assert rc1 == 0 and out1.tolist() == want_out.tolist() and np.array_equal(runs1, want_runs), note
        assert out1[0].tolist() == out[k].tolist(), note
        assert runs1[: out1[0, 6]].tolist() == runs[jobs[k, 7]: jobs[k, 7] + out[k, 6]].tolist(), note


def test_scan_off_diagonal_equals_checker(pkg):
    cases, ref = oc.scanned()
    tcases, tbs = oc.traced()
    notes = [c[0] for c in cases + tcases]
    want = list(ref) + [(tb["distance"], tb["end"]) for tb in tbs]
    got = pkg.verify.scan([(q, t) for _, q, t in cases + tcases], device=0)
    assert len(got) == len(want) == 5 * len(oc.SCAN_SHAPES) + len(tcases)
    bad = [(note, g, w) for note, g, w in zip(notes, got, want) if g != w]
    assert not bad, bad


def test_align_records_off_diagonal(al):
    target, records = oc.paf_batch()
    paf, counts, per = au.expected_batch(target, b"tgt", records, 0.5)
    assert counts["mapped"] == 3 and counts["minus"] == 1
    one = al.align_records(target, b"tgt", records, device=0, max_error=0.5, detail=True)
    assert one["paf"] == paf and one["counts"] == counts and one["launches"] == 1
    need = int(one["detail"]["plan"][:, 5].max())
    cut = al.align_records(target, b"tgt", records, device=0, max_error=0.5, workspace_bytes=2 * need)
    assert cut["launches"] >= 2
    assert cut["paf"] == paf and cut["counts"] == counts
