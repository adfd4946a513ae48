"""The Python drivers' shared pieces on the host (no GPU): align.Launches (scan,
plan and one trace per cut) under two budgets, the messages its TraceError
becomes in align_records and in draft.polish_round, and _native's put_all and
host_check."""
import ctypes

import numpy as np
import pytest

import align_util as au
import draft_util as du


@pytest.fixture(scope="module")
def al(pkg):
    return pkg.align


@pytest.fixture(scope="module")
def nat(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + "._native")


# ---- the messages ------------------------------------------------------------------

def _failing_trace(al, monkeypatch, status):
    """align.trace says E_SCAN, with ``status`` for the last read of every launch that has one."""
    real = al.trace

    def trace(seq, jobs, *args, **kw):
        rc, out, runs = real(seq, jobs, *args, **kw)
        if len(out):
            out[-1, 0] = status
            rc = al.E_SCAN
        return rc, out, runs

    monkeypatch.setattr(al, "trace", trace)


def test_align_records_names_the_read_and_its_status(al, monkeypatch):
    target, max_error, records = au.batches(au.grid())[0]
    det = al.align_records(target, b"tgt", records, device="cpu", max_error=max_error, detail=True)["detail"]
    mapped = [r for r in range(len(det["kept"])) if det["plan"][r, 1]]
    assert det["cuts"] == [0, len(det["kept"])] and len(mapped) >= 2
    name = records[det["kept"][mapped[-1]]][0]
    _failing_trace(al, monkeypatch, 7)
    with pytest.raises(al.AlignError) as e:
        al.align_records(target, b"tgt", records, device="cpu", max_error=max_error)
    assert type(e.value) is al.AlignError
    assert str(e.value) == "read {!r}: the band DP does not reproduce the scan's distance (status 7)".format(name.decode())


def test_polish_round_names_the_read(pkg, al, monkeypatch):
    target, noted = du.vote_reads()
    reads = [r for _, r in noted]
    pl = al.Launches(target, reads, "cpu", du.MAX_ERROR, threads=2).plan
    last = max(r for r in range(len(reads)) if pl[r, 1])
    assert noted[last][0] == "plain" and noted[last - 3][0] == "unmapped"
    _failing_trace(al, monkeypatch, 3)
    with pytest.raises(pkg.draft.DraftError) as e:
        pkg.draft.polish_round(target, reads, "cpu", du.MAX_ERROR, threads=2)
    assert str(e.value) == "read {}: the band DP does not reproduce the scan's distance".format(last)
    with pytest.raises(al.TraceError) as e:
        list(al.Launches(target, reads, "cpu", du.MAX_ERROR, threads=2))
    assert (e.value.read, e.value.status) == (last, 3)


# ---- the launches -------------------------------------------------------------------

def _flat(loop):
    """[(read, its out row, its runs)] over the launches, and how many there were."""
    rows, launches = [], 0
    for reads, jobs, out, runs, kept in loop:
        assert kept is None and len(reads) == len(jobs) == len(out)
        rows += [(r, out[k].tolist(), runs[jobs[k, 7]: jobs[k, 7] + out[k, 6]].tolist()) for k, r in enumerate(reads)]
        launches += 1
    return rows, launches


def test_launches_under_two_budgets(al):
    target, noted = du.vote_reads()
    reads = [r for _, r in noted]
    one = al.Launches(target, reads, "cpu", du.MAX_ERROR, threads=2)
    pk = al.Packed(target, reads)
    scan = al.orient_and_scan(pk, "cpu", 2)
    for budget, loop in ((al.DEFAULT_WORKSPACE, one),
                         (int(one.plan[:, 5].max()), None)):
        loop = loop or al.Launches(target, reads, "cpu", du.MAX_ERROR, budget, threads=2)
        pl, cuts = al.plan(scan, pk.lens, du.MAX_ERROR, budget)
        assert np.array_equal(loop.scan, scan) and np.array_equal(loop.plan, pl) and loop.cuts == cuts
        assert np.array_equal(loop.pk.seq, pk.seq)
        rows, launches = _flat(loop)
        assert launches == len(cuts) - 1
        if loop is one:
            assert launches == 1
            first = rows
        else:
            assert launches >= 3 and rows == first
    assert [r for r, _, _ in first] == [r for r in range(len(reads)) if one.plan[r, 1]]
    assert max(o[6] for _, o, _ in first) > 128


def test_an_empty_launch_is_still_a_launch(al):
    loop = al.Launches(b"ACGTACGTAC" * 10, [b"T" * 50], "cpu")
    (reads, jobs, out, runs, kept), = loop
    assert reads == [] and jobs.shape == (0, 8) and out.shape == (0, 8) and len(runs) == 0 and kept is None
    assert loop.cuts == [0, 1] and not loop.plan[0, 1]


# ---- _native ------------------------------------------------------------------------

class _Tensor:
    def __init__(self, a):
        self.a = a

    def copy_(self, other):
        self.a[:] = other.a

    def data_ptr(self):
        return self.a.ctypes.data


class _Torch:
    """What Device.put takes of torch, over numpy."""
    uint8 = np.uint8
    empty = staticmethod(lambda n, dtype, device: _Tensor(np.empty(n, dtype)))
    from_numpy = staticmethod(_Tensor)


def test_put_all_offsets_and_bytes(nat):
    d = object.__new__(nat.Device)  # (no GPU: the copies alone)
    d.torch, d.dev = _Torch, "cpu"
    rng = np.random.default_rng(3)
    n, S, K = 5, 2, 3
    # what linkage.run passes: cs_off, tstart, pos_off, site_off, site_key, rec_sample, cs
    parts = [rng.integers(0, 99, n + 1).astype(np.int64), rng.integers(0, 99, n).astype(np.int64),
             rng.integers(0, 99, S + 1).astype(np.int64), rng.integers(0, 9, S + 1).astype(np.int64),
             rng.integers(0, 99, K).astype(np.int64), rng.integers(0, S, n).astype(np.int32),
             rng.integers(0, 255, 13).astype(np.uint8)]
    at, blob = d.put_all(parts)
    base = blob.data_ptr()
    assert len(at) == 7 and at[0] == base and len(blob.a) == sum(p.nbytes for p in parts) + 8
    assert not blob.a[-8:].any()
    for p, a, nxt in zip(parts, at, at[1:] + [base + len(blob.a) - 8]):
        assert a + p.nbytes == nxt
        if p.dtype == np.int64:
            assert a % 8 == 0
        assert np.array_equal(blob.a[a - base: a - base + p.nbytes].view(p.dtype), p)
    assert np.array_equal(d.put(parts[5]).a.view(np.int32), parts[5]) and len(d.put(np.zeros(0, np.int64)).a) == 0


def test_host_check(nat, al):
    L = al.host_lib()
    assert nat.host_check(L, "align", al.AlignError, 0) == 0
    assert nat.host_check(L, "align", al.AlignError, al.E_SCAN, accept=(al.E_SCAN,)) == al.E_SCAN
    scan = np.array([[3, 150, 9, 140]], np.int32)
    lens = np.array([100], np.int32)
    out, cuts, nl = np.zeros((1, 8), np.int64), np.zeros(2, np.int32), ctypes.c_int32(0)
    rc = L.mpc_align_plan(scan.ctypes.data, lens.ctypes.data, 1, 0.2, 63, out.ctypes.data, cuts.ctypes.data, ctypes.byref(nl))
    assert rc != 0
    text = L.mpc_align_last_error().decode()
    assert text.startswith("mpc_align_plan: read 0") and "the workspace budget is 63" in text
    with pytest.raises(al.AlignError) as e:
        nat.host_check(L, "align", al.AlignError, rc)
    assert str(e.value) == text
    with pytest.raises(al.AlignError) as e:
        nat.host_check(L, "align", al.AlignError, rc, accept=(al.E_SCAN,))
    assert str(e.value) == text
    with pytest.raises(al.AlignError) as e:
        al.plan(scan, lens, 0.2, 63)
    assert str(e.value) == text
