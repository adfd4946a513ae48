"""Off the diagonal on the host (no GPU): the cases of tests/offdiag_cases.py
are what they claim -- shown from the numpy checker's traceback alone, so the
GPU tests that share them cannot be emptied by a later edit of the generators
-- and the host scan, the host band trace, mpc_verify_script and the PAF
writer equal the checker on every one of them.  Every comparison is exact
equality; no case is skipped."""
import numpy as np
import pytest

import align_util as au
import offdiag_cases as oc
import verify_util as vu


@pytest.fixture(scope="module")
def al(pkg):
    return pkg.align


@pytest.fixture(scope="module")
def geometry():
    """[(note, m, d, W, rows, slots, ops)] of the checker's paths (end -> start)."""
    cases, tbs = oc.traced()
    return [(note, len(q), tb["distance"], 2 * tb["distance"] + 1) + oc.path_geometry(q, t, tb)
            for (note, q, t), tb in zip(cases, tbs)]


def _drift(rows, slots):
    """(up, down): the largest rise and fall of the slot between two steps less than 64 rows apart."""
    # steps s <= e with rows[s] - rows[e] < 64: for every s the furthest such e (rows never increase)
    last = np.searchsorted(-rows, -(rows - 63), side="right")  # first step whose row is <= rows[s] - 64
    idx = np.stack([np.arange(len(rows)), last], axis=1).reshape(-1)
    pad = np.concatenate([slots, slots[-1:]])  # (reduceat takes no index at len)
    hi = np.maximum.reduceat(pad, idx)[::2]
    lo = np.minimum.reduceat(pad, idx)[::2]
    return int((hi - slots).max()), int((slots - lo).max())


def test_drift_of_a_known_path():
    rows = np.array([9, 8, 8, 8, 7, 6, 5])
    assert _drift(rows, np.array([4, 4, 3, 2, 2, 3, 4])) == (2, 2)
    rows = np.arange(200, 0, -1)
    assert _drift(rows, np.arange(200)) == (63, 0) and _drift(rows, np.arange(200)[::-1].copy()) == (0, 63)


def test_path_geometry_is_the_band_of_the_definition():
    """A path that is all D down column 0 runs from slot d at row m to slot 2 d - 1 at row 1."""
    cases, tbs = oc.traced()
    (note, q, t), tb = cases[-1], tbs[-1]
    assert note.startswith("column 0") and (tb["distance"], tb["end"], tb["start"], tb["ops"]) == (4096, 0, 0, "D" * 4096)
    rows, slots, ops = oc.path_geometry(q, t, tb)
    assert rows.tolist() == list(range(4096, 0, -1)) and slots.tolist() == list(range(4096, 8192))
    assert 2 * tb["distance"] + 1 == 8193 and tb["distance"] == au.MAX_EDITS


def test_run_cases_hold_their_runs():
    cases, tbs = oc.traced()
    planted = oc.run_cases()
    assert len(planted) == 2 * (3 * 4 + 3 + 2 + 1 + 1) + 2 + 3 + 3
    assert {ln for _, _, _, runs in planted for _, ln in runs} >= set(oc.RUN_LENGTHS)
    for (note, q, t, runs), (note2, q2, t2), tb in zip(planted, cases, tbs):
        assert (note, q, t) == (note2, q2, t2)
        got = [(r & 3, r >> 2) for r in au.runs_of(tb["ops"]) if r & 3 in (oc.I, oc.D)]
        assert got == runs, (note, vu.cigar(tb["ops"]))  # exactly the planted runs, in order, and no other indel
        assert tb["distance"] == sum(ln for _, ln in runs), note
    by = dict((c[0], tb) for c, tb in zip(cases, tbs))
    assert by["D40 first rows"]["ops"].startswith("D" * 40 + "=") and by["D40 first rows"]["start"] == 0
    assert by["D70 last rows"]["ops"].endswith("=" + "D" * 70)
    tb = by["I50, 60 before column n"]
    assert tb["ops"].endswith("=" + "I" * 50 + "=" * 60) and tb["end"] == oc.LEFT + oc.CORE + 50  # column n cuts the band


def test_cases_reach_the_special_code(geometry):
    """What the kernel's traceback window, chunk carry, band edges and tile rows need, from the checker alone."""
    I, D = ord("I"), ord("D")
    carry, up, down, tile_row, slot0, slot_last = [], [], [], [], [], []
    for note, m, d, W, rows, slots, ops in geometry:
        assert len(rows) and slots.min() >= 0 and slots.max() < W, note  # the path stays in its band
        if W <= 64:
            continue
        # an I step out of a slot that is a multiple of 64: the left move crosses into another 64-slot chunk
        if np.any((ops == I) & (slots % 64 == 0) & (slots > 0)):
            carry.append(note)
        u, dn = _drift(rows, slots)
        if u > 32:
            up.append(note)
        if dn > 32:
            down.append(note)
        # a D run over rows i + 1 and i with (m - i) % 64 == 0: it crosses from one 64-row tile from row m into the next
        dr = rows[ops == D]
        if np.any(((m - dr) % 64 == 0) & (dr < m) & np.isin(dr + 1, dr)):
            tile_row.append(note)
        if slots.min() == 0:
            slot0.append(note)
        if slots.max() == W - 1:
            slot_last.append(note)
    assert len(carry) >= 10 and "I200 at 300" in carry and "unrelated 4000 x 4200" in carry
    assert len(up) >= 8 and len(down) >= 8 and {"D70 then I90", "I90 then D70"} <= set(up) & set(down)
    assert len(tile_row) >= 8 and "column 0, d = 4096" in tile_row
    assert len(slot0) >= 8 and len(slot_last) >= 8
    ds = [d for _, _, d, _, _, _, _ in geometry]
    for lo, hi in ((33, 64), (65, 128), (129, 1024), (1025, 4096)):
        assert any(lo <= d <= hi for d in ds), (lo, hi)
    assert max(ds) == au.MAX_EDITS and sum(d > vu.MAX_EDITS for d in ds) == 2
    assert len(geometry) == len(oc.run_cases()) + 9


def test_scan_cases_are_what_they_claim():
    cases, ref = oc.scanned()
    assert len(cases) == 5 * len(oc.SCAN_SHAPES)
    for m, K, last_k in oc.SCAN_SHAPES:
        L, lk = oc.lanes(m, K)
        mine = [(note, q, t) for note, q, t in cases if note.startswith("m=%d " % m)]
        assert len(mine) == 5 and all(len(q) == m for _, q, _ in mine)
        assert sorted(len(t) for _, _, t in mine)[:2] == [1, L - 1] and L - 1 > 1
        assert all(len(t) >= 3000 for _, _, t in mine[:3])
    by = dict((c[0], r) for c, r in zip(cases, ref))
    assert oc.lanes(8192, 2) == (64, 1) and (8192 - 1) % 64 == 63
    # related texts are found (far below an unrelated text's distance), with the N run and the missing stretch paid for
    assert by["m=4200 N70 in, 70 out"][0] == 140 and by["m=8192 N70 in, 70 out"][0] == 140
    assert 300 < by["m=8400 mutated"][0] < 1700 < by["m=8400 unrelated"][0]


def test_host_trace_scan_and_script_equal_the_checker(al):
    cases, tbs = oc.traced()
    pairs = [(q, t) for _, q, t in cases]
    assert vu.scan_host(pairs) == [(tb["distance"], tb["end"]) for tb in tbs]
    seq, jobs = oc.job_launch(cases, tbs)
    want_out, want_runs = oc.expected_trace(jobs, tbs)
    rc, out, runs = al.trace(seq, jobs, "cpu")
    assert rc == 0
    for k, ((note, q, t), tb) in enumerate(zip(cases, tbs)):
        assert out[k].tolist() == want_out[k].tolist(), note
        a = int(jobs[k, 7])
        assert runs[a: a + out[k, 6]].tolist() == au.runs_of(tb["ops"][::-1]), note
        if tb["distance"] <= vu.MAX_EDITS:
            assert vu.script(q, t, tb["distance"], tb["end"]) == (0, tb["start"], vu.op_counts(tb["ops"]), vu.cigar(tb["ops"])), note
            assert au.cigar_of(runs[a: a + out[k, 6]].tolist()) == vu.cigar(tb["ops"]), note
    assert np.array_equal(runs, want_runs)


def test_host_scan_equals_the_checker():
    cases, ref = oc.scanned()
    got = vu.scan_host([(q, t) for _, q, t in cases])
    bad = [(note, g, r) for (note, _, _), g, r in zip(cases, got, ref) if g != r]
    assert not bad, bad


def test_paf_of_three_run_reads(al):
    target, records = oc.paf_batch()
    paf, counts, per = au.expected_batch(target, b"tgt", records, 0.5)
    assert [e["strand"] for e in per] == [0, 0, 1] and [e["d"] for e in per] == [65, 129, 98]
    res = al.align_records(target, b"tgt", records, device="cpu", max_error=0.5)
    assert res["paf"] == paf and res["counts"] == counts and counts["mapped"] == 3
    lines = res["paf"].splitlines(True)
    assert len(lines) == 3
    for line, (name, s) in zip(lines, records):
        assert line.startswith(name + b"\t")
        au.check_line(line, target, s)
