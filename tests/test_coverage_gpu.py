"""coverage_qc on the GPU: K_covparse + K_covfinish (mpc_coverage_run) against
the independent checker (tests/cov_util.py) over every lane-chunk and tile
boundary in one launch, under same-address contention, with more records than
the grid has waves, record by record, the status codes, the Synth batch against
the host walk, and the CLI on device 0 against --device cpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cov_util as cu

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "minion-plasmid-consensus_amd", "coverage_qc.py")
LENGTHS = [1, 65, 5000]
REGIONS = [(0, 1), (3, 60), (10, 4990)]
_TWO = (b":0", b":1", b"+a", b"-c")
_THREE = (b":00", b":02", b"*ag", b"+ac", b"-ct")


def pad(rng, n):
    """A valid cs of exactly n bytes (n = 0 or n >= 2) from two- and three-byte tokens."""
    assert n == 0 or n >= 2
    out = []
    while n:
        k = 3 if n == 3 or (n > 4 and rng.random() < 0.4) else 2
        out.append((_TWO if k == 2 else _THREE)[int(rng.integers(0, 4 if k == 2 else 5))])
        n -= k
    return b"".join(out)


def boundary_records(T):
    """(what, record): every shape the issue lists, on the 5000-base target
    unless the record is about a target's ends."""
    rng = np.random.default_rng(17)
    out = []
    for n in (0, 2, T - 1, T, T + 1, 2 * T + 3):
        out.append(("len %d" % n, (2, int(rng.integers(0, 3000)), pad(rng, n))))
        out.append(("Z: + len %d" % n, (2, int(rng.integers(0, 3000)), b"Z:" + pad(rng, n))))
    for b in (64, T):
        tail = pad(rng, 9)
        for what, cs in (
                ("number straddles", pad(rng, b - 3) + b":0123"),
                ("number ends at", pad(rng, b - 4) + b":123"),
                ("nine digits straddle", pad(rng, b - 5) + b":000000321"),
                ("operator last before", pad(rng, b - 1) + b":7"),
                ("sub split 1+2", pad(rng, b - 1) + b"*ag"),
                ("sub split 2+1", pad(rng, b - 2) + b"*ct"),
                ("deletion crosses", pad(rng, b - 3) + b"-acgtac"),
                ("insertion crosses", pad(rng, b - 3) + b"+acgtac"),
                ("deletion starts at", pad(rng, b) + b"-acg"),
                ("deletion operator last before", pad(rng, b - 1) + b"-g"),
                ("deletion covers a tile", pad(rng, b - 3) + b"-" + cu.letters(rng, 2 * T + 10)),
                ("insertion covers a tile", pad(rng, b - 3) + b"+" + cu.letters(rng, 2 * T + 10))):
            for suffix in (b"", tail):
                out.append(("%s %d%s" % (what, b, " + tail" if suffix else ""), (2, int(rng.integers(0, 3000)), cs + suffix)))
    # a target's ends: position 0, L - 1, an insertion at L
    out += [("ends", r) for r in (
        (0, 0, b"*ag"), (0, 0, b"+a:1+c"), (0, 0, b"-a"), (0, 1, b"+tt"), (0, 1, b""),
        (1, 0, b":65+a"), (1, 64, b"*ag"), (1, 0, b"-a:63-c"), (1, 0, b"+g*ac"), (1, 65, b"Z:+acgt"),
        (2, 0, b"-ac:4990*ag-acgtacg+t"), (2, 4999, b":1+a+c"), (2, 4999, b"-t"), (2, 0, b":5000"))]
    return out


@pytest.fixture(scope="module")
def tile(pkg):
    T = pkg.coverage.tile_bytes()
    assert T % 64 == 0 and T >= 128
    return T


@pytest.fixture(scope="module")
def boundary(tile):
    cases = boundary_records(tile)
    records = [r for _, r in cases]
    return cases, records, cu.check(records, LENGTHS, REGIONS, min_depth=3)


def test_boundary_batch_one_launch(pkg, boundary):
    cases, records, (status, rows, stats, _) = boundary
    assert status == (cu.OK, 0)
    got_rows, got_stats = cu.run(pkg, records, LENGTHS, REGIONS, min_depth=3, device=0)
    assert np.array_equal(got_stats, stats), (got_stats.tolist(), stats.tolist())
    bad = np.nonzero((got_rows != rows).any(axis=1))[0]
    assert not len(bad), (bad[:8], got_rows[bad[:8]], rows[bad[:8]])
    assert rows[0].all() and rows[1, 3] and not rows[1, :3].any()  # position 0 and the insertion at L of the 1-base target


def test_every_boundary_record_alone(pkg, boundary):
    """One launch per distinct shape would be slow; instead every record gets a
    target of its own in ONE launch, so a wrong record is named."""
    cases, records, _ = boundary
    alone = [(k, ts, cs) for k, (_, ts, cs) in enumerate(records)]
    lengths = [LENGTHS[s] for s, _, _ in records]
    regions = [(0, L) for L in lengths]
    _, rows, stats, _ = cu.check(alone, lengths, regions)
    got_rows, got_stats = cu.run(pkg, alone, lengths, regions, device=0)
    off = np.concatenate([[0], np.cumsum(np.asarray(lengths) + 1)])
    wrong = [cases[k][0] for k in range(len(alone))
             if not (np.array_equal(got_rows[off[k]:off[k + 1]], rows[off[k]:off[k + 1]]) and np.array_equal(got_stats[k], stats[k]))]
    assert not wrong, wrong


def test_single_record_launches(pkg, boundary, tile):
    cases, records, _ = boundary
    picks = [k for k, (what, _) in enumerate(cases) if what in ("number straddles 64", "deletion covers a tile %d + tail" % tile,
                                                                   "sub split 2+1 %d" % tile)]
    assert len(picks) == 3
    total = np.zeros((sum(LENGTHS) + 3, 4), np.uint32)
    for k in picks:
        _, rows, stats, _ = cu.check([records[k]], LENGTHS, REGIONS)
        got_rows, got_stats = cu.run(pkg, [records[k]], LENGTHS, REGIONS, device=0)
        assert np.array_equal(got_rows, rows) and np.array_equal(got_stats, stats), cases[k][0]
        total += got_rows
    assert np.array_equal(cu.run(pkg, [records[k] for k in picks], LENGTHS, REGIONS, device=0)[0], total)


def test_contention_and_determinism(pkg):
    """4,096 identical records and 4,096 random spans on one 120-base target:
    every span edge lands on a handful of words."""
    rng = np.random.default_rng(23)
    same = (0, 0, b"Z::40*ag-ac+t:58-acgtacgtacgtacgtac+g:1")
    records = [same] * 4096
    for _ in range(4096):
        a = int(rng.integers(0, 100))
        records.append((0, a, cu.random_cs(rng, int(rng.integers(1, 121 - a)), 0.05, 0.05, 0.05)))
    order = rng.permutation(len(records))
    records = [records[k] for k in order]
    _, rows, stats, _ = cu.check(records, [120], [(5, 115)], min_depth=5000)
    first = cu.run(pkg, records, [120], [(5, 115)], min_depth=5000, device=0)
    assert np.array_equal(first[0], rows) and np.array_equal(first[1], stats)
    again = cu.run(pkg, records, [120], [(5, 115)], min_depth=5000, device=0)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()


def test_more_records_than_waves(pkg):
    """70,000 one-token records over two targets (the second longer than the
    LDS slice, so its middle rows take the direct path)."""
    rng = np.random.default_rng(29)
    lengths, regions = [50, 9000], [(0, 50), (100, 8000)]
    toks = (b":1", b"*ag", b"-a", b"+c", b":3")
    records = []
    for k in range(70000):
        s = int(k >= 35000)
        records.append((s, int(rng.integers(0, lengths[s] - 3)), toks[int(rng.integers(0, 5))]))
    _, rows, stats, _ = cu.check(records, lengths, regions, min_depth=4)
    got_rows, got_stats = cu.run(pkg, records, lengths, regions, min_depth=4, device=0)
    assert np.array_equal(got_rows, rows) and np.array_equal(got_stats, stats)


def test_finish_carries_across_its_1024_row_steps(pkg):
    """K_covfinish sums 1,024 rows per step and carries the sums into the next:
    targets of 1, 1,024, 1,025 and 2,049 positions, spans and deletions across
    positions 1,023 / 1,024 and 2,047 / 2,048, the regions' ends on those seams;
    rows and stats equal the host walk's."""
    rng = np.random.default_rng(37)
    lengths, regions = [1, 1024, 1025, 2049], [(0, 1), (0, 1024), (1024, 1025), (1024, 2048)]
    records = [(0, 0, b":1"), (0, 0, b"*ag"), (0, 1, b"+a")]
    for s, L in enumerate(lengths[1:], 1):
        for seam in (m for m in (1024, 2048) if m <= L):
            for a, cs in ((seam - 3, b":6"), (seam - 5, b":5"), (seam, b":1"), (seam - 1, b"*ag"), (seam, b"*ct"), (seam, b"+ac"),
                          (seam - 2, b"-acgt"), (seam - 4, b"-acgt"), (seam, b"-a"), (seam - 1, b"-c:1"), (0, b":%d" % seam)):
                if cu.walk(cs, a, L)[0] == cu.OK:
                    records += [(s, a, cs)] * 2
        for _ in range(60):
            a = int(rng.integers(0, L - 1))
            records.append((s, a, cu.random_cs(rng, int(rng.integers(1, L - a + 1)), 0.03, 0.03, 0.03)))
    assert 200 < len(records) < 500
    cs, off, ts, rs = cu.pack(records)
    dev = pkg.coverage.run(cs, off, ts, rs, lengths, regions, 40, device=0)
    host = pkg.coverage.run(cs, off, ts, rs, lengths, regions, 40, device="cpu")
    assert np.array_equal(dev["rows"], host["rows"]) and np.array_equal(dev["stats"], host["stats"])
    pos = np.concatenate([[0], np.cumsum(np.asarray(lengths) + 1)])
    for s, seam in ((1, 1023), (2, 1024), (3, 1024), (3, 2047), (3, 2048)):  # depth and deletions on both sides of a seam
        assert host["rows"][pos[s] + seam, 0] and host["rows"][pos[s] + seam, 1], (s, seam)
    assert host["stats"][:, 7].all() and host["stats"][1:, 11].any()


@pytest.mark.parametrize("name,rec,code", cu.BAD, ids=[b[0] for b in cu.BAD])
def test_status_one_bad_record_per_rule(pkg, name, rec, code):
    batch = cu.GOOD + [rec] + cu.GOOD
    assert cu.status_of(pkg, batch, [20], device=0) == (code, 3)


def test_status_smaller_index_wins_far_apart(pkg, tile):
    rng = np.random.default_rng(31)
    batch = [cu.GOOD[k % 3] for k in range(9000)]
    batch[8900] = (0, 0, b"=A")
    batch[100] = (0, 10, b":11")
    assert cu.status_of(pkg, batch, [20], device=0) == (cu.RANGE, 100)
    batch[100], batch[8900] = batch[8900], batch[100]
    assert cu.status_of(pkg, batch, [20], device=0) == (cu.MALFORMED, 100)
    # malformed late in a long cs, out of range early in the same record: malformed wins
    batch[100] = cu.GOOD[0]
    batch[50] = (0, 0, b":30" + pad(rng, 2 * tile) + b"~")
    assert cu.status_of(pkg, batch, [20], device=0) == (cu.MALFORMED, 50)


def test_sample_index_outside_the_targets(pkg):
    cu.case_bad_sample(pkg, 0)


def test_run_refuses_bad_tables_before_launch(pkg):
    import torch
    L = pkg.engine.lib()
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda:0")
    cs = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    rows = torch.full((11 * 4,), -5, dtype=torch.int32, device="cuda:0")
    stats = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    status = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    smp = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    off, ts = i64([0, 0]), i64([0])

    def call(n_records, pos_off, region, n_samples=1):
        d_pos, d_reg = i64(pos_off), i64(region)
        rc = L.mpc_coverage_run(cs.data_ptr(), off.data_ptr(), ts.data_ptr(), smp.data_ptr(), n_records, d_pos.data_ptr(),
                                d_reg.data_ptr(), n_samples, 0, rows.data_ptr(), stats.data_ptr(), status.data_ptr(), None)
        torch.cuda.synchronize()
        return rc
    for args, word in (((-1, [0, 11], [0, 10]), b"n_records"), ((1, [0, 11], [0, 10], 0), b"n_samples"),
                       ((1, [0, 11], [0, 11]), b"region"), ((1, [0, 2 ** 31], [0, 10]), b"2^31"),
                       ((1, [0, 0], [0, 0]), b"pos_off")):
        assert call(*args) == -1 and word in L.mpc_last_error(), args
    torch.cuda.synchronize()
    assert (rows == -5).all()
    assert call(1, [0, 11], [0, 10]) == 0
    torch.cuda.synchronize()
    assert not rows.any() and status.tolist() == [0, 0] and stats.tolist()[:2] == [1, 0]


def test_synth_batch_device_equals_host(pkg):
    records, lengths, regions, samples = cu.synth_batch(pkg)
    cs, off, ts, rs = cu.pack(records)
    tend = np.concatenate([s["tend"] for s in samples])
    dev = pkg.coverage.run(cs, off, ts, rs, lengths, regions, 295, device=0, tend=tend)
    host = pkg.coverage.run(cs, off, ts, rs, lengths, regions, 295, device="cpu", tend=tend)
    assert np.array_equal(dev["rows"], host["rows"]) and np.array_equal(dev["stats"], host["stats"])
    assert host["stats"][:, 11].any() and host["rows"][:, 1:].any(axis=0).all()


def test_cli_device_equals_cli_cpu(pkg, tmp_path):
    syn = pkg.synth.Synth(n=600, n_reads=300, profile="indel", seed=4)
    pafs = [str(tmp_path / "sense.paf"), str(tmp_path / "antisense.paf")]
    syn.write_files(paf0=pafs[0], paf1=pafs[1])
    outs = {}
    for dev in ("0", "cpu"):
        rep, per = tmp_path / ("cov_%s.tsv" % dev), tmp_path / ("depth_%s.tsv" % dev)
        p = subprocess.run([sys.executable, CLI, "--paf"] + pafs + ["--region", "40:560", "--report", str(rep), "--per-base",
                            str(per), "--min-mean-coverage", "200", "--min-depth", "100", "--device", dev],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        outs[dev] = (rep.read_bytes(), per.read_bytes())
    assert outs["0"] == outs["cpu"]
    lines = outs["0"][0].decode().splitlines()
    assert len(lines) == 2 * 23 + 1 and lines[-1] == "verdict\tPASS" and lines[3] == "records\t300"
    assert len(outs["0"][1].splitlines()) == 1 + 2 * 601
