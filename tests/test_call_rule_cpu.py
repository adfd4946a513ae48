"""tests/call_util.py against the C oracle (no GPU): the restatement of Steps
5-6 that tests/test_consensus_gpu.py holds the consensus kernels to, on every
tie class, on the float64 edges of the two threshold tests, and through the
``tally_sample`` builder.  The golden case t_call_rule (scripts/make_golden.py
--only call_rule) pins the same samples to the reference script itself."""
import itertools

import numpy as np
import pytest

import call_util as cu
import depth_util as du

SAMPLES = cu.TALLY_SAMPLES


def test_float_facts():
    """What the edge tuples rest on.  A platform where one of these fails does
    not compute the reference's two comparisons (:421, :428) as CPython's
    float64 does, and the edge tuples then test nothing."""
    assert 1.12 * 25 > 28, "1.12 * 25 must round above 28: (28, 25) is called N at gtf 1.12"
    assert 1.10 * 50 > 55, "1.10 * 50 must round above 55: (55, 50) is called N at gtf 1.10"
    assert 0.29 * 100 < 29, "0.29 * 100 must round below 29: a count of 29 is emitted at max depth 100"
    assert 0.5 * 10 == 5 and not 5 > 0.5 * 10
    assert np.float32(2 ** 24 + 1) == 2 ** 24, "float32 cannot tell 2^24 + 1 from 2^24: the compares need float64"
    assert float(2 ** 24 + 1) > float(2 ** 24)
    inf = float("inf")
    assert not (3 < inf * 0) and (3 < inf * 1)  # nan compares False: a single observed base survives gtf = inf
    assert cu.call_rule((55, 50, 0, 0), 1.10)[0] == ord("N") and cu.call_rule((55, 50, 0, 0), 1.0)[0] == ord("A")
    assert cu.call_rule((28, 25, 0, 0), 1.12)[0] == ord("N")
    assert cu.call_rule((5, 1, 0, 0), 5.0)[0] == ord("A") and cu.call_rule((4, 1, 0, 0), 5.0)[0] == ord("N")
    assert cu.call_rule((0, 7, 0, 0), inf) == (ord("T"), ord("T"), ord("X"), 7, 0, 7)
    assert cu.call_rule((0, 0, 0, 0), 1.0) is None


def test_depth_edges_straddle():
    for tuples, d, mdf in ((cu.D100, 100, 0.29), (cu.D10, 10, 0.5)):
        assert max(sum(t) for t in tuples) == d
        counts = {cu.call_rule(t, 1.0)[3] for t in tuples}
        thr = d * mdf
        assert {int(thr) - 1, int(thr), int(thr) + 1, int(thr) + 2} <= counts
        assert any(c > thr for c in counts) and any(c <= thr for c in counts)


def test_every_tie_class_in_every_assignment():
    """{0..3}^4 holds every tie class with every assignment of its counts to
    A, T, C, G (all distinct permutations of some count pattern of the class).
    The order among tied counts is fixed (reverse dict order), so where a tie
    decides the place the bases there cannot vary; wherever a place is decided
    by a strictly larger count, every base stands in it."""
    by_class = {}
    for t in cu.SMALL:
        c = cu.tie_class(t)
        if c:
            by_class.setdefault(c, {}).setdefault(tuple(sorted(t)), set()).add(t)
    assert set(by_class) == set(cu.TIE_CLASSES)
    for c, patterns in by_class.items():
        full = [p for p, seen in patterns.items() if seen == set(itertools.permutations(p))]
        assert full, c
    # a unique top over a tied second: every base on top; a top pair over a
    # distinct third: every base absent from the pair, every pair of bases tied
    tops = {cu.call_rule(t, 1.0)[1] for t in cu.SMALL if cu.tie_class(t) in ("second2", "second3")}
    assert tops == {ord(b) for b in cu.BASES}
    pairs = {tuple(i for i in range(4) if t[i] == max(t)) for t in cu.SMALL
             if cu.tie_class(t) == "top2_second_distinct"}
    assert pairs == set(itertools.combinations(range(4), 2))
    # the second of a top pair is one of the tied bases: the lower dict index
    for t in cu.SMALL:
        if cu.tie_class(t) == "top2_second_distinct":
            r = cu.call_rule(t, 1.0)
            lo = min(i for i in range(4) if t[i] == max(t))
            assert r[1] == ord("N") and r[2] == ord(cu.BASES[lo]) and r[3] == 2 * max(t) and r[4] == max(t)
    # the classes of the scaled and the large tuples the GPU test adds
    assert cu.tie_class((2 ** 24 + 1, 2 ** 24, 0, 0)) is None
    assert cu.tie_class((3000, 3000, 3000, 1000)) == "top3"


@pytest.fixture(scope="module")
def samples():
    out = {}
    for name in SAMPLES:
        for ref_n in (False, True):
            out[name, ref_n] = cu.tally_sample_named(name, ref_n)
    return out


@pytest.mark.parametrize("mdf,gtf", cu.SETTINGS)
@pytest.mark.parametrize("name", list(SAMPLES))
def test_restatement_matches_oracle(samples, name, mdf, gtf):
    """The oracle's calls on a tally_sample are call_rule on the intended
    tuples, thresholded by consensus_rows; the all-zero position is absent."""
    tuples = SAMPLES[name]
    meta = np.full(len(tuples), 3, np.uint8)
    exp = cu.consensus_rows(np.array(tuples), meta, [0, len(tuples)], mdf, gtf)[0]
    assert exp["max_depth"] == max(sum(t) for t in tuples)
    for ref_n in (False, True):
        smp = samples[name, ref_n]
        assert (b"N" in bytes(smp["ref"])) == ref_n
        got = du.oracle_one(smp, mdf, gtf)
        du.compare(got, exp, (name, ref_n, mdf, gtf))
    if mdf < 0:
        assert len(exp["base"]) == sum(1 for t in tuples if sum(t) > 0)


def test_tail_positions_are_all_match():
    tuples = cu.SMALL + cu.GTF_EDGE
    smp = cu.tally_sample(tuples, tail=37, ref_n=True, seed=3)
    D = max(sum(t) for t in tuples)
    ref = bytes(smp["ref"]).decode()
    rows = [t for t in tuples] + [tuple(D if b == ref[len(tuples) + k] else 0 for b in cu.BASES) for k in range(37)]
    exp = cu.consensus_rows(np.array(rows), np.full(len(rows), 3, np.uint8), [0, len(rows)], -1.0, 1.0)[0]
    du.compare(du.oracle_one(smp, -1.0, 1.0), exp, "tail")


def test_plain_batch_layout_matches_oracle():
    """plain_batch's predicted rows: the oracle emits one call per predicted
    row with a read on it, in order, with the predicted totals."""
    lengths = [5, 2, 9, 4]
    reads = [3, 1, 4, 0]
    ins = [[(2, "ACG"), (2, "T")], [(1, "GGTA")], [(1, "A"), (8, "CCCCC"), (8, "TT")], []]
    smps, metas = cu.plain_batch(lengths, reads, ins, seed=4)
    assert [len(m) for m in metas] == [5 + 3, 2 + 4, 9 + 1 + 5, 4]
    assert metas[0].tolist() == [3, 3, 2, 0, 0, 3, 3, 3]
    for smp, meta, nr in zip(smps, metas, reads):
        if nr == 0:
            continue
        got = du.oracle_one(smp, -1.0, 1.0)
        assert len(got["base"]) == len(meta)
        assert got["total"][meta == 3].tolist() == [nr] * int((meta == 3).sum())
        assert got["max_depth"] == nr
    # gap 8 of sample 2: CCCCC and TT right-aligned -> totals 1, 1, 1, 2, 2
    got = du.oracle_one(smps[2], -1.0, 1.0)
    assert got["total"][-6:-1].tolist() == [1, 1, 1, 2, 2]


def test_sample_files_roundtrip(tmp_path):
    """sample_files (what the golden case is written from) gives back the
    packed sample through the restated ingest."""
    import oracle
    smp = cu.tally_sample(cu.SMALL[:40] + cu.GTF_EDGE[:2], ref_n=True, seed=1)
    for fn, text in zip(("ref.fa", "reads.fa", "in.paf"), cu.sample_files(smp)):
        (tmp_path / fn).write_text(text)
    d = oracle.ingest_files(str(tmp_path / "ref.fa"), str(tmp_path / "in.paf"), str(tmp_path / "reads.fa"))
    assert bytes(d["ref"]) == bytes(smp["ref"]) and bytes(d["cs"]) == bytes(smp["cs"])
    assert d["cs_off"].tolist() == smp["cs_off"].tolist() and d["tstart"].tolist() == smp["tstart"].tolist()
    assert len(d["up"]) == 0 and len(d["down"]) == 0
