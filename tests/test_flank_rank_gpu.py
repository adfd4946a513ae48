"""K_flank finds the flank of a byte by rank: a bitmap of the start bytes of a
stage (one bit per staged byte, 64 words per wave), a popcount of the starts at
or before the byte (carried over groups, segments and stages) and a table of row
offsets indexed by that rank.  Shapes at which that can go wrong, each as a full
pileup against the oracle (min_depth_factor = -1), and the KeyError bookkeeping
through the engine's status words.  The cases with an exact number of bytes
outside the LDS window were written for a per-wave queue of those bytes (64
global atomics at a time); the queue was measured and dropped,
the cases stay: they mix window and global tallies inside one group.

A wave owns 64 consecutive reads (reads 64 w .. 64 w + 63 of the launch); byte x
of its side's contiguous flank bytes is in stage x // 2032, and inside the stage
in segment (x % 2032) // 256, group (x % 256) // 64, bitmap word (x % 2032) // 32.
The flank lengths are constructed: a Synth sample keeps its reads (ref, cs,
tstart) and gets new up / up_off / down / down_off of random ACGT bytes.

Which bytes miss the window: at these sizes a block is one chunk of 128 reads,
and the window of a side holds the 256 rows from the first row of the gap that
two of the chunk's first, middle and last read use (full-length reads: gap 0
upstream, gap n downstream).  A read that starts at or after base 300 has its
upstream flank more than 256 rows behind gap 0, a read that ends at or before
base 300 its downstream flank that far ahead of gap n.
"""
import numpy as np
import pytest

import neg_util
import oracle

pytestmark = pytest.mark.gpu

KEYS = ("base", "chrom1", "chrom2", "count", "count2", "total")
STAGE, SEG, GROUP, WORD = 2032, 256, 64, 32  # csrc/mpc_k_rows.h: kFStage, kFSeg, bytes per group, per bitmap word
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N_REF = 600


def _oracle(s, mdf=-1.0, gtf=1.0):
    return oracle.run_packed(s["ref"], s["cs"], s["cs_off"], s["tstart"], s["up"], s["up_off"], s["down"],
                             s["down_off"], mdf, gtf)


def _parity(pkg, samples, tag):
    res = pkg.engine.pileup(samples, -1.0, 1.0)
    for s, (smp, got) in enumerate(zip(samples, res)):
        exp = _oracle(smp)
        assert got["max_depth"] == exp["max_depth"], (tag, s)
        for k in KEYS:
            a, b = np.asarray(got[k], dtype=np.int64), np.asarray(exp[k], dtype=np.int64)
            assert a.shape == b.shape, (tag, s, k, a.shape, b.shape)
            bad = np.nonzero(a != b)[0][:5]
            assert bad.size == 0, f"{tag} sample {s} {k} differs at {bad.tolist()}: {a[bad].tolist()} vs {b[bad].tolist()}"


def _with_flanks(smp, ul, dl, seed):
    """The sample with upstream / downstream flanks of the given lengths."""
    rng = np.random.default_rng(seed)
    out = dict(smp)
    for name, ln in (("up", ul), ("down", dl)):
        ln = np.asarray(ln, dtype=np.int64)
        assert len(ln) == len(smp["tstart"]) and ln.min() >= 0
        off = np.zeros(len(ln) + 1, dtype=np.int64)
        np.cumsum(ln, out=off[1:])
        out[name + "_off"] = off
        out[name] = rng.choice(ACGT, int(off[-1])).astype(np.uint8)
    return out


def _starts(ln):
    """Start byte of every non-empty flank, relative to the first lane's."""
    ln = np.asarray(ln, dtype=np.int64)
    return (np.cumsum(ln) - ln)[ln > 0]


@pytest.fixture(scope="module")
def base(pkg):
    """128 reads on 600 bases, half of them partial alignments: one chunk of two
    waves whose three voters (reads 0, 64, 127) are full-length.  Never modified."""
    smp = pkg.synth.Synth(n=N_REF, n_reads=128, profile="indel", seed=201, frac_partial=0.5, flank=(0, 40),
                          antisense=False).sample(0)
    full = (smp["tstart"] == 0) & (smp["tend"] == N_REF)
    assert full[[0, 64, 127]].all()
    return smp


def _random_lengths(seed, n=128, hi=40):
    return np.random.default_rng(seed).integers(0, hi + 1, n)


# ---- starts on word, group, segment and stage edges ---------------------------

def test_starts_on_edges(pkg, base):
    """Wave 0, both sides: flanks start on bytes 31, 32, 63, 64, 255, 256, 2031
    and 2032 (the last bit of a bitmap word and the first of the next, of a
    group, a segment, a stage); the flank from byte 2032 runs to byte 4071, so it
    begins in stage 1 and ends in stage 2 (the bitmap is rebuilt with no start
    for it, its rank comes from the carry); the flank before it is the last byte
    of stage 0.  Downstream the same lengths follow three empty lanes."""
    head = [31, 1, 31, 1, 191, 1, 1775, 1, 2040]
    ul = _random_lengths(1)
    ul[:len(head)] = head
    dl = _random_lengths(2)
    dl[:3] = 0
    dl[3:3 + len(head)] = head
    for ln in (ul, dl):
        st = set(_starts(ln[:64]).tolist())
        assert {0, 31, 32, 63, 64, 255, 256, 2031, 2032, 4072} <= st
        assert int(ln[:64].sum()) > 2 * STAGE
    _parity(pkg, [_with_flanks(base, ul, dl, 3)], "edges")


def test_every_start_offset_in_a_word(pkg, base):
    """Flanks of 33 bytes: consecutive starts fall on bits 0, 1, 2, ... of
    consecutive bitmap words, and 64 x 33 = 2112 bytes end in the second stage."""
    ul = np.full(128, 33)
    dl = np.full(128, 33)
    assert sorted(set((_starts(ul[:64]) % STAGE % WORD).tolist())) == list(range(32))
    _parity(pkg, [_with_flanks(base, ul, dl, 4)], "word_offsets")


# ---- rank extremes ---------------------------------------------------------------

def _rank_case(name):
    ul, dl = _random_lengths(10), _random_lengths(11)
    if name == "all_length_1":      # 64 starts in one group: ranks 1..64
        ul[:64] = 1
    elif name == "only_lane_0":     # one start; every later byte takes rank 1 from the carry
        ul[:64] = 0
        ul[0] = 700
    elif name == "only_lane_63":
        ul[:64] = 0
        ul[63] = 700
    elif name == "alternate_empty":  # rank k = lane 2 k + 1
        ul[0:64:2] = 0
        ul[1:64:2] = np.random.default_rng(12).integers(1, 41, 32)
    elif name == "side_empty":       # wave 0 has no upstream byte, wave 1 no downstream byte
        ul[:64] = 0
        dl[64:] = 0
    return ul, dl


@pytest.mark.parametrize("name", ["all_length_1", "only_lane_0", "only_lane_63", "alternate_empty", "side_empty"])
def test_rank_extremes(pkg, base, name):
    ul, dl = _rank_case(name)
    _parity(pkg, [_with_flanks(base, ul, dl, 13)], name)
    # the same lengths on the other side (downstream flanks of a wave all start on the window's rows)
    _parity(pkg, [_with_flanks(base, dl, ul, 14)], name + "_swapped")


# ---- flanks without a row ----------------------------------------------------------

def test_flanks_without_a_row(pkg):
    """A third of the reads start below 0: K_flank gives their upstream flanks
    no row (the wrapped odd positions take them), between flanks with rows --
    their bytes are skipped, their rank still counts."""
    smp = neg_util.neg_sample(31, n=400, n_reads=300, frac_neg=0.33, flank_max=40)
    neg = smp["tstart"] < 0
    ul = np.diff(smp["up_off"])
    assert 40 < int((neg & (ul > 0)).sum()) < 200
    inner = neg[1:-1] & ~neg[:-2] & ~neg[2:] & (ul[1:-1] > 0) & (ul[:-2] > 0) & (ul[2:] > 0)
    assert inner.sum() > 5  # a flank without a row between two with rows
    _parity(pkg, [smp], "no_row")


# ---- rows outside the window ---------------------------------------------------------

def test_everything_outside_the_window(pkg):
    """Every read a partial alignment, flanks of 100-140 bytes: about 7.7 KB per
    wave and side, nearly all outside the window, across segments and stage
    reloads."""
    smp = pkg.synth.Synth(n=N_REF, n_reads=192, profile="indel", seed=210, frac_partial=1.0, flank=(100, 140),
                          antisense=False).sample(0)
    assert int(smp["up_off"][64]) > 3 * STAGE and int(smp["down_off"][64]) > 3 * STAGE
    _parity(pkg, [smp], "off_window_many")


def _off_window_lengths(base, side, total, seed):
    """Flank lengths with exactly ``total`` bytes of wave 0 outside the window on
    ``side``: spread over wave 0's reads that lie 300 bases from the voted gap;
    its other partial reads get no flank, full-length reads up to 40 bytes."""
    far = (base["tstart"] >= 300) if side == 0 else (base["tend"] <= 300)
    full = (base["tstart"] == 0) & (base["tend"] == N_REF)
    ln = _random_lengths(seed)
    ln[~full] = 0
    ln[[0, 64, 127]] = 20  # the voters: non-empty flanks at the hot gap
    idx = np.nonzero(far[:64])[0]
    assert len(idx) >= 4
    share = np.full(len(idx), total // len(idx))
    share[:total % len(idx)] += 1
    ln[idx] = share
    assert int(ln[:64][far[:64]].sum()) == total and int(ln[:64][~far[:64] & ~full[:64]].sum()) == 0
    return ln


@pytest.mark.parametrize("total", [1, 63, 64, 65, 191, 192, 193])
@pytest.mark.parametrize("side", [0, 1])
def test_exact_count_outside_the_window(pkg, base, side, total):
    """Exactly ``total`` bytes of wave 0 miss the window on one side, in a few
    flanks among the window's: one byte, a group's worth and one more or less,
    three groups' worth and one more or less."""
    ln = _off_window_lengths(base, side, total, 20 + total)
    other = _random_lengths(40 + total)
    ul, dl = (ln, other) if side == 0 else (other, ln)
    _parity(pkg, [_with_flanks(base, ul, dl, 60 + total)], ("off_window", side, total))


# ---- KeyError bookkeeping ------------------------------------------------------------

def _key_sample(base):
    ul = _off_window_lengths(base, 0, 150, 70)
    dl = _random_lengths(71)
    return _with_flanks(base, ul, dl, 72)


def _expect_key_error(pkg, smp, first):
    with pytest.raises(oracle.OracleError) as o:
        _oracle(smp)
    assert (o.value.code, o.value.read) == (1, first)
    with pytest.raises(pkg.engine.DataError) as e:
        pkg.engine.pileup([smp], -1.0, 1.0)
    print("flags %d first read %d" % (e.value.flags, e.value.read))
    assert (e.value.flags, e.value.read) == (pkg.engine.DE_KEY, first)


def _patch(smp, name, read, at, byte):
    smp[name] = smp[name].copy()
    off = smp[name + "_off"]
    assert off[read + 1] - off[read] > at
    smp[name][int(off[read]) + at] = byte


def test_key_error_in_window(pkg, base):
    """A non-ACGT byte in the flank of a full-length read (rows in the window)."""
    smp = _key_sample(base)
    full = (base["tstart"] == 0) & (base["tend"] == N_REF)
    read = int(np.nonzero(full[:64] & (np.diff(smp["up_off"])[:64] > 3))[0][5])
    _patch(smp, "up", read, 2, ord("N"))
    _expect_key_error(pkg, smp, read)


def test_key_error_off_window(pkg, base):
    """A non-ACGT byte in the flank of a read that starts past base 300 (rows
    outside the window)."""
    smp = _key_sample(base)
    far = np.nonzero((base["tstart"] >= 300)[:64])[0]
    read = int(far[2])
    _patch(smp, "up", read, 7, ord("a"))  # (flanks are upper case at ingest: a lower-case base is a KeyError)
    _expect_key_error(pkg, smp, read)


def test_key_error_two_reads_in_a_wave(pkg, base):
    """Two bad reads in wave 0, the later one on the upstream side (tallied
    first) and the earlier one downstream, and a third in wave 1: the smallest
    read index is reported."""
    smp = _key_sample(base)
    ul, dl = np.diff(smp["up_off"]), np.diff(smp["down_off"])
    lo = int(np.nonzero(dl[:64] > 1)[0][3])
    hi = int(np.nonzero((ul[:64] > 1) & (np.arange(64) > lo))[0][4])
    w1 = 64 + int(np.nonzero(ul[64:] > 1)[0][0])
    _patch(smp, "down", lo, 1, ord("N"))
    _patch(smp, "up", hi, 0, ord("-"))
    _patch(smp, "up", w1, 1, ord("N"))
    assert lo < hi < w1
    _expect_key_error(pkg, smp, lo)


# ---- two samples in one wave ------------------------------------------------------------

def test_sample_boundary_inside_a_wave(pkg):
    """40 reads of one sample and 150 of another: the boundary falls inside
    wave 0, whose rank table and bitmap span both; the samples' hot gaps
    differ (300 and 450 bases), so the chunk's window serves one of them and
    the other's flanks take the global atomics."""
    a = pkg.synth.Synth(n=300, n_reads=40, profile="indel", seed=220, frac_partial=0.1, flank=(0, 40),
                        antisense=False).sample(0)
    b = pkg.synth.Synth(n=450, n_reads=150, profile="default", seed=221, frac_partial=0.1, flank=(20, 64),
                        antisense=False).sample(0)
    _parity(pkg, [a, b], "two_samples")
