"""K_flank works a 256-byte segment's four 64-byte groups together (one batch
of LDS reads, four independent owner scans linked by a scalar carry, one batch
of ds_bpermute).  Shapes at which that regrouping can go wrong, each against the
oracle (full pileup: min_depth_factor = -1), and the KeyError bookkeeping per
group against the values the group-after-group kernel reported.

A wave owns 64 consecutive reads (reads 64 w .. 64 w + 63 of the launch); byte x
of its side's contiguous flank bytes is in stage x // 2032, and inside the stage
in segment (x % 2032) // 256, group (x % 256) // 64 of that segment.
"""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

KEYS = ("base", "chrom1", "chrom2", "count", "count2", "total")
STAGE, SEG, GROUP = 2032, 256, 64  # csrc/mpc_k_rows.h: kFStage, kFSeg, bytes per group


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


def _wave_bytes(smp, side, w):
    off = smp["up_off" if side == 0 else "down_off"]
    return int(off[min(64 * w + 64, len(off) - 1)] - off[64 * w])


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 130])
def test_partial_last_wave(pkg, n_reads):
    """A last wave of 1, 63, 64, 1 and 2 reads: dead lanes, last < 63."""
    smp = pkg.synth.Synth(n=300, n_reads=n_reads, profile="indel", seed=90 + n_reads, frac_partial=0.2,
                          flank=(0, 40)).sample(0)
    assert len(smp["tstart"]) == n_reads
    _parity(pkg, [smp], ("last_wave", n_reads))


def test_short_and_empty_flanks(pkg):
    """Flanks of 0-3 bytes: groups without a start (owner from the carry alone,
    or none: every flank of the wave is behind), groups with tens of starts."""
    smp = pkg.synth.Synth(n=400, n_reads=400, profile="indel", seed=96, frac_partial=0.3, flank=(0, 3)).sample(0)
    ul, dl = np.diff(smp["up_off"]), np.diff(smp["down_off"])
    assert (ul == 0).sum() > 50 and (dl == 0).sum() > 50 and (ul > 1).sum() > 50
    assert max(_wave_bytes(smp, 0, w) for w in range(7)) < 4 * GROUP  # the wave's later groups hold no byte
    _parity(pkg, [smp], "short_flanks")


def test_flanks_longer_than_a_segment(pkg):
    """Flanks of 250-270 bytes: most groups and some segments hold no start (the
    owner is the carry, across groups, segments and stages), and the rows run
    past the 256-row LDS window into the global atomics."""
    smp = pkg.synth.Synth(n=500, n_reads=200, profile="indel", seed=97, frac_partial=0.1, flank=(250, 270)).sample(0)
    assert np.diff(smp["up_off"]).min() >= 250 and np.diff(smp["up_off"]).max() > SEG
    assert _wave_bytes(smp, 0, 0) > 7 * STAGE
    _parity(pkg, [smp], "long_flanks")


def test_stage_reload_and_moved_window(pkg):
    """More than 2032 bytes per wave and side: the stage reload, the last
    segment of a full stage (its group 3 reads past the staged bytes on dead
    lanes: the clamped index) and the carry across stages; half of the reads are
    partial alignments, whose flanks lie outside the voted window."""
    smp = pkg.synth.Synth(n=600, n_reads=300, profile="indel", seed=98, frac_partial=0.5, flank=(30, 100)).sample(0)
    assert min(_wave_bytes(smp, side, w) for side in (0, 1) for w in range(4)) > STAGE
    _parity(pkg, [smp], "stage_reload")


def test_chunk_across_two_samples(pkg):
    """Two samples of different reference lengths, 100 and 230 reads: the
    boundary falls inside a wave, and a block's chunk crosses it."""
    a = pkg.synth.Synth(n=300, n_reads=100, profile="indel", seed=99, frac_partial=0.2, flank=(0, 40)).sample(0)
    b = pkg.synth.Synth(n=450, n_reads=230, profile="default", seed=100, frac_partial=0.2, flank=(0, 64)).sample(0)
    _parity(pkg, [a, b], "two_samples")


# ---- KeyError position -------------------------------------------------------
# One valid sample (300 reads, flanks of 30-100 bytes, so wave 1 = reads 64..127
# holds two stages per side).  A first non-ACGT byte is patched into wave 1's
# bytes at stage, segment 1, group k, byte 5 of the group; a second one into the
# upstream flank of read 127 (the wave's last, a later read).  The reference
# raises KeyError at the smallest read index with a non-ACGT flank byte; FIRST
# is that read for each case, as the group-after-group kernel reported it
# (flags = DE_KEY = 8 in every case).
KEY_SPEC = dict(n=600, n_reads=300, profile="indel", seed=98, frac_partial=0.0, flank=(30, 100))
KEY_CASES = [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3), (1, 1, 0), (1, 1, 1), (1, 1, 2), (1, 1, 3)]  # side, stage, k
FIRST = {(0, 0, 0): 68, (0, 0, 1): 68, (0, 0, 2): 70, (0, 0, 3): 71,
         (1, 1, 0): 102, (1, 1, 1): 103, (1, 1, 2): 104, (1, 1, 3): 105}
KEY_FLAGS = 8


@pytest.fixture(scope="module")
def key_sample(pkg):
    return pkg.synth.Synth(**KEY_SPEC).sample(0)


@pytest.mark.parametrize("side,stage,k", KEY_CASES, ids=lambda v: str(v))
def test_key_error_first_read_per_group(pkg, key_sample, side, stage, k):
    eng = pkg.engine
    smp = dict(key_sample)
    name = "up" if side == 0 else "down"
    off = smp[name + "_off"]
    x = stage * STAGE + SEG + GROUP * k + 5  # byte of wave 1's range on this side
    assert x < int(off[128] - off[64])
    p = int(off[64]) + x
    first = int(np.searchsorted(off, p, side="right")) - 1  # the read whose flank holds byte p
    assert 64 <= first < 127 and first == FIRST[side, stage, k]
    smp[name] = smp[name].copy()
    smp[name][p] = ord("N")
    if side == 1:
        smp["up"] = smp["up"].copy()
    smp["up"][int(smp["up_off"][128]) - 1] = ord("R")  # last upstream byte of read 127
    with pytest.raises(oracle.OracleError) as o:
        _oracle(smp)
    assert (o.value.code, o.value.read) == (1, first)
    with pytest.raises(eng.DataError) as e:
        eng.pileup([smp], -1.0, 1.0)
    print("side %d stage %d group %d: flags %d first read %d" % (side, stage, k, e.value.flags, e.value.read))
    assert (e.value.flags, e.value.read) == (KEY_FLAGS, FIRST[side, stage, k])
