"""The handoff's host twins (mpc_align_cs_sizes_host, mpc_align_cs_write_host,
handoff.Pile on the host) against the checker of tests/handoff_util.py: the PAF
align renders, ingested with the reads by ingest.pack_sample.  Every comparison
is array equality.  No GPU."""
import numpy as np
import pytest

import handoff_util as hu


@pytest.fixture(scope="module")
def sets():
    return dict(hu.all_launches())


@pytest.fixture(scope="module")
def ho(pkg):
    return pkg.handoff


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_every_batch_equals_the_checker(pkg, sets, tmp_path, native):
    seen = 0
    for note, lns in sets.items():
        got, sizes = hu.host_sample(pkg, lns)
        hu.assert_same(got, hu.checker(pkg, tmp_path, lns, native=native), note)
        for ln, z in zip(lns, sizes):
            # the size row against the PAF columns the renderer writes
            text, line_len = pkg.align.render(ln.seq, ln.jobs, ln.strand, ln.out, ln.runs, ln.names, b"tgt")
            assert np.array_equal(z[:, 0] == 1, line_len > 0), note
            cols = [line.split(b"\t") for line in text.splitlines()]
            kept = z[z[:, 0] == 1]
            assert [[int(c[7]), int(c[8]), int(c[9]), int(c[10])] for c in cols] == kept[:, 4:8].tolist(), note
            assert not z[z[:, 0] == 0].any()
            seen += len(kept)
    assert seen > 50  # (the grid alone: 7 lengths x at least 8 kinds that get a line)


def test_run_counts_around_the_chunk(pkg, sets):
    (ln,) = sets["run counts"]
    assert [ln.kept_runs(k) for k in range(len(ln.jobs))] == list(hu.RUN_COUNTS)
    # every second read starts with a dropped substitution: one run more than it keeps
    assert [int(ln.out[k, 6]) - ln.kept_runs(k) for k in range(len(ln.jobs))] == [k % 2 for k in range(len(hu.RUN_COUNTS))]
    got, (z,) = hu.host_sample(pkg, [ln])
    assert z[:, 2].tolist() == [k % 2 for k in range(len(hu.RUN_COUNTS))]


def test_digit_counts(pkg, sets):
    (ln,) = sets["digits"]
    assert ln.eq_lengths(0) == list(hu.EQ_LENGTHS) and ln.eq_lengths(1) == [10000, 40]
    got, _ = hu.host_sample(pkg, [ln])
    cs = bytes(got["cs"])
    assert cs.startswith(b"Z::9*") and b":10000*" in cs and b":9999Z:" in cs


def test_end_rule(pkg, sets):
    (ln,) = sets["end rule"]
    got, (z,) = hu.host_sample(pkg, [ln])
    assert ln.strand.tolist() == [0, 0, 0, 0, 0, 1, 1, 1]
    # kept, up_len, down_len: the handoff is defined on the ORIENTED read, so a read handed in
    # reverse-complemented gives the row of the read it was made from
    plus = [[1, 2, 0], [1, 0, 2], [1, 1, 2]]
    assert z[:, [0, 2, 3]].tolist() == plus + [[0, 0, 0], [1, 0, 0]] + plus
    # the core is target[50:250]: tstart moves with the dropped leading target bases, tend with the trailing ones
    assert z[:, 4:6].tolist() == [[52, 250], [50, 248], [51, 248], [0, 0], [50, 250], [52, 250], [50, 248], [51, 248]]
    assert len(got["tstart"]) == 7 and np.array_equal(np.diff(got["cs_off"]), z[z[:, 0] == 1, 1])
    crafted, = sets["crafted"]
    got, (z,) = hu.host_sample(pkg, [crafted])
    # a_q = 2 (X 1, D 1), a_t = 3 (X 1, I 2); b_q = 2, b_t = 6; the read with no '=' owns nothing
    assert z[:, :6].tolist() == [[1, z[0, 1], 2, 2, 13, 10 + 53 - 6], [0, 0, 0, 0, 0, 0], [1, z[0, 1], 2, 2, 43, 87],
                                 [1, z[0, 1], 2, 2, 3, 47], [0, 0, 0, 0, 0, 0]]
    assert crafted.strand.tolist() == [0, 0, 1, 0, 1]
    assert got["cs_off"].tolist() == [0, z[0, 1], 2 * z[0, 1], 3 * z[0, 1]]


def test_letters(pkg, sets):
    (ln,) = sets["letters"]
    got, (z,) = hu.host_sample(pkg, [ln])
    assert z[:, 0].all() and ln.strand.tolist() == [0, 0, 0, 0, 0, 1]
    cs, up = bytes(got["cs"]), bytes(got["up"])
    assert b"+nn" in cs and cs.count(b"n") == 3 and cs == cs[:1] + cs[1:].lower().replace(b"z:", b"Z:")
    assert up == b"NNN" + up[3:] and up.isupper() and bytes(got["down"]) == b"N"


def _small(sets):
    (ln,) = sets["end rule"]
    return ln


def _buffers(z, slack=0):
    return [np.full(int(z[:, k].sum()) + slack, hu.FILL, np.uint8) for k in (1, 2, 3)]


def test_refusals_name_the_row_and_write_nothing(pkg, ho, sets):
    ln = _small(sets)
    args = (ln.seq, ln.jobs, ln.out, ln.runs)
    z = ho.cs_sizes(ln.jobs, ln.out, ln.runs, ln.seq.nbytes, "cpu")
    place, ends = ho.places(z)
    bufs = _buffers(z)
    assert ends == tuple(len(b) for b in bufs)

    def refused(row, why, jobs=ln.jobs, runs=ln.runs, sizes=z, place=place, caps=None):
        with pytest.raises(pkg.align.AlignError, match=r"mpc_align_cs_write_host: read %d: %s" % (row, why)):
            ho.cs_write(ln.seq, jobs, ln.out, runs, sizes, place, *bufs, device="cpu", caps=caps)
        assert all((b == hu.FILL).all() for b in bufs)

    p = place.copy()
    p[1, 0] = p[0, 0] + 1  # read 1's cs overlaps read 0's
    refused(1, "place", place=p)
    p = place.copy()
    p[[0, 1]] = p[[1, 0]]  # descends
    refused(1, "place", place=p)
    p = place.copy()
    p[2, 1] = 0  # read 2's upstream base on top of read 0's
    refused(2, "place", place=p)
    refused(7, "place", caps=(len(bufs[0]) - 1, len(bufs[1]), len(bufs[2])))  # the last read ends past the cs buffer
    refused(7, "place", caps=(len(bufs[0]), len(bufs[1]) - 1, len(bufs[2])))  # ... and past the upstream buffer
    j = ln.jobs.copy()
    j[4, 7] = len(ln.runs)
    refused(4, "runs outside the run buffer", jobs=j)
    r = ln.runs.copy()
    r[ln.jobs[2, 7]] += 1 << 2  # one base more than the read holds
    refused(2, "runs do not span the read", runs=r)
    with pytest.raises(pkg.align.AlignError, match="mpc_align_cs_sizes_host: read 2: runs do not span the read"):
        ho.cs_sizes(ln.jobs, ln.out, r, ln.seq.nbytes, "cpu")
    s = z.copy()
    s[5, 1] += 1  # a size row the runs do not give
    refused(5, "size row", sizes=s)
    ho.cs_write(*args, z, place, *bufs, device="cpu")  # and the tables as they were are taken
    assert not any((b == hu.FILL).all() for b in bufs)


def test_bytes_outside_the_slots_stay(pkg, ho, sets):
    """Places with gaps between the reads: only the reads' own bytes change."""
    ln = _small(sets)
    z = ho.cs_sizes(ln.jobs, ln.out, ln.runs, ln.seq.nbytes, "cpu")
    place, _ = ho.places(z)
    gap = place + 5 * np.arange(1, len(z) + 1)[:, None]
    bufs = _buffers(z, slack=5 * len(z) + 9)
    ho.cs_write(ln.seq, ln.jobs, ln.out, ln.runs, z, gap, *bufs, device="cpu")
    tight = _buffers(z)
    ho.cs_write(ln.seq, ln.jobs, ln.out, ln.runs, z, place, *tight, device="cpu")
    for col, (b, t) in enumerate(zip(bufs, tight)):
        own = np.zeros(len(b), bool)
        for k in range(len(z)):
            a, n = int(gap[k, col]), int(z[k, 1 + col])
            own[a: a + n] = True
            assert np.array_equal(b[a: a + n], t[int(place[k, col]): int(place[k, col]) + n])
        assert (b[~own] == hu.FILL).all()


# ---- the whole path on the host: collect() against align + ingest, and the oracle pileup ----------

COUNTS = {(5, 0): (120, 62, 58), (5, 1): (120, 58, 62), (7, 0): (120, 55, 65), (7, 1): (120, 65, 55)}


@pytest.mark.parametrize("seed,profile", [(5, "default"), (7, "indel")])
def test_collect_equals_the_two_steps_and_the_oracle_agrees(pkg, ho, tmp_path, seed, profile):
    import oracle
    syn = pkg.synth.Synth(600, 120, profile, seed=seed)
    refs = [str(tmp_path / "sense.fa"), str(tmp_path / "antisense.fa")]
    reads = str(tmp_path / "reads.fa")
    syn.write_files(refs[0], reads, None, refs[1], None)
    parts = []
    targets, _ = ho.collect(refs, reads, device="cpu", max_error=0.35, batch_bases=20000, paf=parts.append)
    assert len(parts) >= 3  # several batches accumulated
    longest = 0
    for k, (ref, t) in enumerate(zip(refs, targets)):
        paf = str(tmp_path / ("%d.paf" % k))
        res = pkg.align.align(ref, reads, device="cpu", max_error=0.35)
        with open(paf, "wb") as f:
            f.write(res["paf"])
        if k == 0:
            assert b"".join(parts) == res["paf"]
        assert t.summary == res["summary"]
        assert (t.summary["reads"], t.summary["mapped"], t.summary["plus"], t.summary["minus"]) == (120,) + COUNTS[seed, k]
        want = pkg.ingest.pack_sample(ref, paf, reads)
        got = t.pile.sample(t.ref)
        hu.assert_same(got, want, (seed, k))
        longest = max(longest, int(np.diff(got["up_off"]).max()), int(np.diff(got["down_off"]).max()))
        a, b = (oracle.run_packed(*(s[x] for x in ("ref",) + hu.KEYS), 0.1, 5.0) for s in (got, want))
        assert sorted(a) == sorted(b)
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
        assert len(a["base"]) >= 600
    assert longest > 10


def test_domain_refusals(pkg, ho, tmp_path):
    rng = np.random.default_rng(3)
    import verify_util as vu
    import align_util as au
    target = vu.rand_seq(rng, 300)
    ref, reads = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    hu.write_fasta(ref, [(b"tgt", target)])
    good = target[20:220]
    ok = [(b"a", good), (b"b desc", vu.rand_seq(rng, 150)), (b"c", au.revcomp(target[40:260]))]  # 'b desc' stays unmapped
    hu.write_fasta(reads, ok)
    targets, _ = ho.collect([ref], reads, device="cpu")
    assert targets[0].summary["mapped"] == 2 and targets[0].summary["unmapped_by_distance"] == 1
    minus_r = bytearray(au.revcomp(target[40:260]))
    minus_r[100] = ord("R")
    for recs, word in (([(b"a", good), (b"a", good)], "occurs twice"),
                       ([(b"a descr", good)], "header line holds more"),
                       ([(b"cs:a", good)], "starts with 'cs:'"),
                       ([(b"", good)], "empty"),
                       ([(b"a\x7fb", good)], "printable ASCII"),
                       ([(b"m", bytes(minus_r))], "other than A C G T N")):
        hu.write_fasta(reads, recs)
        with pytest.raises(ho.HandoffError, match=word) as err:
            ho.collect([ref], reads, device="cpu")
        assert repr(recs[-1][0].split()[0].decode() if recs[-1][0] else "") in str(err.value)
    plus_r = bytearray(good)
    plus_r[100] = ord("R")  # on '+' the parser takes it
    hu.write_fasta(reads, [(b"p", bytes(plus_r))])
    assert ho.collect([ref], reads, device="cpu")[0][0].summary["plus"] == 1
