"""The end of a K_parse workgroup: LDS tallies kept while waves finish at
different times, then flushed to the global tallies (mpc_k_parse.h
parse_epilogue).

Written for the early drain of DESIGN.md section 7 (waves that run out of
chunks exchange LDS tally words for their neutral value and add them to the
global tallies while the other waves keep adding to the same words;
exp/early_drain.patch), which was measured and not merged; what changed
instead is the counter those waves take their chunks from (DESIGN.md section
3).  What the cases ask holds for the product kernel as it does for any such
variant, so they
stay: every call and max_depth equal the oracle's at two (mdf, gtf) settings,
on the smallest shapes at which work at a workgroup's end can go wrong -- all
three LDS tally modes with most tally words non-zero, one long read among
thousands of short ones in one workgroup (most waves are done long before the
last one), fewer chunks than waves, counts at the 16-bit bound of the tally
halves, mixed samples and the negative-start kernels, and two batches in
flight run twice (no state left behind for the next launch).
"""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

KEYS = ("base", "chrom1", "chrom2", "count", "count2", "total")
SETTINGS = ((-1.0, 1.0), (0.1, 5.0))
# substitution- and deletion-dense: most tally words of a workgroup are non-zero
DENSE = dict(p_sub=0.2, p_del=0.08, p_ins=0.02, del_len=(1, 4))


def _oracle(s, mdf, gtf):
    return oracle.run_packed(s["ref"], s["cs"], s["cs_off"], s["tstart"], s["up"], s["up_off"], s["down"],
                             s["down_off"], mdf, gtf)


def _cmp(got, exp, tag):
    assert got["max_depth"] == exp["max_depth"], tag
    for k in KEYS:
        a = np.asarray(got[k], dtype=np.int64)
        b = np.asarray(exp[k], dtype=np.int64)
        assert a.shape == b.shape, (tag, k, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0][:5]
            raise AssertionError(f"{tag} {k} differs at {bad.tolist()}: {a[bad].tolist()} vs {b[bad].tolist()}")


def _check(pkg, samples, tag, parse_cus=0, mode=None, want=None):
    """One Runner over ``samples``: the tally mode (and ``want(info)``), then
    every call against the oracle at both settings.  Returns the runner."""
    run = pkg.engine.Runner(samples, parse_cus=parse_cus)
    info = run.plan.info()
    if mode is not None:
        assert info["tally_mode"] == mode, info
    if want is not None:
        assert want(info), info
    for mdf, gtf in SETTINGS:
        run.step(mdf, gtf)
        run.check()
        for s, (got, smp) in enumerate(zip(run.fetch(), samples)):
            _cmp(got, _oracle(smp, mdf, gtf), (tag, s, mdf, gtf))
    return run


def _pack(ref, css, tstarts, seed=0, flank=5):
    """A sample dict (synth layout) from explicit cs strings."""
    rng = np.random.default_rng(seed)
    cs_b = [c if isinstance(c, bytes) else c.encode() for c in css]
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ups = [rng.choice(acgt, int(rng.integers(0, flank + 1))).tobytes() for _ in css]
    dns = [rng.choice(acgt, int(rng.integers(0, flank + 1))).tobytes() for _ in css]
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    arr = lambda xs: np.frombuffer(b"".join(xs) or b"", dtype=np.uint8).copy()
    return dict(ref=np.frombuffer(ref, dtype=np.uint8).copy(), cs=arr(cs_b), cs_off=off(cs_b),
                tstart=np.asarray(tstarts, dtype=np.int64), up=arr(ups), up_off=off(ups), down=arr(dns),
                down_off=off(dns))


def _ref(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()


# (reference length, reads per strand): about 300, 6,000 and 9,000 bases
MODE_SHAPES = {1: (300, 3000), 2: (6000, 1500), 3: (9000, 1000)}


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("parse_cus", [0, 4])
def test_dense_tallies_every_lds_mode(pkg, mode, parse_cus):
    """Both strands of a substitution- and deletion-dense set in each LDS tally
    mode, with the grid of a whole GPU (few reads per workgroup, waves without
    a chunk) and with four workgroups (every wave works through several chunks,
    and every tally word is hit by many waves up to the workgroup's end)."""
    n, reads = MODE_SHAPES[mode]
    syn = pkg.synth.Synth(n=n, n_reads=reads, profile="default", seed=300 + mode, frac_partial=0.3, **DENSE)
    samples = [syn.sample(0), syn.sample(1)]
    want = (lambda i: i["parse_workgroups"] <= 4) if parse_cus else None
    _check(pkg, samples, ("dense", mode, parse_cus), parse_cus=parse_cus, mode=mode, want=want)


def _long_cs(rng, n, ts):
    """A cs that covers [ts, n - 2) in tokens of 2-3 bytes: substitutions,
    one-base deletions and one-base insertions (tens of windows for one read)."""
    out, i = ["Z:"], ts
    while i < n - 2:
        r = rng.random()
        if r < 0.55:
            out.append("*a" + str(rng.choice(list("cgt")))); i += 1
        elif r < 0.8:
            out.append("-" + str(rng.choice(list("acgt")))); i += 1
        else:
            out.append("+" + str(rng.choice(list("acgt"))))
    out.append(":1")
    return "".join(out)


def _short_cs(rng, n, ts):
    a, b = int(rng.integers(1, 30)), int(rng.integers(1, 30))
    k = int(rng.integers(0, 3))
    mid = ("*a" + str(rng.choice(list("cgt"))), "-" + "".join(rng.choice(list("acgt"), 2)), "+ac")[k]
    assert ts + a + b + 2 < n
    return "Z::%d%s:%d" % (a, mid, b)


@pytest.mark.parametrize("n,where", [(2500, (0,)), (2500, (1700, 3999)), (6500, (2000,))],
                         ids=["first", "middle_last", "packed_halves"])
def test_one_long_read_among_short_ones(pkg, n, where):
    """Uneven waves in one workgroup: 4,000 short reads and one or two reads
    whose cs is longer than all of theirs together, the parse grid sized for
    one CU -- the waves with short reads are done early, the wave with the long
    read goes on adding to the same substitution and depth words."""
    rng = np.random.default_rng(n + len(where))
    ts = [int(rng.integers(0, n - 70)) for _ in range(4000)]
    css = [_short_cs(rng, n, t) for t in ts]
    for r in where:
        ts[r] = int(rng.integers(0, 20))
        css[r] = _long_cs(rng, n, ts[r])
    smp = _pack(_ref(rng, n), css, ts, 3)
    short = sum(len(c) for k, c in enumerate(css) if k not in where)
    assert min(len(css[r]) for r in where) * 2 > short // 16  # far above a wave's share of the short reads
    _check(pkg, [smp], ("long read", n, where), parse_cus=1, want=lambda i: i["parse_workgroups"] == 1)


@pytest.mark.parametrize("reads", [1, 2, 5, 15])
def test_fewer_chunks_than_waves(pkg, reads):
    """A workgroup with fewer chunks than waves: the waves without a chunk
    reach the pre-epilogue barrier at once; down to a single chunk."""
    rng = np.random.default_rng(50 + reads)
    n = 1200
    ts = [int(rng.integers(0, 20)) for _ in range(reads)]
    css = [_long_cs(rng, n - 60 * k, t) for k, t in enumerate(ts)]
    smp = _pack(_ref(rng, n), css, ts, 4)
    _check(pkg, [smp], ("few chunks", reads), parse_cus=1, want=lambda i: i["parse_workgroups"] == 1)


def _same_positions(pkg, n, reads, seed):
    """``reads`` full-length reads of an ``n``-base reference, all from position
    0, substitution- and deletion-dense: every depth and substitution word of
    the one workgroup is hit by (nearly) every read."""
    syn = pkg.synth.Synth(n=n, n_reads=reads, profile="default", seed=seed, antisense=False, frac_partial=0.0,
                          flank=(0, 4), p_sub=0.4, p_del=0.1, p_ins=0.05, del_len=(1, 2), ins_len=(1, 2))
    smp = syn.sample(0)
    assert int(np.count_nonzero(smp["tstart"] == 0)) == reads
    return smp


def test_counts_at_the_16_bit_bound_wide(pkg):
    """Tally mode 1: 32767 reads (reads_per_workgroup_cap) of a 96-base
    reference in ONE workgroup, all starting at position 0: the increment half
    of depth word 0 reaches 32767."""
    smp = _same_positions(pkg, 96, 32767, 64)
    _check(pkg, [smp], "cap wide", parse_cus=1, mode=1,
           want=lambda i: i["max_reads_per_workgroup"] == i["reads_per_workgroup_cap"] == 32767)


@pytest.mark.parametrize("mode", [2, 3])
def test_counts_at_the_16_bit_bound_packed(pkg, mode):
    """Tally modes 2 and 3 (a long sample with a few reads sets the mode): 16383
    reads of a 96-base reference in one workgroup, all from position 0 -- the
    biased depth half of position 0 reaches 0x8000 + 16383, the one of the
    last position 0x8000 - 16383."""
    big = pkg.synth.Synth(n=MODE_SHAPES[mode][0], n_reads=40, profile="default", seed=65, antisense=False, **DENSE)
    samples = [big.sample(0), _same_positions(pkg, 96, 16383, 66)]
    _check(pkg, samples, ("cap packed", mode), parse_cus=2, mode=mode,
           want=lambda i: i["max_reads_per_workgroup"] == i["reads_per_workgroup_cap"] == 16383)


def test_two_samples_of_different_length(pkg):
    """Two samples of different length in one launch (a workgroup flushes the
    words of its own sample's length only)."""
    a = pkg.synth.Synth(n=333, n_reads=2500, profile="default", seed=67, antisense=False, frac_partial=0.3, **DENSE)
    b = pkg.synth.Synth(n=2051, n_reads=1200, profile="default", seed=68, antisense=False, frac_partial=0.3, **DENSE)
    _check(pkg, [a.sample(0), b.sample(0)], "two lengths", parse_cus=4, mode=1)


def test_reads_with_an_empty_cs(pkg):
    """Reads with an empty cs among dense ones -- at a chunk's start, in runs
    of more than 63 (windows without a byte) and at the range end: the
    reference raises on the first of them (processOperation('', '')), and so
    does the pileup, with the same read; the same batch without them matches
    the oracle call by call."""
    rng = np.random.default_rng(69)
    n = 700
    ts = [int(rng.integers(0, 40)) for _ in range(1500)]
    css = [_long_cs(rng, n - int(rng.integers(0, 300)), t) for t in ts]
    smp = _pack(_ref(rng, n), css, ts, 5)
    _check(pkg, [smp], "no empty cs", parse_cus=2)
    empty = sorted({0, 700, 1499} | set(range(300, 380)))
    for r in empty:
        css[r] = ""
    bad = _pack(_ref(np.random.default_rng(69), n), css, ts, 5)
    with pytest.raises(oracle.OracleError) as o:
        _oracle(bad, -1.0, 1.0)
    run = pkg.engine.Runner([bad], parse_cus=2)
    run.step(-1.0, 1.0)
    with pytest.raises(pkg.engine.DataError) as e:
        run.check()
    # (the flags of a failed launch hold whatever the later kernels made of the
    # flagged reads as well; the first error is what the reference defines)
    assert e.value.flags & pkg.engine.DE_OP and e.value.read == o.value.read == empty[0]


@pytest.mark.parametrize("big_n", [0, MODE_SHAPES[2][0], MODE_SHAPES[3][0]], ids=["mode1", "mode2", "mode3"])
def test_negative_starts(pkg, big_n):
    """A batch with negative target starts (the NK instantiations of K_parse;
    their workgroups take the rounds of Python's negative wrap) beside a dense
    sample without any, in each LDS tally mode."""
    import neg_util
    samples = [neg_util.edge_sample("neg5"), neg_util.edge_sample("neg105")]
    n2 = big_n or 500
    syn = pkg.synth.Synth(n=n2, n_reads=600 if big_n else 2000, profile="default", seed=70, antisense=False,
                          frac_partial=0.3, **DENSE)
    samples.append(syn.sample(0))
    run = _check(pkg, samples, ("negative starts", big_n), parse_cus=6, mode={0: 1}.get(big_n))
    assert run.batch.neg_reads > 0
    if big_n:
        assert run.plan.info()["tally_mode"] == (2 if big_n == MODE_SHAPES[2][0] else 3)


@pytest.mark.parametrize("mode", [1, 3])
def test_two_batches_in_flight_run_twice(pkg, mode):
    """Two batches on two streams, the parse grids sized for 8 CUs each, steps
    interleaved without host synchronisation; then the same runners again: the
    second round of launches finds the workgroups' counters, the LDS tallies
    and the global tallies as a first launch does."""
    import torch
    n, reads = MODE_SHAPES[mode]
    syns = [pkg.synth.Synth(n=n, n_reads=reads, profile="default", seed=71 + k, frac_partial=0.2, **DENSE)
            for k in range(2)]
    sets = [[s.sample(0), s.sample(1)] for s in syns]
    exp = [[_oracle(s, 0.1, 5.0) for s in ss] for ss in sets]
    runners = [pkg.engine.Runner(ss, parse_cus=8) for ss in sets]
    for r in runners:
        info = r.plan.info()
        assert info["tally_mode"] == mode and info["parse_workgroups"] <= 8, info
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    for rnd in range(2):
        for k in range(6):
            with torch.cuda.stream(streams[k % 2]):
                runners[k % 2].step(0.1, 5.0)
        torch.cuda.synchronize()
        for r, ex in zip(runners, exp):
            r.check()
            for s, (got, e) in enumerate(zip(r.fetch(), ex)):
                _cmp(got, e, ("in flight", mode, rnd, s))
