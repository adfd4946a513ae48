"""The replay of wrapped odd positions (negative target starts: K_parse<NK> ->
K_wopack -> K_woprep -> K_wocover -> K_wofold -> K_layout<true> -> K_worows)
off its canonical shape: the second cs tokenizer against K_parse's ':' forms,
the single-workgroup sort / scans and the per-wave loops past one pass, the
ends of the wrapped range, every tally mode, the re-plan, the error exits and
three shards.  Every comparison is exact integer equality with the C oracle of
the same sample (tests/test_wrap_edges_cpu.py checks the inputs on the CPU).
"""
import importlib

import numpy as np
import pytest

import depth_util as du
import geometry_util as geo
import neg_util
import oracle

pytestmark = pytest.mark.gpu

SETTINGS = ((-1.0, 1.0), (0.1, 5.0))
_EXPECTED = {}


def _dist():
    return importlib.import_module("minion-plasmid-consensus_amd.dist")


def _oracle(name, st):
    """The oracle's calls for a named sample: computed once, shared, never changed."""
    if (name, st) not in _EXPECTED:
        _EXPECTED[name, st] = du.oracle_one(neg_util.edge_sample(name), *st)
    return _EXPECTED[name, st]


def _run(pkg, samples, names=None, row_cap=None):
    """One Runner over the samples at both settings, every sample against the
    oracle; returns (runner, calls per setting)."""
    eng = pkg.engine
    run = eng.Runner(samples, row_cap=row_cap)
    assert run.batch.neg_reads > 0
    out = {}
    for st in SETTINGS:
        run.step(*st)
        run.check()
        status = run.plan.status()
        assert status[eng.MPC_ST_WRAP_EVENTS] > 0 and status[eng.MPC_ST_WRAP_POS] > 0
        out[st] = run.fetch()
        for k, (got, smp) in enumerate(zip(out[st], samples)):
            exp = _oracle(names[k], st) if names else du.oracle_one(smp, *st)
            du.compare(got, exp, (names[k] if names else k, st))
    return run, out


def test_second_tokenizer_takes_the_forms_of_the_first(pkg):
    """K_wocover walks every read's cs again (wo_cover_read) to find its
    one-base writes at the listed positions; K_parse takes a ':' operand as
    int() does (py_int).  With operands written ' d', 'd ', '00d', 'd_dd',
    '\\x0bd\\x0c', '*x??y' and no-op tokens between the units, both must land on
    the same coordinates: the decorated samples give the oracle's calls, and
    the calls of the undecorated sample in the same launch.
    Before wo_cover_read used py_int it stopped a read at the first such
    operand and dropped its later one-base writes at wrapped positions without
    a flag: this test then failed with ('neg5_dec', (-1.0, 1.0)) chrom2
    differing first at call 293.  (One commit earlier it failed sooner, base
    at call 11: K_parse lost the bases of a short '+' behind such an operand,
    test_decorated_reads_without_negative_starts.)"""
    names = ["neg5_dec", "neg105_dec", "neg5"]
    run, out = _run(pkg, [neg_util.edge_sample(n) for n in names], names)
    for st in SETTINGS:
        du.compare(out[st][0], out[st][2], ("decorated vs plain", st))


def test_decorated_reads_without_negative_starts(pkg):
    """The same rewrite on a batch without negative starts (K_parse<NK = false>,
    no replay): a short '+' behind a ':' operand that is not plain digits
    (": 12+ac") is decoded from HBM (analyze_long) and must still carry its
    bases in the event word -- it once arrived as 'A's."""
    plain = neg_util.neg_sample(5, n_reads=800, frac_neg=0.0)
    smp = neg_util.decorate(plain, 3)
    assert pkg.engine.Batch([smp]).neg_reads == 0 and b" +" in bytes(smp["cs"]) and b"\x0c+" in bytes(smp["cs"])
    for st in SETTINGS:
        got = pkg.engine.pileup([smp, plain], *st)
        du.compare(got[0], du.oracle_one(smp, *st), ("decorated, no negative start", st))
        du.compare(got[1], got[0], ("decorated vs plain, no negative start", st))


@pytest.mark.parametrize("name", ["big0", "big1"])
def test_replay_loops_take_a_second_pass(pkg, name):
    """big0: 15,493 strings at 1,744 positions -- K_woprep's bitonic sort with
    P2 = 16384 (eight pairs per thread, the t += blockDim.x stride) and both
    block scans carrying across 1024-entry batches; wrapped positions past the
    first K_layout block.  big1: 93 RIGHT strings at one position -- 94 runs,
    K_worows' j += 64 loop.  The device's own counters equal the host count of
    the rule (neg_util.wrapped_counts), so both sides read it the same way."""
    eng = pkg.engine
    smp = neg_util.edge_sample(name)
    run, _ = _run(pkg, [smp], [name])
    status = run.plan.status()
    ev, pos, right = neg_util.wrapped_counts(smp)
    assert (int(status[eng.MPC_ST_WRAP_EVENTS]), int(status[eng.MPC_ST_WRAP_POS])) == (ev, pos)
    if name == "big0":
        assert status[eng.MPC_ST_WRAP_EVENTS] > 2048 and status[eng.MPC_ST_WRAP_POS] > 1024
    else:
        assert right > 64


def test_strings_longer_than_a_wave(pkg):
    """Flanks up to 200 bases and '+' strings up to 80 in wrapped positions:
    K_worows' bi += 64 loop over a string's bases, and position lists that
    grow by more than 64 slots on either side."""
    smp = neg_util.edge_sample("long")
    assert min(neg_util.longest_wrapped(smp).values()) > 64
    _run(pkg, [smp], ["long"])


@pytest.mark.parametrize("alone", [True, False], ids=["alone", "second_of_three"])
def test_ends_of_the_wrapped_range(pkg, alone):
    """neg_util.boundary_sample: strings at wrapped positions 0, 1 and n - 1
    from starts and ends at exactly -1, -n and -n + 1; alone (gbase 0) and
    behind another sample (gbase > 0: the position keys are global)."""
    if alone:
        _run(pkg, [neg_util.edge_sample("boundary")], ["boundary"])
    else:
        names = ["neg5_400", "boundary", "neg105"]
        _run(pkg, [neg_util.edge_sample(n) for n in names], names)


def _mode_cases():
    # (tally mode, reference length, reads, longest ':' operand): no more reads
    # than test_synthetic_full_pileup / test_long_reference use at that length
    return [(1, 1000, 400, 25), (2, geo.first_length(2), 400, 100), (3, geo.first_length(3), 300, 200),
            (3, geo.first_length(3, 16384), 150, 400), (0, geo.first_length(0), 40, 3000), (4, 400_000, 40, 4000)]


@pytest.mark.parametrize("mode,n,reads,match_max", _mode_cases(), ids=lambda v: str(v))
def test_every_tally_mode_with_wrapped_strings(pkg, mode, n, reads, match_max):
    """K_parse<TM, WIN, NK = true> in each tally mode, on reads that write
    wrapped strings (30 % negative starts): mode 1, 2, 3 with one substitution
    window, 3 with two, 0 (parse_window 2048 each at the planner's current
    thresholds) and 4 (parse_window 1024).  The window the planner chose is
    printed."""
    eng = pkg.engine
    smp = neg_util.neg_sample(50 + mode, n=n, n_reads=reads, frac_neg=0.3, match_max=match_max)
    assert min(neg_util.wrapped_strings(smp)) > 0
    run, _ = _run(pkg, [smp])
    info = run.plan.info()
    print("tally_mode", info["tally_mode"], "parse_window", info["parse_window"], "n", n)
    assert info["tally_mode"] == mode, info


def test_replan_with_wrapped_rows(pkg):
    """test_capacity_replan with wrapped rows: K_worows returns early on
    DE_CAP, the second plan redoes the wrapped rows."""
    got = pkg.engine.pileup([neg_util.edge_sample("neg5_400")], -1.0, 1.0, row_cap=10)
    du.compare(got[0], _oracle("neg5_400", (-1.0, 1.0)), "replan")


N_CLEAN = 120


def _error_sample(bad, ref=b"ACGTTGCA" * 5):
    """120 clean reads (none reaches position 39), the reads of ``bad``, 5 clean reads."""
    clean = lambda k: (b"Z::%d" % (10 + k % 16), k % 15, b"AC"[: k % 3], b"GT"[: k % 2])
    reads = [clean(k) for k in range(N_CLEAN)] + list(bad) + [clean(k) for k in range(5)]
    return neg_util._pack(ref, reads)


ERRORS = {
    "upstream_flank": [(b"Z::10", -3, b"ANG", b"")],
    "downstream_flank": [(b"Z::2", -6, b"", b"GNA")],
    "insertion": [(b"Z:+an:8", -2, b"", b"")],
}


@pytest.mark.parametrize("kind", list(ERRORS))
def test_wrapped_string_outside_acgt(pkg, kind):
    """A flank or '+' base outside ACGT written into a wrapped odd position:
    KeyError in the reference (:61, :71); K_worows flags DE_KEY with the
    launch-order index of the read."""
    eng = pkg.engine
    smp = _error_sample(ERRORS[kind])
    assert neg_util.wrapped_counts(smp)[0] == 1
    with pytest.raises(oracle.OracleError) as o:
        du.oracle_one(smp, -1.0, 1.0)
    assert (o.value.code, o.value.read) == (1, N_CLEAN)
    with pytest.raises(eng.DataError) as e:
        eng.pileup([smp], -1.0, 1.0)
    assert e.value.flags & eng.DE_KEY and e.value.read == N_CLEAN, (e.value.flags, e.value.read)


def test_reference_n_under_a_match_at_a_wrapped_position(pkg):
    """The reference base at a wrapped position (an upstream flank lands on odd
    position 39) is N and another read covers it with a match: KeyError (:61);
    K_layout<true> drops that position's plain tallies but still flags DE_KEY."""
    eng = pkg.engine
    smp = _error_sample([(b"Z::3", -1, b"AC", b""), (b"Z::40", 0, b"", b"")], ref=b"ACGTTGCA" * 4 + b"ACGTTGCN")
    assert [p for p, _, _, _ in neg_util._wrapped(smp)] == [39]
    with pytest.raises(oracle.OracleError) as o:
        du.oracle_one(smp, -1.0, 1.0)
    assert (o.value.code, o.value.read) == (1, N_CLEAN + 1)
    with pytest.raises(eng.DataError) as e:
        eng.pileup([smp], -1.0, 1.0)
    assert e.value.flags & eng.DE_KEY


def test_wrapped_error_index_under_sharding(pkg):
    """The upstream-flank case with the bad read in the last of three shards:
    K_worows reports a shard-local index, pileup_sharded maps it back to the
    launch order -- the flags and the index of one GPU."""
    dist, eng = _dist(), pkg.engine
    other = _error_sample([])
    smp = _error_sample(ERRORS["upstream_flank"])
    n_other = len(other["tstart"])
    assert (np.asarray(dist.split_samples([other, smp], 3)[2][1]["tstart"]) < 0).any()  # in the last shard
    with pytest.raises(eng.DataError) as one:
        eng.pileup([other, smp], -1.0, 1.0)
    assert one.value.flags & eng.DE_KEY and one.value.read == n_other + N_CLEAN
    with pytest.raises(eng.DataError) as three:
        dist.pileup_sharded([other, smp], -1.0, 1.0, [0, 0, 0])
    assert (three.value.flags, three.value.read) == (one.value.flags, one.value.read)


@pytest.mark.parametrize("c", [0x1c, 0x1d, 0x1e, 0x1f, 0x00, 0x08, 0x0e, 0x7f, 0x5f])
def test_int_rejects_what_python_int_rejects(pkg, c):
    """int() of an ASCII str strips space and \\t-\\r only: a ':' operand with
    one of \\x1c-\\x1f (whitespace to str.strip()), another control byte or a
    stray '_' beside its digits is a ValueError (:77; golden n_neg_pyint_fs),
    on a negative-start read too."""
    eng = pkg.engine
    for text in (bytes([c]) + b"4", b"4" + bytes([c])):
        with pytest.raises(ValueError):
            int(text.decode("ascii"))
        smp = _error_sample([(b"Z:+ac:" + text + b":2", -1, b"G", b"")])
        with pytest.raises(eng.DataError) as e:
            eng.pileup([smp], -1.0, 1.0)
        assert e.value.flags & eng.DE_VALUE and e.value.read == N_CLEAN, (text, e.value.flags, e.value.read)


def test_int_accepts_what_python_int_accepts(pkg):
    """The six bytes int() strips, before and after the digits: on
    negative-start reads that write a wrapped '+' string at odd position 39,
    and on reads that reach that position with a match only after such an
    operand (K_wocover's tokenizer).  The oracle's calls, and those of the
    plain spelling in the same launch."""
    reads, twins = [], []
    for ch in b" \t\n\r\x0b\x0c":
        for text in (bytes([ch]) + b"4", b"4" + bytes([ch])):
            assert int(text.decode("ascii")) == 4
            reads += [(b"Z:+ac:" + text + b":2*tg", -1, b"G", b"TT"), (b"Z::" + text + b":36", 0, b"", b"A")]
            twins += [(b"Z:+ac:4:2*tg", -1, b"G", b"TT"), (b"Z::4:36", 0, b"", b"A")]
    smp, plain = _error_sample(reads), _error_sample(twins)
    for st in SETTINGS:
        got = pkg.engine.pileup([smp, plain], *st)
        du.compare(got[0], du.oracle_one(smp, *st), ("int forms", st))
        du.compare(got[1], got[0], ("int forms vs plain", st))


def test_three_shards(pkg):
    """The three samples of the tokenizer test and the first big shape as three
    in-process shards: K_wopack, the gathered-list branch of K_woprep past
    2048 records, K_wofold.  Every shard ends with the unsharded oracle's
    calls and the same number of wrapped positions."""
    dist, eng = _dist(), pkg.engine
    names = ["neg5_dec", "neg105_dec", "neg5", "big0"]
    samples = [neg_util.edge_sample(n) for n in names]
    shards = dist.split_samples(samples, 3)
    sp = dist.ShardedPileup(shards, [0] * 3)
    assert all(p.wrap for p in sp.plans)
    total = sum(neg_util.wrapped_counts(s)[0] for s in samples)
    assert total > 2048
    for st in SETTINGS:
        sp.step(*st)
        sp.check()
        pos = [int(p.status()[eng.MPC_ST_WRAP_POS]) for p in sp.plans]
        assert pos[0] > 0 and pos == [pos[0]] * 3, pos
        assert pos[0] == sum(neg_util.wrapped_counts(s)[1] for s in samples)
        assert sum(int(p.status()[eng.MPC_ST_WRAP_EVENTS]) for p in sp.plans) == total
        for r, plan in enumerate(sp.plans):
            for name, got in zip(names, plan.fetch()):
                du.compare(got, _oracle(name, st), ("three shards", r, name, st))
