"""Seeded batches with negative target starts (minimap2 never writes one; the
reference indexes obsarr / refarr with Python's negative wrap,
mapped_paf_read_parser.py:222, :300-303, :57-61, :67-71, :79-97, :323).

A fraction of the reads start at tstart in [-n, -1] and take ':' / '*' / '+' /
'-' operations through the negative coordinates; some stay below 0 to their
end (downstream flank into the wrapped odd position n + i_end), the others
cross into the reference.  Starts and negative ends are drawn from a few values
so that wrapped odd positions collect several upstream flanks, '+' strings
and downstream flanks from reads in different orders, interleaved with the
one-base writes of the reads covering the same reference base.  Every batch
is valid input (the oracle raises nothing)."""
import functools
import hashlib
import re

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _bases(rng, k, lower=False):
    s = bytes(rng.choice(ACGT, k))
    return s.lower() if lower else s


def _cs(rng, n, ts, stay_negative, neg_end, ins_max=4, match_max=25):
    """cs of one read from coordinate ts; returns (cs bytes, end coordinate).
    '+' operands hold 1..ins_max bases (one fewer at the end coordinate), ':'
    operands 1..match_max."""
    out, i = [b"Z:"], ts
    if stay_negative:
        stop = neg_end
    else:
        stop = int(rng.integers(max(i + 1, 1), n + 1))
    while i < stop:
        r = rng.random()
        room = stop - i
        if r < 0.45:
            k = int(rng.integers(1, min(room, match_max) + 1))
            out.append(b":%d" % k)
            i += k
        elif r < 0.6:
            out.append(b"*" + _bases(rng, 1, True) + _bases(rng, 1, rng.random() < 0.5))
            i += 1
        elif r < 0.8:
            out.append(b"+" + _bases(rng, int(rng.integers(1, ins_max + 1)), rng.random() < 0.5))
        else:
            k = int(rng.integers(1, min(room, 3) + 1))
            out.append(b"-" + _bases(rng, k, True))
            i += k
    if rng.random() < 0.3:  # an insertion right at the end coordinate
        out.append(b"+" + _bases(rng, int(rng.integers(1, ins_max)), True))
    return b"".join(out), i


def neg_sample(seed, n=240, n_reads=2500, frac_neg=0.05, flank_max=6, ins_max=4, match_max=25):
    """One sample dict (synth layout: ref, cs, cs_off, tstart, up, up_off,
    down, down_off, aligned).  flank_max, ins_max, match_max: the longest
    flank, '+' operand and ':' operand (long references: fewer tokens per read)."""
    rng = np.random.default_rng(seed)
    ref = bytes(rng.choice(ACGT, n))
    starts = [-int(x) for x in rng.choice(np.arange(1, n + 1), 6, replace=False)]
    ends = [-int(x) for x in rng.choice(np.arange(1, n // 2), 4, replace=False)]
    cs, ts, ups, dns = [], [], [], []
    for _ in range(n_reads):
        if rng.random() < frac_neg:
            t = int(rng.choice(starts))
            e = [x for x in ends if x > t]
            stay = bool(e) and rng.random() < 0.5
            c, end = _cs(rng, n, t, stay, int(rng.choice(e)) if stay else 0, ins_max, match_max)
        else:
            t = int(rng.integers(0, n - 1))
            c, end = _cs(rng, n, t, False, 0, ins_max, match_max)
        cs.append(c)
        ts.append(t)
        ups.append(_bases(rng, int(rng.integers(0, flank_max + 1))))
        dns.append(_bases(rng, int(rng.integers(0, flank_max + 1))))
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    arr = lambda xs: np.frombuffer(b"".join(xs), dtype=np.uint8).copy()
    return dict(ref=np.frombuffer(ref, dtype=np.uint8).copy(), cs=arr(cs), cs_off=off(cs),
                tstart=np.asarray(ts, dtype=np.int64), up=arr(ups), up_off=off(ups), down=arr(dns),
                down_off=off(dns), aligned=np.zeros(n_reads, np.int64))




def _pack(ref, reads):
    """A sample dict from (cs, tstart, upstream flank, downstream flank) tuples."""
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    arr = lambda xs: np.frombuffer(b"".join(xs), dtype=np.uint8).copy()
    cs, ts, ups, dns = ([r[k] for r in reads] for k in range(4))
    return dict(ref=np.frombuffer(bytes(ref), dtype=np.uint8).copy(), cs=arr(cs), cs_off=off(cs),
                tstart=np.asarray(ts, dtype=np.int64), up=arr(ups), up_off=off(ups), down=arr(dns),
                down_off=off(dns), aligned=np.zeros(len(reads), np.int64))


def _tokens(body):
    """(operator, operand) pairs of one cs, in order (:306-320 splits at SPECIAL_CHARS)."""
    return re.findall(rb"([:Z+*-])([^:Z+*-]*)", body)


def _wrapped(smp):
    """(wrapped odd position, kind, string length, read) of every string the
    negative wrap writes into an odd position: obsarr[2 i] with -n <= i < 0 is
    obsarr[2 (n + i) + 1] (:303 upstream flank at tstart, :87 '+' at the
    running coordinate, :323 downstream flank at the end coordinate).  An
    operator applies when the next one comes after a non-empty operand, the
    last one always (:309, :320); ':' advances by int(operand) (:77)."""
    n = len(smp["ref"])
    cs = bytes(smp["cs"])
    for r, t in enumerate(smp["tstart"]):
        t = int(t)
        ul = int(smp["up_off"][r + 1] - smp["up_off"][r])
        dl = int(smp["down_off"][r + 1] - smp["down_off"][r])
        if ul > 0 and -n <= t < 0:
            yield n + t, "up", ul, r
        i = t
        toks = _tokens(cs[smp["cs_off"][r]: smp["cs_off"][r + 1]])
        for k, (op, opnd) in enumerate(toks):
            if not opnd and k + 1 < len(toks):
                continue
            if op == b":":
                i += max(int(opnd.decode("latin-1")), 0)
            elif op == b"*":
                i += 1
            elif op == b"-":
                i += len(opnd)
            elif op == b"+" and opnd and -n <= i < 0:
                yield n + i, "ins", len(opnd), r
        if dl > 0 and -n <= i < 0:
            yield n + i, "down", dl, r


def wrapped_strings(smp):
    """(upstream, '+', downstream) strings the negative wrap writes into odd
    positions -- a host restatement of the rule, for the tests' coverage checks."""
    kinds = [k for _, k, _, _ in _wrapped(smp)]
    return kinds.count("up"), kinds.count("ins"), kinds.count("down")


def wrapped_counts(smp):
    """(strings, distinct wrapped odd positions, most downstream (RIGHT) strings
    at one position): the sizes the replay's sort, scans and per-position run
    loop work on."""
    ev = list(_wrapped(smp))
    right = {}
    for p, k, _, _ in ev:
        right[p] = right.get(p, 0) + (k == "down")
    return len(ev), len(right), max(right.values(), default=0)


def longest_wrapped(smp):
    """{kind: longest string of that kind in a wrapped odd position}."""
    out = {"up": 0, "ins": 0, "down": 0}
    for _, k, L, _ in _wrapped(smp):
        out[k] = max(out[k], L)
    return out


_FILLER = b"nNxq?.#=%"  # neither bases nor operator bytes
_NOOPS = (b"Zacg", b":0", b":000", b": 0 ", b":", b"*", b"+", b"-", b"Z")


def _int_form(rng, d):
    """Another spelling of the plain digits d with the same int() value."""
    k = int(rng.integers(0, 5))
    if k == 0:
        return b" " + d
    if k == 1:
        return d + b" "
    if k == 2:
        return b"00" + d
    if k == 3:
        return d[:1] + b"_" + d[1:] if len(d) > 1 else b"0_" + d
    return b"\x0b" + d + b"\x0c"


def decorate(smp, seed, p=0.25):
    """The sample with its cs rewritten, value-preserving: at rate p per unit
      * a ':' operand of plain digits becomes an equivalent int() form
        (' d', 'd ', '00d', 'd_ddd' / '0_d', '\\x0bd\\x0c': int() strips
        space and \\t-\\r from an ASCII str, not \\x1c-\\x1f);
      * '*xy' becomes '*x??y' (:96 writes operand[-1] only);
      * a no-op token goes in front of the unit: 'Zacg', ':0', ':000', ': 0 ',
        or an empty-operand ':', '*', '+', '-', 'Z' (skipped at :309 since an
        operator follows it immediately).  Nothing is added after the last
        token, which is applied unconditionally (:320).
    Every read keeps its coordinates; only cs and cs_off change."""
    rng = np.random.default_rng(seed)
    cs = bytes(smp["cs"])
    out = []
    for r in range(len(smp["tstart"])):
        parts = []
        for k, (op, opnd) in enumerate(_tokens(cs[smp["cs_off"][r]: smp["cs_off"][r + 1]])):
            if k > 0 and rng.random() < p:
                parts.append(_NOOPS[int(rng.integers(0, len(_NOOPS)))])
            if op == b":" and opnd.isdigit() and rng.random() < p:
                opnd = _int_form(rng, opnd)
            elif op == b"*" and len(opnd) == 2 and rng.random() < p:
                fill = bytes(_FILLER[int(x)] for x in rng.integers(0, len(_FILLER), int(rng.integers(1, 4))))
                opnd = opnd[:1] + fill + opnd[1:]
            parts.append(op + opnd)
        out.append(b"".join(parts))
    new = dict(smp)
    new["cs"] = np.frombuffer(b"".join(out), dtype=np.uint8).copy()
    new["cs_off"] = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.int64)
    return new


def boundary_sample(n=12):
    """A hand-built sample at the ends of the wrapped range.  Upstream flanks
    at tstart -1 and -n (wrapped odd positions n - 1 and 0), reads ending at -1
    and -n + 1 with downstream flanks (positions n - 1 and 1), a '+' at -1 and
    at -n, and positions 0 and n - 1 covered by matches and by substitutions
    from reads listed before, between and after the negative ones, so each of
    those positions replays LEFT strings, one-base writes and RIGHT strings in
    several runs."""
    ref = (b"ACGTTGCA" * (n // 8 + 1))[:n]
    other = lambda c: b"ACGT"[(b"ACGT".index(c) + 1) % 4: (b"ACGT".index(c) + 1) % 4 + 1].lower()
    low = lambda k: ref[k: k + 1].lower()
    full = b"Z::%d" % n
    subs = b"Z:*" + low(0) + other(ref[0]) + b":%d*" % (n - 2) + low(n - 1) + other(ref[n - 1])
    subs2 = b"Z:*" + low(0) + other(ref[0]).upper() + b":%d*" % (n - 2) + low(n - 1) + low(n - 1)
    reads = [
        (full, 0, b"AC", b"GT"),
        (subs, 0, b"", b"T"),
        (b"Z::3", -1, b"ACG", b""),                     # upstream flank -> position n - 1
        (b"Z::%d" % (n + 2), -n, b"TT", b"C"),          # upstream flank -> position 0
        (b"Z::3", -4, b"G", b"GGA"),                    # ends at -1: downstream flank -> position n - 1
        (full, 0, b"", b""),
        (b"Z::1", -n, b"CAT", b"TG"),                   # ends at -n + 1: downstream flank -> position 1
        (b"Z:+acg:2", -1, b"", b"A"),                   # '+' at -1
        (b"Z:+TG:%d" % (n + 1), -n, b"", b""),          # '+' at -n
        (b"Z:-ac*gt+c", -4, b"TTTT", b"CC"),            # ends at -1 after a deletion, a substitution and a '+'
        (subs2, 0, b"G", b""),
        (b"Z::2", -1, b"GATTA", b"AC"),
        (b"Z::%d+gg" % n, -n, b"A", b"TTT"),            # crosses all of the reference from -n, ends at 0
        (full, 0, b"T", b"T"),
        (b"Z::1", -2, b"", b"ACGTA"),                   # a second RIGHT string at position n - 1
        (subs, 0, b"", b""),
        (full, 0, b"GG", b""),
    ]
    return _pack(ref, reads)


def sample_digest(smp):
    """sha256 over every array of the sample (key, dtype, bytes): pins a generator's output."""
    m = hashlib.sha256()
    for k in sorted(smp):
        a = np.ascontiguousarray(smp[k])
        m.update(k.encode() + a.dtype.str.encode() + a.tobytes())
    return m.hexdigest()


# The shapes of tests/test_wrap_edges_{cpu,gpu}.py: the two canonical samples
# and their decorated twins; two shapes past the bounds of the replay's loops
# (counted in test_wrap_edges_cpu.py: > 2048 strings and > 1024 positions, i.e.
# a second pass of K_woprep's sort stride and a scan carry; > 64 RIGHT strings
# at one position, i.e. a second pass of K_worows' run loop); flanks and '+'
# strings of more than 64 bases (a second pass of K_worows' base loop).
EDGE_SHAPES = {
    "neg5": dict(seed=5),
    "neg105": dict(seed=105, n=500, n_reads=1500, frac_neg=0.06),
    "neg5_400": dict(seed=5, n_reads=400),
    "big0": dict(seed=7, n=2000, n_reads=800, frac_neg=0.7),
    "big1": dict(seed=7, n=1500, n_reads=1200, frac_neg=0.6),
    "long": dict(seed=9, n=150, n_reads=300, frac_neg=0.3, flank_max=200, ins_max=80),
}


@functools.lru_cache(maxsize=None)
def edge_sample(name):
    """A named sample, generated once per process and shared (never modified)."""
    if name == "boundary":
        return boundary_sample()
    if name.endswith("_dec"):
        return decorate(edge_sample(name[:-4]), seed=len(name))
    return neg_sample(**EDGE_SHAPES[name])
