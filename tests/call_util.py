"""Plain restatement of the reference's Steps 5-6 on explicit tallies, and
builders of inputs whose tallies / row layout are known from their arguments
(test infrastructure; plain Python and numpy, no GPU).

``call_rule`` and ``consensus_rows`` restate mapped_paf_read_parser.py
:332-341 and :363-439 on rows of (A, T, C, G) counts; tests/test_call_rule_cpu.py
pins them to the C oracle, and the golden case t_call_rule to the script.
``tally_sample`` builds a sample whose odd position p has exactly the tally
it is given; ``plain_batch`` builds samples whose pileup rows follow from the
arguments alone, so tests/test_consensus_gpu.py can write any tallies into
the rows and run the consensus phase by itself.
"""
import itertools

import numpy as np

KEYS = ("base", "chrom1", "chrom2", "count", "count2", "total")
BASES = "ATCG"  # dict order of the reference's tallies (:59)

# (min_depth_factor, global_threshold_factor) of the call-rule tests
SETTINGS = [(-1.0, 1.0), (0.1, 5.0), (0.5, 2.5), (0.0, 0.0), (0.29, 1.12), (0.5, 1.10), (1.0, 1.0),
            (0.1, float("inf"))]

SMALL = list(itertools.product(range(4), repeat=4))  # {0..3}^4, (A, T, C, G)
# count < gtf * count2 (:421) where float64 and exact arithmetic disagree
# (1.10 * 50 > 55, 1.12 * 25 > 28), and plain cases on either side of it
GTF_EDGE = [(55, 50, 0, 0), (0, 55, 0, 50), (28, 25, 0, 0), (0, 0, 25, 28), (5, 1, 0, 0), (4, 1, 0, 0), (0, 5, 2, 0),
            (10, 1, 1, 0), (1, 0, 1, 10)]


def depth_edge(max_depth, mdf):
    """Tuples whose counts straddle max_depth * mdf (:338, :428), with the
    position that sets max_depth first: unique tops, a top tie (count = the
    sum, :392) and a second-place tie around the threshold."""
    t = int(max_depth * mdf)
    out = [(max_depth, 0, 0, 0)]
    for c in (t - 1, t, t + 1, t + 2):
        if c > 0:
            out += [(c, 0, 0, 0), (0, 0, 0, c), (1, c + 1, 0, 0)]
            if c % 2 == 0:
                out.append((0, c // 2, c // 2, 0))       # N with count c
            if c > 2:
                out.append((0, c, 2, 2))                 # tie for second
    return [x for x in out if sum(x) <= max_depth]


D100 = depth_edge(100, 0.29)  # 0.29 * 100 = 28.999999999999996: a count of 29 is emitted
D10 = depth_edge(10, 0.5)

# the samples of tests/test_call_rule_cpu.py and of the golden cases t_call_rule*
# (one max depth each): name -> tuples
TALLY_SAMPLES = {
    "small_gtf": SMALL + GTF_EDGE,                      # max depth 105
    "d100": D100 + SMALL[:64],                          # max depth 100: 0.29 * 100 < 29
    "d10": D10 + [t for t in SMALL if sum(t) <= 10],    # max depth 10: 0.5 * 10 == 5
}


def tally_sample_named(name, ref_n):
    return tally_sample(TALLY_SAMPLES[name], ref_n=ref_n, seed=len(name))


def call_rule(tally, gtf):
    """:371-423 for one (A, T, C, G) tuple of ints -> (base, chrom1, chrom2,
    count, count2, total) with the bases as character codes; None when no read
    wrote the slot (such a slot does not exist in the reference)."""
    obs = dict(zip(BASES, (int(v) for v in tally)))
    list_of_tuples = [(k, v) for k, v in obs.items() if v > 0]
    summary_x = sorted(list_of_tuples, key=lambda tup: tup[1])[::-1]
    if len(summary_x) == 0:
        return None
    if len(summary_x) == 1 or summary_x[0][1] > summary_x[1][1]:
        base, count = summary_x[0]
    else:
        base = "N"
        count = sum(c[1] for c in summary_x if c[1] == summary_x[0][1])
    if len(summary_x) == 1:
        base2, count2 = "X", 0
    elif len(summary_x) == 2 or summary_x[1][1] > summary_x[2][1]:
        base2, count2 = summary_x[1]
    else:
        base2 = "N"
        count2 = sum(c[1] for c in summary_x if c[1] == summary_x[1][1])
    chrom1 = base
    if count < float(gtf) * count2:  # :421, Python floats (nan compares False)
        base = "N"
    return ord(base), ord(chrom1), ord(base2), count, count2, sum(c[1] for c in summary_x)


def consensus_rows(rows, meta, bounds, mdf, gtf):
    """Steps 5-6 over pileup rows: rows[r] = (A, T, C, G), meta[r] bit 1 = first
    slot of its position, sample s = rows [bounds[s], bounds[s + 1]).  Returns
    one dict per sample in the shape of engine.Plan.fetch()."""
    rows = np.asarray(rows)
    out = []
    cache = {}
    for s in range(len(bounds) - 1):
        a, b = int(bounds[s]), int(bounds[s + 1])
        tl = [tuple(int(v) for v in r) for r in rows[a:b]]
        max_depth = 0
        for t, m in zip(tl, meta[a:b]):
            if int(m) & 2 and sum(t) > max_depth:  # :336 first slot of every position
                max_depth = sum(t)
        thr = max_depth * float(mdf)  # :338
        kept = []
        for t in tl:
            c = cache.get(t)
            if c is None:
                c = cache[t] = call_rule(t, gtf) or ()
            if c and c[3] > thr:  # :428
                kept.append(c)
        k = np.array(kept, dtype=np.int64).reshape(-1, 6)
        d = {key: k[:, i].copy() for i, key in enumerate(KEYS)}
        d["max_depth"] = max_depth
        out.append(d)
    return out


def _off(xs):
    return np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)


def _pack(ref, css):
    cs_b = [c.encode() for c in css]
    empty = np.zeros(0, np.uint8)
    zeros = np.zeros(len(css) + 1, np.int64)
    return dict(ref=np.frombuffer(ref.encode(), dtype=np.uint8).copy(),
                cs=np.frombuffer(b"".join(cs_b), dtype=np.uint8).copy(), cs_off=_off(cs_b),
                tstart=np.zeros(len(css), np.int64), up=empty.copy(), up_off=zeros.copy(), down=empty.copy(),
                down_off=zeros.copy())


def tally_sample(tuples, tail=0, ref_n=False, seed=0):
    """A packed sample (layout of _packed in tests/test_gpu_parity.py) whose odd
    position p has exactly the tally tuples[p] = (A, T, C, G): D = max(sum(t))
    reads, all at tstart 0 with empty flanks; read j takes at position p the
    j-th symbol of 'A'*a + 'T'*t + 'C'*c + 'G'*g, a deletion when there are
    fewer.  ``tail`` appends that many positions every read matches (longer
    references reach the other tally modes).  ``ref_n``: the reference holds
    N wherever no read matches it (nothing is ever written from it there)."""
    rng = np.random.default_rng(seed)
    D = max(sum(t) for t in tuples)
    ref = [BASES[k] for k in rng.integers(0, 4, len(tuples) + tail)]
    syms = []
    for p, (a, t, c, g) in enumerate(tuples):
        syms.append("A" * a + "T" * t + "C" * c + "G" * g)
        if ref_n and ref[p] not in syms[p]:
            ref[p] = "N"
    css = []
    for j in range(D):
        ops, run, dele = [], 0, ""

        def flush():
            nonlocal run, dele
            if run:
                ops.append(":%d" % run)
            if dele:
                ops.append("-" + dele)
            run, dele = 0, ""

        for p, sy in enumerate(syms):
            r = ref[p].lower()
            if j >= len(sy):
                if run:
                    flush()
                dele += r
            elif sy[j] == ref[p]:
                if dele:
                    flush()
                run += 1
            else:
                flush()
                ops.append("*" + r + sy[j].lower())
        if dele:
            flush()
        run += tail
        flush()
        css.append("Z:" + "".join(ops))
    return _pack("".join(ref), css)


def sample_files(smp):
    """(ref.fa, reads.fa, in.paf) texts of a tally_sample / plain_batch sample
    (tstart 0, no flanks): every query is its aligned bases."""
    ref = bytes(smp["ref"]).decode()
    cs_all = bytes(smp["cs"]).decode()
    reads, paf = [], []
    import re
    for j in range(len(smp["tstart"])):
        cs = cs_all[smp["cs_off"][j]: smp["cs_off"][j + 1]]
        assert cs.startswith("Z:")
        q, i = [], 0
        for op, v in re.findall(r"([:*+-])([^:*+-]+)", cs[2:]):
            if op == ":":
                q.append(ref[i: i + int(v)])
                i += int(v)
            elif op == "*":
                q.append(v[-1].upper())
                i += 1
            elif op == "+":
                q.append(v.upper())
            else:
                i += len(v)
        seq = "".join(q)
        reads.append(">q%d\n%s\n" % (j, seq))
        paf.append("q%d\t%d\t0\t%d\t+\tref\t%d\t0\t%d\t0\t0\t60\tcs:%s\n" % (j, len(seq), len(seq), len(ref), i, cs))
    return ">ref\n%s\n" % ref, "".join(reads), "".join(paf)


def plain_batch(lengths, reads_per_sample, insertions, seed=0):
    """Samples whose row layout follows from the arguments: every read of sample
    s is 'Z::<n_s>' at tstart 0 with empty flanks; read i carries the one
    insertion insertions[s][i] = (gap, string) when there is one (interior gaps
    only, 0 < gap < n_s).  Gap g then takes as many rows as its longest string
    (the first with meta 2, the others 0), every odd position one row (meta 3),
    and the sample ends with its n_s-th odd row.  Returns (samples, meta) with
    meta[s] the expected MPC_BUF_ROWMETA bytes of sample s's rows."""
    rng = np.random.default_rng(seed)
    samples, metas = [], []
    for s, (n, nr) in enumerate(zip(lengths, reads_per_sample)):
        ins = list(insertions[s]) if s < len(insertions) else []
        assert len(ins) <= nr and all(0 < g < n and len(x) > 0 for g, x in ins), (s, n, nr, ins)
        ref = "".join(BASES[k] for k in rng.integers(0, 4, n))
        css = []
        for i in range(nr):
            if i < len(ins):
                g, x = ins[i]
                css.append("Z::%d+%s:%d" % (g, x.lower(), n - g))
            else:
                css.append("Z::%d" % n)
        longest = {}
        for g, x in ins:
            longest[g] = max(longest.get(g, 0), len(x))
        meta = []
        for g in range(n):
            L = longest.get(g, 0)
            meta += [2] * min(L, 1) + [0] * max(L - 1, 0) + [3]
        samples.append(_pack(ref, css))
        metas.append(np.array(meta, dtype=np.uint8))
    return samples, metas


def tie_class(t):
    """Name of the tie class of a tally (None: no tie among positive counts
    decides anything), by its counts sorted downwards."""
    c = sorted((v for v in t if v > 0), reverse=True)
    m = len(c)
    if m >= 4 and c[0] == c[3]:
        return "top4"
    if m >= 3 and c[0] == c[2]:
        return "top3"
    if m >= 3 and c[0] == c[1] and c[1] > c[2]:
        return "top2_second_distinct"
    if m == 4 and c[0] > c[1] and c[1] == c[3]:
        return "second3"
    if m >= 3 and c[0] > c[1] and c[1] == c[2]:
        return "second2"
    return None


TIE_CLASSES = ("top4", "top3", "top2_second_distinct", "second3", "second2")
