"""What the handoff tests share.  The checker is what the handoff replaces:
the PAF that align's host renderer writes for a launch, ingested together with
the reads file by ingest.pack_sample (native and Python, which the suite holds
equal) -- cs, cs_off, tstart, up, up_off, down, down_off exactly as the pileup
takes them.  A "launch" here is what align.Launches yields for device="cpu", or
a crafted one whose runs no optimal alignment gives (dropped deletions at the
ends), which the renderer and the handoff take all the same.

The seeded case batches: the grid of align_util and the long runs of
offdiag_cases (imported, not edited), and the handoff's own -- kept run counts
around the 64-run chunk, '=' runs of every digit count, the end rule, letters.
"""
import functools
import os

import numpy as np

import align_util as au
import offdiag_cases as oc
import verify_util as vu

KEYS = ("cs", "cs_off", "tstart", "up", "up_off", "down", "down_off")
FILL = 0xA5  # what output buffers hold before a launch


class Launch:
    """One traced launch against ``target``: the blob, the tables, and per job
    its name, strand and the read as the FASTA holds it."""

    def __init__(self, target, seq, jobs, strand, out, runs, names, originals):
        self.target, self.seq, self.jobs, self.out, self.runs = target, seq, jobs, out, runs
        self.strand, self.names, self.originals = np.asarray(strand, np.uint8), names, originals

    def kept_runs(self, k):
        """The number of runs between the outermost '=' of job k (0: none)."""
        ops = self.runs[self.jobs[k, 7]: self.jobs[k, 7] + self.out[k, 6]] & 3
        eq = np.nonzero(ops == 0)[0]
        return int(eq[-1] - eq[0] + 1) if len(eq) else 0

    def eq_lengths(self, k):
        """The lengths of job k's '=' runs, start -> end."""
        r = self.runs[self.jobs[k, 7]: self.jobs[k, 7] + self.out[k, 6]][::-1]
        return [int(x >> 2) for x in r if x & 3 == 0]


def launches(al, target, records, max_error, workspace_bytes=None):
    """The launches of the records on the host (reads of unsupported length left out)."""
    records = [(n, s) for n, s in records if 1 <= len(s) <= au.MAX_QUERY]
    loop = al.Launches(target, [s for _, s in records], "cpu", max_error, workspace_bytes or al.DEFAULT_WORKSPACE)
    out = []
    for reads, jobs, o, runs, _ in loop:
        out.append(Launch(target, loop.pk.seq, jobs, loop.plan[reads, 0], o, runs, [records[r][0] for r in reads],
                          [records[r][1] for r in reads]))
    return out


def crafted(target, specs):
    """A launch from scripts written by hand.  specs: [(name, oriented read,
    strand, start, [(op letter, length)] start -> end)]; the runs must walk the
    read (checked here), the op letters are verify's = X I D."""
    n = len(target)
    blob, jobs, outs, runs = [bytes(target)], [], [], []
    q_off = n
    for name, q, strand, start, script in specs:
        enc = [(ln << 2) | au.OPS.index(op) for op, ln in script][::-1]
        cnt = [sum(ln for op, ln in script if op == c) for c in au.OPS]
        assert cnt[0] + cnt[1] + cnt[3] == len(q), name
        d = max(cnt[1] + cnt[2] + cnt[3], len(enc))
        jobs.append([q_off, len(q), 0, n, d, start + cnt[0] + cnt[1] + cnt[2], 0, len(runs)])
        outs.append([0, start] + cnt + [len(enc), 0])
        runs += enc + [0] * (2 * d + 1 - len(enc))
        blob.append(bytes(q))
        q_off += len(q)
    seq = np.frombuffer(b"".join(blob) + b"\0" * 8, np.uint8).copy()
    return Launch(bytes(target), seq, np.array(jobs, np.int64).reshape(-1, 8), [s[2] for s in specs],
                  np.array(outs, np.int32).reshape(-1, 8), np.array(runs, np.int32), [s[0] for s in specs],
                  [au.revcomp(s[1]) if s[2] else bytes(s[1]) for s in specs])


def write_fasta(path, records):
    with open(path, "wb") as f:
        for name, s in records:
            f.write(b">" + name + b"\n" + s + b"\n")


def checker(pkg, tmp, launches_, native=True, tname=b"tgt"):
    """ingest.pack_sample of the PAF align renders for the launches and of their reads."""
    al = pkg.align
    ref, paf, reads = (os.path.join(str(tmp), x) for x in ("ref.fa", "x.paf", "reads.fa"))
    write_fasta(ref, [(tname, launches_[0].target)])
    write_fasta(reads, [(n, s) for ln in launches_ for n, s in zip(ln.names, ln.originals)])
    with open(paf, "wb") as f:
        for ln in launches_:
            f.write(al.render(ln.seq, ln.jobs, ln.strand, ln.out, ln.runs, ln.names, tname)[0])
    return pkg.ingest.pack_sample(ref, paf, reads, native=native)


def host_sample(pkg, launches_, threads=3):
    """(the sample the host twins assemble, the size rows of every launch)."""
    pile = pkg.handoff.Pile("cpu")
    sizes = [pile.add(ln.seq, ln.jobs, ln.out, ln.runs, threads) for ln in launches_]
    ref = np.frombuffer(launches_[0].target.upper(), np.uint8)
    return pile.sample(ref), sizes


def assert_same(got, want, note=""):
    for k in KEYS + ("ref",):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), (note, k)


# ---- the case batches: (note, target, max_error, [(name, read)]) -----------------

def _named(prefix, reads):
    return [(("%s%d" % (prefix, k)).encode(), s) for k, s in enumerate(reads)]


def _sub(c):
    """A base that differs from c (upper case)."""
    return b"CGTA"[b"ACGT".index(bytes([c]).upper())]


def _with_subs(s, positions):
    b = bytearray(s)
    for p in positions:
        b[p] = _sub(b[p])
    return bytes(b)


RUN_COUNTS = (1, 63, 64, 65, 127, 128, 129, 193, 194)
SPACING = 6


def run_count_batch():
    """Reads whose kept run count is each of RUN_COUNTS: k substitutions every
    SPACING bases give 2 k + 1 runs; an even count has one base replaced by "nn"
    (a substitution and an insertion: two runs of different ops side by side).  Every
    second read also starts with a substitution, which the end rule drops."""
    rng = np.random.default_rng(301)
    target = vu.rand_seq(rng, 1400)
    reads = []
    for x, want in enumerate(RUN_COUNTS):
        k = (want - 1) // 2 if want % 2 else (want - 4) // 2  # an even count: three runs come from the "nn"
        m = SPACING * (k + 2)
        a = 20 + 3 * x
        s = bytearray(_with_subs(target[a: a + m], range(SPACING, SPACING * (k + 1), SPACING)))
        if want % 2 == 0:
            p = SPACING * (k + 1)
            s[p: p + 1] = b"nn"  # one target base under two read bases that match nothing
        if x % 2:
            s[0] = _sub(s[0])
        reads.append(bytes(s))
    return "run counts", target, 0.5, _named("runs", reads)


EQ_LENGTHS = (9, 10, 99, 100, 999, 1000, 9999)


def digit_batch():
    """'=' runs of 9 .. 9999 bases in one read (six single substitutions), 10000 in another."""
    rng = np.random.default_rng(302)
    target = vu.rand_seq(rng, 12300)
    cuts = np.cumsum([ln + 1 for ln in EQ_LENGTHS])[:-1] - 1  # the substituted positions
    total = sum(EQ_LENGTHS) + len(EQ_LENGTHS) - 1
    one = _with_subs(target[30: 30 + total], cuts)
    two = _with_subs(target[100: 100 + 10000 + 1 + 40], [10000])
    return "digits", target, 0.2, [(b"digits", one), (b"tenthousand", two)]


def end_rule_batch():
    """Dropped leading, trailing and both-end substitutions on both strands, and
    a read with no '=' between two that have one."""
    rng = np.random.default_rng(303)
    target = vu.rand_seq(rng, 400)
    core = target[50:250]
    lead, trail, both = _with_subs(core, [0, 1]), _with_subs(core, [198, 199]), _with_subs(core, [0, 198, 199])
    reads = [lead, trail, both, b"N", core, au.revcomp(lead), au.revcomp(trail), au.revcomp(both)]
    return "end rule", target, 1.0, _named("end", reads)


def letters_batch():
    """Lower-case reads on a target with a lower-case stretch; N inside an
    insertion, inside a substitution and inside a dropped flank of '+' reads."""
    rng = np.random.default_rng(304)
    t = bytearray(vu.rand_seq(rng, 500))
    t[100:220] = bytes(t[100:220]).lower()
    target = bytes(t)
    core = target[60:360].upper()
    low = _with_subs(core, [40, 41, 150]).lower()
    ins = core[:120] + b"NN" + core[120:]
    sub = core[:200] + b"N" + core[201:]
    flank = b"NNN" + _with_subs(core, [0])[0:1] + core[1:] + b"N"
    mixed = bytearray(_with_subs(core, [77]))
    mixed[::2] = bytes(mixed[::2]).lower()
    return "letters", target, 0.5, _named("let", [low, ins, sub, flank, bytes(mixed), au.revcomp(low)])


def crafted_launch():
    """Scripts no optimal alignment gives: dropped deletions (verify's I) at
    either end, so that a_t and b_t are not 0 and tstart moves; on both strands."""
    rng = np.random.default_rng(305)
    target = vu.rand_seq(rng, 300)
    specs = []
    for k, (strand, start) in enumerate(((0, 10), (1, 40), (0, 0))):
        script = [("X", 1), ("I", 2), ("D", 1), ("=", 30), ("X", 2), ("D", 3), ("=", 7), ("I", 4), ("=", 1), ("I", 3),
                  ("X", 2), ("I", 1)]
        q = vu.rand_seq(rng, sum(ln for op, ln in script if op in "=XD"))
        specs.append((b"crafted%d" % k, q, strand, start, script))
    specs.insert(1, (b"nomatch", b"ACN", 0, 5, [("X", 2), ("I", 1), ("D", 1)]))
    specs.append((b"nomatch_minus", b"GTTN", 1, 20, [("D", 1), ("X", 3), ("I", 2)]))  # no '=' on the minus strand either
    return crafted(target, specs)


def natural_batches():
    grid = [("grid %d" % k, t, me, recs) for k, (t, me, recs) in enumerate(au.batches(au.grid()))]
    t, recs = oc.paf_batch()
    return grid + [("offdiag", t, 0.5, recs), run_count_batch(), digit_batch(), end_rule_batch(), letters_batch()]


@functools.lru_cache(maxsize=None)
def all_launches():
    """[(note, [Launch])] of every case batch on the host, computed once per process, never modified."""
    import importlib
    al = importlib.import_module("minion-plasmid-consensus_amd").align
    out = [(note, launches(al, t, recs, me)) for note, t, me, recs in natural_batches()]
    return out + [("crafted", [crafted_launch()])]


def one_launch(sets):
    """The launches of several batches joined into ONE launch over one blob
    (every batch keeps its own target inside the blob)."""
    seqs, jobs, outs, runs, at, run_at = [], [], [], [], 0, 0
    for ln in sets:
        j = ln.jobs.copy()
        j[:, 0] += at
        j[:, 2] += at
        j[:, 7] += run_at
        j[:, 6] = 0
        jobs.append(j)
        outs.append(ln.out)
        runs.append(ln.runs)
        seqs.append(ln.seq)
        at += len(ln.seq)
        run_at += len(ln.runs)
    return (np.concatenate(seqs), np.concatenate(jobs), np.concatenate(outs), np.concatenate(runs))
