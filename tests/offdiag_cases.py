"""Seeded pairs that take K_atrace and K_vscan off the diagonal, with the
checker's answers and the geometry of the checker's path.

Everything here follows from verify_util (the numpy full-matrix DP and its
canonical traceback) and align_util; no constant is read from the kernels.  The
band of include/mpc_align.h, restated: given the checker's (d, end), the cell
(i, j) of a path to (m, end) sits in slot b = j - i - (end - m) + d of row i,
0 <= b < W = 2 d + 1.

A long contiguous run needs a stretch that matches nothing: ``N`` in the target
(one I run) or ``n`` in the read (one D run).  Random inserted bases do not
give one: under unit costs they break into short runs.
"""
import functools

import numpy as np

import align_util as au
import verify_util as vu

RUN_LENGTHS = (31, 32, 33, 63, 64, 65, 200)
CORE, LEFT, RIGHT = 700, 17, 23
I, D = au.OPS.index("I"), au.OPS.index("D")


def _flanked(rng, core, left=LEFT, right=RIGHT):
    return vu.rand_seq(rng, left) + core + vu.rand_seq(rng, right)


def run_cases():
    """[(note, oriented query, target, [(op, length)])]: pairs whose script must
    hold one run of exactly that op and length per planted stretch."""
    rng = np.random.default_rng(91)
    out = []
    for ln in RUN_LENGTHS:
        # a stretch nearer the read's start than its own length is cheaper to skip by the free text start
        for pos in [p for p in (63, 64, 65) if p > ln] + [300]:
            core = vu.rand_seq(rng, CORE)
            out.append(("I%d at %d" % (ln, pos), core, _flanked(rng, core[:pos] + b"N" * ln + core[pos:]), [(I, ln)]))
            core = vu.rand_seq(rng, CORE)
            out.append(("D%d at %d" % (ln, pos), core[:pos] + b"n" * ln + core[pos:], _flanked(rng, core), [(D, ln)]))
    # both directions in one read, in both orders: d = 160, W = 321
    core = vu.rand_seq(rng, 900)
    out.append(("D70 then I90", core[:300] + b"n" * 70 + core[300:], _flanked(rng, core[:600] + b"N" * 90 + core[600:]),
                [(D, 70), (I, 90)]))
    core = vu.rand_seq(rng, 900)
    out.append(("I90 then D70", core[:600] + b"n" * 70 + core[600:], _flanked(rng, core[:300] + b"N" * 90 + core[300:]),
                [(I, 90), (D, 70)]))
    # runs at the ends: down column 0 at the read's first rows, at its last rows, and close before column n
    core = vu.rand_seq(rng, CORE)
    out.append(("D40 first rows", b"n" * 40 + core, _flanked(rng, core, left=0), [(D, 40)]))
    core = vu.rand_seq(rng, CORE)
    out.append(("D70 last rows", core + b"n" * 70, _flanked(rng, core), [(D, 70)]))
    # (a run is crossed only where the read's tail behind it is longer than the run: with 10 bases behind it the
    # checker drops or mismatches the tail instead, so the tail is 60 and end = n)
    core = vu.rand_seq(rng, CORE)
    out.append(("I50, 60 before column n", core, _flanked(rng, core[:CORE - 60] + b"N" * 50 + core[CORE - 60:], right=0),
                [(I, 50)]))
    # three reads of ONE target (paf_batch): the target's N run alone, with an n run behind it, and on the minus strand
    core = vu.rand_seq(rng, CORE)
    target = _flanked(rng, core[:300] + b"N" * 65 + core[300:])
    out.append(("paf I65", core, target, [(I, 65)]))
    out.append(("paf I65 then D64", core[:500] + b"n" * 64 + core[500:], target, [(I, 65), (D, 64)]))
    out.append(("paf minus D33 then I65", core[:100] + b"n" * 33 + core[100:], target, [(D, 33), (I, 65)]))
    return out


def paf_batch():
    """(target, [(name, read)]) of the three 'paf' run cases as align_reads takes
    them: the third read is handed in reverse-complemented."""
    cases = [c for c in run_cases() if c[0].startswith("paf ")]
    assert len(cases) == 3 and len({c[2] for c in cases}) == 1
    reads = [cases[0][1], cases[1][1], au.revcomp(cases[2][1])]
    return cases[0][2], [(("read%d" % k).encode(), s) for k, s in enumerate(reads)]


def trace_cases():
    """[(note, oriented query, target)] for K_atrace: the run cases, dense
    divergence, low complexity, and the widest band the job rule admits."""
    out = [(note, q, t) for note, q, t, _ in run_cases()]
    rng = np.random.default_rng(92)
    q = vu.rand_seq(rng, 640)
    for rate in (0.03, 0.08):
        out.append(("mutate %.2f" % rate, q, _flanked(rng, vu.mutate(rng, q, rate))))
    for m, n in ((500, 700), (1500, 1700), (4000, 4200)):
        out.append(("unrelated %d x %d" % (m, n), vu.rand_seq(rng, m), vu.rand_seq(rng, n)))
    # low complexity: ties decide the script
    out.append(("ACAC phase shifts", b"AC" * 50 + b"A" + b"AC" * 50 + b"GG" + b"AC" * 50 + b"C" + b"AC" * 40, b"AC" * 220))
    out.append(("homopolymer, marker shifted, n < m", b"A" * 150 + b"G" + b"A" * 150, b"A" * 140 + b"G" + b"A" * 145))
    out.append(("homopolymer, two markers", b"A" * 100 + b"G" + b"A" * 100 + b"G" + b"A" * 100,
                b"A" * 90 + b"G" + b"A" * 115 + b"G" + b"A" * 100))
    # a path down column 0: d = MPC_ALIGN_MAX_EDITS, end = 0, one D run, W = 8193
    out.append(("column 0, d = 4096", b"C" * 4096, b"A" * 4101))
    return out


@functools.lru_cache(maxsize=None)
def traced():
    """(cases, [the checker's traceback per case]); computed once per process, never modified."""
    cases = trace_cases()
    return cases, [vu.traceback(q, t) for _, q, t in cases]


def path_geometry(q, t, tb):
    """(rows, slots, ops) of the checker's path, one entry per traceback step in
    the order the traceback takes them (end -> start): the step leaves cell
    (i, j), which is slot b = j - i - (end - m) + d of row i."""
    m, d, end = len(q), tb["distance"], tb["end"]
    ops = np.frombuffer(tb["ops"][::-1].encode(), np.uint8)
    up = (ops != ord("I")).astype(np.int64)    # = X D consume a query row
    left = (ops != ord("D")).astype(np.int64)  # = X I consume a text column
    i = m - (np.cumsum(up) - up)
    j = end - (np.cumsum(left) - left)
    assert len(ops) == 0 or (i[-1] - up[-1] == 0 and j[-1] - left[-1] == tb["start"])
    return i, j - i - (end - m) + d, ops


def job_launch(cases, tbs):
    """(seq, jobs) of one trace launch whose (d, end) are the CHECKER's."""
    seq, tab = vu.pack([(q, t) for _, q, t in cases])
    return seq, au.job_table(tab, [(tb["distance"], tb["end"]) for tb in tbs])


def expected_trace(jobs, tbs):
    """(out int32 [J, 8], runs int32[]) a trace launch must give: the checker's
    start, counts and runs (end -> start) at each job's run_off, zero elsewhere."""
    out = np.zeros((len(tbs), 8), np.int32)
    runs = np.zeros(int((jobs[:, 7] + 2 * jobs[:, 4] + 1).max()), np.int32)
    for k, tb in enumerate(tbs):
        r = au.runs_of(tb["ops"][::-1])
        assert len(r) <= 2 * tb["distance"] + 1
        out[k] = [0, tb["start"]] + vu.op_counts(tb["ops"]) + [len(r), 0]
        runs[jobs[k, 7]: jobs[k, 7] + len(r)] = r
    return out, runs


# ---- K_vscan ---------------------------------------------------------------------

# (m, K, last_k): the last row in an interior block of its lane; 8192: all 64 lanes, top bit 63
SCAN_SHAPES = ((4200, 2, 1), (8192, 2, 1), (8300, 4, 1), (8400, 4, 3), (16700, 8, 4), (33300, 16, 8))
TEXT_CAP = {16700: 4000, 33300: 3000}  # the checker's time grows with m x n: a shorter text, the query whole


def lanes(m, K):
    """(L, last_k): lanes in use and the block of the last lane that holds row m."""
    nblk = -(-m // 64)
    L = -(-nblk // K)
    return L, nblk - 1 - (L - 1) * K


def scan_cases():
    """[(note, query, text)] for K_vscan."""
    rng = np.random.default_rng(93)
    out = []
    for m, K, last_k in SCAN_SHAPES:
        L, lk = lanes(m, K)
        assert lk == last_k and 0 < lk < K and 64 * 64 * K >= m > 64 * 64 * K // 2
        q = vu.rand_seq(rng, m)
        n = TEXT_CAP.get(m, m)
        a = int(rng.integers(0, m - n + 1))
        w = q[a: a + n]  # the stretch of the query the related texts come from
        out.append(("m=%d unrelated" % m, q, vu.rand_seq(rng, n)))
        out.append(("m=%d mutated" % m, q, vu.mutate(rng, w, 0.05)))
        out.append(("m=%d N70 in, 70 out" % m, q, w[:n // 3] + b"N" * 70 + w[n // 3: 2 * n // 3] + w[2 * n // 3 + 70:]))
        out.append(("m=%d n=L-1" % m, q, vu.rand_seq(rng, L - 1)))
        out.append(("m=%d n=1" % m, q, vu.rand_seq(rng, 1)))
    return out


@functools.lru_cache(maxsize=None)
def scanned():
    """(cases, [vu.score per case]); computed once per process, never modified."""
    cases = scan_cases()
    return cases, [vu.score(q, t) for _, q, t in cases]
