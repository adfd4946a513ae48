"""The checker of align_reads: the definition of include/mpc_align.h restated as
a whole on top of verify_util's numpy full-matrix DP and canonical traceback --
strand, mapped or not, the end rule, the PAF fields, the cs tag -- plus a check
of a PAF line that does not depend on the DP (its cs applied to the target span
gives back the read span, and the field sums agree), the seeded case grid the
CPU, sanitizer and GPU tests share, and planted-edit reads."""
import math

import numpy as np

import verify_util as vu

MAX_EDITS = 4096
MAX_QUERY = 65536
OPS = "=XID"  # run op codes 0..3, verify's letters
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    """A C G T complemented case-insensitively (the case kept), everything else kept; reversed."""
    return bytes(s).translate(_COMP)[::-1]


def runs_of(ops):
    """[(length << 2 | op)] of an op string, in the order given."""
    out, k = [], 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out.append(((e - k) << 2) | OPS.index(ops[k]))
        k = e
    return out


def expect(read, target, max_error=0.2, name=b"r", tname=b"t"):
    """Everything the definition says about one read: dict(scan, strand, d, end,
    mapped, why, trace, line).  why: None (a line), "distance" or "no_match";
    trace = (start, [n_eq, n_x, n_i, n_d], runs end -> start) when the read
    passes the distance rule."""
    read, target = bytes(read), bytes(target)
    m, n = len(read), len(target)
    assert 1 <= m <= MAX_QUERY and n >= 1
    qm = revcomp(read)
    (dp, ep), (dm, em) = vu.score(read, target), vu.score(qm, target)
    minus = dm < dp  # a tie is '+'
    q, d, end = (qm, dm, em) if minus else (read, dp, ep)
    res = dict(scan=(dp, ep, dm, em), strand=int(minus), d=d, end=end, q=q, trace=None, line=None, why=None)
    res["mapped"] = d <= min(math.floor(max_error * m), MAX_EDITS)
    if not res["mapped"]:
        res["why"] = "distance"
        return res
    tb = vu.traceback(q, target)
    assert (tb["distance"], tb["end"]) == (d, end)
    ops, start = tb["ops"], tb["start"]
    res["trace"] = (start, vu.op_counts(ops), runs_of(ops[::-1]))
    first, last = ops.find("="), ops.rfind("=")
    if first < 0:
        res["why"] = "no_match"
        return res
    lead, kept, trail = ops[:first], ops[first:last + 1], ops[last + 1:]
    a, b = sum(lead.count(c) for c in "XD"), sum(trail.count(c) for c in "XD")
    ts, te = start + sum(lead.count(c) for c in "XI"), end - sum(trail.count(c) for c in "XI")
    cs, i, j, k = [], a, ts, 0
    while k < len(kept):
        e = k
        while e < len(kept) and kept[e] == kept[k]:
            e += 1
        ln, op = e - k, kept[k]
        if op == "=":
            cs.append(":%d" % ln)
            i, j = i + ln, j + ln
        elif op == "X":
            cs += ["*%s%s" % (chr(target[j + x]).lower(), chr(q[i + x]).lower()) for x in range(ln)]
            i, j = i + ln, j + ln
        elif op == "D":  # a read base missing from the target: an insertion
            cs.append("+" + q[i:i + ln].decode().lower())
            i += ln
        else:            # an extra target base: a deletion
            cs.append("-" + target[j:j + ln].decode().lower())
            j += ln
        k = e
    assert (i, j) == (m - b, te)
    qs, qe = (b, m - a) if minus else (a, m - b)
    n_eq = kept.count("=")
    fields = [name.decode(), m, qs, qe, "-" if minus else "+", tname.decode(), n, ts, te, n_eq, len(kept), 255,
              "NM:i:%d" % (len(kept) - n_eq), "cs:Z:" + "".join(cs)]
    res["line"] = ("\t".join(str(f) for f in fields) + "\n").encode()
    return res


def expected_batch(target, tname, records, max_error=0.2):
    """(PAF bytes, summary counts, [expect() or None per record]) of a batch in order."""
    counts = dict.fromkeys(("reads", "mapped", "plus", "minus", "unmapped_by_distance", "unmapped_no_match", "skipped_length"), 0)
    lines, per = [], []
    for name, s in records:
        counts["reads"] += 1
        if not 1 <= len(s) <= MAX_QUERY:
            counts["skipped_length"] += 1
            per.append(None)
            continue
        e = expect(s, target, max_error, name, tname)
        per.append(e)
        if e["line"] is None:
            counts["unmapped_by_distance" if e["why"] == "distance" else "unmapped_no_match"] += 1
        else:
            lines.append(e["line"])
            counts["mapped"] += 1
            counts["minus" if e["strand"] else "plus"] += 1
    return b"".join(lines), counts, per


def check_line(line, target, read):
    """The DP-free check of one PAF line: applying its cs to target[ts:te] gives
    the oriented read's span, and the columns agree with the cs."""
    f = line.decode().rstrip("\n").split("\t")
    assert len(f) == 14 and line.endswith(b"\n")
    m, qs, qe, n, ts, te, n_eq, n_ops = (int(f[k]) for k in (1, 2, 3, 6, 7, 8, 9, 10))
    assert f[4] in "+-" and f[11] == "255" and f[12].startswith("NM:i:") and f[13].startswith("cs:Z:")
    assert (m, n) == (len(read), len(target)) and 0 <= qs < qe <= m and 0 <= ts < te <= n
    q = revcomp(read) if f[4] == "-" else bytes(read)
    a, b = (m - qe, m - qs) if f[4] == "-" else (qs, qe)  # the span on the oriented read
    cs, k, j = f[13][5:], 0, ts
    built, eq, ops = [], 0, 0
    assert cs[0] == ":" and cs.rsplit(":", 1)[1].isdigit()  # the kept span starts and ends with a match
    while k < len(cs):
        e = k + 1
        while e < len(cs) and cs[e] not in ":*+-":
            e += 1
        body = cs[k + 1:e]
        if cs[k] == ":":
            ln = int(body)
            assert ln >= 1
            seg = target[j:j + ln]
            assert all(vu.codes(seg, 5) < 4)  # a match is an A C G T match
            built.append(seg.upper())
            j, eq, ops = j + ln, eq + ln, ops + ln
        elif cs[k] == "*":
            assert len(body) == 2 and body == body.lower() and chr(target[j]).lower() == body[0]
            assert vu.codes(body[0].encode(), 5)[0] != vu.codes(body[1].encode(), 4)[0]
            built.append(body[1].upper().encode())
            j, ops = j + 1, ops + 1
        elif cs[k] == "+":
            assert body and body == body.lower()
            built.append(body.upper().encode())
            ops += len(body)
        else:
            assert body and body == target[j:j + len(body)].decode().lower()
            j, ops = j + len(body), ops + len(body)
        k = e
    assert j == te
    assert b"".join(built) == q[a:b].upper()
    assert (eq, ops) == (n_eq, n_ops) and f[12] == "NM:i:%d" % (ops - eq)


# ---- seeded cases ----------------------------------------------------------------

def _sub(c, rng):
    return b"ACGT"[(b"ACGT".index(bytes([c]).upper()) + 1 + int(rng.integers(0, 3))) % 4] if bytes([c]).upper() in b"ACGT" else 65


def plant_subs(rng, s, k):
    """s with k substitutions at least 3 apart and off the ends (all of them when s is too short for that)."""
    b = bytearray(s)
    cand = np.arange(5, len(b) - 5, 3) if len(b) >= 16 + 3 * k else np.arange(len(b))
    for p in rng.choice(cand, size=min(k, len(cand)), replace=False):
        b[p] = _sub(b[p], rng)
    return bytes(b)


def planted(rng, m, d, left=17, right=23, indels=False):
    """(read, target, d): a read of m bases with d planted edits, at least 3
    apart and off the ends (substitutions, or with ``indels`` 1-3-base
    insertions and deletions whose lengths sum to the d returned), the target
    with random flanks."""
    core = vu.rand_seq(rng, m)
    if not indels:
        return plant_subs(rng, core, d), vu.rand_seq(rng, left) + core + vu.rand_seq(rng, right), d
    # alternate deleting ln read bases from / inserting ln fresh bases into the target, events >= 12 apart
    tcore, at, todo, flip = bytearray(), 0, d, False
    step = max(12, (m - 16) // max(1, d))
    p = 8
    while todo > 0 and p + 8 < m:
        ln = min(int(rng.integers(1, 4)), todo)
        tcore += core[at:p]
        if flip:   # the target lacks ln read bases (an insertion in the read)
            at = p + ln
        else:      # the target holds ln extra bases (a deletion in the read)
            tcore += vu.rand_seq(rng, ln)
            at = p
        flip, todo, p = not flip, todo - ln, p + step
    tcore += core[at:]
    return bytes(core), vu.rand_seq(rng, left) + bytes(tcore) + vu.rand_seq(rng, right), d - todo


GRID_M = (1, 2, 63, 64, 65, 129, 200)


def grid(seed=21):
    """[dict(kind, m, target, read, max_error)]: for every m of GRID_M a target
    of m + 57 bases (a palindrome in the middle, a lower-case stretch, two N)
    and reads of exactly m bases of every kind the definition distinguishes."""
    rng = np.random.default_rng(seed)
    out = []

    def add(kind, m, target, read, me=0.2):
        assert len(read) == m, (kind, m, len(read))
        out.append(dict(kind=kind, m=m, target=bytes(target), read=bytes(read), max_error=me))

    for m in GRID_M:
        half = vu.rand_seq(rng, m // 2)
        pal = half + (b"N" if m % 2 else b"") + revcomp(half)  # equals its own reverse complement
        assert pal == revcomp(pal) and len(pal) == m
        t = bytearray(vu.rand_seq(rng, 30) + pal + vu.rand_seq(rng, 27))
        t[3:10] = bytes(t[3:10]).lower()
        t[12], t[len(t) - 9] = ord("N"), ord("n")
        t = bytes(t)
        n = len(t)
        k = max(1, m // 40)
        add("inside", m, t, plant_subs(rng, t[20:20 + m], k))
        add("flush0", m, t, plant_subs(rng, t[:m], k))
        add("flushn", m, t, plant_subs(rng, t[n - m:], k))
        add("minus", m, t, revcomp(plant_subs(rng, t[25:25 + m], k)))
        add("tie", m, t, pal, 1.0)
        add("exact", m, t, t[30:30 + m].upper(), 1.0)
        low = bytearray(plant_subs(rng, t[15:15 + m], k))
        low[: m // 2] = bytes(low[: m // 2]).lower()
        if m > 2:
            low[m - 2] = ord("R")
        add("nonacgt", m, t, low, 0.5)
        if m >= 63:  # one insertion and one deletion: the script leaves the main diagonal
            s = bytearray(t[18:18 + m])
            del s[20]
            s[40:40] = b"G" if t[18 + 41] != ord("G") else b"C"
            add("indel", m, t, s)
        # d just at and just above floor(max_error m)
        th = plant_subs(rng, t[22:22 + m], max(1, m // 5))
        if m <= 2:
            th = b"N" + th[1:]
        d = min(vu.score(th, t)[0], vu.score(revcomp(th), t)[0])
        add("at_limit", m, t, th, (d + 0.5) / m)
        if d >= 1:
            add("above_limit", m, t, th, (d - 0.5) / m)
        # read longer than the target; a read of only mismatches
        short = vu.rand_seq(rng, max(1, m // 2))
        pad = m - len(short)
        add("longer", m, short, vu.rand_seq(rng, pad // 2) + short + vu.rand_seq(rng, pad - pad // 2), 1.0)
        add("longer", m, short, vu.rand_seq(rng, pad // 2) + short + vu.rand_seq(rng, pad - pad // 2))
        add("mismatch_only", m, b"A" * (m + 5), b"C" * m, 1.0)
        add("mismatch_only", m, b"A" * (m + 5), b"C" * m)
    return out


def batches(cases):
    """The cases grouped into batches of one (target, max_error) each, in first-seen
    order: [(target, max_error, [(name, read)])]; names are unique."""
    seen, out = {}, []
    for k, c in enumerate(cases):
        key = (c["target"], c["max_error"])
        if key not in seen:
            seen[key] = len(out)
            out.append((c["target"], c["max_error"], []))
        out[seen[key]][2].append((("%s_m%d_%d" % (c["kind"], c["m"], k)).encode(), c["read"]))
    return out


# ---- one launch of the trace: shapes, job table, refused rows ---------------------

def trace_shapes():
    """[(note, oriented query, target, planted d or None)]"""
    rng = np.random.default_rng(77)
    out = []
    # exactly d planted substitutions: W = 2 d + 1 inside, at and past one and two 64-lane rows
    for d in (0, 1, 31, 32, 63, 64, 100):
        q, t, _ = planted(rng, 700, d)
        out.append(("subs d=%d" % d, q, t, d))
    q, t, d = planted(rng, 700, 40, indels=True)
    assert d == 40
    out.append(("indels", q, t, d))
    for m in (1, 63, 64, 65, 1000, 5000):
        d = min(5, m // 16)
        q, t, _ = planted(rng, m, d)
        out.append(("m=%d" % m, q, t, d))
    # bands cut by column 0 and by column n
    q, t, d = planted(rng, 300, 20, left=0, right=30)
    out.append(("column 0", q, t, 20))
    q, t, d = planted(rng, 300, 20, left=30, right=0)
    out.append(("column n", q, t, 20))
    q, t, d = planted(rng, 300, 33, left=3, right=2, indels=True)
    out.append(("both columns", q, t, None))
    # n < m: the read hangs over both ends of the target
    core = vu.rand_seq(rng, 260)
    out.append(("n < m", vu.rand_seq(rng, 12) + core + vu.rand_seq(rng, 9), core, 21))
    out.append(("n = 1", vu.rand_seq(rng, 5), b"G", None))
    # minus strand: the oriented query is the reverse complement
    q, t, _ = planted(rng, 500, 9)
    out.append(("minus", revcomp(q), revcomp(t), 9))
    out.append(("non-ACGT, lower case", vu.sprinkle(rng, q), vu.sprinkle(rng, t), None))
    return out


def job_table(tab, scan):
    """int64 [n, 8] jobs of a pair table and its scan results, flag rows and runs back to back."""
    jobs = np.zeros((len(tab), 8), np.int64)
    jobs[:, :4] = tab
    jobs[:, 4:6] = np.array(scan, np.int64)
    pitch = (2 * jobs[:, 4] + 1 + 63) // 64 * 64
    jobs[:, 6] = np.concatenate([[0], np.cumsum(jobs[:, 1] * pitch)[:-1]])
    jobs[:, 7] = np.concatenate([[0], np.cumsum(2 * jobs[:, 4] + 1)[:-1]])
    return jobs


def refused_jobs(seq):
    """(row, column, value) that each make the job table of trace_shapes() one the job rule refuses;
    column 6 (flag_off) is the device entry point's part of the rule."""
    return ((0, 1, 0), (0, 1, 65537), (1, 4, 4097), (1, 4, -1), (0, 5, -1), (0, 0, seq.nbytes), (3, 6, 0), (0, 6, -1), (0, 7, -1))


def cigar_of(runs):
    """The CIGAR (start -> end) of a read's runs (end -> start)."""
    return "".join("%d%s" % (r >> 2, OPS[r & 3]) for r in reversed(runs))
