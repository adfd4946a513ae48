"""The checker of draft_assembly: the vote and the call of include/mpc_draft.h
restated in plain Python / numpy, one base at a time and without difference
arrays on the way in (every aligned base is expanded), plus the seeded cases the
CPU, sanitizer and GPU tests share: the planted reads of one 900-base target,
and injected tallies for the call."""
import numpy as np

import align_util as au
import verify_util as vu

ROW, SLOTS, MAX_LEN = 48, 8, 131072
STARTS, ENDS, EQ_ON, EQ_OFF, DEL_ON, DEL_OFF, SUB, INS = 0, 1, 2, 3, 4, 5, 8, 16
VOTED, BAD_RUNS, NO_MATCH, NOT_TRACED = 0, 1, 2, 3
OPS = "=XID"


def _code(byte):
    return "ACGT".find(chr(byte).upper())  # -1: votes nothing


def vote(n, reads):
    """uint32 [n + 1, ROW] tallies of reads = [(oriented query, start, runs end -> start)]."""
    t = np.zeros((n + 1, ROW), np.int64)
    for q, start, runs in reads:
        ops = "".join(OPS[r & 3] * (r >> 2) for r in reversed(runs))  # start -> end, one letter per op
        first, last = ops.find("="), ops.rfind("=")
        if first < 0:
            continue
        i, j = 0, start
        prev = None
        slot = 0
        for k, op in enumerate(ops):
            keep = first <= k <= last
            if keep and k == first:
                t[j, STARTS] += 1
            if keep:
                new_run = op != prev
                if op == "=":
                    if new_run:
                        t[j, EQ_ON] += 1
                    if k == last or ops[k + 1] != "=":
                        t[j + 1, EQ_OFF] += 1
                elif op == "X":
                    if _code(q[i]) >= 0:
                        t[j, SUB + _code(q[i])] += 1
                elif op == "I":  # an extra target base: a deletion
                    if new_run:
                        t[j, DEL_ON] += 1
                    if ops[k + 1] != "I":
                        t[j + 1, DEL_OFF] += 1
                else:            # a read base missing from the target: an insertion in front of column j
                    slot = 0 if new_run else slot + 1
                    if slot < SLOTS and _code(q[i]) >= 0:
                        t[j, INS + 4 * slot + _code(q[i])] += 1
            prev = op if keep else None
            if op != "I":
                i += 1
            if op != "D":
                j += 1
            if keep and k == last:
                t[j, ENDS] += 1
        assert i == len(q)
    return t.astype(np.uint32)


def call(tally, draft):
    """(new draft bytes or None, info [8]) from uint32 [n + 1, ROW] tallies."""
    n = len(draft)
    t = np.asarray(tally, np.uint32).astype(np.int64).reshape(n + 1, ROW)
    cov = np.cumsum(t[:, STARTS] - t[:, ENDS])
    eq = np.cumsum(t[:, EQ_ON] - t[:, EQ_OFF])
    dl = np.cumsum(t[:, DEL_ON] - t[:, DEL_OFF])
    maxcov = max(0, int(cov[:n].max()))
    if maxcov == 0:
        return None, [1, 0, 0, 0, 0, 0, 0, 0]
    keep = np.nonzero(2 * cov[:n] >= maxcov)[0]
    lo, hi = int(keep[0]), int(keep[-1]) + 1
    out = bytearray()
    changed = dropped = inserted = 0
    for j in range(lo, hi):
        if j > lo:
            gcov = cov[j] - t[j, STARTS]
            for s in range(SLOTS):
                v = t[j, INS + 4 * s: INS + 4 * s + 4]
                if not 2 * v.sum() > gcov:
                    break
                out.append(b"ACGT"[int(np.argmax(v))])  # (argmax: the first, so the smallest code)
                inserted += 1
        dc = _code(draft[j])
        base = t[j, SUB: SUB + 4].copy()
        if dc >= 0:
            base[dc] += eq[j]
        if base.sum() == 0:
            out.append(draft[j])
        elif 2 * dl[j] > cov[j]:
            dropped += 1
        else:
            code = dc if dc >= 0 and base[dc] == base.max() else int(np.argmax(base))
            out.append(b"ACGT"[code])
            changed += code != dc
    status = 2 if len(out) > MAX_LEN else 0
    return bytes(out), [status, len(out), lo, hi, maxcov, changed, dropped, inserted]


# ---- the planted reads of one target ------------------------------------------------

MAX_ERROR = 0.3


def vote_reads(seed=31):
    """(target of 900 bases, [(note, read)]): reads on both strands (every odd
    one is given as its reverse complement)."""
    rng = np.random.default_rng(seed)
    t = vu.rand_seq(rng, 900)
    n = len(t)
    out = []

    def other(c):
        return b"ACGT"[(b"ACGT".index(bytes([c])) + 1 + int(rng.integers(0, 3))) % 4]

    for d in (0, 1, 31, 70):  # 70 substitutions at least 3 apart: 141 runs, three chunks of 64
        out.append(("subs %d" % d, au.plant_subs(rng, t[40:840], d)))
    gap = [c for c in b"ACGT" if c not in (t[399], t[400])][:1] * 20  # (a base its neighbours cannot match: ONE run)
    for ln in (1, 8, 9, 20):
        out.append(("insertion %d" % ln, t[30:400] + bytes(gap[:ln]) + t[400:830]))
    out.append(("deletions", t[20:200] + t[203:500] + t[512:700] + t[701:860]))
    s = bytearray(t[50:850])
    s[0], s[-1] = other(s[0]), other(s[-1])
    out.append(("ends not '='", bytes(s)))
    out.append(("from column 0", t[:700]))
    out.append(("to column n", au.plant_subs(rng, t[200:], 5)))
    out.append(("whole target", t))
    out.append(("interior partial", t[300:500]))
    s = bytearray(t[60:820])
    s[100] = ord("N")                      # a substitution that votes nothing
    s[200:204] = bytes(s[200:204]).lower()  # lower-case matches
    s[300] = ord(bytes([other(s[300])]).lower())  # a lower-case substitution
    s[400:400] = b"AcnGt"                  # an insertion with N and lower case inside
    out.append(("N and lower case", bytes(s)))
    out.append(("one base", t[450:451]))
    out.append(("unmapped", vu.rand_seq(rng, 400)))
    for a, ln in ((5, 880), (0, 900), (100, 650)):  # depth for the call
        out.append(("plain", au.plant_subs(rng, t[a:a + ln], 4)))
    return t, [(note, au.revcomp(r) if k % 2 else r) for k, (note, r) in enumerate(out)]


def traced(pkg, target, reads, device, workspace_bytes=None, threads=2):
    """The reads aligned to the target as a round does it: [(pk, jobs, out,
    runs, kept, read indices)] per launch, and the plan."""
    al = pkg.align
    loop = al.Launches(target, reads, device, MAX_ERROR, workspace_bytes if workspace_bytes is not None else al.DEFAULT_WORKSPACE,
                       threads, keep_device=True)
    return [(loop.pk, jobs, out, runs, kept or {}, rd) for rd, jobs, out, runs, kept in loop], loop.plan


def checker_reads(launch, skip=()):
    """A launch's reads as vote() takes them."""
    pk, jobs, out, runs, _, _ = launch
    res = []
    for k in range(len(jobs)):
        if k in skip or out[k, 0] != 0:
            continue
        q = bytes(pk.seq[jobs[k, 0]: jobs[k, 0] + jobs[k, 1]])
        res.append((q, int(out[k, 1]), runs[jobs[k, 7]: jobs[k, 7] + out[k, 6]].tolist()))
    return res


# ---- injected tallies for the call ----------------------------------------------------

def tallies_of(cov, eq, dl):
    """uint32 [n + 1, ROW] whose prefix sums are the given per-column cov, eq, del (0 behind column n - 1)."""
    n = len(cov)
    t = np.zeros((n + 1, ROW), np.int64)
    for on, off, v in ((STARTS, ENDS, cov), (EQ_ON, EQ_OFF, eq), (DEL_ON, DEL_OFF, dl)):
        diff = np.diff(np.concatenate([[0], np.asarray(v, np.int64), [0]]))
        t[:, on] = np.maximum(diff, 0)
        t[:, off] = np.maximum(-diff, 0)
    return t


def random_call_case(rng, n, depth=30, trim=True, p_drop=0.02, p_ins=0.02, long_ins=False):
    """(draft, tallies): a coverage that ramps at both ends (trim) or not, most
    columns confirmed, some substituted, dropped, tied, unvoted, and insertion
    slot chains of every length."""
    draft = bytearray(vu.rand_seq(rng, n))
    cov = np.full(n, depth, np.int64)
    if trim and n >= 8:
        ramp = min(n // 4, 40)
        cov[:ramp] = np.minimum(depth, 1 + np.arange(ramp) * depth // (2 * ramp))
        cov[n - ramp:] = cov[:ramp][::-1]
    dl = np.where(rng.random(n) < p_drop, rng.integers(0, depth + 1, n), rng.integers(0, 3, n))
    dl = np.minimum(dl, cov)
    eq = np.maximum(cov - dl - rng.integers(0, 3, n), 0)
    t = tallies_of(cov, eq, dl)
    for j in range(n):
        r = rng.random()
        if r < 0.05:    # substitutions outvote (or tie with) the draft base
            t[j, SUB + int(rng.integers(0, 4))] += int(eq[j]) + int(rng.integers(0, 2))
        elif r < 0.08:  # no vote at all (a draft byte that is no base takes no '='): the byte stays as it is
            draft[j] = ord("n")
        elif r < 0.12:
            t[j, SUB + int(rng.integers(0, 4))] += int(rng.integers(1, 4))
        if rng.random() < p_ins:
            k = SLOTS if long_ins else int(rng.integers(1, SLOTS + 1))
            for s in range(k):
                t[j, INS + 4 * s + int(rng.integers(0, 4))] += int(cov[j]) // 2 + int(rng.integers(0, 3))
                t[j, INS + 4 * s + int(rng.integers(0, 4))] += int(rng.integers(0, 2))
    return bytes(draft), t.astype(np.uint32)


def call_cases(seed=5):
    """[(note, draft, tallies uint32 [n + 1, ROW], expected new draft or None)]:
    the hand-made rule cases (expected given), then seeded ones of the sizes the
    workgroup's tiles cut (expected None: the checker says)."""
    out = []

    def flat(draft, depth, eq=None, dl=None):
        n = len(draft)
        cov = np.full(n, depth, np.int64)
        return tallies_of(cov, cov if eq is None else np.asarray(eq), np.zeros(n, np.int64) if dl is None else np.asarray(dl))

    # ties: column 1 keeps the draft's G (G 2 : A 2), column 2 falls to C (T 1 : C 2 : G 2)
    t = flat(b"AGTA", 4, eq=[4, 2, 1, 4])
    t[1, SUB + 0] = 2
    t[2, SUB + 1], t[2, SUB + 2] = 2, 2
    out.append(("ties", b"AGTA", t, b"AGCA"))
    # 2 del = cov keeps the column, 2 del > cov drops it
    t = flat(b"ACGT", 4, eq=[4, 2, 1, 4], dl=[0, 2, 3, 0])
    out.append(("del at half", b"ACGT", t, b"ACT"))
    # 2 ins = gcov emits nothing, one more vote emits; starts at the column lower its gcov
    t = flat(b"ACGT", 4)
    t[1, INS + 2] = 2
    t[2, INS + 3] = 3
    out.append(("ins at half", b"ACGT", t, b"ACTGT"))
    t = tallies_of(np.array([4, 4, 6, 6]), np.array([4, 4, 6, 6]), np.zeros(4, np.int64))
    t[2, INS + 1] = 3  # gcov = 6 - 2 = 4: 6 > 4 emits although 2 x 3 = cov
    out.append(("ins against gcov", b"ACGT", t, b"ACCGT"))
    # the chain stops at slot 1 although slot 2 would pass; slots in front of column lo are not emitted
    t = flat(b"ACGT", 4)
    t[2, INS + 0], t[2, INS + 4 + 1], t[2, INS + 8 + 2] = 3, 2, 4
    t[0, INS + 0] = 4
    out.append(("slot chain", b"ACGT", t, b"ACAGT"))
    # the smallest code wins a slot's tie; 8 slots
    t = flat(b"AC", 2)
    for s in range(SLOTS):
        t[1, INS + 4 * s + 3], t[1, INS + 4 * s + (s % 3)] = 1, 1
    out.append(("eight slots", b"AC", t, b"A" + b"ACGACGAC" + b"C"))
    # trim at both ends: coverage 1 1 4 4 4 2 1 -> columns 2 .. 5; the unvoted lower-case column stays as it is
    cov = np.array([1, 1, 4, 4, 4, 2, 1])
    eq = cov.copy()
    eq[3] = 0
    out.append(("trim, no vote", b"ACGnTAC", tallies_of(cov, eq, np.zeros(7, np.int64)), b"GnTA"))
    out.append(("no trim", b"ACGTAC", flat(b"ACGTAC", 3), b"ACGTAC"))
    out.append(("maxcov 0", b"ACGT", np.zeros((5, ROW), np.int64), None))
    t = flat(b"a", 2)
    out.append(("n 1", b"a", t, b"A"))
    out = [(note, d, np.asarray(t, np.int64).astype(np.uint32), want) for note, d, t, want in out]
    rng = np.random.default_rng(seed)
    for n in (1, 1024, 1025, 2049):
        d, t = random_call_case(rng, n)
        out.append(("random n %d" % n, d, t, None))
    d, t = random_call_case(rng, 1500, trim=False, p_drop=0.3, p_ins=0.2, long_ins=True)
    out.append(("offsets move", d, t, None))
    return out
