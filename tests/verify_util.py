"""The checker of verify_consensus: the definition of include/mpc_verify.h as a
numpy full-matrix Sellers DP with the canonical traceback, plus seeded pair
generators and the ctypes plumbing the verify tests share.

A row of D from the row above: x[j] = min(D[i-1][j-1] + cost, D[i-1][j] + 1),
x[0] = i, then the left moves D[i][j] = min_k<=j x[k] + (j - k) as
minimum.accumulate(x - arange) + arange."""
import ctypes
import importlib

import numpy as np

MAX_EDITS = 1024
MAX_QUERY = 65536


def codes(seq, other):
    """A C G T -> 0..3 after upper-casing, every other byte -> ``other``."""
    lut = np.full(256, other, np.uint8)
    for k, c in enumerate(b"ACGT"):
        lut[c] = lut[c + 32] = k
    return lut[np.frombuffer(bytes(seq), np.uint8)]


def matrix(q, t):
    """The full D, int32 [m + 1, n + 1]."""
    qc, tc = codes(q, 4), codes(t, 5)
    m, n = len(qc), len(tc)
    ar = np.arange(n + 1, dtype=np.int32)
    D = np.zeros((m + 1, n + 1), np.int32)
    x = np.empty(n + 1, np.int32)
    for i in range(1, m + 1):
        p = D[i - 1]
        x[0] = i
        np.minimum(p[:-1] + (tc != qc[i - 1]), p[1:] + 1, out=x[1:])
        D[i] = np.minimum.accumulate(x - ar) + ar
    return D


def last_row(q, t):
    """D[m] without keeping the matrix (long queries)."""
    qc, tc = codes(q, 4), codes(t, 5)
    n = len(tc)
    ar = np.arange(n + 1, dtype=np.int32)
    p = np.zeros(n + 1, np.int32)
    x = np.empty(n + 1, np.int32)
    for i in range(1, len(qc) + 1):
        x[0] = i
        np.minimum(p[:-1] + (tc != qc[i - 1]), p[1:] + 1, out=x[1:])
        p = np.minimum.accumulate(x - ar) + ar
    return p


def score(q, t):
    """(distance, end): the minimum of the last row and the SMALLEST column attaining it."""
    row = last_row(q, t)
    return int(row.min()), int(row.argmin())


def traceback(q, t, D=None):
    """dict(distance, end, start, ops) with the canonical script (ops from start to end)."""
    D = matrix(q, t) if D is None else D
    qc, tc = codes(q, 4), codes(t, 5)
    m = len(qc)
    end = int(D[m].argmin())
    i, j, ops = m, end, []
    while i > 0:
        cost = int(qc[i - 1] != tc[j - 1]) if j > 0 else 1
        if j > 0 and D[i - 1, j - 1] + cost == D[i, j]:
            ops.append("X" if cost else "=")
            i, j = i - 1, j - 1
        elif D[i - 1, j] + 1 == D[i, j]:
            ops.append("D")
            i -= 1
        else:
            ops.append("I")
            j -= 1
    return dict(distance=int(D[m, end]), end=end, start=j, ops="".join(reversed(ops)))


def cigar(ops):
    out, k = [], 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out.append("%d%s" % (e - k, ops[k]))
        k = e
    return "".join(out)


def op_counts(ops):
    return [ops.count(c) for c in "=XID"]


def expected_row(q, t):
    """What the report says about one pair: (start, end, distance, X, I, D, cigar)."""
    distance, end = score(q, t)
    if distance > MAX_EDITS:
        return (-1, end, distance, -1, -1, -1, "*")
    tb = traceback(q, t)
    c = op_counts(tb["ops"])
    return (tb["start"], tb["end"], tb["distance"], c[1], c[2], c[3], cigar(tb["ops"]))


def edit_lines(name, region, q, t, q_base):
    """The --edits lines of one pair from the checker's script; q_base = 0-based
    position of q[0] in the adapted sequence."""
    tb = traceback(q, t)
    i, j, out = 0, tb["start"], []
    for op in tb["ops"]:
        if op in "=X":
            if op == "X":
                out.append((q_base + i + 1, j + 1, op, chr(q[i]), chr(t[j])))
            i, j = i + 1, j + 1
        elif op == "D":
            out.append((q_base + i + 1, j, op, chr(q[i]), "-"))
            i += 1
        else:
            out.append((q_base + i, j + 1, op, "-", chr(t[j])))
            j += 1
    return ["%s\t%s\t%d\t%d\t%s\t%s\t%s\n" % ((name, region) + e) for e in out]


# ---- seeded inputs -----------------------------------------------------------

def rand_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n))


def mutate(rng, s, rate=0.05):
    """A copy of s with about ``rate`` each of substitutions, insertions, deletions."""
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate:
            out.append(b"ACGT"[(b"ACGT".index(c) + int(rng.integers(1, 4))) % 4] if c in b"ACGT" else 65)
        elif r < 2 * rate:
            out.append(c)
            out.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
        elif r < 3 * rate:
            continue
        else:
            out.append(c)
    return bytes(out)


def sprinkle(rng, s, k=3):
    """Lower-case a stretch and plant k non-ACGT bytes."""
    b = bytearray(s)
    if not b:
        return bytes(b)
    a = int(rng.integers(0, len(b)))
    b[a: a + 7] = bytes(b[a: a + 7]).lower()
    for _ in range(k):
        b[int(rng.integers(0, len(b)))] = int(rng.choice(np.frombuffer(b"NnRy-*", np.uint8)))
    return bytes(b)


def fit(rng, s, n):
    """s cut or padded with random bases to exactly n bytes."""
    if len(s) >= n:
        a = int(rng.integers(0, len(s) - n + 1))
        return s[a: a + n]
    pad = n - len(s)
    left = int(rng.integers(0, pad + 1))
    return rand_seq(rng, left) + s + rand_seq(rng, pad - left)


def small_pairs(seed=11):
    """The CPU grid: m x n over mutated copies, unrelated text, non-ACGT / lower case."""
    rng = np.random.default_rng(seed)
    out = []
    for m in (1, 2, 63, 64, 65, 127, 128, 129, 200):
        for n in (0, 1, 3, 64, 70, 260):
            q = rand_seq(rng, m)
            kind = len(out) % 3
            if kind == 0:
                t = fit(rng, mutate(rng, q), n)
            elif kind == 1:
                t = rand_seq(rng, n)
            else:
                q = sprinkle(rng, q)
                t = sprinkle(rng, fit(rng, mutate(rng, q), n))
            out.append((q, t))
    return out


# ---- ctypes ------------------------------------------------------------------

def pkg():
    return importlib.import_module("minion-plasmid-consensus_amd")


def pack(pairs):
    """(seq uint8[], table int64[n, 4]) as the C-ABI takes them."""
    blob, rows, off = [], [], 0
    for q, t in pairs:
        rows.append((off, len(q), off + len(q), len(t)))
        blob += [q, t]
        off += len(q) + len(t)
    seq = np.frombuffer(b"".join(blob) + b"\0" * 8, np.uint8).copy()
    return seq, np.array(rows, np.int64).reshape(-1, 4)


def scan_host(pairs, threads=0):
    L = pkg().verify.host_lib()
    seq, tab = pack(pairs)
    out = np.full((len(pairs), 2), -7, np.int32)
    rc = L.mpc_verify_scan_host(seq.ctypes.data, tab.ctypes.data, len(pairs), out.ctypes.data, threads)
    assert rc == 0, L.mpc_verify_last_error()
    return [tuple(int(v) for v in r) for r in out]


def script(q, t, distance, end):
    """(rc, start, counts, cigar) of mpc_verify_script."""
    L = pkg().verify.host_lib()
    start = ctypes.c_int32(-9)
    counts = (ctypes.c_int32 * 4)(-9, -9, -9, -9)
    buf = ctypes.create_string_buffer(1 << 16)
    rc = L.mpc_verify_script(bytes(q), len(q), bytes(t), len(t), distance, end, ctypes.byref(start), counts, buf, len(buf))
    return rc, start.value, list(counts), buf.value.decode()
