"""Independent checker of linkage_qc (include/mpc_linkage.h) and the record
batches both test files run: allele codes by a per-base Python loop over the
tokens of cov_util (the grammar is coverage_qc's), pair counts as a numpy
one-hot product (carried out in float64, exact for these counts, read as int64).  Shares no code with linkage.cpp or mpc_link.hip."""
import re

import numpy as np

import cov_util as cu

MAX_SITES = 128
_SUB = {ord("a"): 2, ord("c"): 3, ord("g"): 4, ord("t"): 5}


def base(p):
    return 2 * p + 1


def gap(p):
    return 2 * p


def codes_of(cs, tstart, L, keys):
    """(status code, [allele code per key]) of one record at its target's site keys."""
    code, end, _ = cu.walk(cs, tstart, L)
    if code != cu.OK:
        return code, None
    at, ins, p = {}, set(), tstart
    for op, arg in cu.tokens(cs):
        if op == b":":
            for i in range(int(arg)):
                at[p + i] = 1
            p += int(arg)
        elif op == b"*":
            at[p] = _SUB.get(arg[1] | 32, 6)
            p += 1
        elif op == b"-":
            for i in range(len(arg)):
                at[p + i] = 7
            p += len(arg)
        else:
            ins.add(p)
    assert p == end
    out = []
    for k in keys:
        q = k >> 1
        if k & 1:
            out.append(at.get(q, 0))
        else:
            out.append((7 if q in ins else 1) if tstart <= q <= end else 0)
    return cu.OK, out


def pair_of(alleles):
    """u32[K][K][8][8] of an allele matrix: the one-hot product, in int64."""
    a = np.asarray(alleles, np.uint8) & 7
    n, K = a.shape
    assert n < 2 ** 32
    hot = np.zeros((n, K * 8), np.float64)  # (float64: the BLAS product; counts below 2^53 are exact in it)
    if n:
        hot[np.repeat(np.arange(n), K), (np.arange(K) * 8)[None, :].repeat(n, 0).ravel() + a.ravel()] = 1
    prod = (hot.T @ hot).astype(np.int64)
    return prod.reshape(K, 8, K, 8).transpose(0, 2, 1, 3).astype(np.uint32)


def check(records, lengths, site_off, site_key):
    """records: [(sample, tstart, cs bytes)].  (status, alleles u8[N][K], pair):
    status = (code, record) of the smallest offending record, malformed wins."""
    K = len(site_key)
    alleles = np.zeros((len(records), K), np.uint8)
    for r, (s, ts, cs) in enumerate(records):
        a, b = int(site_off[s]), int(site_off[s + 1])
        code, row = codes_of(cs, ts, lengths[s], [int(k) for k in site_key[a:b]])
        if code != cu.OK:
            return (code, r), None, None
        alleles[r, a:b] = row
    return (cu.OK, 0), alleles, pair_of(alleles)


def tables(sites_per_sample):
    """(site_off, site_key) of [[key, ...] per sample]."""
    off = np.concatenate([[0], np.cumsum([len(k) for k in sites_per_sample])]).astype(np.int64)
    return off, np.array([k for ks in sites_per_sample for k in ks], np.int64)


def run(pkg, records, lengths, site_off, site_key, device="cpu"):
    cs, off, ts, rs = cu.pack(records)
    return pkg.linkage.run(cs, off, ts, rs, lengths, site_off, site_key, device=device)


def status_of(pkg, records, lengths, device="cpu"):
    """(code, record) as linkage.run reports it, at one gap site; (0, 0) when the batch is fine."""
    cs, off, ts, rs = cu.pack(records)
    site_off, site_key = tables([[gap(0)]] + [[] for _ in lengths[1:]])
    try:
        pkg.linkage.run(cs, off, ts, rs, lengths, site_off, site_key, device=device)
    except pkg.linkage.LinkageError as e:
        m = re.match(r"record (\d+): (malformed cs|out of range)", str(e))
        assert m, str(e)
        return (cu.MALFORMED if m.group(2) == "malformed cs" else cu.RANGE), int(m.group(1))
    return cu.OK, 0


# ---------------------------------------------------------------- batches

_TWO = (b":0", b":1", b"+a", b"-c")
_THREE = (b":00", b":02", b"*ag", b"+ac", b"-ct")
BOUNDARY_L = 9000


def pad(rng, n):
    """A valid cs of exactly n bytes (n = 0 or n >= 2) from two- and three-byte tokens."""
    assert n == 0 or n >= 2
    out = []
    while n:
        k = 3 if n == 3 or (n > 4 and rng.random() < 0.4) else 2
        out.append((_TWO if k == 2 else _THREE)[int(rng.integers(0, 4 if k == 2 else 5))])
        n -= k
    return b"".join(out)


def boundary_cases(T):
    """[(what, (tstart, cs), keys)]: the token shapes that straddle byte 64 and
    byte T, each with sites at the straddling token's position (both kinds), at
    the first, an inner and the last base it covers, and one base before and
    after.  Every case is meant for a target of its own (BOUNDARY_L bases)."""
    rng = np.random.default_rng(43)
    out = []
    for b in (64, T):
        tail = pad(rng, 9)
        for what, back, token in (
                ("sub split 1+2", 1, b"*ag"), ("sub split 2+1", 2, b"*ct"), ("sub ends the chunk", 3, b"*ac"),
                ("number last before", 1, b":7"), ("deletion operator last before", 1, b"-g"),
                ("insertion operator last before", 1, b"+g"), ("deletion crosses", 3, b"-acgtac"),
                ("insertion crosses", 3, b"+acgtac"), ("deletion starts at", 0, b"-acg"),
                ("deletion covers two tiles", 3, b"-" + cu.letters(rng, 2 * T + 10))):
            for suffix in (b"", tail, b":5"):
                head = pad(rng, b - back)
                ts = int(rng.integers(1, 3000))
                p = cu.walk(head, ts, BOUNDARY_L)[1]
                n = cu.walk(token, 0, BOUNDARY_L)[1]
                ps = sorted({p - 1, p, p + n // 2, p + max(n, 1) - 1, p + max(n, 1)})
                keys = sorted(k for q in ps for k in (base(q), gap(q)))
                out.append(("%s %d + %r" % (what, b, suffix[:4]), (ts, head + token + suffix), keys))
    return out


def boundary_calls(T):
    """The boundary cases cut into calls of at most MAX_SITES sites:
    [(names, records, lengths, site_off, site_key)], one target per record."""
    calls, cur = [], []
    for case in boundary_cases(T) + [None]:
        if case is None or sum(len(c[2]) for c in cur) + len(case[2]) > MAX_SITES:
            records = [(k, ts, cs) for k, (_, (ts, cs), _) in enumerate(cur)]
            calls.append(([c[0] for c in cur], records, [BOUNDARY_L] * len(cur)) + tables([c[2] for c in cur]))
            cur = []
        if case is not None:
            cur.append(case)
    return calls


def wrong_records(names, site_off, got, want):
    """Names of the records (one target each) whose own sites differ."""
    return [(names[k], got[k, site_off[k]:site_off[k + 1]].tolist(), want[k, site_off[k]:site_off[k + 1]].tolist())
            for k in range(len(names)) if not np.array_equal(got[k], want[k])]


def ends_batch():
    """(names, records, lengths, site_off, site_key, expected rows): the ends of
    a record and of a target, one target per record."""
    L = 20
    cases = [  # (what, target length, (tstart, cs), {site key: expected code})
        ("record ends", L, (5, b":10"), {base(4): 0, base(5): 1, base(14): 1, base(15): 0, gap(4): 0, gap(5): 1, gap(14): 1, gap(15): 1}),
        ("target ends", L, (0, b":20"), {base(0): 1, base(19): 1, gap(0): 1, gap(20): 1}),
        ("insertion at L", L, (18, b":2+ac"), {base(19): 1, gap(20): 7}),
        ("one base sub", 1, (0, b"*ag"), {base(0): 4, gap(0): 1, gap(1): 1}),
        ("one base deleted", 1, (0, b"-a"), {base(0): 7, gap(0): 1, gap(1): 1}),
        ("one base both gaps", 1, (0, b"+t:1+c"), {base(0): 1, gap(0): 7, gap(1): 7}),
        ("one base not reached", 1, (1, b""), {base(0): 0, gap(0): 0, gap(1): 1}),
        ("two insertions at one p", L, (3, b":2+a+c:2"), {base(4): 1, gap(5): 7, base(5): 1, gap(6): 1}),
        ("sub to N", L, (2, b"*aN"), {base(2): 6}),
        ("sub upper case", L, (2, b"*aG"), {base(2): 4}),
        ("sub to n", L, (2, b"*an"), {base(2): 6}),
        ("sub to t then c", L, (2, b"*at*gc"), {base(2): 5, base(3): 3}),
        ("zero run", L, (4, b":0"), {base(3): 0, gap(4): 1, base(4): 0, gap(5): 0}),
        ("empty cs", L, (7, b""), {gap(6): 0, base(6): 0, gap(7): 1, base(7): 0, gap(8): 0}),
        ("Z prefix", L, (0, b"Z::3-ac*ta"), {gap(0): 1, base(2): 1, base(3): 7, base(4): 7, base(5): 2, gap(6): 1, base(6): 0}),
    ]
    records = [(k, ts, cs) for k, (_, _, (ts, cs), _) in enumerate(cases)]
    off, key = tables([sorted(c[3]) for c in cases])
    want = np.zeros((len(cases), len(key)), np.uint8)
    for k, c in enumerate(cases):
        want[k, off[k]:off[k + 1]] = [c[3][q] for q in sorted(c[3])]
    return [c[0] for c in cases], records, [c[1] for c in cases], off, key, want


def samples_batch():
    """Three samples, the middle one without sites, records interleaved."""
    rng = np.random.default_rng(47)
    lengths = [120, 90, 200]
    records = []
    for _ in range(300):
        s = int(rng.integers(0, 3))
        a = int(rng.integers(0, lengths[s] // 2))
        records.append((s, a, cu.random_cs(rng, int(rng.integers(1, lengths[s] - a + 1)), 0.08, 0.08, 0.08)))
    off, key = tables([[gap(0), base(10), gap(30), base(30), base(61), base(119), gap(120)], [],
                       [base(0), base(50), gap(51), base(100), base(199)]])
    return records, lengths, off, key


def one_token_batch():
    """70,000 one-token records on one 40-base target, six sites: more records than the grid has waves."""
    rng = np.random.default_rng(53)
    toks = (b":1", b"*ag", b"-a", b"+c", b":3", b"*ct")
    records = [(0, int(rng.integers(0, 37)), toks[int(rng.integers(0, 6))]) for _ in range(70000)]
    off, key = tables([[base(3), gap(4), base(17), gap(18), base(18), base(30)]])
    return records, [40], off, key


# ---------------------------------------------------------------- the planted sub-population

PLANTED_KEYS = [base(50), base(80), base(120), base(160), gap(200)]
PLANTED_CARRIER_PAIRS = [(0, 2), (0, 4), (2, 4)]


def planted(carriers=True, n=2000, L=300, seed=41):
    """[(0, 0, cs)] of n full-length records on one L-base target: 200 carrier
    records hold *ag at 50, a 1-base deletion at 120 and an insertion before
    200; every record has independent 3 % substitutions at 80 and at 160."""
    rng = np.random.default_rng(seed)
    carrier = np.zeros(n, bool)
    carrier[rng.permutation(n)[:200]] = carriers
    sub80, sub160 = rng.random(n) < 0.03, rng.random(n) < 0.03
    records = []
    for r in range(n):
        ev = []
        if carrier[r]:
            ev += [(50, b"*ag", 1), (120, b"-c", 1), (200, b"+tt", 0)]
        if sub80[r]:
            ev.append((80, b"*ct", 1))
        if sub160[r]:
            ev.append((160, b"*ga", 1))
        cs, p = [], 0
        for q, tok, adv in sorted(ev):
            if q > p:
                cs.append(b":%d" % (q - p))
            cs.append(tok)
            p = q + adv
        cs.append(b":%d" % (L - p))
        records.append((0, 0, b"".join(cs)))
    return records, carrier, sub80, sub160


def r2_numpy(x, y):
    """r^2 of two boolean vectors, as the definition writes it (exact integers, one division)."""
    n, a, b, c = len(x), int(x.sum()), int(y.sum()), int((x & y).sum())
    den = a * (n - a) * b * (n - b)
    return (n * c - a * b) ** 2 / den if den else 0.0


def write_paf(path, records, names, lengths):
    """The records as PAF lines (12 columns + cs:Z:), one read name each."""
    lines = []
    for r, (s, ts, cs) in enumerate(records):
        code, end, res = cu.walk(cs, ts, lengths[s])
        assert code == cu.OK
        c = res[1]
        qlen = c["match"] + c["mism"] + c["insb"]
        lines.append("read%d\t%d\t0\t%d\t+\t%s\t%d\t%d\t%d\t%d\t%d\t60\tcs:Z:%s" % (
            r, qlen, qlen, names[s], lengths[s], ts, end, c["match"], c["match"] + c["mism"] + c["insb"] + c["delb"],
            bytes(cs).decode()))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def synth_sites(pkg, device="cpu"):
    """cov_util.synth_batch with the sites select_sites gives at a 13 % minor
    fraction (112 sites, all on the two indel-profile samples): (cs, off, ts, rs, lengths, site_off, site_key)."""
    records, lengths, regions, _ = cu.synth_batch(pkg)
    cs, off, ts, rs = cu.pack(records)
    cov = pkg.coverage.run(cs, off, ts, rs, lengths, regions, 0, device=device)
    site_off, site_key, dropped = pkg.linkage.select_sites(cov["rows"], cov["pos_off"], regions, 0.13, 10)
    return cs, off, ts, rs, lengths, site_off, site_key, dropped


DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mpc_linkage.h"

// argv[1]: file of lines "tstart<TAB>cs"; one 300-base target, the five planted sites
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 3;
  std::vector<uint8_t> cs;
  std::vector<int64_t> off(1, 0), ts;
  std::vector<int32_t> smp;
  static char line[1 << 16];
  while (fgets(line, sizeof(line), f)) {
    char* tab = strchr(line, '\t');
    if (!tab) return 4;
    size_t n = strlen(tab + 1);
    while (n && (tab[n] == '\n' || tab[n] == '\r')) --n;
    ts.push_back(atoll(line));
    cs.insert(cs.end(), tab + 1, tab + 1 + n);
    off.push_back((int64_t)cs.size());
    smp.push_back(0);
  }
  fclose(f);
  const int64_t N = (int64_t)ts.size(), pos_off[2] = {0, 301}, site_off[2] = {0, 5}, keys[5] = {101, 161, 241, 321, 400};
  std::vector<uint8_t> alleles((size_t)N * 5);
  std::vector<uint32_t> pair(5 * 5 * 64);
  int32_t status[2];
  for (int threads = 1; threads <= 4; threads += 3) {
    if (mpc_linkage_host(cs.data(), off.data(), ts.data(), smp.data(), N, pos_off, 1, site_off, keys, 5, alleles.data(),
                         pair.data(), status, threads) != 0) {
      printf("host: %s\n", mpc_linkage_last_error());
      return 5;
    }
    printf("threads %d records %lld status %d %d joint %u %u %u diag", threads, (long long)N, status[0], status[1],
           pair[(0 * 5 + 2) * 64 + 4 * 8 + 7], pair[(0 * 5 + 4) * 64 + 4 * 8 + 7], pair[(4 * 5 + 2) * 64 + 7 * 8 + 7]);
    for (int k = 0; k < 5; ++k) printf(" %u", pair[(k * 5 + k) * 64 + 9]);
    printf("\n");
  }
  const char* bad[] = {":3*ag-c+tt:2", ":4=A", ":400", "", ":1234567890", "*a", ":5-"};
  for (const char* c : bad) {
    const int64_t o[2] = {0, (int64_t)strlen(c)}, t0 = 1;
    const int32_t s0 = 0;
    uint8_t row[5];
    mpc_linkage_host((const uint8_t*)c, o, &t0, &s0, 1, pos_off, 1, site_off, keys, 5, row, pair.data(), status, 1);
    printf("cs %s status %d\n", c, status[0]);
  }
  const int64_t bad_keys[5] = {101, 101, 241, 321, 400};
  const int rc = mpc_linkage_host(cs.data(), off.data(), ts.data(), smp.data(), N, pos_off, 1, site_off, bad_keys, 5,
                                  alleles.data(), pair.data(), status, 1);
  printf("bad keys %d %s\n", rc, mpc_linkage_last_error());
  if (mpc_linkage_pairs_host(alleles.data(), N, 5, pair.data(), 3) != 0) return 6;
  printf("pairs %u\n", pair[(0 * 5 + 2) * 64 + 4 * 8 + 7]);
  return 0;
}
"""


# ---------------------------------------------------------------- the cases, for either device

def case_boundaries(pkg, device):
    T = pkg.linkage.tile_bytes()
    assert T % 64 == 0 and T >= 128
    calls = boundary_calls(T)
    assert len(calls) > 1 and all(1 <= len(c[4]) <= MAX_SITES for c in calls)
    for names, records, lengths, off, key in calls:
        status, alleles, pair = check(records, lengths, off, key)
        assert status == (cu.OK, 0)
        got_a, got_p = run(pkg, records, lengths, off, key, device)
        assert not wrong_records(names, off, got_a, alleles)
        assert np.array_equal(got_a, alleles) and np.array_equal(got_p, pair)
        assert (alleles >= 2).any() and (alleles == 7).any() and (alleles == 0).any()


def case_ends(pkg, device):
    names, records, lengths, off, key, want = ends_batch()
    status, alleles, pair = check(records, lengths, off, key)
    assert status == (cu.OK, 0) and not wrong_records(names, off, alleles, want)
    got_a, got_p = run(pkg, records, lengths, off, key, device)
    assert not wrong_records(names, off, got_a, want)
    assert np.array_equal(got_a, want) and np.array_equal(got_p, pair)


PAIR_SHAPES = [(n, k) for n in (1, 63, 64, 65, 4160) for k in (1, 2, 128)]


def case_pairs_shape(pkg, device, n, k):
    rng = np.random.default_rng(59 + n + k)
    alleles = rng.integers(0, 8, (n, k)).astype(np.uint8)
    alleles[::3] |= 8 * rng.integers(0, 32, (len(alleles[::3]), k)).astype(np.uint8)  # (codes are taken & 7)
    got = pkg.linkage.pairs(alleles, device=device)
    assert got.shape == (k, k, 8, 8) and got.dtype == np.uint32
    assert np.array_equal(got, pair_of(alleles))


def case_pairs_one_code(pkg, device):
    """70,000 records with one code: a cell past 16 bits, a partial last word."""
    alleles = np.full((70000, 2), 5, np.uint8)
    got = pkg.linkage.pairs(alleles, device=device)
    want = np.zeros((2, 2, 8, 8), np.uint32)
    want[:, :, 5, 5] = 70000
    assert np.array_equal(got, want)
    assert np.array_equal(got, pair_of(alleles))


def case_pairs_limits(pkg, device):
    with __import__("pytest").raises(pkg.linkage.LinkageError):
        pkg.linkage.pairs(np.ones((4, 129), np.uint8), device=device)
    assert not pkg.linkage.pairs(np.zeros((0, 3), np.uint8), device=device).any()
    site_off, site_key = tables([[base(0), gap(1)]])
    a, p = pkg.linkage.run(np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32), [5],
                           site_off, site_key, device=device)
    assert a.shape == (0, 2) and p.shape == (2, 2, 8, 8) and not p.any()


def case_samples(pkg, device):
    records, lengths, off, key = samples_batch()
    status, alleles, pair = check(records, lengths, off, key)
    assert status == (cu.OK, 0)
    got_a, got_p = run(pkg, records, lengths, off, key, device)
    assert np.array_equal(got_a, alleles) and np.array_equal(got_p, pair)
    smp = np.array([s for s, _, _ in records])
    owner = np.repeat(np.arange(3), np.diff(off))
    assert not got_a[smp[:, None] != owner[None, :]].any() and got_a[smp[:, None] == owner[None, :]].any()
    for i in np.nonzero(owner == 0)[0]:
        for j in np.nonzero(owner == 2)[0]:  # cross-sample cells: only row or column 0
            assert not got_p[i, j, 1:, 1:].any() and got_p[i, j].sum() == len(records)


def case_one_token(pkg, device):
    records, lengths, off, key = one_token_batch()
    status, alleles, pair = check(records, lengths, off, key)
    assert status == (cu.OK, 0)
    first = run(pkg, records, lengths, off, key, device)
    assert np.array_equal(first[0], alleles) and np.array_equal(first[1], pair)
    again = run(pkg, records, lengths, off, key, device)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()


def case_status_parity(pkg, device, rec, code):
    batch = cu.GOOD + [rec] + cu.GOOD
    assert status_of(pkg, batch, [20], device) == cu.status_of(pkg, batch, [20], device) == (code, 3)


def case_status_far_apart(pkg, device):
    T = pkg.linkage.tile_bytes()
    rng = np.random.default_rng(31)
    batch = [cu.GOOD[k % 3] for k in range(9000)]
    batch[8900] = (0, 0, b"=A")
    batch[100] = (0, 10, b":11")
    assert status_of(pkg, batch, [20], device) == cu.status_of(pkg, batch, [20], device) == (cu.RANGE, 100)
    batch[100], batch[8900] = batch[8900], batch[100]
    assert status_of(pkg, batch, [20], device) == cu.status_of(pkg, batch, [20], device) == (cu.MALFORMED, 100)
    batch[100] = cu.GOOD[0]
    batch[50] = (0, 0, b":30" + pad(rng, 2 * T) + b"~")
    assert status_of(pkg, batch, [20], device) == cu.status_of(pkg, batch, [20], device) == (cu.MALFORMED, 50)


def run_abi(pkg, packed, pos_off, site_off, site_key, device):
    """mpc_linkage_host / mpc_linkage_run on arrays as they are (linkage.run
    refuses a sample index outside the targets before either): (status, alleles, pair)."""
    cs, off, ts, rs = packed
    n, S, K = len(ts), len(pos_off) - 1, len(site_key)
    cs = np.concatenate([cs, np.zeros(8, np.uint8)])
    if device == "cpu":
        L = pkg.linkage.host_lib()
        alleles, pair, status = np.full((n, K), 9, np.uint8), np.zeros((K, K, 8, 8), np.uint32), np.zeros(2, np.int32)
        rc = L.mpc_linkage_host(cs.ctypes.data, off.ctypes.data, ts.ctypes.data, rs.ctypes.data, n, pos_off.ctypes.data, S,
                                site_off.ctypes.data, site_key.ctypes.data, K, alleles.ctypes.data, pair.ctypes.data,
                                status.ctypes.data, 3)
        assert rc == 0, L.mpc_linkage_last_error()
        return tuple(status.tolist()), alleles, pair
    import torch
    L = pkg.engine.lib()
    dev = "cuda:%d" % device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_cs, d_off, d_ts, d_rs, d_pos, d_so, d_sk = (up(a) for a in (cs, off, ts, rs, pos_off, site_off, site_key))
    d_alleles = torch.full((n, K), 9, dtype=torch.uint8, device=dev)
    d_pair = torch.empty((K, K, 8, 8), dtype=torch.int32, device=dev)
    d_scratch = torch.empty(L.mpc_linkage_scratch_bytes(n, K) // 8, dtype=torch.int64, device=dev)
    d_status = torch.empty(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = L.mpc_linkage_run(d_cs.data_ptr(), d_off.data_ptr(), d_ts.data_ptr(), d_rs.data_ptr(), n, d_pos.data_ptr(), S,
                               d_so.data_ptr(), d_sk.data_ptr(), K, d_alleles.data_ptr(), d_pair.data_ptr(),
                               d_scratch.data_ptr(), d_status.data_ptr(), None)
        assert rc == 0, L.mpc_last_error()
        torch.cuda.synchronize()
    return tuple(d_status.cpu().tolist()), d_alleles.cpu().numpy(), d_pair.cpu().numpy().view(np.uint32)


def case_bad_sample(pkg, device):
    """cov_util.bad_sample_batch: the smaller record with a sample index outside
    the targets is named, out of range; both have an all-zero allele row and
    every other record its codes."""
    records, lengths, bad = cu.bad_sample_batch()
    off, key = tables([[base(3), gap(4), base(17), gap(40)], [gap(0), base(5), gap(18), base(30), base(39)]])
    good = [k for k in range(len(records)) if k not in bad]
    status, want, _ = check([records[k] for k in good], lengths, off, key)
    assert status == (cu.OK, 0) and (want >= 2).any() and (want == 1).any() and (want == 0).any()
    alleles = np.zeros((len(records), len(key)), np.uint8)
    alleles[good] = want
    packed = cu.pack(records)
    packed[3][bad[0]], packed[3][bad[1]] = -7, len(lengths)
    pos_off = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64) + 1)]).astype(np.int64)
    got = run_abi(pkg, packed, pos_off, off, key, device)
    assert got[0] == (cu.RANGE, bad[0])
    assert np.array_equal(got[1], alleles) and np.array_equal(got[2], pair_of(alleles))


# (site_off, site_key, n_sites, word of the message) on two targets of 10 and 6 bases
BAD_TABLES = [
    ([0, 2, 3], [5, 5, 4], 3, b"increasing"), ([0, 2, 3], [7, 5, 4], 3, b"increasing"),
    ([0, 2, 3], [5, 22, 4], 3, b"outside"), ([0, 2, 3], [5, 7, 13], 3, b"outside"), ([0, 2, 3], [5, 21, 4], 3, b"outside"),
    ([0, 2, 1], [5, 7, 4], 3, b"site_off"), ([0, 4, 3], [5, 7, 9], 3, b"site_off"), ([0, 0, 0], [5, 7, 4], 0, b"n_sites"),
    ([0, 2, 3], [-1, 7, 4], 3, b"outside"),
]
GOOD_TABLE = ([0, 2, 3], [5, 20, 12], 3)


def planted_stats(pkg, device, carriers=True):
    """The planted batch through linkage.run: (alleles, {(i, j): pair_stats at r2 0.5 / joint 10})."""
    records, carrier, sub80, sub160 = planted(carriers)
    off, key = tables([PLANTED_KEYS])
    alleles, pair = run(pkg, records, [300], off, key, device)
    return alleles, {(i, j): pkg.linkage.pair_stats(pair, i, j, 0.5, 10) for i in range(5) for j in range(i + 1, 5)}


def case_planted(pkg, device):
    records, carrier, sub80, sub160 = planted()
    vec = [carrier, sub80, carrier, sub160, carrier]
    alleles, stats = planted_stats(pkg, device)
    status, want, _ = check(records, [300], *tables([PLANTED_KEYS]))
    assert status == (cu.OK, 0) and np.array_equal(alleles, want)
    for (i, j), st in stats.items():
        assert (st["n"], st["x"], st["y"], st["n11"]) == (2000, int(vec[i].sum()), int(vec[j].sum()), int((vec[i] & vec[j]).sum()))
        assert st["r2"] == r2_numpy(vec[i], vec[j])
        if (i, j) in PLANTED_CARRIER_PAIRS:
            assert st["r2"] == 1.0 and st["n11"] == 200 and st["linked"]
        else:
            assert st["r2"] <= 0.00103 and not st["linked"]
    _, none = planted_stats(pkg, device, carriers=False)
    assert not any(st["linked"] for st in none.values())
    # the five sites are what the pileup's minor counts select
    cs, off, ts, rs = cu.pack(records)
    cov = pkg.coverage.run(cs, off, ts, rs, [300], None, 0, device=device)
    site_off, site_key, dropped = pkg.linkage.select_sites(cov["rows"], cov["pos_off"], [(0, 300)], 0.02, 10)
    assert site_off.tolist() == [0, 5] and site_key.tolist() == PLANTED_KEYS and dropped == 0


def case_planted_cli(pkg, device, tmp_path, cli):
    import subprocess
    import sys
    outs = {}
    for what, carriers in (("mixed", True), ("clean", False)):
        paf = tmp_path / (what + ".paf")
        write_paf(str(paf), planted(carriers)[0], ["plasmid"], [300])
        rep, prs, hap = (tmp_path / ("%s_%s.tsv" % (what, k)) for k in ("report", "pairs", "hap"))
        p = subprocess.run([sys.executable, cli, "--paf", str(paf), "--report", str(rep), "--pairs", str(prs), "--haplotypes",
                            str(hap), "--min-minor-fraction", "0.02", "--min-minor-count", "10", "--min-r2", "0.5", "--min-joint",
                            "10", "--strict", "--device", str(device)], capture_output=True, text=True, timeout=300)
        outs[what] = (p.returncode, rep.read_text().splitlines(), prs.read_text().splitlines(), hap.read_text().splitlines())
        assert p.returncode in (0, 2), p.stderr[-2000:]
    code, rep, prs, hap = outs["mixed"]
    assert code == 2 and rep[-1] == "verdict\tFAIL" and "sites\t5" in rep and "linked_pairs\t3" in rep
    assert "site_list\t51:base,81:base,121:base,161:base,201:gap" in rep
    linked = [tuple(line.split("\t")[2:4]) for line in prs[1:] if line.endswith("\tyes")]
    assert linked == [("51:base", "121:base"), ("51:base", "201:gap"), ("121:base", "201:gap")] and len(prs) == 11
    assert [h.split("\t")[2] for h in hap[1:3]] == [".....", "G.-.+"]
    code, rep, prs, hap = outs["clean"]
    assert code == 0 and rep[-1] == "verdict\tPASS" and "sites\t2" in rep
    return outs


def case_sanitized_driver(pkg, tmp_path):
    """ASan + UBSan on the host code, as a stand-alone program; no recovery: any report, a leak included, fails the run."""
    import native_util as nu
    drv, data = tmp_path / "lnk_driver.cpp", tmp_path / "planted.txt"
    drv.write_text(DRIVER)
    exe = nu.build("lnk_asan", ["linkage.cpp", drv], ["-pthread"])
    records, carrier, sub80, sub160 = planted()
    data.write_bytes(b"".join(b"%d\t%s\n" % (ts, cs) for _, ts, cs in records))
    out = nu.run(exe, [data]).splitlines()
    diag = [2000 - int(v.sum()) for v in (carrier, sub80, carrier, sub160, carrier)]
    want = "records 2000 status 0 0 joint 200 200 200 diag " + " ".join(map(str, diag))
    assert out[:2] == ["threads 1 " + want, "threads 4 " + want]
    assert out[2:9] == ["cs :3*ag-c+tt:2 status 0", "cs :4=A status 1", "cs :400 status 2", "cs  status 0",
                        "cs :1234567890 status 1", "cs *a status 1", "cs :5- status 1"]
    assert out[9].startswith("bad keys -1 ") and "increasing" in out[9] and out[10] == "pairs 200"
