"""Independent checker of coverage_qc (include/mpc_coverage.h): a per-base
Python / numpy loop over the definition, sharing no code with coverage.cpp or
mpc_cov.hip, plus small generators of cs strings and record batches."""
import re

import numpy as np

OK, MALFORMED, RANGE = 0, 1, 2
_TOKEN = re.compile(rb":([0-9]{1,9})|\*([A-Za-z]{2})|\+([A-Za-z]+)|-([A-Za-z]+)")


def tokens(cs):
    """[(op, operand bytes)] of a cs tag, or None when it is outside the grammar."""
    cs = bytes(cs)
    if cs[:2] == b"Z:":
        cs = cs[2:]
    out, k = [], 0
    while k < len(cs):
        m = _TOKEN.match(cs, k)
        if not m:
            return None
        out.append((cs[k:k + 1], cs[k + 1:m.end()]))
        k = m.end()
    return out


def walk(cs, tstart, L):
    """(code, end, events) of one record; events = [(position, column)] one per
    observation: 0 aligned, 1 deleted, 2 mismatch, 3 insertion."""
    tk = tokens(cs)
    if tk is None:
        return MALFORMED, None, None
    p, ev, c = tstart, [], dict(match=0, mism=0, insev=0, insb=0, delev=0, delb=0)
    for op, arg in tk:
        if op == b":":
            n = int(arg)
            if p + n <= L:  # (past the end the record is out of range whatever it holds)
                ev += [(p + i, 0) for i in range(n)]
            p += n
            c["match"] += n
        elif op == b"*":
            ev += [(p, 0), (p, 2)]
            p += 1
            c["mism"] += 1
        elif op == b"-":
            ev += [(p + i, 1) for i in range(len(arg))]
            p += len(arg)
            c["delev"] += 1
            c["delb"] += len(arg)
        else:
            ev.append((p, 3))
            c["insev"] += 1
            c["insb"] += len(arg)
    if tstart < 0 or p > L:
        return RANGE, p, None
    return OK, p, (ev, c)


def check(records, lengths, regions, min_depth=0):
    """records: [(sample, tstart, cs bytes)].  Returns (status, rows, stats,
    ends): status = (code, record) of the smallest offending record (malformed
    wins), rows / stats as mpc_coverage.h defines them, ends per record."""
    pos_off = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64) + 1)])
    rows = np.zeros((int(pos_off[-1]), 4), np.uint32)
    stats = np.zeros((len(lengths), 16), np.uint64)
    ends = []
    for r, (s, ts, cs) in enumerate(records):
        code, end, res = walk(cs, ts, lengths[s])
        if code != OK:
            return (code, r), None, None, None
        ev, c = res
        ends.append(end)
        for p, col in ev:
            rows[pos_off[s] + p, col] += 1
        for k, key in enumerate(("match", "mism", "insev", "insb", "delev", "delb")):
            stats[s, 1 + k] += c[key]
        stats[s, 0] += 1
    for s, (lo, hi) in enumerate(regions):
        d = rows[pos_off[s] + lo:pos_off[s] + hi, 0].astype(object)
        stats[s, 7] = int(sum(d))
        stats[s, 8] = int(sum(x * x for x in d))
        stats[s, 9] = int(min(d)) if len(d) else 0
        stats[s, 10] = int(max(d)) if len(d) else 0
        stats[s, 11] = int(sum(1 for x in d if x < min_depth))
        stats[s, 12] = int(rows[pos_off[s] + lo:pos_off[s] + hi, 1].astype(np.int64).sum())
    return (OK, 0), rows, stats, ends


def pack(records):
    """(cs, cs_off, tstart, rec_sample) arrays of [(sample, tstart, cs bytes)]."""
    blob = b"".join(bytes(c) for _, _, c in records)
    off = np.concatenate([[0], np.cumsum([len(c) for _, _, c in records])]).astype(np.int64)
    return (np.frombuffer(blob + b"\0" * 8, np.uint8)[:len(blob)], off,
            np.array([t for _, t, _ in records], np.int64), np.array([s for s, _, _ in records], np.int32))


def run(pkg, records, lengths, regions, min_depth=0, device="cpu"):
    """pkg.coverage.run on a record list: (rows, stats)."""
    cs, off, ts, rs = pack(records)
    res = pkg.coverage.run(cs, off, ts, rs, lengths, regions, min_depth, device=device)
    return res["rows"], res["stats"]


def status_of(pkg, records, lengths, device="cpu"):
    """(code, record) as the C-ABI reports it; (0, 0) when the batch is fine."""
    cs, off, ts, rs = pack(records)
    try:
        pkg.coverage.run(cs, off, ts, rs, lengths, None, 0, device=device)
    except pkg.coverage.CoverageError as e:
        m = re.match(r"record (\d+): (malformed cs|out of range)", str(e))
        assert m, str(e)
        return (MALFORMED if m.group(2) == "malformed cs" else RANGE), int(m.group(1))
    return OK, 0


def letters(rng, n):
    return bytes(rng.choice(np.frombuffer(b"acgtn", np.uint8), size=n))


def random_cs(rng, ref_span, p_sub=0.02, p_ins=0.02, p_del=0.02):
    """A cs tag whose walk advances exactly ref_span bases."""
    out, left = [], ref_span
    while left > 0:
        x = rng.random()
        if x < p_sub:
            out.append(b"*" + letters(rng, 2))
            left -= 1
        elif x < p_sub + p_del:
            n = min(left, int(rng.integers(1, 4)))
            out.append(b"-" + letters(rng, n))
            left -= n
        elif x < p_sub + p_del + p_ins:
            out.append(b"+" + letters(rng, int(rng.integers(1, 4))))
        else:
            n = min(left, int(rng.integers(1, 60)))
            out.append(b":%d" % n)
            left -= n
    return b"".join(out)


def synth_batch(pkg):
    """The four-sample Synth batch of the issue: n = 600, 300 reads, profiles
    default and indel, both strands; two distinct regions.  Returns (records,
    lengths, regions, samples)."""
    records, lengths, regions, samples = [], [], [], []
    for profile, seed in (("default", 3), ("indel", 4)):
        syn = pkg.synth.Synth(n=600, n_reads=300, profile=profile, seed=seed)
        for k in (0, 1):
            smp = syn.sample(k)
            s = len(lengths)
            lengths.append(600)
            regions.append((0, 600) if k == 0 else (40, 560))
            samples.append(smp)
            cs = smp["cs"].tobytes()
            off = smp["cs_off"]
            records += [(s, int(smp["tstart"][r]), cs[off[r]:off[r + 1]]) for r in range(len(smp["tstart"]))]
    return records, lengths, regions, samples


def bad_sample_batch():
    """(records, lengths, bad): 2 x 16 x 64 + 17 records of 2-6-byte cs strings
    over two 40-base targets -- two full rounds of a 16-wave workgroup's
    64-record batches and a short third; record 1024 (lane 0 of a batch) and the
    last record are to be given a sample index outside the targets."""
    rng = np.random.default_rng(61)
    toks = (b":1", b"*ag", b"-a", b"+c", b":3", b"*ct:2", b":2-ac", b"+gt:1", b"-acg:1")
    n = 2 * 16 * 64 + 17
    records = [(int(rng.integers(0, 2)), int(rng.integers(0, 34)), toks[int(rng.integers(0, len(toks)))]) for _ in range(n)]
    return records, [40, 40], (1024, n - 1)


def run_abi(pkg, packed, pos_off, region, device):
    """mpc_coverage_host / mpc_coverage_run on arrays as they are (coverage.run
    refuses a sample index outside the targets before either): (status, rows, stats)."""
    cs, off, ts, rs = packed
    n, S, n_pos = len(ts), len(pos_off) - 1, int(pos_off[-1])
    if device == "cpu":
        L = pkg.coverage.host_lib()
        rows, stats, status = np.zeros((n_pos, 4), np.uint32), np.zeros((S, 16), np.uint64), np.zeros(2, np.int32)
        cs = np.concatenate([cs, np.zeros(8, np.uint8)])
        rc = L.mpc_coverage_host(cs.ctypes.data, off.ctypes.data, ts.ctypes.data, rs.ctypes.data, n, pos_off.ctypes.data,
                                 region.ctypes.data, S, 0, rows.ctypes.data, stats.ctypes.data, status.ctypes.data, 3, None)
        assert rc == 0, L.mpc_coverage_last_error()
        return tuple(status.tolist()), rows, stats
    import torch
    L = pkg.engine.lib()
    dev = "cuda:%d" % device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_cs, d_off, d_ts, d_rs, d_pos, d_reg = (up(a) for a in (np.concatenate([cs, np.zeros(8, np.uint8)]), off, ts, rs,
                                                             pos_off, region))
    d_rows = torch.empty((n_pos, 4), dtype=torch.int32, device=dev)
    d_stats = torch.empty((S, 16), dtype=torch.int64, device=dev)
    d_status = torch.empty(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = L.mpc_coverage_run(d_cs.data_ptr(), d_off.data_ptr(), d_ts.data_ptr(), d_rs.data_ptr(), n, d_pos.data_ptr(),
                                d_reg.data_ptr(), S, 0, d_rows.data_ptr(), d_stats.data_ptr(), d_status.data_ptr(), None)
        assert rc == 0, L.mpc_last_error()
        torch.cuda.synchronize()
    return tuple(d_status.cpu().tolist()), d_rows.cpu().numpy().view(np.uint32), d_stats.cpu().numpy().view(np.uint64)


def case_bad_sample(pkg, device):
    """A sample index outside the targets in lane 0 of a wave's batch and in the
    last record: the smaller one is named, out of range; every other record counts."""
    records, lengths, bad = bad_sample_batch()
    regions = [(0, L) for L in lengths]
    _, rows, stats, _ = check([r for k, r in enumerate(records) if k not in bad], lengths, regions)
    packed = pack(records)
    packed[3][bad[0]], packed[3][bad[1]] = len(lengths), -1
    pos_off = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64) + 1)]).astype(np.int64)
    got = run_abi(pkg, packed, pos_off, np.array(regions, np.int64).reshape(-1), device)
    assert got[0] == (RANGE, bad[0])
    assert np.array_equal(got[1], rows) and np.array_equal(got[2], stats)


MALFORMED_CS = {  # one per grammar rule of the issue
    "tenth_digit": b":1234567890",
    "space_in_number": b": 7",
    "underscore": b":1_0",
    "long_form": b"=ACG",
    "one_letter_sub": b"*a",
    "bare_operator": b":5-",
}

# (name, record, code) on one target of 20 bases: one bad record per rule
BAD = [(name, (0, 2, cs), MALFORMED) for name, cs in MALFORMED_CS.items()] + [
    ("negative_start", (0, -1, b":3"), RANGE), ("end_past_L", (0, 10, b":11"), RANGE),
    ("ins_past_L", (0, 20, b":1+a"), RANGE), ("both_malformed_wins", (0, 15, b":9*a"), MALFORMED),
    ("late_malformed_after_range", (0, 0, b":30=A"), MALFORMED), ("empty_insertion", (0, 0, b":3+:2"), MALFORMED),
    ("three_letter_sub", (0, 0, b"*acg"), MALFORMED), ("digit_first", (0, 0, b"5"), MALFORMED),
    ("z_without_colon", (0, 0, b"Z"), MALFORMED), ("empty_number", (0, 0, b":*ac"), MALFORMED),
]
GOOD = [(0, 0, b":20"), (0, 1, b":5*ac-gg+t:3"), (0, 20, b"")]
