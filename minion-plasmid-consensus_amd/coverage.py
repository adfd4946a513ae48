"""coverage_qc: per-position depth and error profile of every PAF target.

Acceptance criterion 1 of the reference README ("at least 100,000x mean
coverage of the plasmid") from the PAF the `consensus` rule already consumes:
the target span and the cs tag of every alignment (include/mpc_coverage.h has
the definition; DESIGN.md "coverage_qc").

  read_paf  one PAF through libmpc_ingest.so (mpc_coverage_ingest): target,
            span, mapq, read length, strand and cs bytes of every kept line
  run       rows + stats of a batch of records: K_covparse + K_covfinish in ONE
            mpc_coverage_run on the GPU (libmpc.so), or the scalar host walk
            (device="cpu")
  qc        every PAF and every target of a call in one run + the derived
            numbers + the verdict

The derived numbers (mean, sd, error rate) are computed here from the exact
integers, identically for both paths.  They follow this module's definition;
no equality with Qualimap's figures is claimed.
"""
import ctypes
import math

import numpy as np

from . import _native

STATS = 16  # mpc_coverage.h MPC_COV_STATS
(ST_RECORDS, ST_MATCH, ST_MISMATCH, ST_INS_EVENTS, ST_INS_BASES, ST_DEL_EVENTS, ST_DEL_BASES, ST_SUM, ST_SUMSQ,
 ST_MIN, ST_MAX, ST_BELOW, ST_SUM_DELETED) = range(13)
CODES = {1: "malformed cs", 2: "out of range"}
MIN_MEAN_COVERAGE = 100000.0


class CoverageError(ValueError):
    """Input that cannot be measured (the CLI exits 1)."""


class _Paf(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_int64), ("n_lines", ctypes.c_int64), ("n_targets", ctypes.c_int64),
                ("target", ctypes.POINTER(ctypes.c_int32)), ("tstart", ctypes.POINTER(ctypes.c_int64)),
                ("tend", ctypes.POINTER(ctypes.c_int64)), ("qlen", ctypes.POINTER(ctypes.c_int64)),
                ("mapq", ctypes.POINTER(ctypes.c_int32)), ("strand", ctypes.POINTER(ctypes.c_uint8)),
                ("cs", ctypes.POINTER(ctypes.c_uint8)), ("cs_off", ctypes.POINTER(ctypes.c_int64)),
                ("target_names", ctypes.POINTER(ctypes.c_char)), ("target_name_off", ctypes.POINTER(ctypes.c_int64)),
                ("target_len", ctypes.POINTER(ctypes.c_int64)), ("owner", ctypes.c_void_p),
                ("status", ctypes.c_int32), ("message", ctypes.c_char * 256)]


def host_lib():
    """libmpc_ingest.so (its prototypes: _native.host_prototypes)."""
    return _native.host(CoverageError)


def tile_bytes():
    """cs bytes K_covparse takes per tile (no GPU needed)."""
    from . import engine
    return engine.lib().mpc_coverage_tile_bytes()


def _copy(ptr, n, dtype):
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype)


def read_paf(path, mode=0, threads=0):
    """dict(target, tstart, tend, qlen, mapq, strand, cs, cs_off, names, lengths,
    n_lines) of one PAF.  mode 0: the first alignment per read name (what the
    consensus is called from); mode 1: every line.  There is no Python parser:
    what libmpc_ingest.so refuses raises CoverageError naming the line."""
    L = host_lib()
    out = _Paf()
    rc = L.mpc_coverage_ingest(str(path).encode(), mode, threads, ctypes.byref(out))
    try:
        if rc != 0:
            raise CoverageError(out.message.decode(errors="replace"))
        n, nt = out.n_records, out.n_targets
        cs_off = _copy(out.cs_off, n + 1, np.int64)
        noff = _copy(out.target_name_off, nt + 1, np.int64)
        blob = ctypes.string_at(out.target_names, int(noff[-1])) if nt else b""
        return dict(target=_copy(out.target, n, np.int32), tstart=_copy(out.tstart, n, np.int64),
                    tend=_copy(out.tend, n, np.int64), qlen=_copy(out.qlen, n, np.int64),
                    mapq=_copy(out.mapq, n, np.int32), strand=_copy(out.strand, n, np.uint8),
                    cs=_copy(out.cs, int(cs_off[-1]), np.uint8), cs_off=cs_off,
                    names=[blob[noff[k]:noff[k + 1]].decode(errors="replace") for k in range(nt)],
                    lengths=[int(x) for x in _copy(out.target_len, nt, np.int64)], n_lines=int(out.n_lines))
    finally:
        L.mpc_coverage_ingest_free(ctypes.byref(out))


def batch_front(err, cs, cs_off, tstart, rec_sample, lengths, more=()):
    """The front of coverage.run and linkage.run: (cs, cs_off, tstart, rec_sample,
    pos_off) as contiguous arrays of the C-ABI's types, checked; what is wrong
    raises err.  more: [(fault found, message)] of the caller's own tables,
    reported once the record and target counts stand."""
    cs = np.ascontiguousarray(cs, np.uint8)
    cs_off = np.ascontiguousarray(cs_off, np.int64)
    tstart = np.ascontiguousarray(tstart, np.int64)
    rec_sample = np.ascontiguousarray(rec_sample, np.int32)
    n, S = len(tstart), len(lengths)
    if len(cs_off) != n + 1 or len(rec_sample) != n:
        raise err("cs_off, tstart and rec_sample disagree on the number of records")
    if S < 1:
        raise err("no target")
    for bad, message in more:
        if bad:
            raise err(message)
    if n and (cs_off[0] < 0 or (np.diff(cs_off) < 0).any() or cs_off[-1] > len(cs)):
        raise err("cs_off does not cut the cs bytes")
    if n and (rec_sample.min() < 0 or rec_sample.max() >= S):
        raise err("a record names a target outside [0, {})".format(S))
    pos_off = np.zeros(S + 1, np.int64)
    pos_off[1:] = np.cumsum(np.asarray(lengths, np.int64) + 1)
    if min(lengths) < 0 or pos_off[-1] >= 2 ** 31:
        raise err("target lengths must be >= 0 and sum (with one extra row each) to below 2^31")
    return cs, cs_off, tstart, rec_sample, pos_off


def raise_status(err, status):
    """The C-ABI's status {code, smallest offending record} as err, if any."""
    if status[0] != 0:
        raise err("record {}: {}".format(int(status[1]), CODES.get(int(status[0]), "code %d" % status[0])))


def run(cs, cs_off, tstart, rec_sample, lengths, regions=None, min_depth=0, device=0, threads=0, tend=None):
    """dict(rows u32[n_pos][4] = {depth, deleted, mismatch, insertion}, stats
    u64[S][16], pos_off) of the records (cs bytes, cs_off[n + 1], tstart[n],
    rec_sample[n]) over samples of the given lengths; regions[s] = (lo, hi),
    default the whole target.  Raises CoverageError naming the smallest
    malformed or out-of-range record.  tend (optional): the PAF's target ends;
    the host path checks every record's walk against it, both paths check the
    aggregate sum(tend - tstart) == match + mismatch + deleted per sample."""
    cs, cs_off, tstart, rec_sample, pos_off = batch_front(CoverageError, cs, cs_off, tstart, rec_sample, lengths)
    n, S = len(tstart), len(lengths)
    region =np.array([(0, L) for L in lengths] if regions is None else regions, np.int64).reshape(S, 2)
    for s, (lo, hi) in enumerate(region):
        if not 0 <= lo <= hi <= lengths[s]:
            raise CoverageError("target {}: region {}:{} is outside 0:{}".format(s, lo, hi, lengths[s]))
    n_pos = int(pos_off[-1])
    rec_out = None
    if device == "cpu":
        L = host_lib()
        rows = np.zeros((n_pos, 4), np.uint32)
        stats = np.zeros((S, STATS), np.uint64)
        status = np.zeros(2, np.int32)
        rec_out = np.zeros((n, 2), np.int64)
        _native.host_check(L, "coverage", CoverageError, L.mpc_coverage_host(
            cs.ctypes.data, cs_off.ctypes.data, tstart.ctypes.data, rec_sample.ctypes.data, n, pos_off.ctypes.data,
            region.ctypes.data, S, min_depth, rows.ctypes.data, stats.ctypes.data, status.ctypes.data, threads,
            rec_out.ctypes.data))
    else:
        with _native.Device(device, "host walk") as d:
            torch, dev = d.torch, d.dev
            # the int64 tables first, then rec_sample, then the cs bytes
            at, d_blob = d.put_all([cs_off, tstart, pos_off, region.reshape(-1), rec_sample, cs])
            d_rows = torch.empty((n_pos, 4), dtype=torch.int32, device=dev)
            d_stats = torch.empty((S, STATS), dtype=torch.int64, device=dev)
            d_status = torch.empty(2, dtype=torch.int32, device=dev)
            d.check(d.lib.mpc_coverage_run(at[5], at[0], at[1], at[4], n, at[2], at[3], S, min_depth, d_rows.data_ptr(),
                                           d_stats.data_ptr(), d_status.data_ptr(), d.stream))
            status = d_status.cpu().numpy()
            rows = d_rows.cpu().numpy().view(np.uint32)
            stats = d_stats.cpu().numpy().view(np.uint64)
    raise_status(CoverageError, status)
    if tend is not None:
        tend = np.asarray(tend, np.int64)
        if rec_out is not None:
            bad = np.nonzero(rec_out[:, 0] != tend)[0]
            if len(bad):
                r = int(bad[0])
                raise CoverageError("record {}: the cs walk ends at {}, the PAF says {}".format(r, int(rec_out[r, 0]), int(tend[r])))
        span = np.zeros(S, np.int64)
        np.add.at(span, rec_sample, tend - tstart)
        for s in range(S):
            walked = int(stats[s, ST_MATCH]) + int(stats[s, ST_MISMATCH]) + int(stats[s, ST_DEL_BASES])
            if int(span[s]) != walked:
                raise CoverageError("target {}: the cs tags cover {} reference bases, the PAF spans {}".format(s, walked, int(span[s])))
    return dict(rows=rows, stats=stats, pos_off=pos_off, rec_out=rec_out)


def derived(st, lo, hi):
    """dict(mean, sd, mean_deleted, error_rate) of one stats row over its
    region [lo, hi): exact Python integers up to the one division each."""
    st = [int(x) for x in st]
    n = hi - lo
    mean = st[ST_SUM] / n if n else 0.0
    var = (n * st[ST_SUMSQ] - st[ST_SUM] ** 2) / (n * n) if n else 0.0
    err = st[ST_MISMATCH] + st[ST_INS_BASES] + st[ST_DEL_BASES]
    return dict(mean=mean, sd=math.sqrt(var), mean_deleted=st[ST_SUM_DELETED] / n if n else 0.0,
                error_rate=err / (st[ST_MATCH] + err) if st[ST_MATCH] + err else 0.0)


def expected_core(expected, err):
    """(adapted length, c0, c1) of the adapter-padded FASTA `expected`: its
    upper-case plasmid core is [c0, c1).  None without a file; what
    verify.read_expected refuses raises err."""
    if expected is None:
        return None
    from . import verify
    try:
        adapted, c0, c1 = verify.read_expected(expected)
    except verify.VerifyError as e:
        raise err(str(e))
    return len(adapted), c0, c1


def target_regions(path, names, lengths, core, region, err):
    """[(lo, hi)] of a PAF's targets: the core (expected_core) of a target as
    long as the adapted sequence, else `region`, else the whole target.  A
    region outside its target raises err."""
    out = []
    for name, L in zip(names, lengths):
        lo, hi = core[1:] if core and L == core[0] else region if region else (0, L)
        if not 0 <= lo <= hi <= L:
            raise err("{}: target {}: region {}:{} is outside 0:{}".format(path, name, lo, hi, L))
        out.append((lo, hi))
    return out


def qc(paf_paths, expected=None, region=None, all_alignments=False, min_mean_coverage=MIN_MEAN_COVERAGE, min_depth=0,
       device=0, threads=0):
    """dict(blocks, verdict): one block per (paf, target) -- every PAF and every
    target of the call in ONE run.  expected: the adapter-padded FASTA; a target
    as long as it is measured over its upper-case plasmid core.  region: (lo,
    hi), 0-based half-open, for every target.  verdict: "PASS" iff every block
    has mean depth >= min_mean_coverage and no region position below min_depth."""
    core = expected_core(expected, CoverageError)
    pafs = [(p, read_paf(p, 1 if all_alignments else 0, threads)) for p in paf_paths]
    lengths, regions, owner = [], [], []
    for p, d in pafs:
        regions += target_regions(p, d["names"], d["lengths"], core, region, CoverageError)
        lengths += d["lengths"]
        owner += [(p, name) for name in d["names"]]
    if not lengths:
        raise CoverageError("no alignment in {}".format(", ".join(map(str, paf_paths))))
    sample_base = np.cumsum([0] + [len(d["names"]) for _, d in pafs])
    cs_base = np.cumsum([0] + [len(d["cs"]) for _, d in pafs])
    cat = lambda k, dt: np.concatenate([d[k] for _, d in pafs]).astype(dt, copy=False)
    rec_sample = np.concatenate([d["target"] + sample_base[k] for k, (_, d) in enumerate(pafs)]).astype(np.int32)
    cs_off = np.concatenate([d["cs_off"][:-1] + cs_base[k] for k, (_, d) in enumerate(pafs)] + [cs_base[-1:]])
    tstart, tend = cat("tstart", np.int64), cat("tend", np.int64)
    try:
        res = run(cat("cs", np.uint8), cs_off, tstart, rec_sample, lengths, regions, min_depth, device, threads, tend=tend)
    except CoverageError as e:
        raise CoverageError("{} (records in the order of the kept PAF lines of {})".format(e, ", ".join(map(str, paf_paths))))
    mapq, qlen, strand = cat("mapq", np.int64), cat("qlen", np.int64), cat("strand", np.uint8)
    blocks, ok = [], True
    for s, (p, name) in enumerate(owner):
        lo, hi = regions[s]
        rows = res["rows"][res["pos_off"][s]:res["pos_off"][s + 1]]
        st = [int(x) for x in res["stats"][s]]
        sel = rec_sample == s
        nrec = int(sel.sum())
        b = dict(paf=str(p), target=name, length=lengths[s], records=st[ST_RECORDS], region=(lo, hi), stats=st, rows=rows,
                 min_position=lo + int(np.argmin(rows[lo:hi, 0])) + 1 if hi > lo else 0,
                 mean_mapq=int(mapq[sel].sum()) / nrec if nrec else 0.0,
                 mean_read_length=int(qlen[sel].sum()) / nrec if nrec else 0.0,
                 plus=int((strand[sel] == ord("+")).sum()), minus=int((strand[sel] == ord("-")).sum()))
        b.update(derived(st, lo, hi))
        ok = ok and b["mean"] >= min_mean_coverage and st[ST_BELOW] == 0
        blocks.append(b)
    return dict(blocks=blocks, verdict="PASS" if ok else "FAIL")
