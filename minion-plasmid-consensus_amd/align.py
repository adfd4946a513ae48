"""align_reads: exact alignment of full-length plasmid reads to a one-record
assembly, written as the cs-tagged PAF the consensus CLI reads (the step the
reference Snakefile's rule final_alignment_paf runs minimap2 for).
include/mpc_align.h has the definition.  Per batch of reads:

  revcomp  the minus-strand queries (K_arevcomp, or the host loop)
  scan     (distance, end) of both orientations of every read against the
           target: ONE K_vscan launch over 2 x reads pairs (mpc_verify_scan), or
           the scalar host scan
  plan     strand, mapped or not, band sizes, the cut into launches under the
           workspace budget (mpc_align_plan, host)
  trace    band DP + canonical traceback + run encoding of a launch's reads
           (K_atrace: one wave per read; or mpc_align_trace_host)
  render   end rule + PAF lines (mpc_align_render, host threads)
(handoff.py goes on from a launch's trace to the pileup's inputs instead.)

Reads stream through in batches of at most ``batch_bases`` bases, so host and
device memory stay bounded whatever the file size.
"""
import ctypes

import numpy as np

from . import _native, verify

MAX_QUERY = 65536                 # mpc_verify.h MPC_VERIFY_MAX_QUERY
MAX_EDITS = 4096                  # mpc_align.h MPC_ALIGN_MAX_EDITS
DEFAULT_WORKSPACE = 2 << 30       # mpc_align.h MPC_ALIGN_DEFAULT_WORKSPACE
DEFAULT_BATCH_BASES = 64 << 20
E_SCAN = -5                       # mpc_align.h MPC_ALIGN_E_SCAN
SUMMARY_FIELDS = ("reads", "mapped", "plus", "minus", "unmapped_by_distance", "unmapped_no_match", "skipped_length")


class AlignError(ValueError):
    """Input that cannot be aligned (the CLI exits 1)."""


class TraceError(AlignError):
    """The band DP of a read does not reproduce its scan distance: ``read`` is
    its index among the batch's reads, ``status`` what the trace says of it."""

    def __init__(self, read, status):
        super().__init__("read {}: the band DP does not reproduce the scan's distance".format(read))
        self.read, self.status = read, status


# ---- FASTA ---------------------------------------------------------------------

def fasta_records(path, headers=False):
    """(name, sequence) of every record, in file order: the name is the header
    up to the first whitespace, the sequence its lines right-stripped and
    joined.  A sequence byte that is not an ASCII letter is refused.
    ``headers``: (name, sequence, header), the header line right-stripped,
    without its '>' (what the consensus parser takes for the name)."""
    name, parts, whole = None, [], b""
    rec = (lambda: (name, b"".join(parts), whole)) if headers else (lambda: (name, b"".join(parts)))
    with open(path, "rb") as f:
        for no, line in enumerate(f, 1):
            if line.startswith(b">"):
                if name is not None:
                    yield rec()
                head = line[1:].split(None, 1)
                name, parts, whole = (head[0] if head else b""), [], line.rstrip()[1:]
                continue
            line = line.rstrip()
            if not line:
                continue
            if name is None:
                raise AlignError("{}: line {}: sequence before the first '>' header".format(path, no))
            if not line.isalpha():  # (bytes.isalpha: ASCII letters only)
                raise AlignError("{}: line {}: a sequence line may hold ASCII letters only".format(path, no))
            parts.append(line)
    if name is not None:
        yield rec()


def read_target(path):
    """(name, sequence) of the assembly: exactly one record of 1 .. 2^31 - 1 bases."""
    recs = list(fasta_records(path))
    if len(recs) != 1:
        raise AlignError("{}: {} FASTA records, the assembly must hold exactly one".format(path, len(recs)))
    name, seq = recs[0]
    if not 1 <= len(seq) < 2 ** 31:
        raise AlignError("{}: a target of {} bases (1 .. 2^31 - 1 supported)".format(path, len(seq)))
    return name, seq


def read_batches(path, batch_bases=DEFAULT_BATCH_BASES, headers=False):
    """Lists of (name, sequence) holding at most ``batch_bases`` bases each (at
    least one read), reads of unsupported length included (``headers``: as for
    fasta_records)."""
    batch, bases = [], 0
    for rec in fasta_records(path, headers):
        if batch and bases + len(rec[1]) > batch_bases:
            yield batch
            batch, bases = [], 0
        batch.append(rec)
        bases += len(rec[1])
    if batch:
        yield batch


# ---- native bindings -----------------------------------------------------------

def host_lib():
    """libmpc_ingest.so (its prototypes: _native.host_prototypes)."""
    return _native.host(AlignError)


def _host_check(L, rc, accept=()):
    return _native.host_check(L, "align", AlignError, rc, accept)


# ---- the steps, one batch at a time --------------------------------------------

class Packed:
    """One batch's sequence blob: the target at offset 0, every read, then room
    for every reverse complement; plus[r] / minus[r] are read r's offsets."""

    def __init__(self, target, reads):
        self.n = len(target)
        self.lens = np.array([len(s) for s in reads], np.int64)
        start = (self.n + 7) // 8 * 8
        total = int(self.lens.sum())
        self.plus = start + np.concatenate([[0], np.cumsum(self.lens)[:-1]]).astype(np.int64) if len(reads) else np.zeros(0, np.int64)
        self.minus = self.plus + total
        self.seq = np.zeros(start + 2 * total + 8, np.uint8)
        self.seq[:self.n] = np.frombuffer(target, np.uint8)
        if total:
            self.seq[start:start + total] = np.frombuffer(b"".join(reads), np.uint8)
        self.minus_span = (start + total, start + 2 * total)
        self.d_seq = None  # the device copy, once a device step made one

    def revcomp_table(self):
        return np.ascontiguousarray(np.stack([self.plus, self.lens, self.minus], axis=1))

    def pair_table(self):
        """int64 [2 R, 4]: pair 2 r is read r as it is, pair 2 r + 1 its reverse complement."""
        R = len(self.lens)
        tab = np.zeros((2 * R, 4), np.int64)
        tab[0::2, 0], tab[1::2, 0] = self.plus, self.minus
        tab[:, 1] = np.repeat(self.lens, 2)
        tab[:, 3] = self.n
        return tab


def orient_and_scan(pk, device=0, threads=0):
    """Fills the blob's reverse complements and returns the scan results
    int32 [R, 4] = {d+, end+, d-, end-}."""
    R = len(pk.lens)
    if R == 0:
        return np.zeros((0, 4), np.int32)
    rc_tab = pk.revcomp_table()
    if device == "cpu":
        L = host_lib()
        _host_check(L, L.mpc_align_revcomp_host(pk.seq.ctypes.data, pk.seq.nbytes, rc_tab.ctypes.data, R, threads))
    else:
        with _native.Device(device) as d:
            pk.d_seq = d.put(pk.seq)
            d_tab = d.put(rc_tab)
            d.check(d.lib.mpc_align_revcomp(pk.d_seq.data_ptr(), pk.seq.nbytes, d_tab.data_ptr(), R, d.stream))
            a, b = pk.minus_span
            pk.seq[a:b] = pk.d_seq[a:b].cpu().numpy()  # the renderer reads the oriented reads on the host
    try:
        return verify.scan_table(pk.seq, pk.pair_table(), device, threads, d_seq=pk.d_seq).reshape(R, 4)
    except verify.VerifyError as e:
        raise AlignError(str(e))


def plan(scan, lens, max_error=0.2, workspace_bytes=DEFAULT_WORKSPACE):
    """(plan int64 [R, 8], cuts): mpc_align_plan.  plan[r] = {strand, mapped, d,
    end, W, flag_bytes, flag_off, run_off}; launch k holds the mapped reads
    among [cuts[k], cuts[k + 1])."""
    L = host_lib()
    R = len(lens)
    scan = np.ascontiguousarray(scan, np.int32)
    lens32 = np.ascontiguousarray(lens, np.int32)
    out = np.zeros((R, 8), np.int64)
    cuts = np.zeros(R + 1, np.int32)
    nl = ctypes.c_int32(0)
    _host_check(L, L.mpc_align_plan(scan.ctypes.data, lens32.ctypes.data, R, float(max_error), int(workspace_bytes),
                                    out.ctypes.data, cuts.ctypes.data, ctypes.byref(nl)))
    return out, [int(c) for c in cuts[:nl.value + 1]]


def jobs_of(pk, pl, reads):
    """The job table int64 [len(reads), 8] of the given (mapped) reads of one launch."""
    reads = np.asarray(reads, np.int64)
    jobs = np.zeros((len(reads), 8), np.int64)
    jobs[:, 0] = np.where(pl[reads, 0] != 0, pk.minus[reads], pk.plus[reads])
    jobs[:, 1] = pk.lens[reads]
    jobs[:, 3] = pk.n
    jobs[:, 4], jobs[:, 5], jobs[:, 6], jobs[:, 7] = pl[reads, 2], pl[reads, 3], pl[reads, 6], pl[reads, 7]
    return jobs


def trace(seq, jobs, device=0, threads=0, d_seq=None, workspace=None, device_tensors=None):
    """(rc, out int32 [J, 8], runs int32[]) of one launch: mpc_align_trace on a
    GPU, mpc_align_trace_host for device="cpu".  rc is 0 or E_SCAN (a read's
    band did not give its scan distance; out holds the statuses); any other
    failure raises.  ``d_seq``: the blob's device copy when there is one;
    ``workspace``: a dict that keeps the flag workspace between launches;
    ``device_tensors``: a dict that receives the launch's device tensors (seq,
    jobs, out, runs) for a step that goes on with them there (draft.vote)."""
    jobs = np.ascontiguousarray(jobs, np.int64).reshape(-1, 8)
    J = len(jobs)
    runs_cap = int((jobs[:, 7] + 2 * jobs[:, 4] + 1).max()) if J else 0
    out = np.zeros((J, 8), np.int32)
    runs = np.zeros(max(runs_cap, 1), np.int32)
    if J == 0:
        return 0, out, runs[:0]
    if device == "cpu":
        L = host_lib()
        rc = _host_check(L, L.mpc_align_trace_host(seq.ctypes.data, seq.nbytes, jobs.ctypes.data, J, out.ctypes.data,
                                                   runs.ctypes.data, runs_cap, threads), accept=(E_SCAN,))
        return rc, out, runs[:runs_cap]
    pitch = (2 * jobs[:, 4] + 1 + 63) // 64 * 64
    flags_bytes = max(int((jobs[:, 6] + jobs[:, 1] * pitch).max()), 64)
    with _native.Device(device) as d:
        torch, dev = d.torch, d.dev
        if d_seq is None:
            d_seq = d.put(seq)
        ws = workspace if workspace is not None else {}
        if ws.get("flags") is None or ws["flags"].numel() < flags_bytes or ws["flags"].device != dev:
            ws["flags"] = None  # (free before growing)
            ws["flags"] = torch.empty(flags_bytes, dtype=torch.uint8, device=dev)
        d_jobs = d.put(jobs)
        d_out = torch.zeros(8 * J, dtype=torch.int32, device=dev)
        d_runs = torch.zeros(max(runs_cap, 1), dtype=torch.int32, device=dev)
        rc = d.check(d.lib.mpc_align_trace(d_seq.data_ptr(), seq.nbytes, d_jobs.data_ptr(), J, ws["flags"].data_ptr(),
                                           ws["flags"].numel(), d_out.data_ptr(), d_runs.data_ptr(), runs_cap, d.stream),
                     accept=(E_SCAN,))
        out = d_out.cpu().numpy().reshape(J, 8)
        runs = d_runs.cpu().numpy()
        if device_tensors is not None:
            device_tensors.update(seq=d_seq, jobs=d_jobs, out=d_out, runs=d_runs)
    return rc, out, runs[:runs_cap]


def render(seq, jobs, strand, out, runs, names, tname, threads=0):
    """(PAF bytes, line_len int64 [J]) of one launch's traced reads, in job order."""
    L = host_lib()
    jobs = np.ascontiguousarray(jobs, np.int64).reshape(-1, 8)
    J = len(jobs)
    if J == 0:
        return b"", np.zeros(0, np.int64)
    out = np.ascontiguousarray(out, np.int32)
    runs = np.ascontiguousarray(runs, np.int32)
    strand = np.ascontiguousarray(strand, np.uint8)
    name_off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.int64)
    blob = b"".join(names)
    edits = out[:, 3].astype(np.int64) + out[:, 4] + out[:, 5]
    cap = int((np.diff(name_off) + len(tname) + 140 + 3 * edits + 7 * out[:, 6].astype(np.int64)).sum())
    buf = ctypes.create_string_buffer(cap)
    line_len = np.zeros(J, np.int64)
    written = ctypes.c_int64(0)
    _host_check(L, L.mpc_align_render(seq.ctypes.data, seq.nbytes, jobs.ctypes.data, J, strand.ctypes.data, out.ctypes.data,
                                      runs.ctypes.data, len(runs), blob, name_off.ctypes.data, tname, ctypes.addressof(buf),
                                      cap, line_len.ctypes.data, ctypes.byref(written), threads))
    return buf.raw[:written.value], line_len


class Launches:
    """The reads of one batch against a target, scanned and planned (pk, scan,
    plan, cuts); iterating traces launch after launch of the plan's cut and
    gives (reads, jobs, out, runs, device tensors) of each, an empty one too:
    the indices of its mapped reads, their job table and what trace returns.
    ``workspace``: the dict that keeps the flag workspace between launches and
    batches; ``keep_device``: hand on each launch's device tensors (else, and
    for device="cpu", None).  A read whose band does not give its scan
    distance raises TraceError.  pk.d_seq stays until the caller drops it."""

    def __init__(self, target, reads, device=0, max_error=0.2, workspace_bytes=DEFAULT_WORKSPACE, threads=0,
                 workspace=None, keep_device=False):
        self.device, self.threads, self.keep_device = device, threads, keep_device
        self.workspace = workspace if workspace is not None else {}
        self.pk = Packed(target, reads)
        self.scan = orient_and_scan(self.pk, device, threads)
        self.plan, self.cuts = plan(self.scan, self.pk.lens, max_error, workspace_bytes)

    def __iter__(self):
        pk, pl = self.pk, self.plan
        for a, b in zip(self.cuts[:-1], self.cuts[1:]):
            reads = [r for r in range(a, b) if pl[r, 1]]
            jobs = jobs_of(pk, pl, reads)
            kept = {} if self.keep_device else None
            rc, out, runs = trace(pk.seq, jobs, self.device, self.threads, d_seq=pk.d_seq, workspace=self.workspace,
                                  device_tensors=kept)
            if rc != 0:
                k = int(np.nonzero(out[:, 0])[0][0])
                raise TraceError(reads[k], int(out[k, 0]))
            yield reads, jobs, out, runs, kept or None


class BatchLoop:
    """One batch of records ((name, sequence, ...) tuples) against a target: the
    Launches of its reads of supported length, and the summary rule, stated
    once for align_records and handoff.feed.  ``counts`` starts with reads,
    skipped_length and unmapped_by_distance; iterating gives what Launches
    gives (a TraceError comes out as the AlignError that names the read) and
    drops the blob's device copy at the end; ``count`` adds one launch's reads
    once the caller knows which of them got a line.  ``keep[r]`` is the record
    of read r, ``names[r]`` its name."""

    def __init__(self, target, records, device=0, max_error=0.2, workspace_bytes=DEFAULT_WORKSPACE, threads=0,
                 workspace=None, keep_device=False):
        self.counts = dict.fromkeys(SUMMARY_FIELDS, 0)
        self.counts["reads"] = len(records)
        self.keep = [k for k, rec in enumerate(records) if 1 <= len(rec[1]) <= MAX_QUERY]
        self.counts["skipped_length"] = len(records) - len(self.keep)
        self.names = [records[k][0] for k in self.keep]
        self.loop = Launches(target, [records[k][1] for k in self.keep], device, max_error, workspace_bytes, threads,
                             workspace, keep_device)
        self.pk, self.plan = self.loop.pk, self.loop.plan
        self.counts["unmapped_by_distance"] = int((self.plan[:, 1] == 0).sum()) if len(self.keep) else 0
        self.launches = len(self.loop.cuts) - 1

    def __iter__(self):
        try:
            yield from self.loop
        except TraceError as e:
            raise AlignError("read {!r}: the band DP does not reproduce the scan's distance (status {})".format(
                self.names[e.read].decode(errors="replace"), e.status))
        self.pk.d_seq = None

    def count(self, reads, wrote):
        """One launch: ``wrote[k]`` says whether read reads[k] got a PAF line."""
        minus = self.plan[reads, 0] != 0
        self.counts["mapped"] += int(wrote.sum())
        self.counts["minus"] += int((wrote & minus).sum())
        self.counts["plus"] += int((wrote & ~minus).sum())
        self.counts["unmapped_no_match"] += int((~wrote).sum())
        return minus


def align_records(target, tname, records, device=0, max_error=0.2, workspace_bytes=DEFAULT_WORKSPACE, threads=0,
                  workspace=None, detail=False):
    """One batch: dict(paf=bytes, counts=dict over SUMMARY_FIELDS, launches=int)
    of the (name, sequence) records, in order.  ``detail``: also plan, scan and
    per read the trace row and runs (tests)."""
    loop = BatchLoop(target, records, device, max_error, workspace_bytes, threads, workspace)
    pk, pl = loop.pk, loop.plan
    parts, det = [], dict(kept=loop.keep, scan=loop.loop.scan, plan=pl, cuts=loop.loop.cuts, out={}, runs={})
    for reads, jobs, out, runs, _ in loop:
        text, line_len = render(pk.seq, jobs, pl[reads, 0], out, runs, [loop.names[r] for r in reads], tname, threads)
        parts.append(text)
        loop.count(reads, line_len > 0)
        if detail:
            for k, r in enumerate(reads):
                det["out"][r] = out[k].copy()
                det["runs"][r] = runs[jobs[k, 7]: jobs[k, 7] + out[k, 6]].copy()
    res = dict(paf=b"".join(parts), counts=loop.counts, launches=loop.launches)
    if detail:
        res["detail"] = det
    return res


def align(ref_path, reads_path, device=0, max_error=0.2, workspace_bytes=DEFAULT_WORKSPACE, write=None,
          batch_bases=DEFAULT_BATCH_BASES, threads=0):
    """Aligns every read of ``reads_path`` to the one record of ``ref_path``.
    Returns dict(paf, summary): the PAF bytes (None when ``write`` is given:
    then every batch's lines go to write(bytes) as they are made) and the
    summary counts.  Raises AlignError on input the definition refuses."""
    if not max_error >= 0:
        raise AlignError("max_error must be >= 0")
    tname, target = read_target(ref_path)
    summary = dict.fromkeys(SUMMARY_FIELDS, 0)
    parts, ws = [], {}
    for batch in read_batches(reads_path, batch_bases):
        res = align_records(target, tname, batch, device, max_error, workspace_bytes, threads, workspace=ws)
        for k in SUMMARY_FIELDS:
            summary[k] += res["counts"][k]
        (write or parts.append)(res["paf"])
    return dict(paf=None if write else b"".join(parts), summary=summary)


def summary_text(summary):
    return "".join("{}\t{}\n".format(k, summary[k]) for k in SUMMARY_FIELDS)
