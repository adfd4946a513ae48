"""draft_assembly: the sense / antisense assembly the reads are then aligned
to, from the first reads of merged.fasta (the step the reference Snakefile's
rules subsample_fasta, canu_denovo_assembly, select_top_assembly and
revcomp_assembly run canu for).  include/mpc_draft.h has the definition.

  sample  the first reads of supported length, upper-cased
  seed    the candidates nearest the median length, each scanned as the target
          of the whole sample (align.orient_and_scan); the best one
  round   align the sample to the draft (align's scan, plan and trace), vote
          every traced read's runs into the tallies (K_dvote, or
          mpc_draft_vote_host), call the new draft (K_dcall, or
          mpc_draft_call_host); on a GPU the sequence blob, the runs and the
          out rows stay on the device between trace and vote

This is not an assembler: every read must be a full-length copy of one molecule.
"""
import math

import numpy as np

from . import _native, align

ROW = 48                # mpc_draft.h MPC_DRAFT_ROW
SLOTS = 8               # mpc_draft.h MPC_DRAFT_SLOTS
MAX_LEN = 131072        # mpc_draft.h MPC_DRAFT_MAX_LEN
VOTED, BAD_RUNS, NO_MATCH, NOT_TRACED = 0, 1, 2, 3
E_RUNS, E_EMPTY, E_LONG = -6, -7, -8
INFO_FIELDS = ("status", "length", "lo", "hi", "maxcov", "changed", "dropped", "inserted")


class DraftError(align.AlignError):
    """Input no draft can be made from (the CLI exits 1)."""


def host_lib():
    """libmpc_ingest.so (its prototypes: _native.host_prototypes)."""
    return _native.host(DraftError)


# ---- vote and call, one launch at a time ----------------------------------------

def new_tally(n, device=0):
    """Zeroed tallies of a draft of n bases: uint32 [n + 1, ROW] (numpy for
    device="cpu", else a flat int32 torch tensor on that GPU)."""
    if device == "cpu":
        return np.zeros((n + 1, ROW), np.uint32)
    d = _native.Device(device)
    return d.torch.zeros((n + 1) * ROW, dtype=d.torch.int32, device=d.dev)


def tally_to_host(tally):
    if isinstance(tally, np.ndarray):
        return tally
    return tally.cpu().numpy().view(np.uint32).reshape(-1, ROW)


def vote(tally, n, seq, jobs, out, runs, device=0, threads=0, device_tensors=None):
    """Adds one launch's votes to ``tally``; (rc, status int32 [J]).  rc is 0 or
    E_RUNS (a read's runs do not walk it; status says which, and nothing of
    that read was added); any other failure raises.  ``device_tensors``: what
    align.trace left on the GPU (else the host arrays are copied there)."""
    jobs = np.ascontiguousarray(jobs, np.int64).reshape(-1, 8)
    J = len(jobs)
    status = np.zeros(J, np.int32)
    if J == 0:
        return 0, status
    if device == "cpu":
        L = host_lib()
        out = np.ascontiguousarray(out, np.int32)
        runs = np.ascontiguousarray(runs, np.int32)
        rc = L.mpc_draft_vote_host(seq.ctypes.data, seq.nbytes, jobs.ctypes.data, J, out.ctypes.data, runs.ctypes.data,
                                   len(runs), tally.ctypes.data, n, status.ctypes.data, threads)
        return _native.host_check(L, "draft", DraftError, rc, accept=(E_RUNS,)), status
    with _native.Device(device) as d:
        t = device_tensors or {}
        d_seq = t["seq"] if "seq" in t else d.put(seq)
        d_jobs = t["jobs"] if "jobs" in t else d.put(jobs)
        d_out = t["out"] if "out" in t else d.put(np.ascontiguousarray(out, np.int32))
        d_runs = t["runs"] if "runs" in t else d.put(np.ascontiguousarray(runs, np.int32))
        runs_cap = d_runs.numel() * d_runs.element_size() // 4
        d_status = d.torch.zeros(J, dtype=d.torch.int32, device=d.dev)
        rc = d.lib.mpc_draft_vote(d_seq.data_ptr(), d_seq.numel(), d_jobs.data_ptr(), J, d_out.data_ptr(), d_runs.data_ptr(),
                                  runs_cap, tally.data_ptr(), n, d_status.data_ptr(), d.stream)
        return d.check(rc, accept=(E_RUNS,)), d_status.cpu().numpy()


def call(tally, draft, device=0, d_draft=None):
    """(new draft bytes, info dict over INFO_FIELDS) from the tallies of
    ``draft``.  Raises DraftError when no read mapped or the new draft is longer
    than MAX_LEN.  ``d_draft``: a device tensor that starts with the draft."""
    n = len(draft)
    cap = min(9 * n, MAX_LEN)
    if device == "cpu":
        L = host_lib()
        new = np.zeros(cap, np.uint8)
        info = np.zeros(8, np.int32)
        h = np.frombuffer(draft, np.uint8)
        _native.host_check(L, "draft", DraftError,
                           L.mpc_draft_call_host(tally.ctypes.data, h.ctypes.data, n, new.ctypes.data, cap, info.ctypes.data))
    else:
        with _native.Device(device) as d:
            torch, dev = d.torch, d.dev
            if d_draft is None:
                d_draft = d.put(np.frombuffer(draft, np.uint8).copy())  # (writable: torch takes no read-only array)
            d_new = torch.zeros(cap, dtype=torch.uint8, device=dev)
            d_work = torch.empty(3 * (n + 1), dtype=torch.int32, device=dev)
            d_info = torch.zeros(8, dtype=torch.int32, device=dev)
            rc = d.lib.mpc_draft_call(tally.data_ptr(), d_draft.data_ptr(), n, d_new.data_ptr(), cap, d_work.data_ptr(),
                                      d_info.data_ptr(), d.stream)
            if d.check(rc, accept=(E_EMPTY, E_LONG)) != 0:  # (no read mapped, or a draft above MAX_LEN: the input's fault)
                raise DraftError(d.lib.mpc_last_error().decode(errors="replace"))
            info = d_info.cpu().numpy()
            new = d_new[:int(info[1])].cpu().numpy()
    info = dict(zip(INFO_FIELDS, (int(v) for v in info)))
    return new[:info["length"]].tobytes(), info


# ---- the driver -------------------------------------------------------------------

def take_sample(reads_path, sample=500):
    """(records, skipped): the first ``sample`` (0: all) records of supported
    length, upper-cased, and how many records before the last taken were skipped."""
    recs, skipped = [], 0
    for name, s in align.fasta_records(reads_path):
        if sample and len(recs) >= sample:
            break
        if 1 <= len(s) <= align.MAX_QUERY:
            recs.append((name, s.upper()))
        else:
            skipped += 1
    return recs, skipped


def _mapped(scan, lens, max_error):
    """(mapped bool [R], d int64 [R]) of a scan table: the rule of mpc_align.h."""
    d = np.minimum(scan[:, 0], scan[:, 2]).astype(np.int64)
    lim = np.array([min(math.floor(max_error * int(m)), align.MAX_EDITS) for m in lens], np.int64)
    return d <= lim, d


def pick_seed(records, candidates=8, max_error=0.3, device=0, threads=0):
    """(index of the seed, [(index, mapped, sum of d)] of every candidate)."""
    lens = np.array([len(s) for _, s in records], np.int64)
    srt = np.sort(lens)
    a, b = int(srt[(len(srt) - 1) // 2]), int(srt[len(srt) // 2])
    order = sorted(range(len(records)), key=lambda k: (abs(2 * int(lens[k]) - (a + b)), k))[:max(1, candidates)]
    reads = [s for _, s in records]
    scored = []
    for k in sorted(order):
        pk = align.Packed(reads[k], reads)
        scan = align.orient_and_scan(pk, device, threads)
        pk.d_seq = None
        ok, d = _mapped(scan, lens, max_error)
        scored.append((k, int(ok.sum()), int(d[ok].sum())))
    best = min(scored, key=lambda t: (-t[1], t[2], t[0]))
    return best[0], scored


def polish_round(draft, reads, device=0, max_error=0.3, workspace_bytes=align.DEFAULT_WORKSPACE, threads=0, workspace=None):
    """One round: (new draft, info) with info["mapped"] = reads voted and
    info["launches"].  The sample is aligned by align.Launches, as align.align_records does it."""
    n = len(draft)
    if not 1 <= n <= MAX_LEN:
        raise DraftError("a draft of {} bases (1 .. {} supported)".format(n, MAX_LEN))
    loop = align.Launches(draft, reads, device, max_error, workspace_bytes, threads, workspace, keep_device=True)
    pk = loop.pk
    tally = new_tally(n, device)
    voted = 0
    try:
        for rd, jobs, out, runs, kept in loop:
            rc, status = vote(tally, n, pk.seq, jobs, out, runs, device, threads, device_tensors=kept)
            if rc != 0:
                raise DraftError("read {}: its runs do not walk the read".format(rd[int(np.nonzero(status == BAD_RUNS)[0][0])]))
            voted += int((status == VOTED).sum())
    except align.TraceError as e:
        raise DraftError(str(e))
    new, info = call(tally, draft, device, d_draft=pk.d_seq)
    pk.d_seq = None
    if not new:
        raise DraftError("the round dropped every column of the draft")
    info.update(mapped=voted, launches=len(loop.cuts) - 1)
    return new, info


def scan_distance(query, text, device=0):
    """The scan distance of ``query`` (upper-cased) placed in ``text``."""
    tab = np.array([[len(text), len(query), 0, len(text)]], np.int64)
    seq = np.frombuffer(text + query.upper() + b"\0" * 8, np.uint8).copy()
    try:
        return int(align.verify.scan_table(seq, tab, device)[0, 0])
    except align.verify.VerifyError as e:
        raise DraftError(str(e))


def assemble(reads_path, sample=500, candidates=8, rounds=3, max_error=0.3, device=0, threads=0, orient_to=None,
             workspace_bytes=align.DEFAULT_WORKSPACE):
    """dict(sense, antisense, report): the two drafts (bytes) and the report's
    (key, value) pairs.  Raises DraftError on input the definition refuses."""
    if not max_error >= 0 or sample < 0 or candidates < 1 or rounds < 0:
        raise DraftError("max_error must be >= 0, sample >= 0, candidates >= 1, rounds >= 0")
    records, skipped = take_sample(reads_path, sample)
    if not records:
        raise DraftError("{}: no read of 1 .. {} bases ({} skipped by length)".format(reads_path, align.MAX_QUERY, skipped))
    orient = None
    if orient_to is not None:
        orient = align.read_target(orient_to)[1]
        if len(orient) > align.MAX_QUERY:
            raise DraftError("{}: {} bases (at most {} supported)".format(orient_to, len(orient), align.MAX_QUERY))
    seed, _ = pick_seed(records, candidates, max_error, device, threads)
    reads = [s for _, s in records]
    draft = reads[seed]
    report = [("sample_reads", len(records)), ("skipped_length", skipped), ("candidates", min(candidates, len(records))),
              ("seed", records[seed][0].decode(errors="replace")), ("seed_length", len(draft))]
    ws, converged = {}, False
    for k in range(1, rounds + 1):
        new, info = polish_round(draft, reads, device, max_error, workspace_bytes, threads, ws)
        report += [("round{}_{}".format(k, key), v) for key, v in (
            ("mapped", info["mapped"]), ("length", info["length"]), ("trim_head", info["lo"]),
            ("trim_tail", len(draft) - info["hi"]), ("changed", info["changed"]), ("dropped", info["dropped"]),
            ("inserted", info["inserted"]))]
        converged = new == draft
        draft = new
        if converged:
            break
    sense, anti = draft, _revcomp(draft)
    if orient is not None and scan_distance(orient, anti, device) < scan_distance(orient, sense, device):
        sense, anti = anti, sense
    return dict(sense=sense, antisense=anti, report=report, converged=converged)


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _revcomp(s):
    return s.translate(_COMP)[::-1]
