"""verify_consensus: is the consensus the expected plasmid?

The reference README ends with a manual step ("Check the results",
"Acceptance criteria"): align each consensus with the adapter-padded reference
and confirm that every plasmid base between the adapters matches and that the
median per-base accuracy is above 99.9 %.  This module does that exactly and
unbanded (include/mpc_verify.h has the definition):

  scan    (distance, end) of every (expected, consensus) pair in ONE launch of
          K_vscan on the GPU (libmpc.so), or the scalar host DP (device="cpu")
  script  the canonical edit script of a pair from its (distance, end)
          (libmpc_ingest.so, banded)
  verify  both regions of every consensus file + the accuracies medians + verdict

The expected sequence is the query (at most 65,536 bases), the consensus the
text it is placed in.
"""
import ctypes
import statistics

import numpy as np

from . import _native

MAX_QUERY = 65536   # mpc_verify.h MPC_VERIFY_MAX_QUERY
MAX_EDITS = 1024    # mpc_verify.h MPC_VERIFY_MAX_EDITS
MIN_MEDIAN_ACCURACY = 99.9
REGIONS = ("plasmid", "adapted")
_CIGAR_CAP = 1 << 16  # <= 2 * MAX_EDITS + 1 runs of at most 11 characters


class VerifyError(ValueError):
    """Input that cannot be verified (the CLI exits 1)."""


def _fasta_sequence(path):
    with open(path, "rb") as f:
        return b"".join(ln.rstrip() for ln in f if not ln.startswith(b">"))


def read_expected(path):
    """(adapted, core_start, core_end): the whole sequence of the expected FASTA
    as add_adapters_to_ref writes it (lower-case adapters around the upper-case
    plasmid) and the plasmid span [core_start, core_end) = first to last
    upper-case letter.  No lower case: the plasmid is the whole sequence."""
    adapted = _fasta_sequence(path)
    upper = [k for k, c in enumerate(adapted) if 65 <= c <= 90]
    if not upper:
        raise VerifyError("{}: no upper-case (plasmid) base in the expected sequence".format(path))
    return adapted, upper[0], upper[-1] + 1


def read_consensus(path):
    """The sequence of a consensus FASTA ('>' lines skipped, the others
    right-stripped and joined; may be empty)."""
    return _fasta_sequence(path)


def host_lib():
    """libmpc_ingest.so (its prototypes: _native.host_prototypes)."""
    return _native.host(VerifyError)


def _check_lengths(pairs):
    for k, (q, t) in enumerate(pairs):
        if not 1 <= len(q) <= MAX_QUERY:
            raise VerifyError("pair {}: expected sequence of {} bases (1 .. {} supported)".format(k, len(q), MAX_QUERY))
        if len(t) >= 2 ** 31:
            raise VerifyError("pair {}: consensus of {} bases (< 2^31 supported)".format(k, len(t)))


def _pack(pairs):
    """One byte blob: the int64 pair table {q_off, q_len, t_off, t_len}, then the
    sequences the offsets point into (each distinct bytes object once)."""
    n = len(pairs)
    tab = np.zeros((n, 4), np.int64)
    seqs, where, off = [], {}, 0
    for k, pair in enumerate(pairs):
        for side, s in enumerate(pair):
            if id(s) not in where:
                where[id(s)] = off
                seqs.append(s)
                off += len(s)
            tab[k, 2 * side], tab[k, 2 * side + 1] = where[id(s)], len(s)
    seq = np.frombuffer(b"".join(seqs) + b"\0" * 8, np.uint8).copy()  # (writable: torch takes no read-only array)
    return tab, seq


def scan_table(seq, tab, device, threads=0, d_seq=None):
    """int32 [n, 2] = (distance, end) of the pairs of an int64 [n, 4] pair
    table {q_off, q_len, t_off, t_len} over the uint8 blob ``seq``:
    mpc_verify_scan_host for device="cpu" (``threads``: 0 = all CPUs), else ONE
    K_vscan launch (mpc_verify_scan) on that GPU.  ``d_seq``: the blob's device
    copy when the caller has one."""
    tab = np.ascontiguousarray(tab, np.int64).reshape(-1, 4)
    n = len(tab)
    out = np.zeros((n, 2), np.int32)
    if n == 0:
        return out
    if device == "cpu":
        L = host_lib()
        _native.host_check(L, "verify", VerifyError,
                           L.mpc_verify_scan_host(seq.ctypes.data, tab.ctypes.data, n, out.ctypes.data, threads))
        return out
    with _native.Device(device) as d:
        if d_seq is None:
            d_seq = d.put(seq)
        d_tab = d.put(tab)
        d_out = d.torch.empty(2 * n, dtype=d.torch.int32, device=d.dev)
        d.check(d.lib.mpc_verify_scan(d_seq.data_ptr(), d_tab.data_ptr(), n, d_out.data_ptr(), d.stream))
        return d_out.cpu().numpy().reshape(n, 2)


def scan(pairs, device=0):
    """[(distance, end)] of every (expected, consensus) pair of bytes.  On a
    GPU: H2D copies of the packed sequences and the pair table, one K_vscan
    launch, one D2H copy of the results; device="cpu": the scalar host DP on
    all CPUs."""
    pairs = [(bytes(q), bytes(t)) for q, t in pairs]  # (bytes(b) is b for a bytes object: shared sequences stay shared)
    _check_lengths(pairs)
    if not pairs:
        return []
    tab, seq = _pack(pairs)
    return [(int(d), int(e)) for d, e in scan_table(seq, tab, device)]


def script(q, t, distance, end):
    """dict(start, matches, mismatches, insertions, deletions, cigar) of the
    canonical edit script; above MAX_EDITS start and the counts are -1 and the
    CIGAR is "*".  Raises VerifyError when (distance, end) is not what the band
    DP finds (a wrong scan result)."""
    L = host_lib()
    start = ctypes.c_int32(-1)
    counts = (ctypes.c_int32 * 4)()
    buf = ctypes.create_string_buffer(_CIGAR_CAP)
    _native.host_check(L, "verify", VerifyError, L.mpc_verify_script(q, len(q), t, len(t), distance, end, ctypes.byref(start),
                                                                     counts, buf, _CIGAR_CAP))
    return dict(start=start.value, matches=counts[0], mismatches=counts[1], insertions=counts[2],
                deletions=counts[3], cigar=buf.value.decode("ascii"))


def cigar_ops(cigar):
    """[(length, op)] of a CIGAR string ("*": none)."""
    out, k = [], 0
    for e, c in enumerate(cigar):
        if not c.isdigit():
            if c != "*":
                out.append((int(cigar[k:e]), c))
            k = e + 1
    return out


def edits(q, t, row, q_base=0):
    """The non-'=' ops of a row's script as (expected_pos, consensus_pos, op,
    expected_base, consensus_base), positions 1-based, expected positions
    shifted by q_base (the query's offset in the adapted sequence).  'X': the
    two bases' positions; 'D': the missing expected base and the consensus base
    it follows; 'I': the extra consensus base and the expected base it follows
    (0: before the first base).  A missing side is '-'."""
    i, j, out = 0, row["start"], []
    for length, op in cigar_ops(row["cigar"]):
        if op in "=X":
            if op == "X":
                out += [(q_base + i + k + 1, j + k + 1, op, chr(q[i + k]), chr(t[j + k])) for k in range(length)]
            i, j = i + length, j + length
        elif op == "D":
            out += [(q_base + i + k + 1, j, op, chr(q[i + k]), "-") for k in range(length)]
            i += length
        else:
            out += [(q_base + i, j + k + 1, op, "-", chr(t[j + k])) for k in range(length)]
            j += length
    return out


def median_accuracy(path):
    """statistics.median of the accuracy column of a per-base accuracies TSV."""
    with open(path, "r") as f:
        lines = f.read().splitlines()
    try:
        vals = [float(ln.split("\t")[1]) for ln in lines[1:] if ln]
    except (IndexError, ValueError) as e:
        raise VerifyError("{}: not a per-base accuracies file ({})".format(path, e))
    if not vals:
        raise VerifyError("{}: no accuracies".format(path))
    return statistics.median(vals)


def verify(expected_path, consensus_paths, accuracies_paths=None, device=0):
    """dict(rows, medians, verdict, adapted, core).  rows: two per consensus
    file (region "plasmid", then "adapted") with the report's columns; every
    pair of the call goes through ONE scan.  verdict: "PASS" iff every plasmid
    row has distance 0 and every accuracies file has a median above 99.9;
    adapter-region edits never fail it (README, Acceptance criteria)."""
    adapted, c0, c1 = read_expected(expected_path)
    queries = {"plasmid": (adapted[c0:c1], c0), "adapted": (adapted, 0)}
    cons = [(p, read_consensus(p)) for p in consensus_paths]
    medians = [(p, median_accuracy(p)) for p in (accuracies_paths or [])]
    jobs = [(p, region, queries[region][0], t) for p, t in cons for region in REGIONS]
    found = scan([(q, t) for _, _, q, t in jobs], device=device)
    rows = []
    for (p, region, q, t), (distance, end) in zip(jobs, found):
        row = dict(consensus=p, region=region, expected_len=len(q), consensus_len=len(t), end=end, distance=distance)
        row.update(script(q, t, distance, end))
        row["edits"] = edits(q, t, row, queries[region][1])
        rows.append(row)
    ok = all(r["distance"] == 0 for r in rows if r["region"] == "plasmid") and \
        all(m > MIN_MEDIAN_ACCURACY for _, m in medians)
    return dict(rows=rows, medians=medians, verdict="PASS" if ok else "FAIL", adapted=adapted, core=(c0, c1))
