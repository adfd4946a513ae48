"""handoff: the alignments of align.py handed to the pileup of engine.py in
memory -- no PAF text, no second pass over the reads (include/mpc_align.h "the
handoff to the pileup"; DESIGN.md "reads_consensus").

Per trace launch of align.Launches, on the launch's own tensors:

  sizes   one int64[8] row per read {kept, cs_len, up_len, down_len, tstart,
          tend, n_eq, n_ops} (K_acslen, or mpc_align_cs_sizes_host)
  places  the three exclusive sums of the lengths, behind what the target's
          Pile holds already (numpy, host: the planner needs the offsets anyway)
  write   "Z:" + cs, the upstream and the downstream flank of every kept read at
          its place (K_acswrite, or mpc_align_cs_write_host)

A Pile keeps one target's pileup inputs across launches and batches: on a GPU
three growing uint8 tensors that engine.Batch.from_device takes as they are, on
the host (device="cpu": the checker of the kernels) three numpy arrays.

reads_consensus.py is the tool; ``consensus`` below is all of it but the
command line.  The domain it accepts, and refuses outside of, is the one in
which its outputs equal align_reads followed by mapped_paf_read_parser: see
``check_kept``.
"""
import numpy as np

from . import _native, align
from .engine import CS_PAD, FLANK_PAD  # readable bytes behind the cs / the flanks (mpc.h)

SIZE_FIELDS = ("kept", "cs_len", "up_len", "down_len", "tstart", "tend", "n_eq", "n_ops")
_RC_LETTERS = b"ACGTNacgtn"  # what the parser's reverse complement accepts (ingest.py read_flanks)
_NAME_BYTES = bytes(range(0x21, 0x7f))


class HandoffError(align.AlignError):
    """Input outside the domain in which the handoff equals the two commands it replaces."""


# ---- the two calls, one launch at a time ----------------------------------------

def cs_sizes(jobs, out, runs, seq_bytes, device=0, threads=0, tensors=None):
    """sizes int64 [J, 8] of one launch's traced reads.  ``tensors``: the launch's
    device tensors (align.trace's device_tensors), else the host arrays are
    uploaded; it then also receives ``sizes``."""
    jobs = np.ascontiguousarray(jobs, np.int64).reshape(-1, 8)
    J = len(jobs)
    sizes = np.zeros((J, 8), np.int64)
    if J == 0:
        return sizes
    out = np.ascontiguousarray(out, np.int32)
    runs = np.ascontiguousarray(runs, np.int32)
    if device == "cpu":
        L = align.host_lib()
        _native.host_check(L, "align", align.AlignError, L.mpc_align_cs_sizes_host(
            jobs.ctypes.data, J, int(seq_bytes), out.ctypes.data, runs.ctypes.data, len(runs), sizes.ctypes.data, threads))
        return sizes
    with _native.Device(device) as d:
        t = tensors if tensors is not None else {}
        _upload(d, t, jobs=jobs, out=out, runs=runs)
        t["sizes"] = d.torch.zeros(8 * J, dtype=d.torch.int64, device=d.dev)
        d.check(d.lib.mpc_align_cs_sizes(t["jobs"].data_ptr(), J, int(seq_bytes), t["out"].data_ptr(), t["runs"].data_ptr(),
                                         _count(t["runs"], 4), t["sizes"].data_ptr(), d.stream), refused=align.AlignError)
        t["sizes_host"] = t["sizes"].cpu().numpy().reshape(J, 8)
        return t["sizes_host"]


def places(sizes, base=(0, 0, 0)):
    """(place int64 [J, 3], ends): every read's {cs_off, up_off, down_off} behind
    ``base``, back to back in job order, and the three ends."""
    lens = np.asarray(sizes, np.int64).reshape(-1, 8)[:, 1:4]
    ends = np.cumsum(lens, axis=0) + np.asarray(base, np.int64)
    place = np.ascontiguousarray(ends - lens)
    return place, tuple(int(x) for x in (ends[-1] if len(ends) else base))


def cs_write(seq, jobs, out, runs, sizes, place, cs, up, down, device=0, threads=0, tensors=None, caps=None):
    """Writes one launch's kept reads into cs / up / down (numpy uint8 arrays for
    device="cpu", uint8 tensors on the device else) at ``place``.  ``caps``:
    the bytes of each buffer the launch may use (default: all of it)."""
    jobs = np.ascontiguousarray(jobs, np.int64).reshape(-1, 8)
    J = len(jobs)
    if J == 0:
        return
    given = sizes
    sizes = np.ascontiguousarray(sizes, np.int64)
    place = np.ascontiguousarray(place, np.int64)
    if device == "cpu":
        L = align.host_lib()
        out = np.ascontiguousarray(out, np.int32)
        runs = np.ascontiguousarray(runs, np.int32)
        caps = caps or (len(cs), len(up), len(down))
        _native.host_check(L, "align", align.AlignError, L.mpc_align_cs_write_host(
            seq.ctypes.data, seq.nbytes, jobs.ctypes.data, J, out.ctypes.data, runs.ctypes.data, len(runs),
            sizes.ctypes.data, place.ctypes.data, cs.ctypes.data, caps[0], up.ctypes.data, caps[1], down.ctypes.data,
            caps[2], threads))
        return
    with _native.Device(device) as d:
        t = tensors if tensors is not None else {}
        _upload(d, t, seq=seq, jobs=jobs, out=np.ascontiguousarray(out, np.int32), runs=np.ascontiguousarray(runs, np.int32))
        caps = caps or (cs.numel(), up.numel(), down.numel())
        # (the rows K_acslen left on the device, when the caller hands on what it read back from them)
        d_sizes = t["sizes"] if t.get("sizes") is not None and t.get("sizes_host") is given else d.put(sizes)
        d_place = d.put(place)
        d_status = d.torch.zeros(J, dtype=d.torch.int32, device=d.dev)
        d.check(d.lib.mpc_align_cs_write(
            t["seq"].data_ptr(), seq.nbytes, t["jobs"].data_ptr(), J,
            t["out"].data_ptr(), t["runs"].data_ptr(), _count(t["runs"], 4), d_sizes.data_ptr(), d_place.data_ptr(),
            cs.data_ptr(), caps[0], up.data_ptr(), caps[1], down.data_ptr(), caps[2], d_status.data_ptr(), d.stream),
            refused=align.AlignError)


def _upload(d, t, **arrays):
    """The host arrays a launch's tensor dict lacks, uploaded into it."""
    for key, a in arrays.items():
        if t.get(key) is None:
            t[key] = d.put(a)


def _count(tensor, item):
    """Elements of ``item`` bytes a launch tensor holds (uploads are uint8 views of any type)."""
    return tensor.numel() * tensor.element_size() // item


# ---- one target's pileup inputs, accumulated --------------------------------------

class Pile:
    """cs, up and down of every kept read of one target, in read order, with
    their host offsets and tstart.  ``add`` takes one traced launch."""

    def __init__(self, device=0):
        self.device = device
        self.buf = [None, None, None]  # cs, up, down: numpy arrays (cpu) or tensors
        self.used = (0, 0, 0)
        self.lens, self.tstart = [], []  # per launch: int64 [kept, 3], int64 [kept]

    def _room(self, ends):
        """Buffers that hold ``ends`` bytes plus the readable room behind them
        (doubling: the bytes written so far are copied once per growth)."""
        for k, (end, pad) in enumerate(zip(ends, (CS_PAD, FLANK_PAD, FLANK_PAD))):
            have = 0 if self.buf[k] is None else len(self.buf[k])
            if have >= end + pad:
                continue
            size = max(end + pad, 2 * have, 1 << 12)
            if self.device == "cpu":
                new = np.zeros(size, np.uint8)
            else:
                with _native.Device(self.device) as d:
                    new = d.torch.empty(size, dtype=d.torch.uint8, device=d.dev)
            if self.used[k]:
                new[: self.used[k]] = self.buf[k][: self.used[k]]
            self.buf[k] = new

    def add(self, seq, jobs, out, runs, threads=0, tensors=None):
        """One launch's reads behind what the pile holds; returns their size rows."""
        sizes = cs_sizes(jobs, out, runs, seq.nbytes, self.device, threads, tensors)
        place, ends = places(sizes, self.used)
        self._room(ends)
        cs, up, down = self.buf
        caps = (len(cs) - CS_PAD, len(up) - FLANK_PAD, len(down) - FLANK_PAD)
        cs_write(seq, jobs, out, runs, sizes, place, cs, up, down, self.device, threads, tensors, caps)
        self.used = ends
        kept = sizes[:, 0] == 1
        self.lens.append(sizes[kept, 1:4])
        self.tstart.append(sizes[kept, 4])
        return sizes

    @property
    def n_reads(self):
        return sum(len(t) for t in self.tstart)

    def sample(self, ref):
        """The packed sample of ``ref`` (uint8, upper-cased: ingest.read_reference)
        and the pile: what ingest.pack_sample gives for the PAF of these reads --
        host arrays for device="cpu", device tensors (engine.Batch.from_device) else."""
        self._room(self.used)
        lens = np.concatenate(self.lens) if self.lens else np.zeros((0, 3), np.int64)
        off = np.concatenate([np.zeros((1, 3), np.int64), np.cumsum(lens, axis=0)]).astype(np.int64)
        cs, up, down = self.buf
        if self.device == "cpu":
            cs, up, down = (b[:n] for b, n in zip(self.buf, self.used))
        return dict(ref=ref, cs=cs, cs_off=np.ascontiguousarray(off[:, 0]),
                    tstart=np.concatenate(self.tstart) if self.tstart else np.zeros(0, np.int64),
                    up=up, up_off=np.ascontiguousarray(off[:, 1]), down=down, down_off=np.ascontiguousarray(off[:, 2]))


# ---- the domain --------------------------------------------------------------------

def check_names(records, seen):
    """Read names are unique over the whole file (``seen``: the names so far).
    With duplicates the parser joins the first alignment with the last sequence."""
    for rec in records:
        if rec[0] in seen:
            raise HandoffError("read {!r}: the name occurs twice in the reads file".format(_text(rec[0])))
        seen.add(rec[0])


def check_kept(name, seq, header, minus):
    """What must hold of a read that gets a PAF line for the parser to find it
    and to cut its flanks as the handoff does."""
    if not name or name.startswith(b"cs:") or name.translate(None, _NAME_BYTES):
        raise HandoffError("read {!r}: a name that is empty, starts with 'cs:' or holds a byte outside printable "
                           "ASCII".format(_text(name)))
    if header != name:
        raise HandoffError("read {!r}: its header line holds more than the name ({!r}): the parser looks reads up by "
                           "the whole line".format(_text(name), _text(header)))
    if minus and seq.translate(None, _RC_LETTERS):
        raise HandoffError("read {!r}: mapped to '-' and holds a letter other than A C G T N, which the parser's "
                           "reverse complement refuses".format(_text(name)))


def _text(b):
    return b.decode(errors="replace")


# ---- reads -> alignment -> pileup inputs, one batch at a time ------------------------

class Target:
    """One assembly: its name and sequence as align_reads takes them, the
    reference as the pileup takes it, its Pile and its summary counts."""

    def __init__(self, path, device):
        from . import ingest
        self.path = path
        self.name, self.seq = align.read_target(path)
        self.ref = np.frombuffer(ingest.transcode_ref(ingest.read_reference(path)), np.uint8)
        self.pile = Pile(device)
        self.summary = dict.fromkeys(align.SUMMARY_FIELDS, 0)


def domain_flags(records):
    """(plain, rc_ok) per record of a batch, once for all targets: the name and
    the header line pass check_kept; the sequence holds only A C G T N."""
    plain = np.fromiter((bool(n) and h == n and not n.startswith(b"cs:") and not n.translate(None, _NAME_BYTES)
                         for n, _, h in records), bool, len(records))
    rc_ok = np.fromiter((not s.translate(None, _RC_LETTERS) for _, s, _ in records), bool, len(records))
    return plain, rc_ok


def feed(target, records, device=0, max_error=0.2, workspace_bytes=align.DEFAULT_WORKSPACE, threads=0, workspace=None,
         paf=None, flags=None):
    """One batch of (name, sequence, header) records against one target: the
    launches of align.BatchLoop, each handed to the target's pile.  ``paf``: a
    function that receives the batch's PAF lines, rendered on the host as
    align_reads does; ``flags``: domain_flags(records) when the caller has
    them.  Returns the number of launches."""
    plain, rc_ok = flags if flags is not None else domain_flags(records)
    loop = align.BatchLoop(target.seq, records, device, max_error, workspace_bytes, threads, workspace,
                           keep_device=device != "cpu")
    pk, rec_of = loop.pk, np.asarray(loop.keep, np.int64)
    for reads, jobs, out, runs, tensors in loop:
        sizes = target.pile.add(pk.seq, jobs, out, runs, threads, tensors)
        wrote = sizes[:, 0] == 1
        minus = loop.count(reads, wrote)
        rec = rec_of[reads]
        for k in np.nonzero(wrote & ~(plain[rec] & (rc_ok[rec] | ~minus)))[0][:1]:  # the first read outside the domain
            check_kept(*records[rec[k]][:3], minus=bool(minus[k]))
        if paf is not None:
            text, line_len = align.render(pk.seq, jobs, loop.plan[reads, 0], out, runs, [loop.names[r] for r in reads],
                                          target.name, threads)
            assert np.array_equal(line_len > 0, wrote)
            paf(text)
    for key, v in loop.counts.items():
        target.summary[key] += v
    return loop.launches


def collect(ref_paths, reads_path, device=0, max_error=0.2, workspace_bytes=align.DEFAULT_WORKSPACE,
            batch_bases=align.DEFAULT_BATCH_BASES, threads=0, paf=None):
    """Every target of ``ref_paths`` with the whole reads file fed to it, one pass
    over the reads.  ``paf``: receives the first target's PAF lines.  Returns
    (targets, launches of the first target)."""
    if not max_error >= 0:
        raise align.AlignError("max_error must be >= 0")
    targets = [Target(p, device) for p in ref_paths]
    seen, ws, launches = set(), {}, 0
    for batch in align.read_batches(reads_path, batch_bases, headers=True):
        check_names(batch, seen)
        flags = domain_flags(batch)
        for k, t in enumerate(targets):
            n = feed(t, batch, device, max_error, workspace_bytes, threads, ws, paf if k == 0 else None, flags)
            launches += n if k == 0 else 0
    return targets, launches


def consensus(ref_paths, reads_path, mdf, gtf, device=0, **kw):
    """The calls of every target (engine.Plan.fetch's dicts), all targets as the
    samples of ONE pileup launch, and the targets: (results, targets)."""
    from . import engine
    targets, _ = collect(ref_paths, reads_path, device, **kw)
    batch = engine.Batch.from_device([t.pile.sample(t.ref) for t in targets], device=device)
    return engine.pileup_batch(batch, mdf, gtf), targets
