"""Multi-GPU pileup: reads sharded across GPUs, one global pileup.

Shards own CONTIGUOUS global read ranges in shard order (rank k holds the
k-th block of every sample's reads).  This preserves the one piece of the
reference that depends on read order: the slot layout at gaps that receive
both LEFT and RIGHT strings (processBaseString_leftIndel / _rightIndel,
mapped_paf_read_parser.py:37-72, driven in PAF first-occurrence order :292).
Everything else is an order-free integer tally.  See SURVEY.md 8(e).

Every shard runs the phases of include/mpc.h on its own reads.  Between the
phases it exchanges small per-gap / per-run arrays (no read data moves), four
collectives per step:

    after parse     OR      hasleft bitmap        (which gaps hold LEFT events)
    after index     GATHER  per-gap mixed RIGHT counts -> global run index space
    after tally     MAX     MAXR | M[:used] | RUN_R[:used] (RUN_R parked in M's
                            unused tail: one reduction), used = the runs in use
                            (G + all shards' mixed RIGHT events, read on the host
                            once per batch): longest RIGHT string at RIGHT-only
                            gaps, longest LEFT string per run, RIGHT string
                            closing each run
    after rows      SUM     rows                  (every shard's rows hold its own
                            reads' counts, odd positions included)

The depth difference array and the substitution tallies are never exchanged:
they are linear, so they reach the result through the rows SUM.  Layout and
consensus are then identical on every shard.  The protocol
is written once against an ``Exchange``: ``DistExchange`` is one shard per
process over torch.distributed (RCCL over xGMI on GPUs; gloo in the CPU
tests), ``LocalExchange`` drives several shards in one process (the CLI's
``--gpus N`` through ``pileup_sharded``, and the GPU parity tests that check
the sharded kernels bit-exactly against one GPU).

A batch with negative target starts (any shard: the plans are sized from the
totals, so every shard knows) performs six collectives.  Python's negative
wrap writes strings into odd positions, and such a position is replayed like a
gap over ALL reads' strings in global read order (mpc.h):

    after parse     GATHER  each shard's strings as records (position, global
                            read, length, kind, owner, owner's index): only the
                            records present move, their counts are read on the
                            host once per batch and cached like ``used``
    after wrap      MAX     per run of those positions: some shard's read has a
                            one-base write in it (the counts stay per shard and
                            reach the result through the rows SUM)

``wrap`` is the phase between tally and layout in which every shard sorts the
gathered records -- the same positions, runs and longest strings everywhere --
and counts its own reads' one-base writes into the runs.
"""
import numpy as np

from . import engine as eng


class LocalExchange:
    """Collectives over a list of tensors that all live in this process (one per shard)."""

    def reduce(self, ts, op):
        acc = ts[0].clone()
        for t in ts[1:]:
            t = t.to(acc.device)
            if op == "sum":
                acc += t
            elif op == "max":
                acc = acc.maximum(t)
            elif op == "or":
                acc |= t
            else:
                raise ValueError(op)
        for t in ts:
            t.copy_(acc.to(t.device))

    def gather(self, ts, outs):
        """outs[i] (shape [n_shards * k]) <- concatenation of ts in shard order."""
        import torch
        for o in outs:
            o.copy_(torch.cat([t.to(o.device) for t in ts]))

    def gatherv(self, ts, outs, counts, width):
        """outs[i][: sum(counts) * width] <- the first counts[k] * width
        elements of every ts[k], in shard order."""
        for o in outs:
            at = 0
            for t, c in zip(ts, counts):
                o[at: at + c * width].copy_(t[: c * width])
                at += c * width

    def max_int(self, xs):
        return [max(xs)] * len(xs)

    def sizes(self, ns):
        return list(ns)

    def shards(self, local):
        """(numbers of the ``local`` shards this process holds, shards in all)."""
        return list(range(local)), local


class DistExchange:
    """One shard per process over a torch.distributed process group."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        # RCCL ("nccl") works on device tensors in place; gloo (CPU tests, the
        # one-GPU rehearsal of N ranks) gets host copies of device tensors
        self.host_staged = dist.get_backend(group) != "nccl"

    def reduce(self, ts, op):
        (t,) = ts
        if self.host_staged and t.is_cuda:
            h = t.cpu()
            self.reduce([h], op)
            t.copy_(h)
            return
        d = self.dist
        if op == "sum":
            d.all_reduce(t, op=d.ReduceOp.SUM, group=self.group)
        elif op == "max":
            d.all_reduce(t, op=d.ReduceOp.MAX, group=self.group)
        elif op == "or":
            # RCCL has no bitwise reduction: gather the bitmaps, OR them as a tree
            # (a fresh output per call: one exchange may serve pipelines on several streams)
            st = self._gather_rows(t)
            k = self.world
            while k > 2:
                h = (k + 1) // 2  # rows [h, k) fold onto [0, k - h)
                st[: k - h] |= st[h:k]
                k = h
            if k == 2:
                import torch
                torch.bitwise_or(st[0], st[1], out=t)  # the last fold straight into t
            else:
                t.copy_(st[0])
        else:
            raise ValueError(op)

    def _gather_rows(self, t, out=None):
        """(world, len(t)) tensor of every rank's t, by one all_gather_into_tensor
        (straight into ``out`` when given; RCCL and gloo alike)."""
        import torch
        if out is None:
            out = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        self.dist.all_gather_into_tensor(out.view(-1), t.contiguous(), group=self.group)
        return out

    def gather(self, ts, outs):
        (t,), (o,) = ts, outs
        if self.host_staged and (t.is_cuda or o.is_cuda):
            h = self._gather_rows(t.cpu())
            o.copy_(h.view(-1))
            return
        self._gather_rows(t, o.view(self.world, -1))

    def gatherv(self, ts, outs, counts, width):
        """Parts of unequal length (``counts`` of all ranks, known on the host):
        one all-gather of the longest part's size, then every rank's valid
        head copied behind the previous one.  The bytes moved follow the
        counts, not the buffers' capacity."""
        (t,), (o,) = ts, outs
        m = max(1, max(counts)) * width
        send = t[:m]
        rows = self._gather_rows(send.cpu() if self.host_staged and send.is_cuda else send)
        at = 0
        for k, c in enumerate(counts):
            o[at: at + c * width].copy_(rows[k, : c * width])
            at += c * width

    def _ints(self, xs, op):
        import torch
        dev = "cuda" if self.dist.get_backend(self.group) == "nccl" else "cpu"
        t = torch.tensor(xs, dtype=torch.int64, device=dev)
        if op == "max":
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX, group=self.group)
            return [int(t.item())]
        parts = [torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(parts, t, group=self.group)
        return [int(p.item()) for p in parts]

    def max_int(self, xs):
        return self._ints(xs, "max")

    def sizes(self, ns):
        return self._ints(ns, "gather")

    def shards(self, local):
        assert local == 1, "one shard per process"
        return [self.rank], self.world


def split_samples(samples, n_shards):
    """Per-shard sample lists: shard k gets the k-th contiguous block of every
    sample's reads (buffers are shared, offsets sliced)."""
    out = [[] for _ in range(n_shards)]
    for s in samples:
        n = len(s["tstart"])
        cuts = [n * k // n_shards for k in range(n_shards + 1)]
        for k in range(n_shards):
            a, b = cuts[k], cuts[k + 1]
            part = dict(s)
            for key in ("cs_off", "up_off", "down_off"):
                part[key] = np.asarray(s[key])[a: b + 1]
            for key in ("tstart", "aligned", "tend"):
                if key in s:
                    part[key] = np.asarray(s[key])[a:b]
            out[k].append(part)
    return out


def shard_layout(n_reads_per_shard):
    """(read_offset, n_reads_global) of every shard: shards are contiguous, in order."""
    offs = np.concatenate([[0], np.cumsum(n_reads_per_shard)]).astype(np.int64)
    return [int(o) for o in offs[:-1]], int(offs[-1])


def wrap_counts(plans, ex):
    """Records every shard (all shards, in shard order) sends of its strings
    in wrapped odd positions.  Reads the local counts on the host (after the
    parse) and, over a process group, exchanges them: once per batch."""
    import torch
    cap = plans[0].buffer(eng.BUF_WRAP_REC, torch.int32).numel() // eng.WRAP_REC_WORDS
    local = [min(int(p.buffer(eng.BUF_STATUS, torch.int32)[eng.MPC_ST_WRAP_EVENTS].item()) & 0xFFFFFFFF, cap)
             for p in plans]
    return ex.sizes(local)


def _wrap_gather(plans, ex, counts):
    """Collective A: every shard's valid records, in shard order, behind the
    header record that tells K_woprep how many they are.  Returns the gathered
    record count."""
    import torch
    i32, W = torch.int32, eng.WRAP_REC_WORDS
    cap = plans[0].buffer(eng.BUF_WRAP_REC, i32).numel() // W
    keep, room = [], cap  # (past the list bound: dropped; the header's true total flags DE_UNSUPPORTED)
    for c in counts:
        keep.append(min(c, room))
        room -= keep[-1]
    ex.gatherv([p.buffer(eng.BUF_WRAP_REC, i32) for p in plans],
               [p.buffer(eng.BUF_WRAP_ALL, i32)[W:] for p in plans], keep, W)
    for p in plans:
        head = p.buffer(eng.BUF_WRAP_ALL, i32)[:W]
        head.zero_()
        head[:1].fill_(min(sum(counts), 2 ** 31 - 1))
    return sum(keep)


def exchange_step(plans, ex, mdf, gtf, stream=None, cache=None):
    """One global pileup over the shards in ``plans`` (all of this process's
    shards; with DistExchange exactly one).  Collective: every shard must call it.
    Returns ``used`` (the runs in use, see below).  It and the record counts of
    a batch with negative starts are properties of the shards' reads: each is
    read on the host once and kept in ``cache`` ("used", "wrap": a dict the
    caller owns, one per set of batches), so a later step over the same batches
    has no host synchronisation.  Without a cache nothing is kept."""
    import torch
    i32 = torch.int32
    cache = {} if cache is None else cache
    # negative starts anywhere in the batch (a plan attribute, the same on every
    # shard: the plans were sized from the totals): two more collectives
    wrap = bool(getattr(plans[0], "wrap", False))

    def each(phase, *args):
        for p in plans:
            p.phase(phase, stream, *args)

    each("parse")
    ex.reduce([p.buffer(eng.BUF_HASLEFT, i32) for p in plans], "or")
    if wrap:
        if cache.get("wrap") is None:
            cache["wrap"] = wrap_counts(plans, ex)
        n_wrap = _wrap_gather(plans, ex, cache["wrap"])
    each("index")
    ex.gather([p.buffer(eng.BUF_RIGHT_CNT, i32) for p in plans], [p.buffer(eng.BUF_RIGHT_CNT_ALL, i32) for p in plans])
    each("runs")
    each("tally")
    # MAXR (RIGHT-only gaps) and the USED runs of RUN_M / RUN_R: the run index
    # space is sized for every read being a mixed RIGHT event (runs_cap = global
    # reads + G: ~13 MB at C2 x 8 GPUs), the runs in use are G + all shards'
    # mixed RIGHT events (~35 k there).  One host read of that count (after the
    # gather it is on every shard), then two MAX reductions over the used parts
    # (MAXR and RUN_M are adjacent in the workspace)
    if cache.get("used") is None:
        cache["used"] = (int(plans[0].buffer(eng.BUF_MAXR, i32).numel())
                         + int(plans[0].buffer(eng.BUF_RIGHT_CNT_ALL, i32).sum()))
    used = cache["used"]
    heads, tails, parked = [], [], []
    for p in plans:
        span = p.span(eng.BUF_MAXR, eng.BUF_RUN_M, i32)
        m = p.buffer(eng.BUF_RUN_M, i32)
        moff = (m.data_ptr() - span.data_ptr()) // 4
        rr = p.buffer(eng.BUF_RUN_R, i32)[:used]
        if 2 * used <= m.numel():
            # ONE max: RUN_R[:used] parked in RUN_M's unused tail [used, 2 used)
            # (no kernel reads runs >= used; the next clear zeroes it)
            m[used: 2 * used].copy_(rr)
            heads.append(span[: moff + 2 * used])
            parked.append((m[used: 2 * used], rr))
        else:
            heads.append(span[: moff + used])
            tails.append(rr)
    ex.reduce(heads, "max")
    if tails:
        ex.reduce(tails, "max")
    for src, dst in parked:
        dst.copy_(src)
    if wrap:
        # the runs of the wrapped odd positions over all shards' strings, each
        # shard's one-base writes counted into them; whether ANY shard has one
        # in a run decides the layout (the counts themselves reach the result
        # through the rows SUM).  Runs <= 2 x the gathered strings.
        each("wrap")
        ex.reduce([p.buffer(eng.BUF_WRAP_COVER, i32)[: 2 * n_wrap + 1] for p in plans], "max")
    each("layout")
    each("rows")
    ex.reduce([p.buffer(eng.BUF_ROWS, i32) for p in plans], "sum")
    each("consensus", mdf, gtf)
    return used


class ShardedPileup:
    """Shards of one global pileup.  ``shards`` is a list of per-shard sample
    lists (every shard holds the same samples, i.e. the same references, and
    its own contiguous block of each sample's reads).

    With ``ex=None`` all shards live in this process (LocalExchange); with a
    DistExchange this process holds exactly one shard (``rank`` of the group).
    """

    def __init__(self, shards, devices, ex=None, row_cap=None, parse_cus=0):
        self.ex = ex or LocalExchange()
        ranks, n_shards = self.ex.shards(len(shards))
        # reads of every sample on every local shard: maps a shard's read index
        # back to the launch order of one GPU (data_error)
        self._counts = [[len(s["tstart"]) for s in smp] for smp in shards]
        offs, ng = shard_layout(self.ex.sizes([sum(c) for c in self._counts]))
        self.batches = [eng.Batch(smp, device=dev, read_offset=offs[r], n_reads_global=ng, shard=r,
                                  n_shards=n_shards, parse_cus=parse_cus) for smp, dev, r in zip(shards, devices, ranks)]
        # negative starts: every shard sizes its plan from the totals over all
        # shards (mpc.h neg_reads), so all of them plan the same kernels and
        # the same collectives, also those holding no negative start
        neg = sum(self.ex.sizes([b.neg_reads for b in self.batches]))
        neg_cs = sum(self.ex.sizes([b.neg_cs_bytes for b in self.batches]))
        for b in self.batches:
            b.neg_reads, b.neg_cs_bytes = neg, neg_cs
        cap = row_cap or max(b.row_estimate() for b in self.batches)
        cap = self.ex.max_int([cap] * len(shards))[0]
        self.plans = [eng.Plan(b, cap) for b in self.batches]
        self._sized = False
        # the once-per-batch host reads of exchange_step (the runs in use, the
        # record counts of the wrapped odd positions): valid for THESE batches
        # only -- the batches are fixed for the object's lifetime
        # (mpc_plan_set_input is never called on them)
        self._cache = {}

    # bench.py interface (one local shard)
    @property
    def batch(self):
        return self.batches[0]

    @property
    def plan(self):
        return self.plans[0]

    def step(self, mdf, gtf, stream=None):
        # the cached counts depend only on the reads: read back once, reused by
        # later steps over the same batches (no host sync inside a step)
        exchange_step(self.plans, self.ex, mdf, gtf, stream, self._cache)
        if not self._sized:
            # the layout (and so the row count) is identical on every shard
            st = self.plans[0].status()
            flags = self.ex.max_int([eng.status_error(st)[0]] * len(self.plans))[0]
            need = eng.replan_rows(st, alone=False, flags=flags)
            if need:
                self.plans = [eng.Plan(b, need) for b in self.batches]
                del self._cache["used"]  # (read again from the new plans; the record counts stay)
                exchange_step(self.plans, self.ex, mdf, gtf, stream, self._cache)
            self._sized = True

    def check(self):
        for p in self.plans:
            p.check()

    def data_error(self):
        """(OR of all local shards' MPC_DE_* flags, read index) -- the index
        one GPU would report for the same samples: every shard's first
        offending read mapped back through the contiguous split to the launch
        order (sample by sample, reads in order), the smallest of them; None
        when no shard names a read.  (0, None): no error."""
        flags, first = 0, None
        totals = [sum(c[s] for c in self._counts) for s in range(len(self._counts[0]))]
        for k, p in enumerate(self.plans):
            f, r = eng.status_error(p.status())
            flags |= f
            if not f or r == 0xFFFFFFFF:
                continue
            s, r = eng.locate_read(r, self._counts[k])
            g = sum(totals[:s]) + sum(self._counts[j][s] for j in range(k)) + r
            first = g if first is None else min(first, g)
        return flags, first

    def fetch(self):
        return self.plans[0].fetch()


def shard_count(n_devices, n_reads):
    """Shards a group of ``n_reads`` reads is split into over ``n_devices``."""
    return max(1, min(int(n_devices), int(n_reads)))


def assign(n_groups, n_gpus, device=0, visible=1):
    """How ``--gpus N`` spreads job groups: a pure function of its arguments.
    The devices are ``device + k`` (k < N) modulo the visible ones.  With at
    least N groups, group i goes to worker ``i % N`` (one device each, no
    collective): returns ("partition", devices, worker of every group).
    With fewer, every group is read-sharded over all N devices:
    ("shard", devices, None)."""
    n, visible = max(1, int(n_gpus)), max(1, int(visible))
    devices = [(int(device) + k) % visible for k in range(n)]
    if n_groups >= n:
        return "partition", devices, [i % n for i in range(n_groups)]
    return "shard", devices, None


def pileup_sharded(samples, mdf, gtf, devices):
    """engine.pileup over the reads split into contiguous shards, one per
    entry of ``devices`` (entries may repeat: several shards on one device),
    at most one shard per read.  Same result, same DataError (flags of all
    shards, the read index in the launch order of one GPU)."""
    import torch
    k = shard_count(len(devices), sum(len(s["tstart"]) for s in samples))
    if k == 1:
        return eng.pileup(samples, mdf, gtf, devices[0])
    sp = ShardedPileup(split_samples(samples, k), list(devices[:k]))
    sp.step(mdf, gtf)
    flags, first = sp.data_error()
    if flags:
        raise eng.DataError(flags, 0xFFFFFFFF if first is None else first)
    res = sp.fetch()
    for d in set(devices[:k]):
        torch.cuda.synchronize(d)
    return res
