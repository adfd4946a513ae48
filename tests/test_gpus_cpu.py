"""``--gpus N`` and the sharded negative starts, the parts that need no GPU.

  * dist.assign / dist.shard_count: which device every job group or shard
    goes to is a pure function of (groups, N, --device, visible devices)
  * dist.exchange_step around stand-in plans (the approach of
    test_dist_cpu.py): a batch without negative starts performs exactly the
    four collectives it always did, in the same order; a batch with negative
    starts performs six, gathers the shards' records in shard order behind
    the header, and reads the record counts on the host once per batch
"""
import importlib

import numpy as np
import torch

import test_dist_cpu as tdc

G = tdc.G
CAP = 40  # list capacity of the stand-in plans (records)


def _mod():
    return importlib.import_module("minion-plasmid-consensus_amd.dist"), importlib.import_module(
        "minion-plasmid-consensus_amd.engine")


def test_assign_round_robin_and_modulo():
    dist, _ = _mod()
    # at least N groups: dealt round-robin, one worker per device
    assert dist.assign(4, 2, 0, 8) == ("partition", [0, 1], [0, 1, 0, 1])
    assert dist.assign(5, 3, 2, 8) == ("partition", [2, 3, 4], [0, 1, 2, 0, 1])
    assert dist.assign(2, 2, 0, 2) == ("partition", [0, 1], [0, 1])
    # the devices wrap modulo the visible ones (a one-GPU box rehearses the path)
    assert dist.assign(4, 2, 0, 1) == ("partition", [0, 0], [0, 1, 0, 1])
    assert dist.assign(3, 3, 6, 8) == ("partition", [6, 7, 0], [0, 1, 2])
    # fewer groups than GPUs: every group sharded over all of them
    assert dist.assign(1, 2, 0, 1) == ("shard", [0, 0], None)
    assert dist.assign(4, 8, 1, 4) == ("shard", [1, 2, 3, 0, 1, 2, 3, 0], None)
    # N = 1: one worker on --device
    assert dist.assign(3, 1, 5, 8) == ("partition", [5], [0, 0, 0])


def test_shard_count():
    dist, _ = _mod()
    assert dist.shard_count(2, 1000) == 2
    assert dist.shard_count(8, 3) == 3  # never more shards than reads
    assert dist.shard_count(8, 1) == 1
    assert dist.shard_count(4, 0) == 1  # at least one


class Counting:
    """An exchange that records every collective before handing it on."""

    def __init__(self):
        dist, _ = _mod()
        self.ex = dist.LocalExchange()
        self.ops, self.host = [], []

    def reduce(self, ts, op):
        self.ops.append((op, int(ts[0].numel())))
        self.ex.reduce(ts, op)

    def gather(self, ts, outs):
        self.ops.append(("gather", int(ts[0].numel())))
        self.ex.gather(ts, outs)

    def gatherv(self, ts, outs, counts, width):
        self.ops.append(("gatherv", tuple(counts)))
        self.ex.gatherv(ts, outs, counts, width)

    def sizes(self, ns):
        self.host.append(list(ns))
        return self.ex.sizes(ns)

    def max_int(self, xs):
        return self.ex.max_int(xs)


class WrapPlan(tdc.FakePlan):
    """A stand-in shard of a batch with negative starts: ``events`` strings of
    its own in wrapped odd positions."""

    def __init__(self, shard, n_shards, events):
        super().__init__(shard, n_shards, mlen=3 * G)
        _, eng = _mod()
        W = eng.WRAP_REC_WORDS
        self.wrap = True
        st = torch.zeros(8, dtype=torch.int32)
        st[eng.MPC_ST_WRAP_EVENTS] = events
        rec = torch.full((CAP * W,), -1, dtype=torch.int32)
        rec[: events * W] = 1000 * shard + torch.arange(events * W, dtype=torch.int32)
        self.buf.update({eng.BUF_STATUS: st, eng.BUF_WRAP_REC: rec,
                         eng.BUF_WRAP_ALL: torch.full(((CAP + 1) * W,), -7, dtype=torch.int32),
                         eng.BUF_WRAP_COVER: torch.zeros(2 * CAP + 1, dtype=torch.int32)})
        self.buf[eng.BUF_WRAP_COVER][shard] = 1  # run `shard` covered by this shard only


def test_four_collectives_without_negative_starts():
    dist, _ = _mod()
    plans = [tdc.FakePlan(k, 3, 3 * G) for k in range(3)]
    ex = Counting()
    dist.exchange_step(plans, ex, 0.1, 5.0, cache={})
    assert [op for op, _ in ex.ops] == ["or", "gather", "max", "sum"]
    assert ex.host == []
    for p in plans:
        assert [x[0] for x in p.log] == tdc.PHASES
        assert tdc._check(p, tdc.expected(3, 3 * G))


def test_six_collectives_with_negative_starts():
    dist, eng = _mod()
    W = eng.WRAP_REC_WORDS
    events = [5, 0, 3]  # (a shard without a string of its own still takes part)
    plans = [WrapPlan(k, 3, e) for k, e in enumerate(events)]
    ex, cache = Counting(), {}
    dist.exchange_step(plans, ex, 0.1, 5.0, cache=cache)
    assert [op for op, _ in ex.ops] == ["or", "gatherv", "gather", "max", "max", "sum"]
    assert ex.ops[1] == ("gatherv", (5, 0, 3))       # the events present, not the capacity
    assert ex.ops[4] == ("max", 2 * sum(events) + 1)  # the cover flags of the runs in use
    assert ex.host == [events] and cache["wrap"] == events
    for p in plans:
        phases = [x[0] for x in p.log]
        assert phases == tdc.PHASES[:4] + ["wrap"] + tdc.PHASES[4:]
        al = p.buf[eng.BUF_WRAP_ALL]
        assert al[:W].tolist() == [sum(events)] + [0] * (W - 1)
        got = al[W: (1 + sum(events)) * W]
        exp = torch.cat([1000 * k + torch.arange(e * W, dtype=torch.int32) for k, e in enumerate(events)])
        assert torch.equal(got, exp)
        assert (al[(1 + sum(events)) * W:] == -7).all()  # nothing past the gathered records is touched
        assert p.buf[eng.BUF_WRAP_COVER][:4].tolist() == [1, 1, 1, 0]  # MAX over the shards
    # a second step over the same batches: the cached counts, no host exchange
    dist.exchange_step(plans, ex, 0.5, 2.5, cache=cache)
    assert ex.host == [events]
    assert [op for op, _ in ex.ops[6:]] == ["or", "gatherv", "gather", "max", "max", "sum"]


def test_records_past_the_list_bound_are_dropped():
    """More records than the list holds: the copies stay inside the buffer and
    the header carries the true total (K_woprep flags MPC_DE_UNSUPPORTED)."""
    dist, eng = _mod()
    W = eng.WRAP_REC_WORDS
    plans = [WrapPlan(k, 2, CAP - 2) for k in range(2)]
    ex = Counting()
    dist.exchange_step(plans, ex, 0.1, 5.0)
    assert ex.ops[1] == ("gatherv", (CAP - 2, 2))
    assert int(plans[0].buf[eng.BUF_WRAP_ALL][0]) == 2 * (CAP - 2)
    assert plans[0].buf[eng.BUF_WRAP_ALL].numel() == (CAP + 1) * W
    assert np.array_equal(plans[0].buf[eng.BUF_WRAP_ALL].numpy(), plans[1].buf[eng.BUF_WRAP_ALL].numpy())


def _status(eng, flags, rows_needed=1000):
    st = np.zeros(8, np.uint32)
    st[eng.MPC_ST_FLAGS], st[eng.MPC_ST_ROWS_NEEDED], st[eng.MPC_ST_FIRST_READ] = flags, rows_needed, 0xFFFFFFFF
    return st


def test_replan_rows_two_conditions():
    """engine.replan_rows: the rows needed + 16 when the capacity flag asks for
    a re-plan; "alone" (one GPU) only when no other flag is set, "any" (the
    sharded step) whenever the capacity bit is."""
    _, eng = _mod()
    cap, key = eng.DE_CAPACITY, eng.DE_KEY
    for flags, alone, any_ in ((0, None, None), (cap, 1016, 1016), (cap | key, None, 1016), (key, None, None)):
        assert eng.replan_rows(_status(eng, flags), alone=True) == alone, flags
        assert eng.replan_rows(_status(eng, flags), alone=False) == any_, flags
    # the flags the ranks agreed on decide, the rows come from the status words
    assert eng.replan_rows(_status(eng, 0, 77), alone=False, flags=cap) == 93
    assert eng.replan_rows(_status(eng, cap), alone=False, flags=0) is None


def test_locate_read():
    _, eng = _mod()
    # 3: the empty group is skipped; 9: past the end, the last group takes it
    for r, exp in ((0, (0, 0)), (2, (0, 2)), (3, (2, 0)), (6, (2, 3)), (9, (2, 6))):
        assert eng.locate_read(r, [3, 0, 4]) == exp, r
    for r in (0, 4, 5, 1000):
        assert eng.locate_read(r, [5]) == (0, r)


def test_used_is_cached_with_the_record_counts():
    """The runs in use are read once per set of batches: a step with a cache
    leaves them in cache["used"], and the next step does not read them again
    (RIGHT_CNT_ALL poisoned in between: a second read would change the lengths
    of the MAX reductions)."""
    dist, eng = _mod()
    plans = [tdc.FakePlan(k, 3, 3 * G) for k in range(3)]
    ex, cache = Counting(), {}
    used = dist.exchange_step(plans, ex, 0.1, 5.0, cache=cache)
    assert used == tdc.expected(3, 3 * G)[2] and cache == {"used": used}
    first = list(ex.ops)
    for p in plans:  # (RIGHT_CNT too: the step's own gather rewrites RIGHT_CNT_ALL from it)
        p.buf[eng.BUF_RIGHT_CNT_ALL].fill_(1000)
        p.buf[eng.BUF_RIGHT_CNT].fill_(1000)
    assert dist.exchange_step(plans, ex, 0.1, 5.0, cache=cache) == used and cache == {"used": used}
    assert ex.ops[len(first):] == first
    assert int(plans[0].buf[eng.BUF_RIGHT_CNT_ALL].sum()) == 1000 * 3 * G  # (the poison was there when "used" was due)
    # without a cache nothing is kept: the poisoned counts are read
    assert dist.exchange_step(plans, ex, 0.1, 5.0) == G + 1000 * 3 * G
