"""Negative target starts under read sharding (dist.py, six collectives).

A wrapped odd position is replayed like a gap: its runs are split at its RIGHT
strings in GLOBAL read order, so every shard must derive the same positions,
runs and slot layout from all shards' strings, and tally only its own reads'
bytes onto rows that are summed afterwards.  Every shard's calls are compared
with the C oracle of the unsharded sample, call by call.
"""
import importlib
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import depth_util as du
import neg_util

pytestmark = pytest.mark.gpu

SETTINGS = ((-1.0, 1.0), (0.1, 5.0), (0.5, 2.5))


def _dist():
    return importlib.import_module("minion-plasmid-consensus_amd.dist")


def _random_samples(pkg):
    """The shapes of test_gpu_parity.py::test_negative_starts_random, seed 5."""
    syn = pkg.synth.Synth(n=700, n_reads=600, profile="indel", seed=5, frac_partial=0.3, antisense=False)
    return [neg_util.neg_sample(5), neg_util.neg_sample(105, n=500, n_reads=1500, frac_neg=0.06), syn.sample(0)]


@pytest.fixture(scope="module")
def random_case(pkg):
    """(samples, oracle calls per setting): computed once, shared, never changed."""
    samples = _random_samples(pkg)
    exp = {st: [du.oracle_one(s, *st) for s in samples] for st in SETTINGS}
    return samples, exp


@pytest.mark.parametrize("k", [2, 3, 4])
def test_sharded_negative_starts(pkg, random_case, k):
    """Every shard of every split holds negative starts, and the batch writes
    upstream, '+' and downstream strings: positions collect strings across
    the seams.  Three settings stepped on the same object (the second and
    third step reuse the cached record counts)."""
    dist, eng = _dist(), pkg.engine
    samples, exp = random_case
    shards = dist.split_samples(samples, k)
    for smp in shards:
        assert sum(int((np.asarray(s["tstart"]) < 0).sum()) for s in smp) > 0
    assert all(x > 0 for x in np.sum([neg_util.wrapped_strings(s) for s in samples[:2]], axis=0))
    sp = dist.ShardedPileup(shards, [0] * k)
    assert all(p.wrap for p in sp.plans)
    for st in SETTINGS:
        sp.step(*st)
        sp.check()
        pos = [int(p.status()[eng.MPC_ST_WRAP_POS]) for p in sp.plans]
        assert pos[0] > 0 and pos == [pos[0]] * k, pos
        for r, plan in enumerate(sp.plans):
            for s, (got, e) in enumerate(zip(plan.fetch(), exp[st])):
                du.compare(got, e, ("wrap sharded", k, r, s, st))
    assert sp._cache["wrap"] is not None and len(sp._cache["wrap"]) == k


def test_repeated_step_is_capturable(pkg):
    """Once the record counts are cached a step has no host synchronisation:
    it is captured into a HIP graph (a host read during capture would raise)
    and the replay, after a step with other settings, gives the oracle's calls
    on both shards."""
    import torch
    dist = _dist()
    smp = neg_util.neg_sample(5, n_reads=400)
    sp = dist.ShardedPileup(dist.split_samples([smp], 2), [0, 0])
    graph, cap = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(cap):
        sp.step(0.1, 5.0)  # sizes the rows, reads and caches the counts
        cap.synchronize()
        with torch.cuda.graph(graph, stream=cap):
            sp.step(0.1, 5.0)
    torch.cuda.synchronize()
    sp.step(-1.0, 1.0)  # so that the replay has to rewrite every output
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    sp.check()
    exp = du.oracle_one(smp, 0.1, 5.0)
    for r, plan in enumerate(sp.plans):
        du.compare(plan.fetch()[0], exp, ("wrap graph", r))
    del graph


def _permuted(smp, order):
    """The sample with its reads in another order."""
    def take(buf, off):
        parts = [bytes(buf[off[r]: off[r + 1]]) for r in order]
        o = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
        return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), o
    out = dict(smp)
    out["cs"], out["cs_off"] = take(smp["cs"], smp["cs_off"])
    out["up"], out["up_off"] = take(smp["up"], smp["up_off"])
    out["down"], out["down_off"] = take(smp["down"], smp["down_off"])
    out["tstart"] = np.asarray(smp["tstart"])[order]
    out["aligned"] = np.asarray(smp["aligned"])[order]
    return out


@pytest.mark.parametrize("where", ["first", "last"])
def test_seams_with_shards_without_negative_starts(pkg, where):
    """All negative-start reads first / last, three shards: some shards own no
    negative start (an empty record list) yet their reads cover the wrapped
    positions -- the cover flag MAX and the ranks without strings."""
    dist = _dist()
    base = neg_util.neg_sample(5)
    neg = np.asarray(base["tstart"]) < 0
    a, b = np.nonzero(neg)[0], np.nonzero(~neg)[0]
    smp = _permuted(base, np.concatenate([a, b] if where == "first" else [b, a]))
    shards = dist.split_samples([smp], 3)
    negs = [int((np.asarray(s[0]["tstart"]) < 0).sum()) for s in shards]
    assert negs.count(0) == 2, negs
    sp = dist.ShardedPileup(shards, [0] * 3)
    for st in ((-1.0, 1.0), (0.1, 5.0)):
        exp = du.oracle_one(smp, *st)
        sp.step(*st)
        sp.check()
        for r, plan in enumerate(sp.plans):
            du.compare(plan.fetch()[0], exp, ("seam", where, r, st))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch
        import torch.distributed as tdist
        torch.cuda.set_device(0)
        tdist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            dmod = importlib.import_module("minion-plasmid-consensus_amd.dist")
            smp = neg_util.neg_sample(5, n_reads=400)
            mine = dmod.split_samples([smp], world)[rank]
            sp = dmod.ShardedPileup([mine], [0], ex=dmod.DistExchange())
            out = []
            for mdf, gtf in SETTINGS[:2]:
                sp.step(mdf, gtf)
                sp.check()
                out.append([dict(r) for r in sp.fetch()])
            q.put((rank, out, int((np.asarray(mine[0]["tstart"]) < 0).sum()), None))
        finally:
            tdist.destroy_process_group()
    except Exception as e:  # reported to the parent
        import traceback
        q.put((rank, None, 0, traceback.format_exc() + repr(e)))


@pytest.mark.timeout(300)
def test_process_group_unequal_parts(pkg):
    """World size 2 over gloo on cuda:0 (DistExchange, host-staged): the ranks
    hold different numbers of negative starts, so the gathered parts are
    unequal; both ranks end with the oracle's calls."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda x: x[0])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank, _, _, err in res:
        assert err is None, (rank, err)
    for p in procs:
        assert p.exitcode == 0
    assert [n for _, _, n, _ in res] == [14, 9]
    smp = neg_util.neg_sample(5, n_reads=400)
    for rank, out, _, _ in res:
        for st, got in zip(SETTINGS[:2], out):
            du.compare(got[0], du.oracle_one(smp, *st), ("wrap pg", rank, st))


def _plain_sample(n_reads, bad_read):
    """Reads of 40 matches with a 2-base insertion; read ``bad_read`` inserts a base outside ACGT."""
    rng = np.random.default_rng(11)
    ref = rng.choice(neg_util.ACGT, 300)
    cs = [b"Z::20+%s:20" % (b"an" if r == bad_read else b"ac") for r in range(n_reads)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
    z = np.zeros(n_reads + 1, np.int64)
    return dict(ref=ref.copy(), cs=np.frombuffer(b"".join(cs), dtype=np.uint8).copy(), cs_off=off,
                tstart=rng.integers(0, 250, n_reads).astype(np.int64), up=np.zeros(0, np.uint8), up_off=z,
                down=np.zeros(0, np.uint8), down_off=z.copy(), aligned=np.zeros(n_reads, np.int64))


def test_error_index_is_the_one_gpu_index(pkg):
    """A data error in the second shard: pileup_sharded raises DataError with
    the flags and the launch-order read index engine.pileup reports."""
    dist, eng = _dist(), pkg.engine
    other = _plain_sample(50, -1)
    smp = _plain_sample(200, 137)
    with pytest.raises(eng.DataError) as one:
        eng.pileup([other, smp], -1.0, 1.0)
    assert one.value.flags & eng.DE_KEY and one.value.read == 50 + 137
    with pytest.raises(eng.DataError) as two:
        dist.pileup_sharded([other, smp], -1.0, 1.0, [0, 0])
    assert (two.value.flags, two.value.read) == (one.value.flags, one.value.read)


@pytest.fixture(scope="module")
def small_case(pkg):
    """(sample, oracle calls, engine.pileup's calls) at (0.1, 5.0): 240 bases,
    400 reads with insertions and negative starts; computed once, never changed."""
    smp = neg_util.neg_sample(5, n_reads=400)
    return smp, du.oracle_one(smp, 0.1, 5.0), pkg.engine.pileup([smp], 0.1, 5.0)[0]


def test_sharded_replan_from_a_small_row_cap(pkg, small_case):
    """Three shards planned with 10 rows: the first step re-plans every shard
    with the rows needed + 16 and runs again (the record counts of the wrapped
    positions are kept, the runs in use read again), and gives the calls of
    one GPU and of the oracle; so does a second step, on the same plans."""
    dist, eng = _dist(), pkg.engine
    smp, exp, one = small_case
    sp = dist.ShardedPileup(dist.split_samples([smp], 3), [0] * 3, row_cap=10)
    assert [p.row_cap for p in sp.plans] == [10] * 3 and all(p.wrap for p in sp.plans)
    sp.step(0.1, 5.0)
    sized = sp.plans
    need = [int(p.status()[eng.MPC_ST_ROWS_NEEDED]) for p in sized]
    print("rows needed", need, "row_cap", [p.row_cap for p in sized])
    assert need[0] > 10 and need == [need[0]] * 3
    assert [p.row_cap for p in sized] == [need[0] + 16] * 3
    assert len(sp._cache["wrap"]) == 3
    for step in range(2):
        if step:
            sp.step(0.1, 5.0)
        sp.check()
        assert sp.data_error() == (0, None) and sp.plans is sized
        got = sp.fetch()[0]
        du.compare(got, exp, ("replan oracle", step))
        du.compare(got, one, ("replan one GPU", step))
        assert np.array_equal(got["raw"], one["raw"])


# (flags, read index) with 10 rows planned and read 137 of 200 inserting a base
# outside ACGT, as the code before the capacity rule was stated once reported
# them.  One GPU re-plans only when capacity is the only flag, so the error is
# raised from the 10-row run with the capacity bit still set; the sharded step
# re-plans whenever the capacity bit is set and reports from the sized run.
ONE_GPU_ERROR = (16 | 8, 137)  # MPC_DE_CAPACITY | MPC_DE_KEY
SHARDED_ERROR = (8, 137)  # MPC_DE_KEY


def test_small_row_cap_with_a_rejected_read_one_gpu(pkg):
    eng = pkg.engine
    with pytest.raises(eng.DataError) as err:
        eng.pileup([_plain_sample(200, 137)], -1.0, 1.0, row_cap=10)
    print("one GPU", (err.value.flags, err.value.read))
    assert (err.value.flags, err.value.read) == ONE_GPU_ERROR


def test_small_row_cap_with_a_rejected_read_three_shards(pkg):
    dist, eng = _dist(), pkg.engine
    sp = dist.ShardedPileup(dist.split_samples([_plain_sample(200, 137)], 3), [0] * 3, row_cap=10)
    sp.step(-1.0, 1.0)
    print("three shards", sp.data_error(), [p.row_cap for p in sp.plans])
    assert sp.data_error() == SHARDED_ERROR
    with pytest.raises(eng.DataError):
        sp.check()
