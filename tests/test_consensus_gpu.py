"""K_call / K_select (mpc_consensus) on injected tallies.

The other GPU tests reach the consensus kernels only through the tallies that
synthetic pileups happen to produce.  Here a batch whose row layout is known
from its construction (call_util.plain_batch) is laid out once, any tallies
are written into MPC_BUF_ROWS -- as dist.py's all-reduce does between mpc_rows
and mpc_consensus -- and the consensus phase runs by itself.  The expectation
is call_util.consensus_rows, the plain restatement of the reference's Steps
5-6 (tests/test_call_rule_cpu.py pins it to the oracle, the golden cases
t_call_rule* to the script).  Everything is compared exactly.
"""
import itertools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import call_util as cu
import depth_util as du
import geometry_util as geo

pytestmark = pytest.mark.gpu

NAN = float("nan")
SETTINGS = cu.SETTINGS + [(NAN, 1.0), (0.1, NAN)]

# the tie and threshold table: {0..3}^4, the same times 1000, counts a float32
# compare cannot tell apart, and the float64 edges of the two threshold tests
TABLE = list(dict.fromkeys(
    cu.SMALL + [tuple(1000 * v for v in t) for t in cu.SMALL]
    + sorted(set(itertools.permutations((2 ** 24 + 1, 2 ** 24, 0, 0))))
    + cu.GTF_EDGE + cu.D100 + cu.D10))
# total exactly 2^31: only ever on a row that is not a first slot (a first
# slot's total is a depth, and depths are read counts, below 2^31)
BIG = [(2 ** 30, 2 ** 30 - 1, 1, 0), (0, 1, 2 ** 30 - 1, 2 ** 30)]


class Injected:
    """The injection protocol.  Batch -> Plan with an explicit row capacity ->
    one full run at (-1, 1); the layout must be the one plain_batch predicted
    (row count, MPC_BUF_ROWMETA byte for byte, hence every sample's bounds).
    ``inject`` then writes tallies into MPC_BUF_ROWS[:rows], nonzero garbage
    (tallies, and meta 3) into [rows, row_cap), and zeroes MPC_BUF_MAXDEPTH:
    K_call only ever raises the maxima, and it is mpc_parse's clear that
    normally zeroes them -- the consensus phase alone does not.  ``consensus``
    runs the phase and returns (fetch(), ncalls)."""

    def __init__(self, pkg, samples, metas, row_cap=None):
        import torch
        self.torch = torch
        eng = self.eng = pkg.engine
        self.rows = int(sum(len(m) for m in metas))
        self.meta = np.concatenate(metas)
        self.bounds = np.concatenate([[0], np.cumsum([len(m) for m in metas])]).astype(np.int64)
        self.row_cap = int(row_cap or self.rows + 16)
        assert self.row_cap >= self.rows
        self.batch = eng.Batch(samples)
        self.plan = eng.Plan(self.batch, self.row_cap)
        self.plan.run(-1.0, 1.0)
        torch.cuda.synchronize()
        st = self.plan.status()
        assert int(st[eng.MPC_ST_FLAGS]) == 0
        assert int(st[eng.MPC_ST_ROWS_NEEDED]) == self.rows
        got = self.plan.buffer(eng.BUF_ROWMETA, torch.uint8)[: self.rows].cpu().numpy()
        odd = np.concatenate([[0], np.cumsum(got & 1)])
        for s, smp in enumerate(samples):  # a sample ends with its n_s-th odd row
            a, b = self.bounds[s], self.bounds[s + 1]
            assert odd[b] - odd[a] == len(smp["ref"]) and got[b - 1] == 3, s
        assert np.array_equal(got, self.meta)

    def inject(self, rows):
        torch, eng = self.torch, self.eng
        rows = np.asarray(rows, dtype=np.int64)
        assert rows.shape == (self.rows, 4) and rows.min() >= 0 and rows.sum(axis=1).max() <= 2 ** 31
        first = (self.meta & 2) != 0
        assert rows[first].sum(axis=1).max(initial=0) < 2 ** 31
        full = np.empty((self.row_cap, 4), dtype=np.uint32)
        full[: self.rows] = rows.astype(np.uint32)
        k = np.arange(self.row_cap - self.rows, dtype=np.uint32)[:, None]
        full[self.rows:] = 7 + 13 * k + np.arange(4, dtype=np.uint32)[None, :] * 1001
        buf = self.plan.buffer(eng.BUF_ROWS, torch.int32)
        assert buf.numel() == 4 * self.row_cap
        buf.copy_(torch.from_numpy(full.view(np.int32).reshape(-1)))
        mbuf = self.plan.buffer(eng.BUF_ROWMETA, torch.uint8)
        mbuf[self.rows:].fill_(3)
        self.plan.buffer(eng.BUF_MAXDEPTH, torch.int32).zero_()

    def consensus(self, mdf, gtf):
        self.plan.phase("consensus", None, mdf, gtf)
        res = self.plan.fetch()
        nc = self.plan.buffer(self.eng.BUF_NCALLS, self.torch.int32).cpu().numpy().astype(np.int64)
        return res, nc

    def check(self, rows, mdf, gtf, tag):
        """One consensus phase against the restatement; returns (expected, raw calls, ncalls)."""
        exp = cu.consensus_rows(rows, self.meta, self.bounds, mdf, gtf)
        got, nc = self.consensus(mdf, gtf)
        assert len(got) == len(exp)
        want = np.concatenate([[0], np.cumsum([len(e["base"]) for e in exp])])
        assert np.array_equal(nc, want), (tag, np.nonzero(nc != want)[0][:5].tolist())
        for s, (g, e) in enumerate(zip(got, exp)):
            du.compare(g, e, (tag, s, mdf, gtf))
        return exp, np.concatenate([g["raw"] for g in got]), nc


# ---------------------------------------------------------------------------
# one sample: the tie and threshold table on every kind of row
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table_sample(pkg):
    rng = np.random.default_rng(61)
    n, n_ins = 1500, 640
    gaps = rng.choice(np.arange(1, n), n_ins, replace=False)
    ins = [(int(g), "".join(cu.BASES[k] for k in rng.integers(0, 4, int(rng.integers(3, 6))))) for g in gaps]
    samples, metas = cu.plain_batch([n], [n_ins + 3], [ins], seed=62)
    inj = Injected(pkg, samples, metas)
    kinds = [np.nonzero(inj.meta == m)[0] for m in (3, 2, 0)]  # odd, first slot of a gap, later slot of a gap
    assert all(len(k) >= len(TABLE) for k in kinds), [len(k) for k in kinds]
    return inj, kinds


def _table_rows(inj, kinds, first_max, seed):
    """Every tuple of TABLE on every kind of row, in a seeded shuffle; first
    slots only take the tuples with a total <= first_max (None: all), so the
    sample's max depth is first_max; BIG on later slots only."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((inj.rows, 4), dtype=np.int64)
    for k, idx in enumerate(kinds):
        tbl = [t for t in TABLE if k == 2 or first_max is None or sum(t) <= first_max]
        tbl = np.array(tbl, dtype=np.int64)[rng.permutation(len(tbl))]
        where = rng.permutation(idx)
        rows[where] = tbl[np.arange(len(where)) % len(tbl)]
        assert len(where) >= len(tbl)  # every tuple is on some row of this kind
    later = rng.permutation(kinds[2])[: len(BIG)]
    rows[later] = np.array(BIG, dtype=np.int64)
    return rows


@pytest.mark.parametrize("first_max", [None, 100, 10], ids=["mixed", "depth100", "depth10"])
def test_tie_and_threshold_table(table_sample, first_max):
    """Every tie class in every assignment, scaled by 1000, past 2^24, and the
    float64 edges of count < gtf * count2 and count > max_depth * mdf, on odd
    rows, first slots of gaps and later slots, at every setting incl. inf and
    nan.  The largest total of the sample (2^31) sits on a later slot: it must
    not set max_depth, and at mdf = 1.0 only later slots are emitted."""
    inj, kinds = table_sample
    rows = _table_rows(inj, kinds, first_max, seed=7 + (first_max or 0))
    inj.inject(rows)
    first = (inj.meta & 2) != 0
    depth = int(rows[first].sum(axis=1).max())
    assert depth == (first_max or 2 ** 25 + 1) and int(rows[~first].sum(axis=1).max()) == 2 ** 31
    for mdf, gtf in SETTINGS:
        exp, _, _ = inj.check(rows, mdf, gtf, "table")
        assert exp[0]["max_depth"] == depth
        n = len(exp[0]["base"])
        if mdf == 1.0:  # count <= total <= max_depth on every first slot
            later = [cu.call_rule(t, gtf) for t in rows[~first]]
            assert n == sum(1 for c in later if c and c[3] > depth) and n >= len(BIG)
        elif mdf != mdf:
            assert n == 0
        elif mdf <= 0:
            assert n == int((rows.sum(axis=1) > 0).sum())
        else:
            assert 0 < n < inj.rows


# ---------------------------------------------------------------------------
# many samples: the paths past kSmpLds = 512, blocks spanning dozens of samples
# ---------------------------------------------------------------------------
def _count_batch(S):
    """S samples, lengths cycling through 2..9, three long ones (second, middle,
    last but one), zero-read samples first, last and three in a row; the
    second sample's length is then tuned so that some later sample starts
    exactly at a multiple of 1024 rows (a K_select block seam)."""
    lengths = [2 + s % 8 for s in range(S)]
    reads = [1 + s % 3 for s in range(S)]
    long_s = (1, S // 2, S - 2)
    for k, s in enumerate(long_s):
        lengths[s], reads[s] = 1500 - 7 * k, 3
    for s in (0, 100, 101, 102, S - 1):
        reads[s] = 0

    def insertions():
        out = []
        for s in range(S):
            n = lengths[s]
            if s in long_s:
                out.append([(10, "ACGT"), (700, "TTG"), (n - 1, "GATCA")])
            elif reads[s] and s % 2 == 0:
                out.append([(1 + s % (n - 1), "ACGTA"[: 2 + s % 3])])
            else:
                out.append([])
        return out

    _, metas = cu.plain_batch(lengths, reads, insertions())
    b = np.cumsum([len(m) for m in metas])
    t = int(np.searchsorted(b, 2048))  # sample t + 1 starts at b[t]
    lengths[1] += int(-b[t] % 1024)
    samples, metas = cu.plain_batch(lengths, reads, insertions(), seed=S)
    return samples, metas, long_s


def _count_rows(inj, long_s, seed):
    """Tallies with a different max depth per sample, set on one first slot (in
    the long samples more than a block past the sample's first row); later
    slots hold deeper rows; some samples are all zero, some stay below
    0.5 * max_depth everywhere."""
    rng = np.random.default_rng(seed)
    small = np.array(cu.SMALL, dtype=np.int64)
    rows = np.zeros((inj.rows, 4), dtype=np.int64)
    depths, silent = [], []
    S = len(inj.bounds) - 1
    for s in range(S):
        a, b = int(inj.bounds[s]), int(inj.bounds[s + 1])
        m = inj.meta[a:b]
        if s % 7 == 3 or s in (200, 201, 202):  # no tallies at all
            depths.append(0)
            silent.append(s)
            continue
        rows[a:b] = small[rng.integers(0, len(small), b - a)]
        firsts = np.nonzero(m & 2)[0]
        pos = a + int(firsts[firsts >= 1100][0] if s in long_s else rng.choice(firsts))
        if (s % 5 == 1 and s not in long_s) or s in (300, 301, 302):  # every count <= 12 < 0.5 * 27
            rows[pos] = (10, 9, 8, 0)
            depths.append(27)
            silent.append(s)
            continue
        later = a + np.nonzero(m == 0)[0]
        rows[later[::2]] *= 1000  # the sample's deepest rows are no first slots
        d = 20 + s % 50
        rows[pos] = np.roll((d, 0, 0, 0), s % 4)
        depths.append(d)
    return rows, depths, silent


@pytest.fixture(scope="module")
def counted(pkg):
    cache = {}

    def get(S, row_cap=None):
        if (S, row_cap) not in cache:
            samples, metas, long_s = _count_batch(S)
            inj = Injected(pkg, samples, metas, row_cap)
            rows, depths, silent = _count_rows(inj, long_s, seed=S)
            cache[S, row_cap] = (inj, rows, depths, silent)
        return cache[S, row_cap]
    return get


COUNT_SETTINGS = [(-1.0, 1.0), (0.1, 5.0), (0.5, 2.5), (0.29, 1.12)]


@pytest.mark.parametrize("S", [512, 513, 700])
def test_sample_counts(counted, S):
    """S = 512 keeps every sample's first row and max depth in LDS; 513 and 700
    take sample_of_row's global search, K_select's d.maxdepth[s] / d.srow[s]
    for s >= 512 and K_call's s_blk range under it.  First rows at every
    residue mod 4 and at a 1024-row seam, blocks of 256 and 1024 rows spanning
    dozens of samples and blocks inside one sample, zero-read samples (with
    injected tallies: what a shard sees whose rows arrive through the
    all-reduce), samples that emit nothing, ncalls compared itself."""
    inj, rows, depths, silent = counted(S)
    b = inj.bounds
    assert {int(x) % 4 for x in b[:-1]} == {0, 1, 2, 3}
    assert any(int(x) % 1024 == 0 for x in b[2:-1])
    assert max(np.diff(np.searchsorted(b, np.arange(0, inj.rows, 256)))) >= 24  # samples starting inside one block
    assert max(np.diff(b)) > 1024 and len(set(depths)) > 40
    assert inj.batch.read_begin[1] == 0 and inj.batch.read_begin[-1] == inj.batch.read_begin[-2]
    assert rows[b[-2]: b[-1]].sum() > 0 and rows[b[0]: b[1]].sum() > 0
    inj.inject(rows)
    for mdf, gtf in COUNT_SETTINGS:
        exp, _, nc = inj.check(rows, mdf, gtf, ("S", S))
        assert [e["max_depth"] for e in exp] == depths
        if (mdf, gtf) == (0.5, 2.5):
            assert all(len(exp[s]["base"]) == 0 for s in silent)
            assert sum(1 for e in exp if len(e["base"]) == 0) == len(silent) and nc[-1] > 0
        if mdf < 0:
            assert nc[-1] == int((rows.sum(axis=1) > 0).sum())


def test_row_capacity(counted):
    """The same 513 samples at a row capacity of rows + 16, 131072, 131073 and
    300000.  mpc_consensus launches K_call<1> while ceil(row_cap / 256) <=
    kCallBlocksMax = 512, i.e. up to 131072, and K_call<kCRBig> (kCRBig = 8
    rows per thread) above; which one ran cannot be observed, so the two sides
    of the switch are named here.  The rows in [rows, row_cap) hold garbage and
    must be ignored.  Identical calls and ncalls at all four."""
    ref = None
    for cap in (None, 131072, 131073, 300000):
        inj, rows, depths, _ = counted(513, cap)
        assert inj.rows + 16 < 131072
        inj.inject(rows)
        out = [inj.check(rows, mdf, gtf, ("cap", cap))[1:] for mdf, gtf in COUNT_SETTINGS]
        if ref is None:
            ref = out
        for (raw, nc), (raw0, nc0) in zip(out, ref):
            assert np.array_equal(raw, raw0) and np.array_equal(nc, nc0), cap


def test_phase_repeatable(counted):
    """The consensus phase at three settings in turn, and back, on the same
    injected rows without touching MPC_BUF_MAXDEPTH in between: the maxima
    K_call finds are the same every time, so every result is the restatement."""
    import torch
    inj, rows, depths, _ = counted(700)
    inj.inject(rows)
    md = inj.plan.buffer(inj.eng.BUF_MAXDEPTH, torch.int32)
    order = [(0.5, 2.5), (-1.0, 1.0), (0.29, 1.12), (-1.0, 1.0), (0.5, 2.5)]
    for mdf, gtf in order:
        inj.check(rows, mdf, gtf, "repeat")
        assert md.cpu().numpy().tolist() == depths


# ---------------------------------------------------------------------------
# end to end: the explicit tallies through the whole pipeline, every tally mode
# ---------------------------------------------------------------------------
E2E_SETTINGS = [(-1.0, 1.0), (0.29, 1.12), (0.5, 1.10)]


def _oracle_settings(smp, settings):
    with ThreadPoolExecutor(max_workers=len(settings)) as ex:
        return list(ex.map(lambda st: du.oracle_one(smp, *st), settings))


def _e2e_sample(mode):
    tuples = cu.TALLY_SAMPLES["small_gtf"]
    n = {1: len(tuples), 4: 400_000}.get(mode) or geo.first_length(mode)
    return cu.tally_sample(tuples, tail=n - len(tuples), ref_n=True, seed=5)


@pytest.mark.parametrize("mode", [1, 2, 3, 0, 4])
def test_tallies_end_to_end(pkg, mode):
    """tally_sample (every tie class, N in the reference wherever no read
    matches: K_layout's match == 0 branch; up to all reads substituting at a
    position: K_subs / K_subsum) through parse .. consensus in every tally
    mode, against the oracle."""
    smp = _e2e_sample(mode)
    assert b"N" in bytes(smp["ref"])
    batch = pkg.engine.Batch([smp])
    plan = pkg.engine.Plan(batch)
    assert plan.info()["tally_mode"] == mode
    exp = _oracle_settings(smp, E2E_SETTINGS)
    for (mdf, gtf), e in zip(E2E_SETTINGS, exp):
        plan.run(mdf, gtf)
        du.compare(plan.fetch()[0], e, ("e2e", mode, mdf, gtf))


def test_tallies_end_to_end_sharded(pkg):
    """The same sample as three in-process read shards on one device."""
    import importlib
    dist = importlib.import_module("minion-plasmid-consensus_amd.dist")
    smp = _e2e_sample(1)
    sp = dist.ShardedPileup(dist.split_samples([smp], 3), [0] * 3)
    exp = _oracle_settings(smp, E2E_SETTINGS)
    for (mdf, gtf), e in zip(E2E_SETTINGS, exp):
        sp.step(mdf, gtf)
        sp.check()
        for k, plan in enumerate(sp.plans):
            du.compare(plan.fetch()[0], e, ("e2e shard", k, mdf, gtf))
