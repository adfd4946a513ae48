"""The shape grid of the host planner's golden (tests/golden/plan_shapes.json):
the inputs, how a case is recorded through the ctypes binding, and the text
forms the stand-alone driver (tests/native/plan_driver.cpp) reads and prints.
scripts/make_plan_golden.py records the fixture; tests/test_plan_golden.py and
tests/test_plan_sanitized.py compare against it."""
import ctypes
import json
import os
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "plan_shapes.json")
N_BUFFERS = 17  # include/mpc.h MPC_BUF_COUNT
INFO_FIELDS = ("tally_mode", "parse_window", "parse_waves", "parse_lds_bytes", "parse_workgroups", "overrides",
               "max_reads_per_workgroup", "reads_per_workgroup_cap", "workspace_bytes", "deferred_placement", "reserved")

C1 = ([5000], [20_000], 20_000 * 600)
C2 = ([2686, 2686], [100_000, 100_000], 63 << 20)
C3 = ([10_000], [1_000_000], 1200 << 20)
C4 = ([10_000] * 2, [100_000] * 2, 1070 << 20)
C5 = ([30_000] * 24, [10_000] * 24, 24 * 3600 * 10_000 // 100)
# tests/test_abi.py::test_parse_split
SPLIT = {"c2": ([2686, 2686], [100_000, 100_000]), "c3": ([10_000], [200_000]), "c5": ([30_000] * 6, [10_000] * 6),
         "ragged": ([500, 40_000], [37, 3])}


def split_offsets(counts):
    """The seeded cs offsets of test_parse_split."""
    rng = np.random.default_rng(7)
    lens = rng.integers(20, 4000, size=sum(counts)) * rng.choice([1, 1, 1, 9], size=sum(counts))
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _case(name, ref_lens, counts, cs_bytes, cs_off=None, null=0, **kw):
    c = dict(name=name, ref_lens=list(ref_lens), counts=list(counts), cs_bytes=int(cs_bytes), cs_off=cs_off, null=null,
             n_samples=len(ref_lens), read_offset=0, n_reads_global=None, shard=0, n_shards=1, parse_cus=0,
             neg_reads=0, neg_cs_bytes=0)
    c.update(kw)
    return c


def cases(lds_limit):
    """Every planned shape; ``lds_limit``: the longest reference whose parse
    state fits LDS (bisected as in test_planner_reference_limit, kept in the
    fixture)."""
    out = []
    for name, cfg in (("c1", C1), ("c2", C2), ("c3", C3), ("c4", C4), ("c5", C5)):
        out.append(_case(name, *cfg))
        for cus in (128, 224):
            out.append(_case("%s_cus%d" % (name, cus), *cfg, parse_cus=cus))
    out.append(_case("cap_binds", [10_000, 30], [100, 16383 * 300], 16383 * 300 * 12))
    for name, (ref_lens, counts) in SPLIT.items():
        off = split_offsets(counts)
        out.append(_case("split_" + name, ref_lens, counts, off[-1], cs_off=off))
    out.append(_case("split_c5_no_off", *SPLIT["c5"], split_offsets(SPLIT["c5"][1])[-1]))
    out.append(_case("c2_neg", *C2, neg_reads=1, neg_cs_bytes=700))
    out.append(_case("c2_neg_shard1of4", [2686, 2686], [25_000, 25_000], (63 << 20) // 4, read_offset=50_000,
                     n_reads_global=200_000, shard=1, n_shards=4, neg_reads=1, neg_cs_bytes=700))
    out.append(_case("c3_shard3of8", [10_000], [125_000], (1200 << 20) // 8, read_offset=375_000,
                     n_reads_global=1_000_000, shard=3, n_shards=8))
    out.append(_case("empty_sample", [2686, 900, 2686], [3000, 0, 500], 3500 * 700))
    out.append(_case("no_reads", [2686, 2686], [0, 0], 0))
    out.append(_case("lds_limit", [lds_limit], [12], lds_limit * 3))
    out.append(_case("lds_limit_plus1", [lds_limit + 1], [12], (lds_limit + 1) * 3))
    out.append(_case("longest_ref", [(1 << 22) - 2], [12], (1 << 22) * 3))
    for n in (8000, 11_000, 13_000, 20_000, 50_000, 70_000, 100_000, 200_000):  # down the geometry candidates
        out.append(_case("ref_%d" % n, [n, n // 2], [4000, 700], 4700 * 900))
    out.append(_case("rsort_multi",[5000], [512 * 1024 + 1], (512 * 1024 + 1) * 300))
    return out


def error_cases():
    return [
        _case("null_input", *C2, null=1),
        _case("null_output", *C2, null=2),
        _case("shard_out_of_range", *C2, shard=4, n_shards=4),
        _case("read_shard_outside", *C2, read_offset=1, n_reads_global=200_000),
        _case("reference_too_long", [(1 << 22) - 1], [12], (1 << 22) * 3),
        _case("negative_neg_reads", *C2, neg_reads=-1),
        _case("no_samples", [], [], 0, n_samples=0),
        _case("negative_samples", [], [], 0, n_samples=-2),
    ]


def _arrays(c):
    ref_len = np.ascontiguousarray(c["ref_lens"], dtype=np.int64)
    rb = np.ascontiguousarray(np.concatenate([[0], np.cumsum(np.asarray(c["counts"], dtype=np.int64))]), dtype=np.int64)
    return ref_len, rb, int((4 * ref_len + 8).sum() + 1024)


def record(engine, c):
    """One case through the ctypes binding of the loaded libmpc.so."""
    L = engine.lib()
    p64 = ctypes.POINTER(ctypes.c_int64)
    ref_len, rb, row_cap = _arrays(c)
    n = int(rb[-1])
    inp = engine._Input(n_samples=c["n_samples"], h_ref_len=ref_len.ctypes.data_as(p64), h_read_begin=rb.ctypes.data_as(p64),
                        n_reads=n, cs_bytes=c["cs_bytes"], cs_base=0, read_offset=c["read_offset"],
                        n_reads_global=c["n_reads_global"] or n, shard=c["shard"], n_shards=c["n_shards"],
                        parse_cus=c["parse_cus"], neg_reads=c["neg_reads"], neg_cs_bytes=c["neg_cs_bytes"])
    if c["cs_off"] is not None:
        inp.h_cs_off = c["cs_off"].ctypes.data_as(p64)
    L.mpc_plan_parse_tables.argtypes = [ctypes.c_void_p] * 3
    h = ctypes.c_void_p()
    rc = L.mpc_plan_create(None if c["null"] == 1 else ctypes.byref(inp), row_cap, None if c["null"] == 2 else ctypes.byref(h))
    if rc != 0:
        return {"rc": rc, "error": L.mpc_last_error().decode()}
    try:
        info = engine.PlanInfo()
        assert L.mpc_plan_get_info(h, ctypes.byref(info)) == 0
        n_wg = L.mpc_plan_parse_tables(h, None, None)
        work = np.zeros((n_wg, 4), np.int32)
        chunks = np.zeros((n_wg, engine.PARSE_CHUNKS + 1), np.int32)
        assert L.mpc_plan_parse_tables(h, work.ctypes.data, chunks.ctypes.data) == n_wg
        ws = ctypes.c_size_t()
        assert L.mpc_plan_workspace_bytes(h, ctypes.byref(ws)) == 0
        bufs = []
        for b in range(N_BUFFERS):
            off, cnt = ctypes.c_size_t(), ctypes.c_int64()
            assert L.mpc_plan_buffer(h, b, ctypes.byref(off), ctypes.byref(cnt)) == 0
            bufs.append([off.value, cnt.value])
        return {"rc": 0, "info": [int(getattr(info, k)) for k in INFO_FIELDS], "workspace_bytes": ws.value,
                "parse_workgroups": n_wg, "work_crc": zlib.crc32(work.tobytes()), "chunks_crc": zlib.crc32(chunks.tobytes()),
                "buffers": bufs}
    finally:
        L.mpc_plan_destroy(h)


def bisect_lds_limit(engine):
    lo, hi = 100_000, 1_000_000
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if engine.geometry([mid], [12], mid * 3)["tally_mode"] == 4:
            hi = mid
        else:
            lo = mid
    return lo


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def write_case_file(path, case_list):
    """The driver's input: per case a header line, the reference lengths, the
    read boundaries and (if given) the cs offsets."""
    with open(path, "w") as f:
        for c in case_list:
            ref_len, rb, row_cap = _arrays(c)
            n = int(rb[-1])
            f.write("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (
                c["name"], c["null"], row_cap, c["n_samples"], len(ref_len), n, c["cs_bytes"], c["read_offset"],
                c["n_reads_global"] or n, c["shard"], c["n_shards"], c["parse_cus"], c["neg_reads"], c["neg_cs_bytes"],
                c["cs_off"] is not None))
            f.write(" ".join(map(str, ref_len)) + "\n" + " ".join(map(str, rb)) + "\n")
            if c["cs_off"] is not None:
                np.savetxt(f, c["cs_off"][None, :], fmt="%d")


def parse_driver_output(text):
    """{name: record} from the driver's lines: ``name rc`` then either the
    message or info (11), workspace bytes, workgroups, two CRCs, 17 x (offset, count)."""
    out = {}
    for line in text.splitlines():
        name, rc, rest = line.split(" ", 2)
        if int(rc) != 0:
            out[name] = {"rc": int(rc), "error": rest}
            continue
        v = [int(x) for x in rest.split()]
        k = len(INFO_FIELDS)
        out[name] = {"rc": 0, "info": v[:k], "workspace_bytes": v[k], "parse_workgroups": v[k + 1], "work_crc": v[k + 2],
                     "chunks_crc": v[k + 3], "buffers": [v[k + 4 + 2 * b: k + 6 + 2 * b] for b in range(N_BUFFERS)]}
    return out
