#!/usr/bin/env python3
"""Times the verify_consensus scan: K_vscan (mpc_verify_scan, HIP events)
against the 16-thread host scan (mpc_verify_scan_host, wall clock) on the same
seeded input, for a C5-sized batch per GPU (48 pairs of m = 30,000: 12 plasmids
x 2 strands x 2 regions) and for one pair.  Needs a GPU; the results of the two
paths must be equal or nothing is reported.

  python scripts/verify_bench.py [--m 30000] [--pairs 48 1] [--repeats 7] [--warmup 2]
                                 [--host-threads 16] [--out profiles/verify_bench.json]

Prints one JSON line per batch size; --out also writes them to a file."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_pairs(n_pairs, m, seed):
    """Consensus-like texts: the query with a few substitutions and a short
    indel, between 17 and 23 flanking bases (n = m + 40 +- 1)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for _ in range(n_pairs):
        q = rng.choice(acgt, size=m)
        t = q.copy()
        for p in rng.choice(m, size=12, replace=False):
            t[p] = acgt[(int(np.where(acgt == t[p])[0][0]) + 1) % 4]
        cut = int(rng.integers(100, m - 100))
        t = np.concatenate([rng.choice(acgt, size=17), t[:cut], t[cut + 1:], rng.choice(acgt, size=23)])
        out.append((q.tobytes(), t.tobytes()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=30000)
    ap.add_argument("--pairs", type=int, nargs="+", default=[48, 1])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()

    pkg = importlib.import_module("minion-plasmid-consensus_amd")
    v = pkg.verify
    L = v.device_lib()
    import torch
    if not torch.cuda.is_available():
        sys.exit("verify_bench.py measures on a GPU; none is visible")
    H = v.host_lib()
    dev = torch.device("cuda", args.device)
    results = []
    for n_pairs in args.pairs:
        pairs = make_pairs(n_pairs, args.m, seed=100 + n_pairs)
        tab, seq = v._pack(pairs)
        cells = int(sum(len(q) * len(t) for q, t in pairs))
        blob = np.concatenate([tab.reshape(-1).view(np.uint8), seq])
        d_blob = torch.empty(len(blob), dtype=torch.uint8, device=dev)
        d_blob.copy_(torch.from_numpy(blob))
        d_out = torch.empty(2 * n_pairs, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev)

        def launch():
            pkg.engine._check(L.mpc_verify_scan(d_blob.data_ptr() + tab.nbytes, d_blob.data_ptr(), n_pairs,
                                                d_out.data_ptr(), ctypes.c_void_p(stream.cuda_stream)))

        with torch.cuda.device(dev):
            for _ in range(args.warmup):
                launch()
            torch.cuda.synchronize(dev)
            times = []
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            got = d_out.cpu().numpy().reshape(n_pairs, 2)
        host = np.zeros((n_pairs, 2), np.int32)
        t0 = time.perf_counter()
        rc = H.mpc_verify_scan_host(seq.ctypes.data, tab.ctypes.data, n_pairs, host.ctypes.data, args.host_threads)
        host_s = time.perf_counter() - t0
        if rc != 0 or not np.array_equal(got, host):
            sys.exit("device and host scans disagree on %d pairs: nothing to report" % n_pairs)
        dev_ms = statistics.median(times)
        rec = dict(bench="verify_scan", pairs=n_pairs, m=args.m, n=len(pairs[0][1]), dp_cells=cells,
                   device_ms_median=round(dev_ms, 3), device_ms_min=round(min(times), 3),
                   device_ms_max=round(max(times), 3), repeats=args.repeats, warmup=args.warmup,
                   device_cells_per_s=round(cells / (dev_ms * 1e-3), 1),
                   host_threads=args.host_threads, host_s=round(host_s, 3), host_cells_per_s=round(cells / host_s, 1),
                   device_over_host=round(host_s / (dev_ms * 1e-3), 2),
                   gpu=torch.cuda.get_device_name(dev), distances=sorted(set(int(d) for d in got[:, 0])))
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
