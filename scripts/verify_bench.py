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
import statistics
import sys
import time

import numpy as np

import _toolbench as tb


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
    args = tb.parse(ap, repeats=7, warmup=2)

    pkg, d = tb.gpu(args.device)
    v, torch = pkg.verify, d.torch
    H = v.host_lib()
    results = []
    for n_pairs in args.pairs:
        pairs = make_pairs(n_pairs, args.m, seed=100 + n_pairs)
        tab, seq = v._pack(pairs)
        cells = int(sum(len(q) * len(t) for q, t in pairs))
        with d:
            (at_tab, at_seq), d_blob = d.put_all([tab.reshape(-1), seq])
            d_out = torch.empty(2 * n_pairs, dtype=torch.int32, device=d.dev)
            times = tb.timed(d, lambda: d.check(d.lib.mpc_verify_scan(at_seq, at_tab, n_pairs, d_out.data_ptr(), d.stream)),
                             args.warmup, args.repeats)
            got = d_out.cpu().numpy().reshape(n_pairs, 2)
        host = np.zeros((n_pairs, 2), np.int32)
        t0 = time.perf_counter()
        rc = H.mpc_verify_scan_host(seq.ctypes.data, tab.ctypes.data, n_pairs, host.ctypes.data, args.host_threads)
        host_s = time.perf_counter() - t0
        if rc != 0 or not np.array_equal(got, host):
            sys.exit("device and host scans disagree on %d pairs: nothing to report" % n_pairs)
        dev_ms = statistics.median(times)
        tb.report(results, dict(
            bench="verify_scan", pairs=n_pairs, m=args.m, n=len(pairs[0][1]), dp_cells=cells,
            device_ms_median=round(dev_ms, 3), device_ms_min=round(min(times), 3),
            device_ms_max=round(max(times), 3), repeats=args.repeats, warmup=args.warmup,
            device_cells_per_s=round(cells / (dev_ms * 1e-3), 1),
            host_threads=args.host_threads, host_s=round(host_s, 3), host_cells_per_s=round(cells / host_s, 1),
            device_over_host=round(host_s / (dev_ms * 1e-3), 2),
            gpu=torch.cuda.get_device_name(d.dev), distances=sorted(set(int(x) for x in got[:, 0]))))
    tb.write(results, args.out)


if __name__ == "__main__":
    main()
