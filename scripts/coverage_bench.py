#!/usr/bin/env python3
"""Times the coverage_qc pass: mpc_coverage_run (K_covparse + K_covfinish, HIP
events around the call, so the two table read-backs and the three clears are
inside) against the 16-thread host walk (mpc_coverage_host, wall clock) on the
same seeded input: bench.py's C2 batch (2 x 100k reads of 2,686 bp) and its C5
batch (24 x 10k reads of 30 kb).  Needs a GPU; the results of the two paths
must be equal or nothing is reported.

  python scripts/coverage_bench.py [--configs c2 c5] [--repeats 20] [--warmup 3] [--host-threads 16]
                                   [--pileup-steps 0] [--out profiles/coverage_bench.json]

--pileup-steps K also runs K steps of the pileup engine on the same batch, so
one `rocprofv3 --kernel-trace --stats` run of this script holds K_parse beside
K_covparse and K_covfinish (the yardstick: both read the same cs bytes).
Prints one JSON line per config; --out also writes them to a file."""
import argparse
import statistics
import sys
import time

import numpy as np

import _toolbench as tb

# bench.py CONFIGS: (n, reads per sample, profile, seed, plasmids)
SHAPES = {"c2": (2686, 100_000, "default", 2, 1), "c5": (30_000, 10_000, "default", 5000, 12)}


def batch(pkg, cfg):
    n, reads, profile, seed, plasmids = SHAPES[cfg]
    samples = []
    for k in range(plasmids):
        syn = pkg.synth.Synth(n=n, n_reads=reads, profile=profile, seed=seed + k, antisense=True)
        samples += [syn.sample(0), syn.sample(1)]
    return samples, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c2", "c5"], choices=sorted(SHAPES))
    ap.add_argument("--pileup-steps", type=int, default=0)
    args = tb.parse(ap, repeats=20, warmup=3)

    pkg, d = tb.gpu(args.device)
    cov, torch, dev = pkg.coverage, d.torch, d.dev
    H = cov.host_lib()
    results = []
    for cfg in args.configs:
        samples, n = batch(pkg, cfg)
        S = len(samples)
        cs_base = np.cumsum([0] + [len(s["cs"]) for s in samples])
        cs = np.concatenate([s["cs"] for s in samples])
        cs_off = np.concatenate([s["cs_off"][:-1] + cs_base[k] for k, s in enumerate(samples)] + [cs_base[-1:]]).astype(np.int64)
        tstart = np.concatenate([s["tstart"] for s in samples]).astype(np.int64)
        rec_sample = np.concatenate([np.full(len(s["tstart"]), k, np.int32) for k, s in enumerate(samples)])
        n_rec = len(tstart)
        pos_off = (np.arange(S + 1, dtype=np.int64) * (n + 1))
        region = np.tile(np.array([0, n], np.int64), S)
        n_pos = int(pos_off[-1])
        with d:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            d_cs, d_off, d_ts, d_rs, d_pos, d_reg = (up(a) for a in (np.concatenate([cs, np.zeros(8, np.uint8)]), cs_off,
                                                                      tstart, rec_sample, pos_off, region))
            d_rows = torch.empty((n_pos, 4), dtype=torch.int32, device=dev)
            d_stats = torch.empty((S, cov.STATS), dtype=torch.int64, device=dev)
            d_status = torch.empty(2, dtype=torch.int32, device=dev)

            def launch():
                d.check(d.lib.mpc_coverage_run(d_cs.data_ptr(), d_off.data_ptr(), d_ts.data_ptr(), d_rs.data_ptr(), n_rec,
                                               d_pos.data_ptr(), d_reg.data_ptr(), S, 0, d_rows.data_ptr(),
                                               d_stats.data_ptr(), d_status.data_ptr(), d.stream))

            times = [t * 1e3 for t in tb.timed(d, launch, args.warmup, args.repeats)]
            got = (d_rows.cpu().numpy().view(np.uint32), d_stats.cpu().numpy().view(np.uint64), d_status.cpu().numpy())
            if args.pileup_steps:
                runner = pkg.engine.Runner(samples, device=args.device)
                for _ in range(args.pileup_steps):
                    runner.step(0.1, 5.0)
                torch.cuda.synchronize(dev)
                runner.check()
        rows = np.zeros((n_pos, 4), np.uint32)
        stats = np.zeros((S, cov.STATS), np.uint64)
        status = np.zeros(2, np.int32)
        t0 = time.perf_counter()
        rc = H.mpc_coverage_host(cs.ctypes.data, cs_off.ctypes.data, tstart.ctypes.data, rec_sample.ctypes.data, n_rec,
                                 pos_off.ctypes.data, region.ctypes.data, S, 0, rows.ctypes.data, stats.ctypes.data,
                                 status.ctypes.data, args.host_threads, None)
        host_s = time.perf_counter() - t0
        if rc != 0 or status[0] != 0 or not (np.array_equal(got[0], rows) and np.array_equal(got[1], stats)
                                             and np.array_equal(got[2], status)):
            sys.exit("device and host walks disagree on %s: nothing to report" % cfg)
        med = statistics.median(times)
        tb.report(results, dict(
            bench="coverage_run", config=cfg, samples=S, records=n_rec, target_len=n, cs_bytes=int(len(cs)),
            device_us_min=round(min(times), 1), device_us_median=round(med, 1), device_us_max=round(max(times), 1),
            repeats=args.repeats, warmup=args.warmup, cs_gbytes_per_s=round(len(cs) / med / 1e3, 1),
            host_threads=args.host_threads, host_ms=round(host_s * 1e3, 1), host_over_device=round(host_s * 1e6 / med, 1),
            mean_depth=round(float(stats[0, 7]) / n, 1), gpu=torch.cuda.get_device_name(dev)))
    tb.write(results, args.out)


if __name__ == "__main__":
    main()
