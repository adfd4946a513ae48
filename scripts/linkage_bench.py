#!/usr/bin/env python3
"""Times the linkage_qc pass: mpc_linkage_run (K_lnkparse + K_lnkplanes +
K_lnkpair, HIP events around the call, so the table read-back and the clears
are inside) against the 16-thread host walk (mpc_linkage_host, wall clock), and
mpc_coverage_run on the same batch in the same session as the yardstick (the
same walk over the same cs bytes).  Input: bench.py's C2 batch (2 x 100k reads
of 2,686 bp) and its C5 batch (24 x 10k reads of 30 kb).  Sites: once what
select_sites gives at its defaults, once the 128 highest-fraction sites.  Needs
a GPU; the results of the two paths must be equal or nothing is reported.

  python scripts/linkage_bench.py [--configs c2 c5] [--repeats 20] [--warmup 3] [--host-threads 16]
                                  [--out profiles/linkage_bench.json]

One `rocprofv3 --kernel-trace --stats` run of this script gives the per-kernel
times.  Prints one JSON line per config and site set; --out also writes them
to a file."""
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
    args = tb.parse(ap, repeats=20, warmup=3)

    pkg, d = tb.gpu(args.device)
    cov, lnk, torch, dev = pkg.coverage, pkg.linkage, d.torch, d.dev
    H = lnk.host_lib()
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
        regions = [(0, n)] * S
        n_pos = int(pos_off[-1])
        with d:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            d_cs, d_off, d_ts, d_rs, d_pos, d_reg = (up(a) for a in (np.concatenate([cs, np.zeros(8, np.uint8)]), cs_off,
                                                                      tstart, rec_sample, pos_off, region))
            d_rows = torch.empty((n_pos, 4), dtype=torch.int32, device=dev)
            d_stats = torch.empty((S, cov.STATS), dtype=torch.int64, device=dev)
            d_status = torch.empty(2, dtype=torch.int32, device=dev)

            def cov_launch():
                d.check(d.lib.mpc_coverage_run(d_cs.data_ptr(), d_off.data_ptr(), d_ts.data_ptr(), d_rs.data_ptr(), n_rec,
                                               d_pos.data_ptr(), d_reg.data_ptr(), S, 0, d_rows.data_ptr(),
                                               d_stats.data_ptr(), d_status.data_ptr(), d.stream))

            cov_times = [t * 1e3 for t in tb.timed(d, cov_launch, args.warmup, args.repeats)]
            rows = d_rows.cpu().numpy().view(np.uint32)
            if d_status.cpu().numpy()[0] != 0:
                sys.exit("coverage_run refuses the %s batch" % cfg)
            cov_med = statistics.median(cov_times)
            for what, sel in (("defaults", lnk.select_sites(rows, pos_off, regions)),
                              ("top128", lnk.select_sites(rows, pos_off, regions, 0.0, 0))):
                site_off, site_key, dropped = sel
                K = len(site_key)
                rec = dict(bench="linkage_run", config=cfg, sites=what, n_sites=K, sites_dropped=int(dropped), samples=S,
                           records=n_rec, target_len=n, cs_bytes=int(len(cs)), coverage_us_median=round(cov_med, 1),
                           coverage_us_min=round(min(cov_times), 1), coverage_us_max=round(max(cov_times), 1))
                if K == 0:
                    rec["note"] = "no site qualifies: nothing to run"
                    tb.report(results, rec)
                    continue
                d_so, d_sk = up(site_off), up(site_key)
                d_alleles = torch.empty((n_rec, K), dtype=torch.uint8, device=dev)
                d_pair = torch.empty((K, K, 8, 8), dtype=torch.int32, device=dev)
                d_scratch = torch.empty(lnk.scratch_bytes(n_rec, K) // 8, dtype=torch.int64, device=dev)

                def launch():
                    d.check(d.lib.mpc_linkage_run(d_cs.data_ptr(), d_off.data_ptr(), d_ts.data_ptr(), d_rs.data_ptr(), n_rec,
                                                  d_pos.data_ptr(), S, d_so.data_ptr(), d_sk.data_ptr(), K, d_alleles.data_ptr(),
                                                  d_pair.data_ptr(), d_scratch.data_ptr(), d_status.data_ptr(), d.stream))

                times = [t * 1e3 for t in tb.timed(d, launch, args.warmup, args.repeats)]
                got = (d_alleles.cpu().numpy(), d_pair.cpu().numpy().view(np.uint32), d_status.cpu().numpy())
                alleles = np.zeros((n_rec, K), np.uint8)
                pair = np.zeros((K, K, 8, 8), np.uint32)
                status = np.zeros(2, np.int32)
                t0 = time.perf_counter()
                rc = H.mpc_linkage_host(cs.ctypes.data, cs_off.ctypes.data, tstart.ctypes.data, rec_sample.ctypes.data, n_rec,
                                        pos_off.ctypes.data, S, site_off.ctypes.data, site_key.ctypes.data, K,
                                        alleles.ctypes.data, pair.ctypes.data, status.ctypes.data, args.host_threads)
                host_s = time.perf_counter() - t0
                if rc != 0 or status[0] != 0 or not (np.array_equal(got[0], alleles) and np.array_equal(got[1], pair)
                                                     and np.array_equal(got[2], status)):
                    sys.exit("device and host disagree on %s / %s: nothing to report" % (cfg, what))
                med = statistics.median(times)
                rec.update(device_us_min=round(min(times), 1), device_us_median=round(med, 1), device_us_max=round(max(times), 1),
                           repeats=args.repeats, warmup=args.warmup, cs_gbytes_per_s=round(len(cs) / med / 1e3, 1),
                           run_over_coverage_run=round(med / cov_med, 3), host_threads=args.host_threads,
                           host_ms=round(host_s * 1e3, 1), host_over_device=round(host_s * 1e6 / med, 1),
                           gpu=torch.cuda.get_device_name(dev))
                tb.report(results, rec)
    tb.write(results, args.out)


if __name__ == "__main__":
    main()
