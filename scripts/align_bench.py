#!/usr/bin/env python3
"""Times the two device steps of align_reads against their host forms on the
same seeded input: the scan of both orientations (mpc_verify_scan, K_vscan:
2 x reads pairs in one launch) and the trace (mpc_align_trace, K_atrace), HIP
events around each call, against mpc_verify_scan_host and mpc_align_trace_host
on 16 threads (wall clock).  Workloads: a C2-like batch (Synth's reads of a
2,686 bp plasmid) and one batch of 10 kb reads.  Needs a GPU; the two paths'
results must be equal or nothing is reported.

  python scripts/align_bench.py [--batches 2686:4096 10000:512] [--repeats 7] [--warmup 2]
                                [--host-threads 16] [--out profiles/align_bench.json]

Prints one JSON line per batch; --out also writes them to a file.  The
whole-tool wall times (align_records: pack, copies, plan, render included) of
both devices are reported next to the kernels'."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

import _toolbench as tb


def synth_batch(pkg, n, n_reads, seed):
    """(target name, target, [(name, read)]) as Synth writes them."""
    with tempfile.TemporaryDirectory() as tmp:
        ref, reads = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fa")
        pkg.synth.Synth(n=n, n_reads=n_reads, seed=seed, antisense=False).write_files(ref, reads)
        tname, target = pkg.align.read_target(ref)
        return tname, target, list(pkg.align.fasta_records(reads))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", default=["2686:4096", "10000:512"], help="plasmid length:reads")
    ap.add_argument("--max-error", type=float, default=0.2)
    args = tb.parse(ap, repeats=7, warmup=2)

    pkg, d = tb.gpu(args.device)
    al, torch, dev = pkg.align, d.torch, d.dev
    H = al.host_lib()
    results = []
    for spec in args.batches:
        n, n_reads = (int(x) for x in spec.split(":"))
        tname, target, records = synth_batch(pkg, n, n_reads, seed=300 + n_reads)
        reads = [s for _, s in records]
        # the batch as the tool takes it (the device's reverse complements, scan and one traced launch):
        # its blob, plan and job table are what both paths are then timed on
        loop = al.Launches(target, reads, args.device, args.max_error, 8 << 30)
        pk, pl, R = loop.pk, loop.plan, len(reads)
        if len(loop.cuts) != 2:
            sys.exit("the batch does not fit one launch under 8 GiB of flags: nothing to report")
        (mapped, jobs, tool_out, tool_runs, _), = loop
        pk.d_seq = None
        loop.workspace.clear()
        J = len(jobs)
        pairs, rc_tab = pk.pair_table(), pk.revcomp_table()
        cells = int(2 * pk.n * pk.lens.sum())

        # host: reverse complements, scan, trace
        clean = pk.seq.copy()
        clean[pk.minus_span[0]: pk.minus_span[1]] = 0
        host_seq = clean.copy()
        assert H.mpc_align_revcomp_host(host_seq.ctypes.data, host_seq.nbytes, rc_tab.ctypes.data, R, args.host_threads) == 0
        host_scan = np.zeros((R, 4), np.int32)
        t0 = time.perf_counter()
        rc = H.mpc_verify_scan_host(host_seq.ctypes.data, pairs.ctypes.data, 2 * R, host_scan.ctypes.data, args.host_threads)
        host_scan_s = time.perf_counter() - t0
        assert rc == 0
        runs_cap = int((jobs[:, 7] + 2 * jobs[:, 4] + 1).max())
        flags_bytes = int((jobs[:, 6] + pl[mapped, 5]).max())
        host_out, host_runs = np.zeros((J, 8), np.int32), np.zeros(runs_cap, np.int32)
        t0 = time.perf_counter()
        rc = H.mpc_align_trace_host(host_seq.ctypes.data, host_seq.nbytes, jobs.ctypes.data, J, host_out.ctypes.data,
                                    host_runs.ctypes.data, runs_cap, args.host_threads)
        host_trace_s = time.perf_counter() - t0
        assert rc == 0

        # device: the same blob (its reverse complements made by K_arevcomp), the same tables
        with d:
            L, st = d.lib, d.stream
            d_seq, d_tab, d_pairs, d_jobs = (d.put(a) for a in (clean, rc_tab, pairs, jobs))
            d_scan = torch.empty(4 * R, dtype=torch.int32, device=dev)
            d_flags = torch.empty(flags_bytes, dtype=torch.uint8, device=dev)
            d_out = torch.zeros(8 * J, dtype=torch.int32, device=dev)
            d_runs = torch.zeros(runs_cap, dtype=torch.int32, device=dev)
            rev_ms = tb.timed(d, lambda: d.check(L.mpc_align_revcomp(
                d_seq.data_ptr(), pk.seq.nbytes, d_tab.data_ptr(), R, st)), args.warmup, args.repeats)
            scan_ms = tb.timed(d, lambda: d.check(L.mpc_verify_scan(
                d_seq.data_ptr(), d_pairs.data_ptr(), 2 * R, d_scan.data_ptr(), st)), args.warmup, args.repeats)
            trace_ms = tb.timed(d, lambda: d.check(L.mpc_align_trace(
                d_seq.data_ptr(), pk.seq.nbytes, d_jobs.data_ptr(), J, d_flags.data_ptr(), flags_bytes, d_out.data_ptr(),
                d_runs.data_ptr(), runs_cap, st)), args.warmup, args.repeats)
            same = (np.array_equal(d_seq.cpu().numpy(), host_seq) and np.array_equal(pk.seq, host_seq) and
                    np.array_equal(d_scan.cpu().numpy().reshape(R, 4), host_scan) and np.array_equal(loop.scan, host_scan) and
                    np.array_equal(tool_out, host_out) and np.array_equal(tool_runs, host_runs) and
                    np.array_equal(d_out.cpu().numpy().reshape(J, 8), host_out) and
                    np.array_equal(d_runs.cpu().numpy(), host_runs))
            del d_flags
        if not same:
            sys.exit("device and host disagree on %d reads: nothing to report" % R)

        # the whole tool on this batch (pack, copies, plan, render included), both devices
        wall = {}
        for device in (args.device, "cpu"):
            al.align_records(target, tname, records[:64], device=device, max_error=args.max_error)  # (warm)
            t0 = time.perf_counter()
            res = al.align_records(target, tname, records, device=device, max_error=args.max_error,
                                   threads=args.host_threads)
            wall[device] = (time.perf_counter() - t0, res["paf"])
        if wall[args.device][1] != wall["cpu"][1]:
            sys.exit("device and host PAF bytes differ: nothing to report")

        med = statistics.median
        rec = dict(bench="align_reads", plasmid=n, reads=R, mapped=J, read_len_median=int(np.median(pk.lens)),
                   d_median=int(np.median(pl[mapped, 2])), d_max=int(pl[mapped, 2].max()), scan_cells=cells,
                   flag_bytes=flags_bytes, repeats=args.repeats, warmup=args.warmup,
                   device_revcomp_ms=round(med(rev_ms), 3),
                   device_scan_ms=round(med(scan_ms), 3), device_scan_ms_min=round(min(scan_ms), 3),
                   device_scan_ms_max=round(max(scan_ms), 3),
                   device_scan_cells_per_s=round(cells / (med(scan_ms) * 1e-3), 1),
                   device_trace_ms=round(med(trace_ms), 3), device_trace_ms_min=round(min(trace_ms), 3),
                   device_trace_ms_max=round(max(trace_ms), 3),
                   host_threads=args.host_threads, host_scan_s=round(host_scan_s, 3), host_trace_s=round(host_trace_s, 3),
                   scan_device_over_host=round(host_scan_s / (med(scan_ms) * 1e-3), 2),
                   trace_device_over_host=round(host_trace_s / (med(trace_ms) * 1e-3), 2),
                   tool_device_s=round(wall[args.device][0], 3), tool_host_s=round(wall["cpu"][0], 3),
                   tool_device_over_host=round(wall["cpu"][0] / wall[args.device][0], 2),
                   paf_bytes=len(wall["cpu"][1]), gpu=torch.cuda.get_device_name(dev))
        tb.report(results, rec)
    tb.write(results, args.out)


if __name__ == "__main__":
    main()
