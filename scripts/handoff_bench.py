#!/usr/bin/env python3
"""Times the handoff's kernel pair against the work it replaces, on the two
batches of scripts/align_bench.py (a C2-like batch of Synth's reads of a 2,686 bp
plasmid, and one batch of 10 kb reads), for ONE traced launch each:

  device  mpc_align_cs_sizes (K_acslen) + the host's exclusive sums and the
          upload of the place table + mpc_align_cs_write (K_acswrite), HIP
          events around the whole step (the calls' own read-backs and stream
          waits included)
  host    mpc_align_render on --host-threads threads, then the native ingest
          (ingest.pack_sample) of that PAF and the reads file: the PAF text
          written, read back and cut again -- what the two-command path does
          between the trace and the pileup's inputs (wall clock; the files are
          in a temporary directory)

Needs a GPU.  The device's bytes must equal the ingest's or nothing is reported.

  python scripts/handoff_bench.py [--batches 2686:4096 10000:512] [--repeats 7] [--warmup 2]
                                  [--host-threads 16] [--out profiles/handoff_bench.json]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

import _toolbench as tb
from align_bench import synth_batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", default=["2686:4096", "10000:512"], help="plasmid length:reads")
    ap.add_argument("--max-error", type=float, default=0.2)
    args = tb.parse(ap, repeats=7, warmup=2)
    pkg, d = tb.gpu(args.device)
    al, ho, torch = pkg.align, pkg.handoff, d.torch
    results = []
    for spec in args.batches:
        n, n_reads = (int(x) for x in spec.split(":"))
        tname, target, records = synth_batch(pkg, n, n_reads, seed=300 + n_reads)
        loop = al.Launches(target, [s for _, s in records], args.device, args.max_error, 8 << 30, keep_device=True)
        if len(loop.cuts) != 2:
            sys.exit("the batch does not fit one launch under 8 GiB of flags: nothing to report")
        (mapped, jobs, out, runs, tensors), = loop
        pk, J = loop.pk, len(jobs)
        names = [records[r][0] for r in mapped]

        # device: sizes, places, write into buffers with the pileup's readable room
        sizes = ho.cs_sizes(jobs, out, runs, pk.seq.nbytes, args.device, tensors=tensors)
        place, ends = ho.places(sizes)
        with d:
            bufs = [torch.zeros(e + pad, dtype=torch.uint8, device=d.dev) for e, pad in zip(ends, (ho.CS_PAD, ho.FLANK_PAD, ho.FLANK_PAD))]

            def step():
                z = ho.cs_sizes(jobs, out, runs, pk.seq.nbytes, args.device, tensors=tensors)
                p, _ = ho.places(z)
                ho.cs_write(pk.seq, jobs, out, runs, z, p, *bufs, device=args.device, tensors=tensors, caps=ends)

            dev_ms = tb.timed(d, step, args.warmup, args.repeats)
            got = [b.cpu().numpy()[:e] for b, e in zip(bufs, ends)]

        # host: render, write, ingest
        host_s, render_s = [], []
        with tempfile.TemporaryDirectory() as tmp:
            ref, reads, paf = (os.path.join(tmp, x) for x in ("ref.fa", "reads.fa", "x.paf"))
            with open(ref, "wb") as f:
                f.write(b">" + tname + b"\n" + target + b"\n")
            with open(reads, "wb") as f:
                for name, s in records:
                    f.write(b">" + name + b"\n" + s + b"\n")
            for k in range(args.warmup + args.repeats):
                t0 = time.perf_counter()
                text, _ = al.render(pk.seq, jobs, loop.plan[mapped, 0], out, runs, names, tname, args.host_threads)
                t1 = time.perf_counter()
                with open(paf, "wb") as f:
                    f.write(text)
                want = pkg.ingest.pack_sample(ref, paf, reads)
                t2 = time.perf_counter()
                if k >= args.warmup:
                    host_s.append(t2 - t0)
                    render_s.append(t1 - t0)
            paf_bytes = len(text)
        kept = sizes[:, 0] == 1
        same = (np.array_equal(got[0], want["cs"]) and np.array_equal(got[1], want["up"]) and
                np.array_equal(got[2], want["down"]) and np.array_equal(sizes[kept, 4], want["tstart"]) and
                np.array_equal(np.cumsum(sizes[kept, 1]), want["cs_off"][1:]))
        if not same:
            sys.exit("the device's bytes and the ingest's differ on %d reads: nothing to report" % J)
        med = statistics.median
        tb.report(results, dict(
            bench="handoff", device_what="the whole step: both entry points with their read-backs, table checks and "
            "stream waits, the numpy sums and the place upload, not the two kernels alone", plasmid=n, reads=len(records), mapped=J, kept=int(kept.sum()), runs=int(out[:, 6].sum()),
            cs_bytes=ends[0], up_bytes=ends[1], down_bytes=ends[2], paf_bytes=paf_bytes, repeats=args.repeats,
            warmup=args.warmup, device_ms=round(med(dev_ms), 3), device_ms_min=round(min(dev_ms), 3),
            device_ms_max=round(max(dev_ms), 3), host_threads=args.host_threads, host_ms=round(1e3 * med(host_s), 3),
            host_ms_min=round(1e3 * min(host_s), 3), host_ms_max=round(1e3 * max(host_s), 3),
            host_render_ms=round(1e3 * med(render_s), 3), host_over_device=round(1e3 * med(host_s) / med(dev_ms), 2),
            gpu=torch.cuda.get_device_name(d.dev)))
        pk.d_seq = None
    tb.write(results, args.out)


if __name__ == "__main__":
    main()
