#!/usr/bin/env python3
"""Times the two device steps of draft_assembly against their host forms on the
same seeded input: the vote of one round (mpc_draft_vote, K_dvote: one launch
per launch of the trace, HIP events around each call, summed over the round's
launches) against mpc_draft_vote_host on 16 threads (wall clock), and the call
(mpc_draft_call, K_dcall: ONE workgroup) against mpc_draft_call_host.  The
draft is the seed read; the tallies and the new draft of both paths must be
equal or nothing is reported.  Workloads: the first 500 reads and all reads
(--sample 0) of a C2-sized read set (Synth's reads of a 2,686 bp plasmid).
Needs a GPU.

  python scripts/draft_bench.py [--sets 2686:500:500 2686:100000:0] [--repeats 5] [--host-threads 16]
                                [--out profiles/draft_bench.json]

Prints one JSON line per set; --out also writes them to a file.  The whole
tool's wall time (draft.assemble: FASTA, seed, rounds) is reported for the
device, and for the host path where the sample is at most --host-tool-reads."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

import _toolbench as tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["2686:500:500", "2686:100000:0"], help="plasmid length:reads in the file:--sample")
    ap.add_argument("--host-tool-reads", type=int, default=1000, help="largest sample the whole tool is also run on the host for")
    ap.add_argument("--max-error", type=float, default=0.3)
    args = tb.parse(ap, repeats=5, warmup=0)

    pkg, d = tb.gpu(args.device)
    al, dr, torch, dev = pkg.align, pkg.draft, d.torch, d.dev
    med = statistics.median
    results = []
    for spec in args.sets:
        n_ref, n_reads, sample = (int(x) for x in spec.split(":"))
        with tempfile.TemporaryDirectory() as tmp:
            reads_fa = os.path.join(tmp, "reads.fa")
            pkg.synth.Synth(n=n_ref, n_reads=n_reads, seed=41).write_files(None, reads_fa)
            records, _ = dr.take_sample(reads_fa, sample)
            reads = [s for _, s in records]
            t0 = time.perf_counter()
            seed, _ = dr.pick_seed(records, 8, args.max_error, args.device, args.host_threads)
            seed_s = time.perf_counter() - t0
            draft = reads[seed]
            n = len(draft)

            # one round by hand: per launch of the trace, the device vote (timed, repeats into a spare
            # tally) and the host vote of the same tables
            loop = al.Launches(draft, reads, args.device, args.max_error, threads=args.host_threads, keep_device=True)
            pk, cuts = loop.pk, loop.cuts
            d_tally, d_spare, h_tally = dr.new_tally(n, args.device), dr.new_tally(n, args.device), dr.new_tally(n, "cpu")
            vote_ms, vote_first_ms, host_vote_s, voted, n_runs = 0.0, 0.0, 0.0, 0, 0
            with d:
                for rd, jobs, out, runs, kept in loop:
                    status = []
                    vote_first_ms += tb.timed(d, lambda: status.append(
                        dr.vote(d_tally, n, pk.seq, jobs, out, runs, args.device, device_tensors=kept)), 0, 1)[0]
                    assert status[0][0] == 0
                    voted += int((status[0][1] == dr.VOTED).sum())
                    n_runs += int(out[:, 6].sum())
                    vote_ms += med(tb.timed(d, lambda: dr.vote(d_spare, n, pk.seq, jobs, out, runs, args.device, device_tensors=kept),
                                            args.warmup, args.repeats))
                    t0 = time.perf_counter()
                    hrc, hstatus = dr.vote(h_tally, n, pk.seq, jobs, out, runs, "cpu", args.host_threads)
                    host_vote_s += time.perf_counter() - t0
                    assert hrc == 0 and np.array_equal(hstatus, status[0][1])
                if not np.array_equal(dr.tally_to_host(d_tally), h_tally):
                    sys.exit("device and host tallies differ: nothing to report")
                got = []
                call_ms = tb.timed(d, lambda: got.append(dr.call(d_tally, draft, args.device, d_draft=pk.d_seq)), 1, args.repeats)
                new = got[0]
                host_call_s = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    host_new = dr.call(h_tally, draft, "cpu")
                    host_call_s.append(time.perf_counter() - t0)
                if new != host_new:
                    sys.exit("device and host drafts differ: nothing to report")
            pk.d_seq = None
            del d_tally, d_spare, loop

            # the whole tool
            wall = {}
            for device in [args.device] + (["cpu"] if len(reads) <= args.host_tool_reads else []):
                t0 = time.perf_counter()
                res = dr.assemble(reads_fa, sample=sample, max_error=args.max_error, device=device, threads=args.host_threads)
                wall[device] = (time.perf_counter() - t0, res["sense"])
            if "cpu" in wall and wall["cpu"][1] != wall[args.device][1]:
                sys.exit("device and host tools differ: nothing to report")

        rec = dict(bench="draft_assembly", plasmid=n_ref, reads_in_file=n_reads, sample=len(reads), draft_len=n,
                   launches=len(cuts) - 1, voted=voted, runs=n_runs, repeats=args.repeats, seed_scan_s=round(seed_s, 3),
                   device_vote_ms=round(vote_ms, 3), device_vote_first_ms=round(vote_first_ms, 3),
                   host_threads=args.host_threads, host_vote_ms=round(host_vote_s * 1e3, 3),
                   vote_device_over_host=round(host_vote_s * 1e3 / vote_ms, 2),
                   device_call_ms=round(med(call_ms), 3), device_call_ms_min=round(min(call_ms), 3),
                   device_call_ms_max=round(max(call_ms), 3), host_call_ms=round(med(host_call_s) * 1e3, 3),
                   new_draft_len=new[1]["length"], tool_device_s=round(wall[args.device][0], 3),
                   tool_host_s=round(wall["cpu"][0], 3) if "cpu" in wall else None,
                   final_draft_len=len(wall[args.device][1]), gpu=torch.cuda.get_device_name(dev))
        tb.report(results, rec)
    tb.write(results, args.out)


if __name__ == "__main__":
    main()
