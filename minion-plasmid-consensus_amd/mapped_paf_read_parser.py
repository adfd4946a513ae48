"""Drop-in CLI for src/mapped_paf_read_parser.py (reference v5.1, :108-465).

Same flags, same output files, same exit status; Steps 4-6 run on an MI355X
through libmpc.so.  The Snakemake rule `consensus` (Snakefile:401-423) only has
to point ``params.script`` here.

Extra, optional flags (defaults keep the reference behaviour):
  --device N         HIP device index (default 0)
  --gpus N           use N GPUs (default 1), devices --device .. --device + N - 1
                     modulo the visible ones.  Jobs with their own reads files
                     (--job) are dealt round-robin to the GPUs; with fewer reads
                     files than GPUs every pileup is read-sharded over all N
                     (dist.py).  Same files, same exit status as with one GPU.
  --also REF PAF CONSENSUS CHROMAT ACCURACIES
                     run another (assembly, PAF) pair against the same --reads in
                     the SAME launch (e.g. the antisense strand); repeatable
  --revcomp SRC DST  after writing, reverse-complement consensus SRC into DST
                     (Snakefile rule revcomp_antisense_consensus, :425-450);
                     repeatable
  --job REF PAF READS CONSENSUS CHROMAT ACCURACIES
                     another job with its OWN reads file, same launch (a batch of
                     plasmids: BASELINE configs[4]); repeatable.  With --job the
                     primary --ref/--paf/--reads/... flags may be omitted.
"""
import argparse
import importlib
import sys
import time

if __package__:
    from . import _cli
else:  # run by path: sys.path[0] is this directory
    import _cli

statprint = _cli.statprint
TITLE = "Mapped PAF Read Parser"


def build_parser():
    p = argparse.ArgumentParser(description=TITLE)
    p.add_argument("--ref", dest="REF", help="Reference fasta file of plasmid sequence", type=str)
    p.add_argument("--reads", dest="READS", help="Raw reads fasta file", type=str)
    p.add_argument("--paf", dest="PAF", help="Mapped reads .paf file", type=str)
    p.add_argument("--consensus", help="Consensus output file", type=str)
    p.add_argument("--chromat", help="Chromatogram data output file", type=str)
    p.add_argument("--accuracies", help="Per position consensus accuracies output file", type=str)
    p.add_argument("--min_depth_factor", dest="MIN_DEPTH_FACTOR", type=float,
                   help="Minimum number of reads needed to call a base is set to max_depth*MIN_DEPTH_FACTOR")
    p.add_argument("--global_threshold_factor", dest="GLOBAL_THRESHOLD_FACTOR", type=float,
                   help="Value of minimum most frequent to second most frequent base ratio to make call")
    p.add_argument("-d", "--debug", action="store_true", dest="DEBUG", help="Flag for setting debug/test state.")
    p.add_argument("-v", "--verbose", action="store_true", dest="VERB", help="Flag for setting verbose output.")
    p.add_argument("--device", type=int, default=0, help="HIP device index")
    p.add_argument("--gpus", type=int, default=1,
                   help="GPUs to use: job groups dealt round-robin, or read-sharded when there are fewer groups")
    p.add_argument("--also", nargs=5, action="append", default=[],
                   metavar=("REF", "PAF", "CONSENSUS", "CHROMAT", "ACCURACIES"),
                   help="additional (assembly, PAF) job against the same reads, same launch")
    p.add_argument("--revcomp", nargs=2, action="append", default=[], metavar=("SRC", "DST"),
                   help="reverse-complement a written consensus file (rule revcomp_antisense_consensus)")
    p.add_argument("--job", nargs=6, action="append", default=[],
                   metavar=("REF", "PAF", "READS", "CONSENSUS", "CHROMAT", "ACCURACIES"),
                   help="additional job with its own reads file, same launch")
    return p


def _ingest_and_pileup(ingest, engine, jobs, args, tm):
    """Steps 1-6 of every job.  Jobs sharing a reads file are ingested together
    (one scan of it); a group's pileup runs on the device (a worker thread: the
    native ingest and the HIP calls release the GIL) while the next group is
    ingested.  Errors as the jobs would raise them in order: the first job
    (in job order) the ingest rejects, else the first group's device error.
    Returns the per-job call dicts, or None when --min_depth_factor is missing
    (every file is still read first, as the reference does).  ``tm`` receives
    the phase walls: ingest (all groups), device (what the ingest did not
    hide).

    ``--gpus N`` (dist.assign): with at least N groups, group i runs whole on
    the worker thread of device i % N; with fewer, every group is read-sharded
    over all N devices by one worker (dist.pileup_sharded).  The results, the
    error a run reports and their order are those of one GPU."""
    import concurrent.futures as cf
    import contextlib
    mdf, gtf = args.MIN_DEPTH_FACTOR, args.GLOBAL_THRESHOLD_FACTOR
    triples = [(ref, paf, reads) for ref, paf, reads, *_ in jobs]
    groups = ingest.job_groups(triples)
    packed, futs, t_ing = [None] * len(jobs), [], 0.0
    mode, devices, worker_of = "partition", [args.device], [0] * len(groups)
    if args.gpus > 1:
        import torch
        dist = importlib.import_module(engine.__name__.rsplit(".", 1)[0] + ".dist")
        engine.lib()  # (loaded once, before the workers race for it)
        visible = torch.cuda.device_count()
        if args.gpus > visible:
            statprint("--gpus {} with {} visible: several shards or partitions share a device.".format(
                args.gpus, visible), "WARNING")
        mode, devices, worker_of = dist.assign(len(groups), args.gpus, args.device, visible)
    with contextlib.ExitStack() as stack:
        pools = [stack.enter_context(cf.ThreadPoolExecutor(max_workers=1))
                 for _ in range(len(devices) if mode == "partition" else 1)]
        for gi, idx in enumerate(groups):
            t = time.perf_counter()
            got = ingest.pack_group([triples[j] for j in idx])
            t_ing += time.perf_counter() - t
            for j, x in zip(idx, got):
                packed[j] = x
            ok = not any(isinstance(x, Exception) for x in got)
            if ok:
                for x in got:
                    statprint("There were {} mapped reads.".format(x["n_alignments"]))
            if ok and mdf is not None:
                if not futs:
                    statprint("Pileup and consensus on device {}...".format(",".join(str(d) for d in devices)))
                if mode == "partition":
                    w = worker_of[gi]
                    fut = pools[w].submit(engine.pileup, got, mdf, 1.0 if gtf is None else gtf, devices[w])
                else:
                    fut = pools[0].submit(dist.pileup_sharded, got, mdf, 1.0 if gtf is None else gtf, devices)
                futs.append((idx, fut))
        t1 = time.perf_counter()
        tm["ingest"] = t_ing
        errs = [x for x in packed if isinstance(x, Exception)]
        if errs:
            for _, f in futs:  # let launched pileups finish before reporting
                f.exception()
            raise errs[0]
        if mdf is None:
            return None
        results = [None] * len(jobs)
        # reads of every job, and the job-order prefix: a device error is
        # reported as the read index in the launch of all jobs in JOB order
        n_of = [len(packed[j]["tstart"]) for j in range(len(jobs))]
        before = [sum(n_of[:j]) for j in range(len(jobs))]
        first = None  # (job, read within it, flags) of the earliest failing job
        for idx, f in futs:
            try:
                res = f.result()
            except engine.DataError as e:
                # the group's samples are its jobs in idx order: map the launch's
                # read index back to (job, read in the job)
                k, r = engine.locate_read(e.read, [n_of[j] for j in idx])
                j = idx[k]
                if first is None or j < first[0]:
                    first = (j, r, e.flags)
                continue
            for j, r in zip(idx, res):
                results[j] = r
        if first is not None:
            j, r, flags = first
            raise engine.DataError(flags, before[j] + r)
    tm["device"] = time.perf_counter() - t1
    return results


def main(argv=None, timings=None):
    """CLI entry.  ``timings`` (a dict, optional) receives the wall seconds of
    the phases: ingest, device (H2D + kernels + D2H), write."""
    t_main = time.perf_counter()
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.gpus < 1:
        parser.error("--gpus must be at least 1")
    tm = timings if timings is not None else {}
    pkg = _cli.package(__file__, __package__)
    ingest, engine, writers = pkg.ingest, pkg.engine, pkg.writers
    _cli.banner(["Engine: libmpc (HIP, gfx950)"])
    # (ref, paf, reads, consensus, chromat, accuracies) per job
    jobs = [] if (args.job and args.REF is None) else \
        [(args.REF, args.PAF, args.READS, args.consensus, args.chromat, args.accuracies)]
    jobs += [(r, p, args.READS, c, ch, a) for r, p, c, ch, a in args.also] + [tuple(j) for j in args.job]
    t0 = time.perf_counter()
    tm["setup"] = t0 - t_main
    try:
        for ref, paf, reads, *_ in jobs:
            statprint(f"Ingesting {paf} against {ref}...")
        results = _ingest_and_pileup(ingest, engine, jobs, args, tm)
        if results is None:  # (:338) max_depth * None, after every file was read
            raise ingest.IngestError("TypeError: --min_depth_factor is required")
        if args.GLOBAL_THRESHOLD_FACTOR is None and any(len(r["count"]) or r["max_depth"] for r in results):
            raise ingest.IngestError("TypeError: --global_threshold_factor is required")  # (:421)
    except (ingest.IngestError, engine.DataError, engine.MpcError, OSError, UnicodeDecodeError) as e:
        return _cli.fail(e)  # (MpcError: input past the engine's limits, e.g. a reference over 2^22 - 2 bases)
    t2 = time.perf_counter()
    for (ref, paf, _, c, ch, acc), res in zip(jobs, results):
        statprint("Max depth is {}.".format(res["max_depth"]))
        statprint("DEPTH_THRESHOLD is {}.".format(res["max_depth"] * args.MIN_DEPTH_FACTOR))
        statprint("Writing consensus, chromatogram data and per-position consensus accuracies...")
        try:
            writers.write_outputs(res, c, ch, acc)
        except OSError as e:  # WriteError included: the reference's open()/write() raise -> exit 1
            return _cli.fail(e)
    tm["write"] = time.perf_counter() - t2
    for src, dst in args.revcomp:
        statprint("Reverse-complementing {} into {}...".format(src, dst))
        try:
            writers.revcomp_consensus(src, dst)
        except (writers.RevcompError, OSError, UnicodeDecodeError) as e:
            return _cli.fail(e)
    statprint("Done.")
    tm["main"] = time.perf_counter() - t_main
    return 0


if __name__ == "__main__":
    sys.exit(main())
