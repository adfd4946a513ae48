"""reads_consensus: reads -> alignment -> pileup -> consensus in one run.

  reads_consensus.py --reads merged.fasta --ref assembled_sense.fasta \\
      --consensus sense_consensus.fasta --chromat sense_chromatogram-data.tsv \\
      --accuracies sense_per-base-accuracies.tsv --min_depth_factor 0.1 --global_threshold_factor 5 \\
      [--also assembled_antisense.fasta CONSENSUS CHROMAT ACCURACIES] [--paf sense_final.paf] \\
      [--max-error 0.2] [--summary align.tsv] [--device N]

Replaces, for the inputs below, two commands per strand,

  align_reads.py --ref T --reads R --paf P --max-error E
  mapped_paf_read_parser.py --ref T --reads R --paf P ... (the same factors)

with one pass over the reads: every batch is aligned to every target as
align_reads aligns it, and each launch's edit scripts become the pileup's
inputs on the device (handoff.py: K_acslen, K_acswrite).  At the end all
targets are the samples of one pileup launch.  The three files of every target,
and the exit status, are those of the two commands; --paf (the first target's
PAF, rendered on the host as align_reads does, for coverage_qc / linkage_qc)
and --summary (align_reads' table for the first target) are optional.

The tool refuses up front, with an Error: line naming the read and exit status
1, what it could not answer as the two commands do: a read name that occurs
twice; a mapped read whose header line holds more than its name, whose name is
empty, starts with "cs:" or holds a byte outside printable ASCII; a read mapped
to '-' with a letter other than A C G T N.  (For the last and for a header with
a description the two commands exit 1 as well.)  A data error of the pileup, an
assembly that is not one record or is longer than 2^22 - 2 bases: exit 1, no
output files, as before.

There is no --device cpu: the pileup has no host path.
"""
import argparse
import importlib
import os
import sys

if __package__:
    from . import _cli
else:  # run by path: sys.path[0] is this directory
    import _cli

statprint = _cli.statprint
TITLE = "Reads Consensus"


def build_parser():
    p = argparse.ArgumentParser(description=TITLE)
    p.add_argument("--reads", required=True, help="Raw reads fasta file")
    p.add_argument("--ref", required=True, help="Assembly fasta (exactly one record)")
    p.add_argument("--consensus", required=True, help="Consensus output file")
    p.add_argument("--chromat", required=True, help="Chromatogram data output file")
    p.add_argument("--accuracies", required=True, help="Per position consensus accuracies output file")
    p.add_argument("--min_depth_factor", dest="MIN_DEPTH_FACTOR", type=float,
                   help="Minimum number of reads needed to call a base is set to max_depth*MIN_DEPTH_FACTOR")
    p.add_argument("--global_threshold_factor", dest="GLOBAL_THRESHOLD_FACTOR", type=float,
                   help="Value of minimum most frequent to second most frequent base ratio to make call")
    p.add_argument("--also", nargs=4, action="append", default=[], metavar=("REF", "CONSENSUS", "CHROMAT", "ACCURACIES"),
                   help="another assembly against the same reads, same pass, same pileup launch; repeatable")
    p.add_argument("--paf", help="also write the first assembly's PAF (as align_reads writes it)")
    p.add_argument("--max-error", type=_cli.fraction_arg, default=0.2, help="Largest distance of a mapped read, as a fraction of its length")
    p.add_argument("--summary", help="align_reads' summary of the first assembly (TSV)")
    p.add_argument("--device", type=_cli.gpu_arg, default=0, help="HIP device index")
    return p


def _discard(path):
    try:
        os.remove(path)
    except OSError:
        pass


def main(argv=None):
    args = build_parser().parse_args(argv)
    pkg = _cli.package(__file__, __package__)
    handoff = importlib.import_module(pkg.__name__ + ".handoff")
    align, engine, ingest, writers = handoff.align, pkg.engine, pkg.ingest, pkg.writers
    _cli.banner(["Engine: libmpc (HIP, gfx950)"])
    jobs = [(args.ref, args.consensus, args.chromat, args.accuracies)] + [tuple(j) for j in args.also]
    mdf, gtf = args.MIN_DEPTH_FACTOR, args.GLOBAL_THRESHOLD_FACTOR
    statprint("Aligning {} to {} on {}...".format(args.reads, ", ".join(j[0] for j in jobs), _cli.place(args.device)))
    tmp = "{}.tmp.{}".format(args.paf, os.getpid()) if args.paf else None  # renamed once everything succeeded
    try:
        f = open(tmp, "wb") if tmp else None
        try:
            targets, _ = handoff.collect([j[0] for j in jobs], args.reads, args.device, args.max_error,
                                         paf=f.write if f else None)
        finally:
            if f:
                f.close()
        for t in targets:
            statprint("There were {} mapped reads.".format(t.pile.n_reads))
        if mdf is None:  # (the drop-in: max_depth * None, after every file was read)
            raise ingest.IngestError("TypeError: --min_depth_factor is required")
        statprint("Pileup and consensus on device {}...".format(args.device))
        batch = engine.Batch.from_device([t.pile.sample(t.ref) for t in targets], device=args.device)
        results = engine.pileup_batch(batch, mdf, 1.0 if gtf is None else gtf)
        if gtf is None and any(len(r["count"]) or r["max_depth"] for r in results):
            raise ingest.IngestError("TypeError: --global_threshold_factor is required")
    except (align.AlignError, ingest.IngestError, engine.DataError, engine.MpcError, OSError, UnicodeDecodeError) as e:
        if tmp:
            _discard(tmp)
        return _cli.fail(e)
    except BaseException:
        if tmp:
            _discard(tmp)
        raise
    for (_, c, ch, acc), res in zip(jobs, results):
        statprint("Max depth is {}.".format(res["max_depth"]))
        statprint("DEPTH_THRESHOLD is {}.".format(res["max_depth"] * mdf))
        statprint("Writing consensus, chromatogram data and per-position consensus accuracies...")
        try:
            writers.write_outputs(res, c, ch, acc)
        except OSError as e:
            if tmp:
                _discard(tmp)
            return _cli.fail(e)
    try:
        if tmp:
            os.replace(tmp, args.paf)
        if args.summary:
            with open(args.summary, "w") as f:
                f.write(align.summary_text(targets[0].summary))
    except OSError as e:
        return _cli.fail(e)
    s = targets[0].summary
    statprint("{} reads: {} mapped ({} +, {} -), {} unmapped, {} skipped by length".format(
        s["reads"], s["mapped"], s["plus"], s["minus"], s["unmapped_by_distance"] + s["unmapped_no_match"],
        s["skipped_length"]))
    statprint("Done.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
