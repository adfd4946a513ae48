"""draft_assembly: the sense and antisense assembly from the first reads of merged.fasta.

  draft_assembly.py --reads merged.fasta --sense assembled_sense.fasta --antisense assembled_antisense.fasta \\
      [--sample 500] [--candidates 8] [--rounds 3] [--max-error 0.3] [--orient-to FASTA] [--report FILE]
      [--device N|cpu] [--threads N]

Replaces canu in the reference Snakefile's rules subsample_fasta,
canu_denovo_assembly, select_top_assembly and revcomp_assembly for their
input: every read a full-length copy of one linearised plasmid on either
strand.  The most central of the first reads is the first draft; the sample is
aligned to it exactly (as align_reads does), every column and every gap is put
to a majority vote against the coverage of that place, and the result is the
next draft (include/mpc_draft.h has the definition).  It runs on the GPU
(--device N) or on the host CPUs (--device cpu); the two write the same bytes.
It is not an assembler: reads that are not full-length copies of one molecule
give no meaningful draft.

--sense      '>draft_sense' and the draft on one line
--antisense  '>draft_antisense' and its reverse complement
--sample     reads taken from the head of --reads (0: all); 500 mirrors head -1000
--orient-to  a one-record FASTA: when the reverse complement of the draft lies
             nearer to it than the draft, the two outputs swap
--report     key<TAB>value lines: the sample, the seed, every round's mapped reads,
             length, trimmed head / tail, changed / dropped / inserted bases, and
             'converged yes|no' (a round returned its draft unchanged)
Exit status: 0 when both files were written, 1 (and no output file) on
unreadable or rejected input: no read of supported length, a sequence byte that
is not an ASCII letter, no read that maps to the draft.
"""
import argparse
import importlib
import sys

if __package__:
    from . import _cli
else:  # run by path: sys.path[0] is this directory
    import _cli

statprint = _cli.statprint
TITLE = "Draft Assembly"


def _count(least):
    def parse(text):
        try:
            v = int(text)
        except ValueError:
            v = least - 1
        if v < least:
            raise argparse.ArgumentTypeError("an integer >= {}".format(least))
        return v
    return parse


def build_parser():
    p = argparse.ArgumentParser(description=TITLE)
    p.add_argument("--reads", required=True, help="Reads fasta")
    p.add_argument("--sense", required=True, help="Sense assembly output (fasta)")
    p.add_argument("--antisense", required=True, help="Antisense assembly output (fasta)")
    p.add_argument("--sample", type=_count(0), default=500, help="Reads taken from the head of the file (0: all)")
    p.add_argument("--candidates", type=_count(1), default=8, help="Reads nearest the median length tried as the seed")
    p.add_argument("--rounds", type=_count(0), default=3, help="Most rounds of align, vote and call")
    p.add_argument("--max-error", type=_cli.fraction_arg, default=0.3, help="Largest distance of a mapped read, as a fraction of its length")
    p.add_argument("--orient-to", help="Fasta (one record) whose strand the sense output takes")
    p.add_argument("--report", help="Report output file (key<TAB>value)")
    p.add_argument("--device", type=_cli.device_arg, default=0, help="HIP device index, or 'cpu' for the host path")
    p.add_argument("--threads", type=_count(0), default=0, help="Host threads of the host path (0: the job's CPU share)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    pkg = _cli.package(__file__, __package__)
    draft = importlib.import_module(pkg.__name__ + ".draft")
    statprint("Drafting the assembly from {} on {}...".format(args.reads, _cli.place(args.device)))
    try:
        res = draft.assemble(args.reads, sample=args.sample, candidates=args.candidates, rounds=args.rounds,
                             max_error=args.max_error, device=args.device, threads=args.threads, orient_to=args.orient_to)
    except (draft.DraftError, pkg.align.AlignError, pkg.engine.MpcError, OSError) as e:
        return _cli.fail(e)
    texts = [(args.sense, ">draft_sense\n{}\n".format(res["sense"].decode("ascii"))),
             (args.antisense, ">draft_antisense\n{}\n".format(res["antisense"].decode("ascii")))]
    if args.report:
        keys, values = zip(*res["report"])
        texts.append((args.report, _cli.key_value_report(keys, [values], "yes" if res["converged"] else "no", "converged")))
    rep = dict(res["report"])
    statprint("{} reads sampled, seed {} ({:,} bases), draft of {:,} bases, {}".format(
        rep["sample_reads"], rep["seed"], rep["seed_length"], len(res["sense"]),
        "converged" if res["converged"] else "not converged"))
    rc = _cli.write_texts(texts)
    if rc == 0:
        statprint("Done.")
    return rc


if __name__ == "__main__":
    sys.exit(main())
