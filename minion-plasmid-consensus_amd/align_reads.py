"""align_reads: the reads of merged.fasta aligned to an assembly, as a cs-tagged PAF.

  align_reads.py --ref assembled_sense.fasta --reads merged.fasta --paf sense_final.paf \\
      [--max-error 0.2] [--summary FILE] [--device N|cpu]

Replaces `minimap2 -x map-ont --cs` of the reference Snakefile's rule
final_alignment_paf for its inputs: every read a full-length copy of the
plasmid on either strand, the assembly one sequence.  Every read is aligned
exactly (unit costs, both strands, no heuristics; include/mpc_align.h has the
definition) on the GPU (--device N) or on the host CPUs (--device cpu); the two
write the same bytes.

--paf        one line per mapped read, in the order of --reads: the twelve PAF
             columns, NM:i: and the short-form cs:Z: tag.  A read is mapped iff
             its distance is at most floor(max-error x its length) (and at most
             4096) and its alignment holds at least one match.
--summary    TSV: reads, mapped, plus, minus, unmapped_by_distance,
             unmapped_no_match, skipped_length (reads of 0 or more than 65,536
             bases are skipped and counted).
Exit status: 0 when the PAF was written, 1 (and no PAF) on unreadable or
rejected input: an assembly that is not exactly one non-empty record, a
sequence byte that is not an ASCII letter.
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
TITLE = "Align Reads"


def build_parser():
    p = argparse.ArgumentParser(description=TITLE)
    p.add_argument("--ref", required=True, help="Assembly fasta (exactly one record)")
    p.add_argument("--reads", required=True, help="Reads fasta")
    p.add_argument("--paf", required=True, help="PAF output file")
    p.add_argument("--max-error", type=_cli.fraction_arg, default=0.2, help="Largest distance of a mapped read, as a fraction of its length")
    p.add_argument("--summary", help="Summary output file (TSV)")
    p.add_argument("--device", type=_cli.device_arg, default=0, help="HIP device index, or 'cpu' for the host path")
    return p


def _discard(path):
    try:
        os.remove(path)
    except OSError:
        pass


def main(argv=None):
    args = build_parser().parse_args(argv)
    pkg = _cli.package(__file__, __package__)
    align = importlib.import_module(pkg.__name__ + ".align")
    statprint("Aligning {} to {} on {}...".format(args.reads, args.ref, _cli.place(args.device)))
    tmp = "{}.tmp.{}".format(args.paf, os.getpid())  # renamed once complete: no PAF on rejected input
    try:
        with open(tmp, "wb") as f:
            res = align.align(args.ref, args.reads, device=args.device, max_error=args.max_error, write=f.write)
        os.replace(tmp, args.paf)
        if args.summary:
            with open(args.summary, "w") as f:
                f.write(align.summary_text(res["summary"]))
    except (align.AlignError, pkg.engine.MpcError, OSError) as e:
        _discard(tmp)
        return _cli.fail(e)
    except BaseException:
        _discard(tmp)
        raise
    s = res["summary"]
    statprint("{} reads: {} mapped ({} +, {} -), {} unmapped, {} skipped by length".format(
        s["reads"], s["mapped"], s["plus"], s["minus"], s["unmapped_by_distance"] + s["unmapped_no_match"],
        s["skipped_length"]))
    statprint("Done.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
