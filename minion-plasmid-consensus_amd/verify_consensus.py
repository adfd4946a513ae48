"""verify_consensus: the README's "Check the results" step as a tool.

  verify_consensus.py --expected X_adapted_sense.fasta \\
      --consensus sense_consensus.fasta antisense_consensus_revcomp.fasta \\
      [--accuracies sense_per-base-accuracies.tsv antisense_per-base-accuracies.tsv] \\
      --report verify.tsv [--edits edits.tsv] [--device N|cpu] [--strict]

Every consensus is aligned, exactly and unbanded, with the plasmid core (the
upper-case span of the expected FASTA) and with the whole adapter-padded
sequence; all pairs of a call run in one launch on the GPU (--device N) or on
the host CPUs (--device cpu).

--report  header line, two rows per consensus file (plasmid, adapted), one
          "<path> median_accuracy <median>" row per accuracies file, then
          "verdict PASS|FAIL" (tab-separated).  PASS iff every plasmid row has
          distance 0 and every accuracies median is above 99.9; edits in the
          adapter region never fail the verdict.
--edits   one line per non-'=' op: consensus, region, expected_pos,
          consensus_pos, op, expected_base, consensus_base (1-based positions;
          expected_pos in coordinates of the adapted sequence for both regions;
          a missing side is '-'; an insertion carries the expected position it
          follows, a deletion the consensus position it follows).
Exit status: 0 when the report was written, 2 on FAIL with --strict, 1 (and no
output file) on unreadable or invalid input.
"""
import argparse
import importlib
import sys

if __package__:
    from . import _cli
else:  # run by path: sys.path[0] is this directory
    import _cli

statprint = _cli.statprint
TITLE = "Verify Consensus"
REPORT_HEADER = "consensus\tregion\texpected_len\tconsensus_len\tstart\tend\tdistance\tmismatches\tinsertions\tdeletions\tcigar\n"


def build_parser():
    p = argparse.ArgumentParser(description=TITLE)
    p.add_argument("--expected", required=True, help="Adapter-padded reference fasta (lower-case adapters, upper-case plasmid)")
    p.add_argument("--consensus", required=True, nargs="+", help="Consensus fasta files (antisense: reverse-complemented)")
    p.add_argument("--accuracies", nargs="*", default=[], help="Per-base accuracies files")
    p.add_argument("--report", required=True, help="Report output file (TSV)")
    p.add_argument("--edits", help="Edit list output file (TSV)")
    p.add_argument("--device", type=_cli.device_arg, default=0, help="HIP device index, or 'cpu' for the host scan")
    p.add_argument("--strict", action="store_true", help="Exit status 2 when the verdict is FAIL")
    return p


def report_text(res):
    out = [REPORT_HEADER]
    for r in res["rows"]:
        out.append("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(
            r["consensus"], r["region"], r["expected_len"], r["consensus_len"], r["start"], r["end"], r["distance"],
            r["mismatches"], r["insertions"], r["deletions"], r["cigar"]))
    for path, median in res["medians"]:
        out.append("{}\tmedian_accuracy\t{!r}\n".format(path, median))
    out.append("verdict\t{}\n".format(res["verdict"]))
    return "".join(out)


def edits_text(res):
    return "".join("{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(r["consensus"], r["region"], *e)
                   for r in res["rows"] for e in r["edits"])


def main(argv=None):
    args = build_parser().parse_args(argv)
    pkg = _cli.package(__file__, __package__)
    verify = importlib.import_module(pkg.__name__ + ".verify")
    statprint("Aligning {} consensus file(s) with {} on {}...".format(
        len(args.consensus), args.expected, _cli.place(args.device)))
    try:
        res = verify.verify(args.expected, args.consensus, args.accuracies, device=args.device)
        texts = [(args.report, report_text(res))]
        if args.edits:
            texts.append((args.edits, edits_text(res)))
    except (verify.VerifyError, pkg.engine.MpcError, OSError, UnicodeDecodeError) as e:
        return _cli.fail(e)
    for r in res["rows"]:
        statprint("{} [{}]: distance {} over consensus [{}, {})".format(r["consensus"], r["region"], r["distance"],
                                                                        r["start"], r["end"]))
    return _cli.write_texts(texts) or _cli.verdict_exit("Verdict", args.strict, res["verdict"])


if __name__ == "__main__":
    sys.exit(main())
