"""coverage_qc: the README's coverage criterion as a tool, from the PAF alone.

  coverage_qc.py --paf sense_final.paf [more.paf ...] --report coverage.tsv [--per-base depth.tsv]
      [--expected X_adapted_sense.fasta | --region START:END] [--all-alignments]
      [--min-mean-coverage 100000] [--min-depth 0] [--device N|cpu] [--strict]

Every alignment's target span and cs tag are walked once; all PAFs and all
their targets go through one launch on the GPU (--device N) or the scalar walk
on the host CPUs (--device cpu).  By default the first alignment per read name
counts (what the consensus is called from); --all-alignments keeps every line.

Region      --expected: a target as long as the adapter-padded sequence is
            measured over its upper-case plasmid core; --region START:END
            (0-based, half-open) applies to every target; neither: the whole
            target.
--report    one block of "key<TAB>value" lines per (paf, target) in a fixed key
            order (REPORT_KEYS; depth = aligned bases, deletions do not count;
            min_depth_position is 1-based, the first position of the minimum;
            floats as Python repr), then "verdict<TAB>PASS|FAIL".  PASS iff
            every block has mean_depth >= --min-mean-coverage and no region
            position below --min-depth.
--per-base  "paf target pos depth deleted mismatch insertion" (tab-separated,
            1-based positions), one line per row, row L + 1 (insertions after
            the last base) included.
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
TITLE = "Coverage QC"
REPORT_KEYS = ("paf", "target", "length", "records", "region", "mean_depth", "sd_depth", "min_depth",
               "min_depth_position", "max_depth", "positions_below_min_depth", "mean_deleted", "match_bases",
               "mismatch_bases", "inserted_bases", "deleted_bases", "insertion_events", "deletion_events", "error_rate",
               "mean_mapq", "mean_read_length", "plus_strand_records", "minus_strand_records")
PER_BASE_HEADER = "paf\ttarget\tpos\tdepth\tdeleted\tmismatch\tinsertion\n"


def build_parser():
    p = argparse.ArgumentParser(description=TITLE)
    p.add_argument("--paf", required=True, nargs="+", help="PAF files with cs tags (minimap2 --cs)")
    p.add_argument("--report", required=True, help="Report output file (TSV)")
    p.add_argument("--per-base", help="Per-position output file (TSV)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--expected", help="Adapter-padded reference fasta: measure the upper-case plasmid core")
    g.add_argument("--region", type=_cli.region_arg, help="START:END (0-based, half-open) of every target")
    p.add_argument("--all-alignments", action="store_true", help="Keep every PAF line, not the first per read name")
    p.add_argument("--min-mean-coverage", type=float, default=100000.0, help="Mean depth every target needs to PASS")
    p.add_argument("--min-depth", type=int, default=0, help="Depth every region position needs to PASS")
    p.add_argument("--device", type=_cli.device_arg, default=0, help="HIP device index, or 'cpu' for the host walk")
    p.add_argument("--strict", action="store_true", help="Exit status 2 when the verdict is FAIL")
    return p


def block_values(cov, b):
    st = b["stats"]
    return (b["paf"], b["target"], b["length"], b["records"], "{}:{}".format(*b["region"]), repr(b["mean"]),
            repr(b["sd"]), st[cov.ST_MIN], b["min_position"], st[cov.ST_MAX], st[cov.ST_BELOW], repr(b["mean_deleted"]),
            st[cov.ST_MATCH], st[cov.ST_MISMATCH], st[cov.ST_INS_BASES], st[cov.ST_DEL_BASES], st[cov.ST_INS_EVENTS],
            st[cov.ST_DEL_EVENTS], repr(b["error_rate"]), repr(b["mean_mapq"]), repr(b["mean_read_length"]), b["plus"],
            b["minus"])


def per_base_text(res):
    out = [PER_BASE_HEADER]
    for b in res["blocks"]:
        head = "{}\t{}\t".format(b["paf"], b["target"])
        out += ["{}{}\t{}\t{}\t{}\t{}\n".format(head, k + 1, *row) for k, row in enumerate(b["rows"].tolist())]
    return "".join(out)


def main(argv=None):
    args = build_parser().parse_args(argv)
    pkg = _cli.package(__file__, __package__)
    cov = importlib.import_module(pkg.__name__ + ".coverage")
    if args.min_depth < 0 or args.min_depth >= 2 ** 32:
        return _cli.fail("--min-depth must be in [0, 2^32)")
    statprint("Walking {} PAF file(s) on {}...".format(len(args.paf), _cli.place(args.device)))
    try:
        res = cov.qc(args.paf, expected=args.expected, region=args.region, all_alignments=args.all_alignments,
                     min_mean_coverage=args.min_mean_coverage, min_depth=args.min_depth, device=args.device)
        report = _cli.key_value_report(REPORT_KEYS, (block_values(cov, b) for b in res["blocks"]), res["verdict"])
        texts = [(args.report, report)]
        if args.per_base:
            texts.append((args.per_base, per_base_text(res)))
    except (cov.CoverageError, pkg.engine.MpcError, OSError, UnicodeDecodeError) as e:
        return _cli.fail(e)
    for b in res["blocks"]:
        statprint("{} [{}]: mean {:,.1f}x, minimum {:,}x at position {:,}, {:,} records".format(
            b["paf"], b["target"], b["mean"], b["stats"][cov.ST_MIN], b["min_position"], b["records"]))
    return _cli.write_texts(texts) or _cli.verdict_exit("Coverage", args.strict, res["verdict"])


if __name__ == "__main__":
    sys.exit(main())
