"""linkage_qc: do the minor alleles of a plasmid's variable positions travel together?

  linkage_qc.py --paf sense_final.paf [more.paf ...] --report linkage.tsv [--pairs pairs.tsv] [--haplotypes hap.tsv]
      [--sites FILE | --min-minor-fraction 0.05 --min-minor-count 10]
      [--expected X_adapted_sense.fasta | --region START:END] [--all-alignments]
      [--min-r2 0.1 --min-joint 10] [--max-haplotypes 50] [--device N|cpu] [--strict]

A second peak of 5 % at a few positions is either independent per-position
error, or the same 5 % of the reads carry all of them: a sub-population, a
second clone in the prep.  Per PAF the tool takes the per-position counts
(coverage_qc's walk), selects the variable sites, reads the allele of every
alignment at every site and counts the joint alleles of every site pair, on the
GPU (--device N) or on the host CPUs (--device cpu).

Sites       --sites FILE: lines "target<TAB>1-based position<TAB>base|gap"
            ("gap": the gap before that base; position L + 1 is the gap after
            the last base).  Otherwise selected inside the region (--expected:
            the upper-case plasmid core of a target as long as the
            adapter-padded sequence; --region START:END, 0-based half-open;
            neither: the whole target): a base with mismatch + deleted, a gap
            with insertions, of at least --min-minor-count observations and
            --min-minor-fraction of depth + deleted.  At most 128 sites per
            PAF; beyond that the highest fractions are kept and sites_dropped
            says how many were not.
--report    one block of "key<TAB>value" lines per (paf, target) in a fixed key
            order (REPORT_KEYS), then "verdict<TAB>PASS|FAIL".  A pair is
            linked iff n11 >= --min-joint, the minor alleles co-occur more
            often than chance (n n11 > x y) and r2 >= --min-r2; PASS iff no
            pair of any target is linked.  The default thresholds are starting
            values, not validated on real runs.
--pairs     one line per site pair: the counts n, x, y, n11 over the records
            covered at both sites, r2, linked.
--haplotypes  per target the allele strings of the records covered at every
            site, one character per site ('.' reference, ACGTN substituted
            base, '-' deleted, '+' insertion), with counts, by descending
            count and then by string, at most --max-haplotypes of them.
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
TITLE = "Linkage QC"
REPORT_KEYS = ("paf", "target", "length", "records", "region", "sites", "sites_dropped", "site_list", "major_alleles",
               "minor_counts", "pairs", "linked_pairs", "max_r2", "max_r2_pair", "haplotypes", "records_covered_everywhere")
PAIRS_HEADER = "paf\ttarget\tsite_i\tsite_j\tn\tminor_i\tminor_j\tminor_both\tr2\tlinked\n"
HAPLOTYPES_HEADER = "paf\ttarget\thaplotype\tcount\n"
_ALLELE = "0.ACGTN"


def build_parser():
    p = argparse.ArgumentParser(description=TITLE)
    p.add_argument("--paf", required=True, nargs="+", help="PAF files with cs tags (minimap2 --cs)")
    p.add_argument("--report", required=True, help="Report output file (TSV)")
    p.add_argument("--pairs", help="Per-pair output file (TSV)")
    p.add_argument("--haplotypes", help="Haplotype output file (TSV)")
    p.add_argument("--sites", help="Sites file: target<TAB>1-based position<TAB>base|gap")
    p.add_argument("--min-minor-fraction", type=float, default=0.05, help="Minor fraction a selected site needs")
    p.add_argument("--min-minor-count", type=int, default=10, help="Minor observations a selected site needs")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--expected", help="Adapter-padded reference fasta: select inside the upper-case plasmid core")
    g.add_argument("--region", type=_cli.region_arg, help="START:END (0-based, half-open) of every target")
    p.add_argument("--all-alignments", action="store_true", help="Keep every PAF line, not the first per read name")
    p.add_argument("--min-r2", type=float, default=0.1, help="r2 a linked pair needs")
    p.add_argument("--min-joint", type=int, default=10, help="Records minor at both sites a linked pair needs")
    p.add_argument("--max-haplotypes", type=int, default=50, help="Haplotypes listed per target")
    p.add_argument("--device", type=_cli.device_arg, default=0, help="HIP device index, or 'cpu' for the host walk")
    p.add_argument("--strict", action="store_true", help="Exit status 2 when the verdict is FAIL")
    return p


def _allele(code, key):
    return ("-" if key & 1 else "+") if code == 7 else _ALLELE[code]


def block_values(lnk, b):
    labels = [lnk.site_label(k) for k in b["keys"]]
    minor = [sum(c[1:]) - c[m] for c, m in zip(b["counts"], b["majors"])]
    best = max(b["pairs"], key=lambda t: t[2]["r2"], default=None)
    covered = sum(n for _, n in b["haplotypes"])
    return (b["paf"], b["target"], b["length"], b["records"], "{}:{}".format(*b["region"]), len(labels), b["dropped"],
            ",".join(labels), ",".join(_allele(m, k) for m, k in zip(b["majors"], b["keys"])), ",".join(map(str, minor)),
            len(b["pairs"]), sum(1 for _, _, st in b["pairs"] if st["linked"]), repr(best[2]["r2"]) if best else repr(0.0),
            "{}/{}".format(labels[best[0]], labels[best[1]]) if best else "", len(b["haplotypes"]), covered)


def pairs_text(lnk, res):
    out = [PAIRS_HEADER]
    for b in res["blocks"]:
        head = "{}\t{}\t".format(b["paf"], b["target"])
        labels = [lnk.site_label(k) for k in b["keys"]]
        out += ["{}{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n".format(head, labels[i], labels[j], st["n"], st["x"], st["y"], st["n11"],
                                                           repr(st["r2"]), "yes" if st["linked"] else "no")
                for i, j, st in b["pairs"]]
    return "".join(out)


def haplotypes_text(res, limit):
    out = [HAPLOTYPES_HEADER]
    for b in res["blocks"]:
        out += ["{}\t{}\t{}\t{}\n".format(b["paf"], b["target"], h, n) for h, n in b["haplotypes"][:limit]]
    return "".join(out)


def main(argv=None):
    args = build_parser().parse_args(argv)
    pkg = _cli.package(__file__, __package__)
    lnk = importlib.import_module(pkg.__name__ + ".linkage")
    cov = importlib.import_module(pkg.__name__ + ".coverage")
    if args.min_minor_count < 0 or args.min_joint < 0 or args.max_haplotypes < 0 or not 0.0 <= args.min_minor_fraction <= 1.0:
        return _cli.fail("counts must be >= 0 and --min-minor-fraction in [0, 1]")
    statprint("Reading alleles of {} PAF file(s) on {}...".format(len(args.paf), _cli.place(args.device)))
    try:
        sites = lnk.read_sites(args.sites) if args.sites else None
        res = lnk.qc(args.paf, sites=sites, min_minor_fraction=args.min_minor_fraction, min_minor_count=args.min_minor_count,
                     expected=args.expected, region=args.region, all_alignments=args.all_alignments, min_r2=args.min_r2,
                     min_joint=args.min_joint, device=args.device)
        report = _cli.key_value_report(REPORT_KEYS, (block_values(lnk, b) for b in res["blocks"]), res["verdict"])
        texts = [(args.report, report)]
        if args.pairs:
            texts.append((args.pairs, pairs_text(lnk, res)))
        if args.haplotypes:
            texts.append((args.haplotypes, haplotypes_text(res, args.max_haplotypes)))
    except (lnk.LinkageError, cov.CoverageError, pkg.engine.MpcError, OSError, UnicodeDecodeError) as e:
        return _cli.fail(e)
    for b in res["blocks"]:
        statprint("{} [{}]: {:,} sites, {:,} of {:,} pairs linked, {:,} records".format(
            b["paf"], b["target"], len(b["keys"]), sum(1 for _, _, st in b["pairs"] if st["linked"]), len(b["pairs"]),
            b["records"]))
    return _cli.write_texts(texts) or _cli.verdict_exit("Linkage", args.strict, res["verdict"])


if __name__ == "__main__":
    sys.exit(main())
