"""Inputs that pin the host pieces csrc/host_file.h states once for the three
PAF parsers (ingest.cpp, coverage.cpp, pseudopair.cpp): the decimal fields
each parser's plain_int takes, and the files whose cuts at line starts are the
edge cases of line_start_at_or_after.  One PAF text serves all three parsers
(12 columns, a tp tag, the cs tag)."""

D18, D19 = "123456789012345678", "1234567890123456789"

# field -> (ingest, coverage, pseudopair).  The expectations restate the rules,
# not the code: ingest follows Python's int() ("ok": [-]digits, at most 18, read
# natively; "error": int() raises; "python": int() accepts a form the native
# parser leaves to it); coverage takes 1-18 digits and nothing else; pseudopair
# takes [+-] and 1-18 digits, everything else it declines.
PLAIN_INT = {
    "": ("error", False, False),
    "0": ("ok", True, True),
    "-5": ("ok", False, True),
    "+5": ("python", False, True),
    "1_0": ("python", False, False),
    " 7": ("python", False, False),
    D18: ("ok", True, True),
    D19: ("python", False, False),
}

REF = ">r\nACGTACGTAC\n"
READS = ">a\nACGTACGTACGT\n>b\nTTACGTACGTACGG\n>c\nACGTACGTAC\n"


def paf_line(name, qlen, qs, qe, strand, ts, cs):
    return "\t".join([name, str(qlen), str(qs), str(qe), strand, "ref", "100", str(ts), "9", "9", "9", "60", "tp:A:P",
                      "cs:Z:" + cs]) + "\n"


A, B, C = paf_line("a", 12, 1, 11, "+", 0, ":10"), paf_line("b", 14, 2, 12, "-", 0, ":4*ag:5"), paf_line("c", 10, 0, 10, "+", 0, ":10")

# 16 threads cut a file at n k / 16: in `long_line` one line of 1.2 MB spans most
# of them, so consecutive cuts coincide at its end (coverage's ingest takes one
# thread per 64 KiB, so only a file this long gives it 16)
PAF_FILES = {
    "empty": "",
    "one_line": A,
    "one_line_no_newline": A.rstrip("\n"),
    "fewer_lines_than_threads": A + B + C,
    "long_line": A + paf_line("b", 14, 2, 12, "-", 0, ":1" * 600_000) + C,
}


def write_paf_files(folder):
    """{name: path} of PAF_FILES written under folder."""
    paths = {}
    for name, text in PAF_FILES.items():
        paths[name] = str(folder / (name + ".paf"))
        with open(paths[name], "w") as f:
            f.write(text)
    return paths
