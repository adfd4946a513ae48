"""The invocations whose transcripts tests/cli_transcripts/ holds, how one is
run and masked, and the recorder.

A transcript is the exit status, stdout, stderr and every file an invocation
left in its working directory beside its inputs.  A case builds its inputs from
the test helpers' seeded generators into that directory and names them
relatively, so no path needs masking; masked are the [YYYY/MM/DD HH:MM:SS] stamp
and, in the two drop-ins' banners, the value of every line but Engine:.

The transcripts are recorded from the command-line files of the commit BEFORE
the one that changes that layer, never from the tree under test:

    python tests/cli_cases.py <package dir of that commit> [cpu|gpu]

(gpu: the --device 0 cases, on an MI355X).  Where that commit's tool cannot run
by path -- pseudopair_reads.py did not, its relative import failed -- the case
is recorded through main(argv) of the imported module instead.
"""
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TRANSCRIPTS = os.path.join(HERE, "cli_transcripts")
PKGDIR = os.path.join(os.path.dirname(HERE), "minion-plasmid-consensus_amd")
_STAMP = re.compile(r"\[\d{4}/\d\d/\d\d \d\d:\d\d:\d\d\]")
_RULE = "=" * 55
_KEY = re.compile(r"[A-Z][A-Za-z ]*: ")


def mask(text):
    out, banner = [], False
    for line in _STAMP.sub("[STAMP]", text).split("\n"):
        if line == _RULE:
            banner = not banner
        elif banner and not line.startswith("Engine:"):
            m = _KEY.match(line)
            if not m:
                continue  # the second line of a two-line sys.version
            line = m.group(0) + "*"
        out.append(line)
    return "\n".join(out)


# ---------------------------------------------------------------- the cases
# build(d, device) writes the inputs into directory d and returns the argv

def _write(d, name, data):
    with open(os.path.join(d, name), "wb") as f:
        f.write(data if isinstance(data, bytes) else data.encode())
    return name


def _verify_inputs(d):
    import verify_util as vu
    rng = np.random.default_rng(61)
    up, core, down = vu.rand_seq(rng, 12).lower(), vu.rand_seq(rng, 60), vu.rand_seq(rng, 10).lower()
    hit = bytearray(core)
    hit[30] = ord("A") if hit[30] != ord("A") else ord("C")
    _write(d, "x_adapted.fasta", b">x\n" + up + core + down + b"\n")
    _write(d, "exact.fasta", b">consensus\n" + (up + core + down).upper() + b"\n")
    _write(d, "sub.fasta", b">consensus\n" + up.upper() + bytes(hit) + down.upper())
    for name, vals in (("a1.tsv", [100.0, 99.95, 99.99]), ("a2.tsv", [100.0, 99.0, 98.5, 100.0])):
        _write(d, name, "pos\taccuracy\n" + "".join("%d\t%r\n" % (k + 1, v) for k, v in enumerate(vals)))


def verify_fail(d, device):
    _verify_inputs(d)
    return ["--expected", "x_adapted.fasta", "--consensus", "exact.fasta", "sub.fasta", "--accuracies", "a1.tsv", "a2.tsv",
            "--report", "verify.tsv", "--edits", "edits.tsv", "--strict", "--device", device]


def verify_missing(d, device):
    _verify_inputs(d)
    return ["--expected", "x_adapted.fasta", "--consensus", "exact.fasta", "missing.fasta", "--report", "verify.tsv",
            "--edits", "edits.tsv", "--device", device]


def _coverage_inputs(d):
    """a.paf: 'plasmid' (40 bases) and 'other' (30 bases, nothing on 0-2 and 23-29); b.paf: 'plasmid' alone."""
    import link_util as lu
    a = [(0, 0, b":40"), (0, 0, b":10*ag:29"), (0, 5, b":10-ac:8+tt:5"), (0, 12, b":20"), (1, 3, b":20"), (1, 5, b":5*ct:9")]
    lu.write_paf(os.path.join(d, "a.paf"), a, ["plasmid", "other"], [40, 30])
    lu.write_paf(os.path.join(d, "b.paf"), [(0, 0, b":40"), (0, 2, b":30")], ["plasmid"], [40])
    return ["--paf", "a.paf", "b.paf", "--report", "cov.tsv"]


def coverage_region(d, device):
    return _coverage_inputs(d) + ["--per-base", "depth.tsv", "--region", "5:25", "--min-mean-coverage", "1", "--device", device]


def coverage_expected(d, device):
    _write(d, "x_adapted.fasta", b">x\nacgta" + b"ACGTTGCAAG" * 3 + b"tgcat\n")  # 5 + 30 + 5 = 'plasmid'
    return _coverage_inputs(d) + ["--per-base", "depth.tsv", "--expected", "x_adapted.fasta", "--min-mean-coverage", "1",
                                  "--device", device]


def coverage_strict_fail(d, device):
    return _coverage_inputs(d) + ["--min-mean-coverage", "0", "--min-depth", "1", "--strict", "--device", device]


def coverage_bad_cs(d, device):
    argv = _coverage_inputs(d)
    with open(os.path.join(d, "b.paf")) as f:
        lines = f.read().split("\n")
    lines[1] = lines[1].replace("cs:Z::", "cs:Z:=")
    _write(d, "b.paf", "\n".join(lines))
    return argv + ["--per-base", "depth.tsv", "--device", device]


def coverage_min_depth(d, device):
    return _coverage_inputs(d) + ["--min-depth", "-1", "--device", device]


def coverage_region_outside(d, device):
    return _coverage_inputs(d) + ["--region", "5:900", "--device", device]


def coverage_unwritable(d, device):
    os.mkdir(os.path.join(d, "depth_dir"))
    return _coverage_inputs(d) + ["--per-base", "depth_dir", "--min-mean-coverage", "1", "--device", device]


PLANTED_N = 6  # the first records of link_util.planted(): the fewest (two carriers) with which the thresholds below still link
_LINK_FLAGS = ["--min-minor-fraction", "0.02", "--min-minor-count", "2", "--min-r2", "0.5", "--min-joint", "2"]


def _linkage_inputs(d, carriers=True):
    import link_util as lu
    lu.write_paf(os.path.join(d, "in.paf"), lu.planted(carriers)[0][:PLANTED_N], ["plasmid"], [300])
    return ["--paf", "in.paf", "--report", "linkage.tsv"]


def linkage_planted(d, device):
    return _linkage_inputs(d) + ["--pairs", "pairs.tsv", "--haplotypes", "hap.tsv", "--strict", "--device", device] + _LINK_FLAGS


def linkage_clean(d, device):
    return _linkage_inputs(d, False) + ["--pairs", "pairs.tsv", "--haplotypes", "hap.tsv", "--strict", "--device", device] + _LINK_FLAGS


def linkage_sites_missing(d, device):
    _write(d, "sites.tsv", "nosuch\t51\tbase\n")
    return _linkage_inputs(d) + ["--sites", "sites.tsv", "--device", device]


def linkage_fraction(d, device):
    return _linkage_inputs(d) + ["--min-minor-fraction", "2", "--device", device]


def _align_reads(d):
    import align_util as au
    import verify_util as vu
    rng = np.random.default_rng(67)
    ref = vu.rand_seq(rng, 80)
    reads = [(b"plus", au.plant_subs(rng, ref[10:60], 1)), (b"minus", au.revcomp(ref[20:70])),
             (b"far", vu.rand_seq(rng, 50)), (b"empty", b"")]
    _write(d, "reads.fa", b"".join(b">" + n + b"\n" + s + b"\n" for n, s in reads))
    return ref


def align_four(d, device):
    _write(d, "ref.fa", b">plasmid\n" + _align_reads(d) + b"\n")
    return ["--ref", "ref.fa", "--reads", "reads.fa", "--paf", "out.paf", "--summary", "summary.tsv", "--device", device]


def align_two_records(d, device):
    ref = _align_reads(d)
    _write(d, "ref.fa", b">a\n" + ref + b"\n>b\n" + ref + b"\n")
    return ["--ref", "ref.fa", "--reads", "reads.fa", "--paf", "out.paf", "--summary", "summary.tsv", "--device", device]


def pseudopair_thrice(d, device):
    rows = [("f1", 100, 0, 90, "+"), ("r1", 100, 5, 95, "-"), ("f1", 100, 0, 50, "+"), ("f2", 80, 0, 3, "+"),
            ("f1", 100, 10, 70, "+"), ("r2", 60, 0, 60, "-")]
    _write(d, "in.paf", "".join("%s\t%d\t%d\t%d\t%s\tplasmid\n" % r for r in rows))
    return ["--paf", "in.paf", "--min_align_length", "5", "--pseudopairs", "pairs.txt"]


def pseudopair_short_line(d, device):
    _write(d, "in.paf", "f1\t100\t0\t90\t+\tplasmid\nr1\t100\t5\t95\n")
    return ["--paf", "in.paf", "--min_align_length", "5", "--pseudopairs", "pairs.txt"]


def _golden(d, case, more=()):
    import golden_util as gu
    gu.materialize(case, d)
    run = next(iter(gu.runs(case)))[1]
    return ["--ref", "ref.fa", "--reads", "reads.fa", "--paf", "in.paf", "--consensus", "c.fa", "--chromat", "ch.tsv",
            "--accuracies", "acc.tsv", "--min_depth_factor", repr(run["mdf"]), "--global_threshold_factor", repr(run["gtf"])] + list(more)


def dropin_missing_read(d, device):
    return _golden(d, "t4_missing_read")


SMALLEST_PASSING = "e_empty_paf"      # the smallest golden case that exits 0: no alignment at all
SMALLEST_ALIGNED = "e_del_past_end_ok"  # the smallest that exits 0 with an alignment in its PAF
NEGATIVE_START = "n_neg_far_del"
_ALSO = ["--gpus", "2", "--also", "ref.fa", "in.paf", "c_also.fa", "ch_also.tsv", "acc_also.tsv"]


def dropin_device(d, device):
    return _golden(d, SMALLEST_ALIGNED, ["--device", device])


def dropin_gpus2_also(d, device):
    return _golden(d, SMALLEST_ALIGNED, _ALSO)


def dropin_device_empty(d, device):
    return _golden(d, SMALLEST_PASSING, ["--device", device])


def dropin_gpus2_also_empty(d, device):
    return _golden(d, SMALLEST_PASSING, _ALSO)


def dropin_negative_start(d, device):
    return _golden(d, NEGATIVE_START, ["--device", device])


# name -> (tool, build); the CPU cases run with --device cpu, the GPU cases with --device 0
CPU_CASES = {
    "verify_fail": ("verify_consensus", verify_fail), "verify_missing": ("verify_consensus", verify_missing),
    "coverage_region": ("coverage_qc", coverage_region), "coverage_expected": ("coverage_qc", coverage_expected),
    "coverage_strict_fail": ("coverage_qc", coverage_strict_fail), "coverage_bad_cs": ("coverage_qc", coverage_bad_cs),
    "coverage_min_depth": ("coverage_qc", coverage_min_depth), "coverage_region_outside": ("coverage_qc", coverage_region_outside),
    "coverage_unwritable": ("coverage_qc", coverage_unwritable),
    "linkage_planted": ("linkage_qc", linkage_planted), "linkage_clean": ("linkage_qc", linkage_clean),
    "linkage_sites_missing": ("linkage_qc", linkage_sites_missing), "linkage_fraction": ("linkage_qc", linkage_fraction),
    "align_four": ("align_reads", align_four), "align_two_records": ("align_reads", align_two_records),
    "pseudopair_thrice": ("pseudopair_reads", pseudopair_thrice), "pseudopair_short_line": ("pseudopair_reads", pseudopair_short_line),
    "dropin_missing_read": ("mapped_paf_read_parser", dropin_missing_read),
}
# one case per tool that main(argv) of the imported module repeats
IMPORTED = ("verify_fail", "coverage_region", "linkage_planted", "align_four", "pseudopair_thrice", "dropin_missing_read")
GPU_CASES = {
    "verify_fail": CPU_CASES["verify_fail"], "coverage_region": CPU_CASES["coverage_region"],
    "linkage_planted": CPU_CASES["linkage_planted"], "align_four": CPU_CASES["align_four"],
    "dropin_device": ("mapped_paf_read_parser", dropin_device), "dropin_gpus2_also": ("mapped_paf_read_parser", dropin_gpus2_also),
    "dropin_negative_start": ("mapped_paf_read_parser", dropin_negative_start),
    "dropin_device_empty": ("mapped_paf_read_parser", dropin_device_empty),
    "dropin_gpus2_also_empty": ("mapped_paf_read_parser", dropin_gpus2_also_empty),
}


def gpu_env(name):
    """--gpus 2 names the devices it uses and warns where they are one: that case sees one device on every box."""
    return dict(os.environ, HIP_VISIBLE_DEVICES="0") if name.startswith("dropin_gpus2_also") else None


# (tool, argv): argparse's own refusals; only the last stderr line is compared
USAGE = [(tool, ["--device", "x"]) for tool in ("verify_consensus", "coverage_qc", "linkage_qc", "align_reads")] + \
        [(tool, ["--region", "5"]) for tool in ("coverage_qc", "linkage_qc")] + [("mapped_paf_read_parser", ["--gpus", "0"])]


# ---------------------------------------------------------------- running one

def _left(d, inputs):
    out = {}
    for name in sorted(set(os.listdir(d)) - inputs):
        path = os.path.join(d, name)
        if os.path.isfile(path):
            with open(path, "rb") as f:
                out[name] = f.read().decode("ascii")
    return out


_IMPORTED = "import importlib, sys; sys.path.insert(0, sys.argv[1]); sys.exit(importlib.import_module(sys.argv[2]).main(sys.argv[3:]))"


def run_by_path(pkgdir, tool, build, d, device, env=None, imported=False):
    """The transcript of `python <pkgdir>/<tool>.py argv` in directory d
    (imported, the recorder's way out: of main(argv) of the imported module in a process of its own)."""
    d = str(d)
    argv = build(d, device)
    inputs = set(os.listdir(d))
    cmd = [os.path.join(pkgdir, tool + ".py")]
    if imported:
        cmd = ["-c", _IMPORTED, os.path.dirname(pkgdir), os.path.basename(pkgdir) + "." + tool]
    p = subprocess.run([sys.executable] + cmd + argv, cwd=d, capture_output=True, text=True, timeout=300, env=env)
    return dict(exit=p.returncode, stdout=mask(p.stdout), stderr=mask(p.stderr), files=_left(d, inputs))


def run_imported(pkg_name, tool, build, d, device, capfd):
    """The same through main(argv) of the imported module; the caller has made d the working directory."""
    d = str(d)
    argv = build(d, device)
    inputs = set(os.listdir(d))
    main = importlib.import_module(pkg_name + "." + tool).main
    capfd.readouterr()
    try:
        rc = main(argv)
    except SystemExit as e:
        rc = e.code
    sys.stdout.flush()
    out, err = capfd.readouterr()
    return dict(exit=rc, stdout=mask(out), stderr=mask(err), files=_left(d, inputs))


def usage_line(pkgdir, tool, argv, d):
    p = subprocess.run([sys.executable, os.path.join(pkgdir, tool + ".py")] + argv, cwd=str(d), capture_output=True, text=True,
                       timeout=300)
    return dict(exit=p.returncode, stderr_last=p.stderr.rstrip("\n").split("\n")[-1])


def load(name):
    with open(os.path.join(TRANSCRIPTS, name + ".json")) as f:
        return json.load(f)


# ---------------------------------------------------------------- the recorder

def _save(name, transcript):
    os.makedirs(TRANSCRIPTS, exist_ok=True)
    with open(os.path.join(TRANSCRIPTS, name + ".json"), "w") as f:
        json.dump(transcript, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", name, "exit", transcript["exit"])
    if transcript["exit"] not in (0, 1, 2):  # a crash is no transcript; nothing more is started after one
        sys.exit("{}: exit status {}\n{}".format(name, transcript["exit"], transcript["stderr"]))


def record(pkgdir, which):
    import tempfile
    sys.path.insert(0, HERE)
    pkgdir = os.path.abspath(pkgdir)
    if which == "cpu":
        for name, (tool, build) in CPU_CASES.items():
            with tempfile.TemporaryDirectory() as d:  # (pseudopair_reads.py could not run by path at that commit)
                _save(name, run_by_path(pkgdir, tool, build, d, "cpu", imported=tool == "pseudopair_reads"))
        with tempfile.TemporaryDirectory() as d:
            _save("usage", dict(exit=2, lines={tool + " " + " ".join(argv): usage_line(pkgdir, tool, argv, d)
                                               for tool, argv in USAGE}))
    else:
        for name, (tool, build) in GPU_CASES.items():
            with tempfile.TemporaryDirectory() as d:
                _save("gpu_" + name, run_by_path(pkgdir, tool, build, d, "0", gpu_env(name)))


if __name__ == "__main__":
    record(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "cpu")
