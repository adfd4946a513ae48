"""The native host ingest (libmpc_ingest.so, include/mpc_ingest.h) gives exactly
the Python restatement's result (ingest.pack_sample_python, itself pinned to the
reference through the golden CLI cases), raises where it raises, and declines
(falls back) on the input features it does not restate.  CPU only."""
import importlib
import os

import numpy as np
import pytest

import glue_cases as gc
import golden_util as gu

KEYS = ("ref", "cs", "cs_off", "tstart", "up", "up_off", "down", "down_off", "aligned")


@pytest.fixture(scope="module")
def ing():
    m = importlib.import_module("minion-plasmid-consensus_amd.ingest")
    assert m._native() is not None, "libmpc_ingest.so did not build"
    return m


def _run(ing, fn, *paths):
    try:
        return fn(*paths), None
    except (ing.IngestError, UnicodeDecodeError) as e:  # the reference raises (exit 1) on both
        return None, e


def _same(ing, ref, paf, reads, expect_native=True):
    nat, ne = _run(ing, ing.pack_sample_native, ref, paf, reads)
    py, pe = _run(ing, ing.pack_sample_python, ref, paf, reads)
    if expect_native:
        assert nat is not None or ne is not None, "native parser declined"
    if nat is None and ne is None:  # declined: pack_sample must give the Python result
        nat, ne = _run(ing, ing.pack_sample, ref, paf, reads)
    assert (ne is None) == (pe is None), (ne, pe)
    if pe is None:
        for k in KEYS:
            assert np.array_equal(np.asarray(nat[k]), np.asarray(py[k])), k
        assert nat["n_alignments"] == py["n_alignments"]
    return nat


@pytest.mark.parametrize("case", gu.cases())
def test_golden_inputs(ing, case, tmp_path):
    ref, reads, paf = gu.materialize(case, str(tmp_path))
    # the native parser declines CR line ends and non-ASCII text (u_*: Python path)
    _same(ing, ref, paf, reads, expect_native="crlf" not in case and not case.startswith("u_"))


@pytest.mark.parametrize("spec", [
    dict(n=700, n_reads=400, profile="default", seed=11, frac_partial=0.3),
    dict(n=1500, n_reads=300, profile="indel", seed=12, frac_partial=0.5, flank=(0, 300)),
    dict(n=300, n_reads=900, profile="c1probe", seed=13, frac_partial=0.8, frac_minus=0.7),
])
def test_synthetic_files(ing, spec, tmp_path):
    syn = importlib.import_module("minion-plasmid-consensus_amd.synth").Synth(**spec)
    p = {k: str(tmp_path / k) for k in ("ref.fa", "reads.fa", "s.paf", "ras.fa", "as.paf")}
    syn.write_files(p["ref.fa"], p["reads.fa"], p["s.paf"], p["ras.fa"], p["as.paf"])
    a = _same(ing, p["ref.fa"], p["s.paf"], p["reads.fa"])
    b = _same(ing, p["ras.fa"], p["as.paf"], p["reads.fa"])
    assert len(a["tstart"]) == len(b["tstart"]) > 0
    for n_threads in (1, 3, 8):  # chunking does not change the result
        c = ing.pack_sample_native(p["ref.fa"], p["s.paf"], p["reads.fa"], n_threads=n_threads)
        for k in KEYS:
            assert np.array_equal(c[k], a[k]), (n_threads, k)


def _files(tmp_path, ref, paf, reads, mode="w"):
    out = []
    for name, txt in (("r.fa", ref), ("a.paf", paf), ("q.fa", reads)):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(txt.encode("latin-1") if isinstance(txt, str) else txt)
        out.append(path)
    return out


def paf_line(name, qlen, qs, qe, strand, ts, cs, extra=""):
    return "\t".join([name, str(qlen), str(qs), str(qe), strand, "ref", "100", str(ts), "9", "9", "9", "60",
                      "tp:A:P"] + ([extra] if extra else []) + ["cs:Z:" + cs]) + "\n"


EDGE = {
    # duplicate PAF names: the first line wins; duplicate FASTA names: the last record wins
    "dups": ("> r\nacgtacgtac\n",
             paf_line("a", 14, 2, 12, "+", 0, ":10") + paf_line("a", 14, 0, 10, "+", 0, ":10") +
             paf_line("b", 12, 0, 10, "-", 0, ":10"),
             ">a\nTTACGTACGTACGG\n>b\nACGTACGTACGT\n>a\nCCACGTACGTACAA\n"),
    # minus strand: revcomp, flipped coordinates; multi-line records, lower case, trailing spaces
    "minus": (">r\nACGTA\nCGTAC  \n",
              paf_line("m", 13, 1, 11, "-", 0, ":10"),
              ">x\nGG\n>m\nttgtac \ngtacgtg\n"),
    # Python slicing with out-of-range coordinates (qs > len, qe < 0 after the flip)
    "slicing": (">r\nACGTACGTAC\n",
                paf_line("s", 30, 25, 35, "+", 0, ":10") + paf_line("t", 5, 1, 40, "-", 0, ":10"),
                ">s\nACGTACGTACGT\n>t\nACGTACGTACGTAAA\n"),
    # flank cuts across line boundaries, blank and whitespace-only lines inside records, lower-case n
    "spans": (">r\nACGTACGTACGT\n",
              paf_line("p", 17, 3, 14, "+", 0, ":11") + paf_line("q", 17, 2, 15, "-", 0, ":13"),
              ">p\nac\n\ngTa  \n \nCGTAcgtnacGT\n>q\nAC\ngtA\n\nnCGTACg\t\ntacg\n"),
    "empty_paf": (">r\nACGT\n", "", ">a\nACGT\n"),
    "no_newline_at_end": (">r\nACGTACGTAC", paf_line("a", 10, 0, 10, "+", 0, ":10").rstrip("\n"), ">a\nACGTACGTAC"),
    "cs_first_field_wins": (">r\nACGTACGTAC\n", paf_line("a", 10, 0, 10, "+", 0, ":10", extra="cs:Z::3"),
                            ">a\nACGTACGTAC\n"),
    "header_only_fasta_name": (">r\nACGT\n", paf_line("a", 4, 0, 4, "+", 0, ":4"), ">\nAC\n>a\nACGT\n"),
}
ERRORS = {
    "missing_read": (">r\nACGT\n", paf_line("a", 4, 0, 4, "+", 0, ":4"), ">b\nACGT\n"),
    "minus_bad_char": (">r\nACGT\n", paf_line("a", 4, 0, 4, "-", 0, ":4"), ">a\nACXT\n"),
    "minus_bad_lower": (">r\nACGT\n", paf_line("a", 6, 0, 6, "-", 0, ":4"), ">a\nAC\ngt\nAx\n"),
    "no_cs": (">r\nACGT\n", "a\t4\t0\t4\t+\tref\t4\t0\t4\t4\t4\t60\n", ">a\nACGT\n"),
    "short_line": (">r\nACGT\n", "a\t4\t0\n", ">a\nACGT\n"),
    "bad_int": (">r\nACGT\n", paf_line("a", 4, 0, 4, "+", 0, ":4").replace("\t4\t0\t4\t", "\t4\tx\t4\t", 1), ">a\nACGT\n"),
    "blank_paf_line": (">r\nACGT\n", paf_line("a", 4, 0, 4, "+", 0, ":4") + "\n", ">a\nACGT\n"),
}
DECLINED = {
    "crlf": (">r\r\nACGT\r\n", paf_line("a", 4, 0, 4, "+", 0, ":4").replace("\n", "\r\n"), ">a\r\nACGT\r\n"),
    "plus_int": (">r\nACGT\n", paf_line("a", 4, 0, 4, "+", 0, ":4").replace("\t4\t0\t4\t", "\t+4\t0\t4\t", 1),
                 ">a\nACGT\n"),
    "non_ascii": (">r\nACGT\n", paf_line("a", 4, 0, 4, "+", 0, ":4"), ">a \xe9\nACGT\n"),
}


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_cases(ing, name, tmp_path):
    r = _same(ing, *_files(tmp_path, *EDGE[name]))
    assert r is not None


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_reference_errors(ing, name, tmp_path):
    paths = _files(tmp_path, *ERRORS[name])
    with pytest.raises(ing.IngestError):
        ing.pack_sample_native(*paths)
    with pytest.raises(ing.IngestError):
        ing.pack_sample_python(*paths)


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_inputs_use_python(ing, name, tmp_path):
    paths = _files(tmp_path, *DECLINED[name])
    assert ing.pack_sample_native(*paths) is None
    _same(ing, *paths, expect_native=False)


def test_dups_semantics(ing, tmp_path):
    r = ing.pack_sample(*_files(tmp_path, *EDGE["dups"]))
    assert list(r["aligned"]) == [10, 10]  # 'a' keeps its first PAF line (qs 2, qe 12)
    assert bytes(r["up"][r["up_off"][0]:r["up_off"][1]]) == b"CC"  # the last '>a' record


def test_multi_job_shared_reads(ing, tmp_path):
    """Jobs against one reads file, ingested in one scan, equal the one-job results
    (including a job the reference rejects and one the native parser declines)."""
    (tmp_path / "r1.fa").write_text(">r\nACGTACGTAC\n")
    (tmp_path / "r2.fa").write_text(">r\nGGGGACGTAC\n")
    reads = tmp_path / "reads.fa"
    reads.write_text(">a\nTTACGTACGTACGG\n>b\nACGTACGTACGT\n>c\nacgtNCGTAC\n")
    (tmp_path / "p1.paf").write_text(paf_line("a", 14, 2, 12, "+", 0, ":10") + paf_line("b", 12, 0, 10, "-", 0, ":10"))
    (tmp_path / "p2.paf").write_text(paf_line("c", 10, 1, 9, "-", 0, ":8") + paf_line("a", 14, 0, 10, "-", 0, ":10"))
    (tmp_path / "p3.paf").write_text(paf_line("z", 10, 1, 9, "-", 0, ":8"))  # z not in the reads: KeyError
    jobs = [(str(tmp_path / "r1.fa"), str(tmp_path / "p1.paf"), str(reads)),
            (str(tmp_path / "r2.fa"), str(tmp_path / "p2.paf"), str(reads))]
    multi = ing.pack_samples(jobs)
    for (ref, paf, rd), m in zip(jobs, multi):
        one = ing.pack_sample_python(ref, paf, rd)
        for k in ("ref", "cs", "cs_off", "tstart", "up", "up_off", "down", "down_off", "aligned"):
            assert np.array_equal(np.asarray(m[k]), np.asarray(one[k])), k
        assert m["n_alignments"] == one["n_alignments"]
    r = ing.pack_samples_native([(jobs[0][0], jobs[0][1]), (str(tmp_path / "r1.fa"), str(tmp_path / "p3.paf"))], str(reads))
    assert isinstance(r[0], dict) and isinstance(r[1], ing.IngestError)
    with pytest.raises(ing.IngestError):
        ing.pack_samples(jobs + [(str(tmp_path / "r1.fa"), str(tmp_path / "p3.paf"), str(reads))])


def _fuzz_files(rng, tmp_path, interior, trailing, paf_errors=False):
    """Random FASTA/PAF text: line lengths around the 64-byte blocks of the native
    scan, lower case, trailing whitespace, rare non-base bytes, blank lines,
    duplicate names in both files, records no PAF line names."""
    names = [f"r{i}" for i in range(60)]
    recs = []
    for r in range(90):  # every name once (no KeyError for a missing read), then duplicates
        nm = names[r] if r < len(names) else names[int(rng.integers(len(names)))]
        lines = []
        for _ in range(int(rng.integers(0, 5))):
            L = int(rng.choice([0, 1, 63, 64, 65, 127, 128, 129, int(rng.integers(0, 300))]))
            s = "".join(rng.choice(list("ACGTNacgtn"), size=L))
            if L and rng.random() < interior:
                k = int(rng.integers(L))
                s = s[:k] + str(rng.choice(list("X .*\t"))) + s[k + 1:]
            if rng.random() < trailing:
                s += str(rng.choice([" ", "\t", "  \t", "\x0b"]))
            lines.append(s)
        recs.append(">" + nm + ("\n" + "\n".join(lines) if lines else "") + "\n")
    rng.shuffle(recs)
    reads = "".join(recs)
    paf = ""
    for _ in range(80):
        nm = names[int(rng.integers(len(names)))]
        qlen = int(rng.integers(1, 400))
        qs, qe = sorted(int(x) for x in rng.integers(-5, qlen + 5, size=2))
        line = paf_line(nm, qlen, qs, qe, "-" if rng.random() < 0.5 else "+", int(rng.integers(0, 5)), ":3",
                        extra=str(rng.choice(["", "NM:i:3", "cs:Z::3", "tp:A:P\tcs:Z::3"])))
        u = rng.random()
        if u < 0.15:  # trailing whitespace, tabs included (rstrip() before split)
            line = line[:-1] + str(rng.choice(["\t", " \t", "\t\t ", "\x0c"])) + "\n"
        elif u < 0.25:  # a tag after the cs field, long enough to cross 64-byte blocks
            line = line[:-1] + "\tzz:Z:" + "x" * int(rng.integers(0, 150)) + "\n"
        paf += line
    if paf_errors:  # lines the reference rejects: short, no cs tag, non-integer fields
        paf += str(rng.choice(["a\t4\t0\n", "a\t4\t0\t4\t+\tref\t4\t0\t4\t4\t4\t60\n",
                               paf_line("a", 4, 0, 4, "+", 0, ":4").replace("\t4\t0\t4\t", "\t4\tx\t4\t", 1)]))
    return _files(tmp_path, ">r\nACGTACGTACGT\n", paf, reads)


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_block_scan_and_name_table(ing, seed, tmp_path):
    """The byte-class scan (64-byte blocks, fast path for lines of bases only) and
    the shared name table give the Python result on random text, for any thread
    count.  Non-base bytes inside lines (a minus-strand KeyError) in a third of
    the seeds; trailing whitespace (stripped, no error) in two thirds."""
    rng = np.random.default_rng(seed)
    interior = 0.08 if seed % 3 == 1 else 0.0
    paths = _fuzz_files(rng, tmp_path, interior, 0.0 if seed % 3 == 2 else 0.15, paf_errors=seed % 4 == 3)
    nat = _same(ing, *paths)
    if not interior and seed % 4 != 3:
        assert nat is not None and len(nat["tstart"]) > 20
    for n_threads in (1, 2, 5, 16):
        try:
            c = ing.pack_sample_native(*paths, n_threads=n_threads)
        except ing.IngestError:
            assert nat is None
            continue
        for k in KEYS:
            assert np.array_equal(np.asarray(c[k]), np.asarray(nat[k])), (n_threads, k)


# ---- the pieces shared with the other PAF parsers (csrc/host_file.h) ---------------

@pytest.mark.parametrize("name", sorted(gc.PAF_FILES))
def test_thread_cuts_do_not_change_the_result(ing, name, tmp_path):
    """1 thread and 16 threads cut the PAF at different line starts (none, or
    several cuts inside one line): both give the Python restatement's result."""
    ref, paf, reads = _files(tmp_path, gc.REF, gc.PAF_FILES[name], gc.READS)
    py = ing.pack_sample_python(ref, paf, reads)
    assert py["n_alignments"] == gc.PAF_FILES[name].count("\n") + (name == "one_line_no_newline")
    for n_threads in (1, 16):
        nat = ing.pack_sample_native(ref, paf, reads, n_threads=n_threads)
        assert nat is not None, n_threads
        for k in KEYS:
            assert np.array_equal(nat[k], py[k]), (n_threads, k)
        assert nat["n_alignments"] == py["n_alignments"]


@pytest.mark.parametrize("field", sorted(gc.PLAIN_INT))
def test_plain_int_policy(ing, field, tmp_path):
    """What the native int() of a PAF column takes itself, refuses like Python, or leaves to Python."""
    want = gc.PLAIN_INT[field][0]
    try:
        int(field)
        python_takes = True
    except ValueError:
        python_takes = False
    assert python_takes == (want != "error")
    paths = _files(tmp_path, gc.REF, gc.paf_line("a", 12, field, 11, "+", 0, ":10"), gc.READS)
    if want == "error":
        for fn in (ing.pack_sample_native, ing.pack_sample_python):
            with pytest.raises(ing.IngestError, match="ValueError"):
                fn(*paths)
    elif want == "python":
        assert ing.pack_sample_native(*paths) is None
        assert _same(ing, *paths, expect_native=False) is not None
    else:
        assert _same(ing, *paths) is not None
