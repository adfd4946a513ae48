"""verify_consensus without a GPU: the host scan (mpc_verify_scan_host) and the
banded edit script (mpc_verify_script) against the numpy full-matrix checker
(tests/verify_util.py), the FASTA readers, the CLI with --device cpu, the
exported symbols of include/mpc_verify.h and an ASan + UBSan run of
csrc/verify.cpp through a stand-alone driver."""
import ctypes
import os
import re
import statistics
import subprocess
import sys

import numpy as np
import pytest

import native_util as nu
import verify_util as vu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "minion-plasmid-consensus_amd", "verify_consensus.py")
HEADER = "consensus\tregion\texpected_len\tconsensus_len\tstart\tend\tdistance\tmismatches\tinsertions\tdeletions\tcigar\n"


@pytest.fixture(scope="module")
def grid():
    """The seeded pairs and the checker's script of each, computed once."""
    pairs = vu.small_pairs()
    return pairs, [vu.traceback(q, t) for q, t in pairs]


def test_grid_covers_what_it_should(grid):
    pairs, ref = grid
    assert {len(q) for q, _ in pairs} == {1, 2, 63, 64, 65, 127, 128, 129, 200}
    assert {len(t) for _, t in pairs} == {0, 1, 3, 64, 70, 260}
    assert any(r["distance"] == 0 for r in ref) and any(r["distance"] > 20 for r in ref)
    ops = "".join(r["ops"] for r in ref)
    assert all(c in ops for c in "=XID")
    assert any(re.search(rb"[a-z]", q) and re.search(rb"[^ACGTacgt]", q) for q, _ in pairs)
    assert any(re.search(rb"[a-z]", t) and re.search(rb"[^ACGTacgt]", t) for _, t in pairs)


def test_scan_host_matches_checker(grid):
    pairs, ref = grid
    for threads in (1, 5):
        got = vu.scan_host(pairs, threads)
        for k, (g, r) in enumerate(zip(got, ref)):
            assert g == (r["distance"], r["end"]), (k, len(pairs[k][0]), len(pairs[k][1]))


def test_script_matches_checker(grid):
    pairs, ref = grid
    for (q, t), r in zip(pairs, ref):
        rc, start, counts, cigar = vu.script(q, t, r["distance"], r["end"])
        assert rc == 0
        assert (start, counts, cigar) == (r["start"], vu.op_counts(r["ops"]), vu.cigar(r["ops"])), (len(q), len(t))


def test_script_cross_checks_the_scan(grid):
    """A (distance, end) the band DP does not reproduce is an error, not a script."""
    pairs, ref = grid
    L = vu.pkg().verify.host_lib()
    k = next(k for k, r in enumerate(ref) if r["distance"] >= 2 and len(pairs[k][1]) >= 64)
    (q, t), r = pairs[k], ref[k]
    assert vu.script(q, t, r["distance"] - 1, r["end"])[0] != 0
    assert b"band" in L.mpc_verify_last_error()
    assert vu.script(q, t, r["distance"], len(t) + 1)[0] != 0


def test_non_acgt_matches_nothing():
    """An N is an unverified base: it counts as an edit even against an N."""
    assert vu.scan_host([(b"ACGNACG", b"ACGNACG"), (b"acgtacg", b"ACGTACG"), (b"N", b"N"), (b"N", b"")]) == \
        [(1, 7), (0, 7), (1, 0), (1, 0)]
    assert vu.script(b"ACGNACG", b"ACGNACG", 1, 7)[1:] == (0, [6, 1, 0, 0], "3=1X3=")


def test_tie_takes_the_smaller_end():
    """Two equally good placements: end is the first one's."""
    rng = np.random.default_rng(5)
    q = vu.rand_seq(rng, 70)
    t = vu.rand_seq(rng, 9) + q + b"TT" + q + vu.rand_seq(rng, 4)
    ref = vu.traceback(q, t)
    assert (ref["distance"], ref["end"], ref["start"]) == (0, 79, 9)
    assert vu.scan_host([(q, t)]) == [(0, 79)]
    assert vu.script(q, t, 0, 79)[1:] == (9, [70, 0, 0, 0], "70=")
    # a tie between an edited placement and a later equal one
    q2 = b"ACGTTGCA"
    t2 = b"ACGTAGCAGGACGTTGCT"
    assert vu.score(q2, t2) == (1, 8) and vu.scan_host([(q2, t2)]) == [(1, 8)]


def test_above_max_edits_no_script():
    """distance > 1024: exact distance and end, CIGAR '*', start and counts -1."""
    rng = np.random.default_rng(17)
    q, t = vu.rand_seq(rng, 4000), vu.rand_seq(rng, 4100)
    distance, end = vu.score(q, t)
    assert distance > vu.MAX_EDITS
    assert vu.scan_host([(q, t)]) == [(distance, end)]
    assert vu.script(q, t, distance, end) == (0, -1, [-1] * 4, "*")
    v = vu.pkg().verify
    assert v.script(q, t, distance, end) == dict(start=-1, matches=-1, mismatches=-1, insertions=-1, deletions=-1,
                                                 cigar="*")


def test_lengths_refused_host_side():
    v = vu.pkg().verify
    L = v.host_lib()
    seq = np.zeros(16, np.uint8)
    out = np.zeros(2, np.int32)
    for m, n in ((0, 4), (vu.MAX_QUERY + 1, 4), (4, -1), (4, 2 ** 31)):
        tab = np.array([0, m, 0, n], np.int64)
        assert L.mpc_verify_scan_host(seq.ctypes.data, tab.ctypes.data, 1, out.ctypes.data, 1) != 0, (m, n)
        assert b"pair 0" in L.mpc_verify_last_error()
    for dev in ("cpu", 0):  # refused before any library or device is touched
        with pytest.raises(v.VerifyError):
            v.scan([(b"A" * (vu.MAX_QUERY + 1), b"ACGT")], device=dev)
        with pytest.raises(v.VerifyError):
            v.scan([(b"", b"ACGT")], device=dev)
    assert v.scan([], device="cpu") == []
    assert v.scan([(b"ACGT", b"")], device="cpu") == [(4, 0)]


def test_pair_rule_names_the_row():
    """The refused lengths above, and a negative offset, in row 2 of a table
    whose other rows are fine: the message names that row, nothing is written."""
    L = vu.pkg().verify.host_lib()
    seq = np.frombuffer(b"ACGTACGTACGTACGT", np.uint8).copy()
    good = [[0, 4, 4, 8], [2, 3, 0, 0], [0, 1, 1, 15]]
    bad = [[0, m, 0, n] for m, n in ((0, 4), (vu.MAX_QUERY + 1, 4), (4, -1), (4, 2 ** 31))] + [[-1, 4, 4, 8], [0, 4, -4, 8]]
    for row in bad:
        tab = np.array(good[:2] + [row] + good[2:], np.int64)
        out = np.full((4, 2), -7, np.int32)
        assert L.mpc_verify_scan_host(seq.ctypes.data, tab.ctypes.data, 4, out.ctypes.data, 2) != 0, row
        assert b"mpc_verify_scan_host: pair 2: " in L.mpc_verify_last_error()
        assert (out == -7).all()
    tab = np.array(good, np.int64)
    out = np.full((3, 2), -7, np.int32)
    assert L.mpc_verify_scan_host(seq.ctypes.data, tab.ctypes.data, 3, out.ctypes.data, 2) == 0
    assert out.tolist() == [[0, 4], [3, 0], [0, 4]]


def test_read_expected(tmp_path):
    v = vu.pkg().verify
    p = tmp_path / "e.fa"
    p.write_bytes(b">x\naacc\nGGTTa  \nAc\ngg")
    assert v.read_expected(str(p)) == (b"aaccGGTTaAcgg", 4, 10)          # lower/UPPER/lower, multi-line, no last newline
    p.write_bytes(b">x\nACGT\nNNAC\n")
    assert v.read_expected(str(p)) == (b"ACGTNNAC", 0, 8)                 # all upper
    p.write_bytes(b">x\nacgtGacgt\n")
    assert v.read_expected(str(p)) == (b"acgtGacgt", 4, 5)
    for bad in (b">x\nacgt\n", b">x\n", b""):
        p.write_bytes(bad)
        with pytest.raises(v.VerifyError):
            v.read_expected(str(p))
    p.write_bytes(b">consensus\nACGT\n")
    assert v.read_consensus(str(p)) == b"ACGT"
    p.write_bytes(b">consensus\nACGT")
    assert v.read_consensus(str(p)) == b"ACGT"
    p.write_bytes(b">consensus\n\n")
    assert v.read_consensus(str(p)) == b""


# ---- CLI ---------------------------------------------------------------------

def _run_cli(*args):
    return subprocess.run([sys.executable, CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _case(tmp_path, seed, damage):
    """An adapter-padded expected file, a sense consensus and a 'revcomp'
    consensus (no trailing newline); ``damage`` edits the plasmid part."""
    rng = np.random.default_rng(seed)
    up, core, down = vu.rand_seq(rng, 30).lower(), vu.rand_seq(rng, 400), vu.rand_seq(rng, 25).lower()
    exp = tmp_path / "x_adapted_sense.fasta"
    exp.write_bytes(b">x\n" + up + core + down)
    c1 = up[5:].upper() + damage(core) + down[:-3].upper()
    c2 = up[9:].upper() + core + down.upper()[:-1] + b"G"
    s1, s2 = tmp_path / "sense_consensus.fasta", tmp_path / "antisense_consensus_revcomp.fasta"
    s1.write_bytes(b">consensus\n" + c1 + b"\n")
    s2.write_bytes(b">consensus\n" + c2)
    return exp, up + core + down, (len(up), len(up) + len(core)), [(s1, c1), (s2, c2)]


def _expected_report(adapted, core, cons, medians, verdict):
    lines = [HEADER]
    for path, t in cons:
        for region, q in (("plasmid", adapted[core[0]:core[1]]), ("adapted", adapted)):
            lines.append("%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % ((str(path), region, len(q), len(t)) + vu.expected_row(q, t)))
    for path, med in medians:
        lines.append("%s\tmedian_accuracy\t%s\n" % (path, med))
    lines.append("verdict\t%s\n" % verdict)
    return "".join(lines)


def _acc(path, vals):
    path.write_text("pos\taccuracy\n" + "".join("%d\t%r\n" % (k + 1, v) for k, v in enumerate(vals)))
    return path


def test_cli_pass_report(tmp_path):
    exp, adapted, core, cons = _case(tmp_path, 23, lambda c: c)
    v1, v2 = [100.0, 99.95, 99.99, 98.0], [100.0, 100.0, 99.0]
    a1, a2 = _acc(tmp_path / "a1.tsv", v1), _acc(tmp_path / "a2.tsv", v2)
    rep, edits = tmp_path / "verify.tsv", tmp_path / "edits.tsv"
    p = _run_cli("--expected", exp, "--consensus", cons[0][0], cons[1][0], "--accuracies", a1, a2, "--report", rep,
                 "--edits", edits, "--device", "cpu", "--strict")
    assert p.returncode == 0, p.stderr
    want = _expected_report(adapted, core, cons, [(a1, repr(statistics.median(v1))), (a2, "100.0")], "PASS")
    assert rep.read_text() == want
    rows = [ln.split("\t") for ln in want.splitlines()]
    assert [r[6] for r in rows[1:5]] == ["0", "8", "0", "10"]  # plasmid exact; the adapters are clipped / edited
    want_edits = []
    for path, t in cons:
        want_edits += vu.edit_lines(str(path), "plasmid", adapted[core[0]:core[1]], t, core[0])
        want_edits += vu.edit_lines(str(path), "adapted", adapted, t, 0)
    assert edits.read_text() == "".join(want_edits) and len(want_edits) == 18
    assert "STATUS [" in p.stdout and "Verdict: PASS" in p.stdout


def test_cli_fail_report_and_strict(tmp_path):
    def damage(c):  # a substitution, a deleted base, a foreign insert
        return c[:100] + b"N" + c[101:200] + c[201:300] + b"GATTACAGATTACA" + c[300:]
    exp, adapted, core, cons = _case(tmp_path, 29, damage)
    rep, edits = tmp_path / "verify.tsv", tmp_path / "edits.tsv"
    args = ["--expected", exp, "--consensus", cons[0][0], cons[1][0], "--report", rep, "--edits", edits, "--device", "cpu"]
    p = _run_cli(*args)
    assert p.returncode == 0, p.stderr
    want = _expected_report(adapted, core, cons, [], "FAIL")
    assert rep.read_text() == want
    first = want.splitlines()[1].split("\t")
    assert first[6:10] == ["16", "1", "14", "1"]
    lines = edits.read_text().splitlines()
    plasmid = [ln.split("\t") for ln in lines if ln.split("\t")[:2] == [str(cons[0][0]), "plasmid"]]
    assert len(plasmid) == 16
    assert plasmid[0][2:] == [str(core[0] + 101), str(25 + 101), "X", chr(adapted[core[0] + 100]), "N"]
    assert sum(1 for e in plasmid if e[4] == "D" and e[6] == "-") == 1
    assert sum(1 for e in plasmid if e[4] == "I" and e[5] == "-") == 14
    rep.unlink()
    p = _run_cli(*args, "--strict")
    assert p.returncode == 2 and rep.read_text() == want
    # an accuracies median at the bar fails a clean plasmid (the bar is "above 99.9")
    exp, adapted, core, cons = _case(tmp_path, 23, lambda c: c)
    a = _acc(tmp_path / "a.tsv", [99.9, 99.9, 100.0])
    p = _run_cli("--expected", exp, "--consensus", cons[0][0], "--accuracies", a, "--report", rep, "--device", "cpu", "--strict")
    assert p.returncode == 2
    assert rep.read_text() == _expected_report(adapted, core, cons[:1], [(a, "99.9")], "FAIL")


def test_cli_invalid_input_exit_1(tmp_path):
    exp, adapted, core, cons = _case(tmp_path, 23, lambda c: c)
    rep, edits = tmp_path / "verify.tsv", tmp_path / "edits.tsv"

    def refused(*args):
        p = _run_cli(*args, "--report", rep, "--edits", edits, "--device", "cpu")
        assert p.returncode == 1 and p.stderr.startswith("Error: "), (p.returncode, p.stderr)
        assert not rep.exists() and not edits.exists()

    refused("--expected", exp, "--consensus", cons[0][0], tmp_path / "missing.fasta")
    refused("--expected", tmp_path / "missing.fasta", "--consensus", cons[0][0])
    refused("--expected", exp, "--consensus", cons[0][0], "--accuracies", tmp_path / "missing.tsv")
    low = tmp_path / "low.fasta"
    low.write_bytes(b">x\nacgtacgt\n")
    refused("--expected", low, "--consensus", cons[0][0])
    big = tmp_path / "big.fasta"  # m = 65,537
    big.write_bytes(b">x\n" + vu.rand_seq(np.random.default_rng(2), vu.MAX_QUERY + 1) + b"\n")
    refused("--expected", big, "--consensus", cons[0][0])


# ---- ABI ---------------------------------------------------------------------

def _declared(header):
    txt = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"^(?:int|void|size_t|const char\*)\s+(mpc_\w+)\(", txt, re.M)))


def test_verify_header_exports(pkg):
    """Every function of mpc_verify.h is exported: the scan by libmpc.so, the
    host half by libmpc_ingest.so; mpc.h and mpc_ingest.h still are, and their
    version numbers did not move."""
    names = _declared("mpc_verify.h")
    assert names == ["mpc_verify_last_error", "mpc_verify_scan", "mpc_verify_scan_host", "mpc_verify_script"]
    pkg._build.build_hip()
    hip = pkg.engine.lib()
    host = ctypes.CDLL(pkg._build.build_ingest())
    assert hasattr(hip, "mpc_verify_scan")
    for name in names:
        if name != "mpc_verify_scan":
            assert hasattr(host, name), name
    for name in _declared("mpc.h"):
        assert hasattr(hip, name), name
    for name in _declared("mpc_ingest.h"):
        assert hasattr(host, name), name
    assert hip.mpc_version() == 9
    assert not hasattr(hip, "mpc_fail_")  # (internal: hidden)
    assert pkg.verify.MAX_QUERY == vu.MAX_QUERY == 65536 and pkg.verify.MAX_EDITS == vu.MAX_EDITS == 1024
    hdr = open(os.path.join(REPO, "include", "mpc_verify.h")).read()
    assert "#define MPC_VERIFY_MAX_QUERY 65536" in hdr and "#define MPC_VERIFY_MAX_EDITS 1024" in hdr


# ---- sanitizers (host code, stand-alone program) ------------------------------

def test_verify_host_code_sanitized(grid, tmp_path):
    pairs, ref = grid
    picked = [k for k in range(len(pairs)) if k % 4 == 0 and b"\t" not in pairs[k][0] + pairs[k][1]]
    rng = np.random.default_rng(31)
    extra = [(vu.rand_seq(rng, 2400), vu.rand_seq(rng, 2300))]  # distance > 1024: the '*' path
    assert vu.score(*extra[0])[0] > vu.MAX_EDITS
    use = [pairs[k] for k in picked] + extra
    want = [vu.traceback(q, t) for q, t in use[:-1]]
    inp = tmp_path / "pairs.txt"
    inp.write_bytes(b"".join(q + b"\t" + t + b"\n" for q, t in use))
    binary = nu.build("verify_asan", ["verify.cpp", os.path.join(nu.NATIVE, "verify_driver.cpp")], ["-pthread"])
    for threads in (1, 4):
        got = nu.run(binary, [inp, threads], timeout=120).splitlines()
        assert len(got) == len(use)
        for line, r in zip(got, want):
            assert line == "%d %d %d %d %d %d %d %s" % ((r["distance"], r["end"], r["start"]) + tuple(vu.op_counts(r["ops"])) + (vu.cigar(r["ops"]),))
        d, e = vu.score(*extra[0])
        assert got[-1] == "%d %d -1 -1 -1 -1 -1 *" % (d, e)
