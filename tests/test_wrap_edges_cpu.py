"""The inputs of tests/test_wrap_edges_gpu.py, checked on the CPU: the
generators of tests/neg_util.py give valid input (the C oracle accepts it),
the rewrites keep its value, and the shapes reach the sizes at which the
replay of the wrapped odd positions (K_woprep .. K_worows) takes another path.
"""
import numpy as np
import pytest

import depth_util as du
import neg_util
import oracle

SETTINGS = ((-1.0, 1.0), (0.1, 5.0))


def test_neg_sample_defaults_unchanged():
    """The keyword arguments added to neg_sample (ins_max, match_max) leave the
    rng call sequence of the existing calls alone: the samples the older tests
    and their recorded counts rest on are byte-identical (digests taken before
    the arguments were added)."""
    assert neg_util.sample_digest(neg_util.edge_sample("neg5")) == \
        "cee8d11a3b535ec71b9e76316d05ee5959e9f430009dd9ddf3e8e6bb4f27dad6"
    assert neg_util.sample_digest(neg_util.edge_sample("neg105")) == \
        "29f5feafe5547d02218b804b397cfdb7184c82caa8f82676e758d04059665c1b"
    assert neg_util.sample_digest(neg_util.edge_sample("neg5_400")) == \
        "3619733c9555e921cd5bf2a9f49a73d2e8e4d81c122f80cdaf5b662e7c42a191"
    assert neg_util.wrapped_counts(neg_util.edge_sample("neg5")) == (506, 125, 21)


@pytest.mark.parametrize("name", ["neg5", "neg105"])
def test_decorate_is_value_preserving(name):
    """oracle(decorate(s)) == oracle(s): pins decorate, not the kernel.  The
    rewrite holds every form it promises, on reads with a negative start too."""
    plain, dec = neg_util.edge_sample(name), neg_util.edge_sample(name + "_dec")
    for key in ("ref", "tstart", "up", "up_off", "down", "down_off"):
        assert np.array_equal(plain[key], dec[key]), key
    cs = bytes(dec["cs"])
    assert len(cs) > 1.1 * len(plain["cs"])
    for form in (b": ", b" :", b":00", b"_", b":\x0b", b"\x0c", b"Zacg", b":000", b": 0 ", b"::", b"*:", b"+*", b"-+",
                 b"Z-"):
        assert form in cs, form
    neg = np.nonzero(np.asarray(dec["tstart"]) < 0)[0]
    changed = [r for r in neg if bytes(dec["cs"][dec["cs_off"][r]: dec["cs_off"][r + 1]])
               != bytes(plain["cs"][plain["cs_off"][r]: plain["cs_off"][r + 1]])]
    assert len(changed) > len(neg) // 2
    assert neg_util.wrapped_counts(dec) == neg_util.wrapped_counts(plain)
    for st in SETTINGS:
        du.compare(du.oracle_one(dec, *st), du.oracle_one(plain, *st), ("decorate", name, st))


def test_big_shapes_exceed_the_loop_bounds():
    """K_woprep: 1024 threads, one pair per thread up to 2048 sorted entries,
    one scan batch per 1024 entries; K_worows: 64 runs of a position per pass.
    The two big shapes are past each of these (and valid input)."""
    ev, pos, right = neg_util.wrapped_counts(neg_util.edge_sample("big0"))
    assert (ev, pos, right) == (15493, 1744, 60)
    assert ev > 2048 and pos > 1024
    ev, pos, right = neg_util.wrapped_counts(neg_util.edge_sample("big1"))
    assert (ev, pos, right) == (13911, 981, 93)
    assert right > 64
    for name in ("big0", "big1"):
        smp = neg_util.edge_sample(name)
        assert len(du.oracle_one(smp, -1.0, 1.0)["base"]) > len(smp["ref"])


def test_long_strings_in_wrapped_positions():
    """An upstream flank, a downstream flank and a '+' string of more than 64
    bases each, all in wrapped odd positions: K_worows lays a string's bases on
    the 64 lanes of a wave, a longer one takes a second pass."""
    smp = neg_util.edge_sample("long")
    longest = neg_util.longest_wrapped(smp)
    assert min(longest.values()) > 64, longest
    du.oracle_one(smp, -1.0, 1.0)


def test_boundary_sample_hits_both_ends():
    """Strings at the first and the last wrapped odd position, of every kind
    the ends can take, and valid input."""
    smp = neg_util.boundary_sample()
    n = len(smp["ref"])
    got = {(p, k) for p, k, _, _ in neg_util._wrapped(smp)}
    assert {(n - 1, "up"), (0, "up"), (n - 1, "down"), (1, "down"), (n - 1, "ins"), (0, "ins")} <= got
    ts = np.asarray(smp["tstart"])
    first, last = np.nonzero(ts < 0)[0][[0, -1]]
    assert (ts[:first] == 0).all() and (ts[last + 1:] == 0).all() and first >= 2 and last < len(ts) - 2
    for st in SETTINGS:
        res = du.oracle_one(smp, *st)
        assert len(res["base"]) > n


def _one_read(cs, tstart=0):
    return neg_util._pack(b"ACGTACGTAC", [(cs, tstart, b"", b"")])


@pytest.mark.parametrize("where", ["before", "after"])
def test_oracle_int_takes_what_python_int_takes(where):
    """Every ASCII byte next to the digits of a ':' operand: the oracle raises
    ValueError exactly where int() does on the same text (:77).  int() strips
    space and \\t-\\r from an ASCII str but not \\x1c-\\x1f, which str.strip()
    would: the reference rejects ':\\x1f4' (golden n_neg_pyint_fs)."""
    for c in range(128):
        ch = bytes([c])
        if ch in b":Z+-*":
            continue
        text = ch + b"4" if where == "before" else b"4" + ch
        try:
            int(text.decode("ascii"))
            ok = True
        except ValueError:
            ok = False
        try:
            du.oracle_one(_one_read(b"Z::" + text + b":2"), -1.0, 1.0)
            code = 0
        except oracle.OracleError as e:
            code = e.code
        assert (code != 3) == ok, (c, where, code)
        assert ok == (ch in b" \t\n\r\x0b\x0c" or ch.isdigit()), c
