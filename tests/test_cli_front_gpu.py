"""The command-line front on the device: the four tools' success cases of
test_cli_front.py with --device 0, and the drop-in on the smallest passing
golden case (an empty PAF) and on the smallest with an alignment (each with
--device 0, and with --gpus 2 and one --also job) and on a negative-start case,
against transcripts recorded the same way on an MI355X; the drop-in's files
are the golden ones as well."""
import pytest

import cli_cases as cc
import golden_util as gu

pytestmark = pytest.mark.gpu

DROPIN = {"dropin_device": (cc.SMALLEST_ALIGNED, [""]), "dropin_gpus2_also": (cc.SMALLEST_ALIGNED, ["", "_also"]),
          "dropin_device_empty": (cc.SMALLEST_PASSING, [""]), "dropin_gpus2_also_empty": (cc.SMALLEST_PASSING, ["", "_also"]),
          "dropin_negative_start": (cc.NEGATIVE_START, [""])}


@pytest.mark.parametrize("name", sorted(cc.GPU_CASES))
def test_by_path_matches_the_transcript(name, tmp_path):
    tool, build = cc.GPU_CASES[name]
    got = cc.run_by_path(cc.PKGDIR, tool, build, tmp_path, "0", cc.gpu_env(name))
    assert got == cc.load("gpu_" + name)
    if name in DROPIN:
        case, suffixes = DROPIN[name]
        exp = next(iter(gu.runs(case)))[2]
        assert got["exit"] == 0
        for s in suffixes:
            for ours, golden in (("c%s.fa", "c.fa"), ("ch%s.tsv", "ch.tsv"), ("acc%s.tsv", "acc.tsv")):
                assert got["files"][ours % s].encode() == exp[golden], (name, ours % s)
