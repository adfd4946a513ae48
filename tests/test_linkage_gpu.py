"""linkage_qc on the GPU: K_lnkparse + K_lnkplanes + K_lnkpair (mpc_linkage_run,
mpc_linkage_pairs) against the independent checker of tests/link_util.py: every
token shape across a lane-chunk and a tile boundary, the ends of records and
targets, the shapes of the contraction on injected codes, several samples, more
records than the grid has waves, status parity with coverage_qc, the tables
refused before the launch, the planted sub-population, the Synth batch against
the host walk, and the CLI on device 0 against --device cpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cov_util as cu
import link_util as lu

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "minion-plasmid-consensus_amd", "linkage_qc.py")
DEV = 0


def test_boundaries(pkg):
    lu.case_boundaries(pkg, DEV)


def test_ends_of_record_and_target(pkg):
    lu.case_ends(pkg, DEV)


@pytest.mark.parametrize("n,k", lu.PAIR_SHAPES)
def test_pairs_shapes(pkg, n, k):
    lu.case_pairs_shape(pkg, DEV, n, k)


def test_pairs_one_code_past_16_bits(pkg):
    lu.case_pairs_one_code(pkg, DEV)


def test_pairs_limits(pkg):
    lu.case_pairs_limits(pkg, DEV)


def test_pairs_refuses_129_sites_untouched(pkg):
    import torch
    L = pkg.engine.lib()
    alleles = torch.ones((4, 129), dtype=torch.uint8, device="cuda:0")
    pair = torch.full((64,), -5, dtype=torch.int32, device="cuda:0")
    scratch = torch.full((64,), -5, dtype=torch.int64, device="cuda:0")
    assert L.mpc_linkage_scratch_bytes(4, 129) == 0 and L.mpc_linkage_scratch_bytes(65, 3) == 64 + 2 * 3 * 64
    assert L.mpc_linkage_pairs(alleles.data_ptr(), 4, 129, pair.data_ptr(), scratch.data_ptr(), None) == -1
    assert b"n_sites" in L.mpc_last_error()
    torch.cuda.synchronize()
    assert (pair == -5).all() and (scratch == -5).all()


def test_samples(pkg):
    lu.case_samples(pkg, DEV)


def test_more_records_than_waves_and_determinism(pkg):
    lu.case_one_token(pkg, DEV)


@pytest.mark.parametrize("name,rec,code", cu.BAD, ids=[b[0] for b in cu.BAD])
def test_status_parity_with_coverage(pkg, name, rec, code):
    lu.case_status_parity(pkg, DEV, rec, code)


def test_status_smaller_index_wins_far_apart(pkg):
    lu.case_status_far_apart(pkg, DEV)


def test_sample_index_outside_the_targets(pkg):
    lu.case_bad_sample(pkg, DEV)


def test_run_refuses_bad_tables_before_launch(pkg):
    import torch
    L = pkg.engine.lib()
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda:0")
    cs = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    cs[:2] = torch.tensor(list(b":3"), dtype=torch.uint8)
    off, ts, pos = i64([0, 2]), i64([0]), i64([0, 11, 18])
    smp = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    alleles = torch.full((4,), 9, dtype=torch.uint8, device="cuda:0")
    pair = torch.full((9 * 64,), -5, dtype=torch.int32, device="cuda:0")
    scratch = torch.full((64,), -5, dtype=torch.int64, device="cuda:0")
    status = torch.full((2,), -5, dtype=torch.int32, device="cuda:0")

    def call(site_off, site_key, k):
        so, sk = i64(site_off), i64(site_key)
        rc = L.mpc_linkage_run(cs.data_ptr(), off.data_ptr(), ts.data_ptr(), smp.data_ptr(), 1, pos.data_ptr(), 2, so.data_ptr(),
                               sk.data_ptr(), k, alleles.data_ptr(), pair.data_ptr(), scratch.data_ptr(), status.data_ptr(), None)
        torch.cuda.synchronize()
        return rc
    for site_off, site_key, k, word in lu.BAD_TABLES:
        assert call(site_off, site_key, k) == -1 and word in L.mpc_last_error(), (site_off, site_key)
    assert call([0, 64, 129], list(range(129)), 129) == -1 and b"n_sites" in L.mpc_last_error()
    assert (alleles == 9).all() and (pair == -5).all() and (scratch == -5).all() and (status == -5).all()
    assert call(*lu.GOOD_TABLE) == 0
    assert alleles.tolist() == [1, 0, 0, 9] and status.tolist() == [0, 0]
    assert pair.view(3, 3, 8, 8)[0, 1, 1, 0] == 1 and pair.sum() == 9


def test_planted_subpopulation(pkg):
    lu.case_planted(pkg, DEV)


def test_synth_batch_device_equals_host(pkg):
    cs, off, ts, rs, lengths, site_off, site_key, dropped = lu.synth_sites(pkg, DEV)
    assert 8 <= len(site_key) <= 128 and dropped == 0
    dev = pkg.linkage.run(cs, off, ts, rs, lengths, site_off, site_key, device=DEV)
    host = pkg.linkage.run(cs, off, ts, rs, lengths, site_off, site_key, device="cpu")
    assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])
    assert (host[0] >= 2).any(axis=0).all()  # every selected site has a minor allele in some record


def test_planted_subpopulation_cli(pkg, tmp_path):
    lu.case_planted_cli(pkg, DEV, tmp_path, CLI)


def test_cli_device_equals_cli_cpu(pkg, tmp_path):
    syn = pkg.synth.Synth(n=600, n_reads=300, profile="indel", seed=4)
    pafs = [str(tmp_path / "sense.paf"), str(tmp_path / "antisense.paf")]
    syn.write_files(paf0=pafs[0], paf1=pafs[1])
    files = {}
    for dev in ("0", "cpu"):
        names = [str(tmp_path / ("%s_%s.tsv" % (k, dev))) for k in ("report", "pairs", "hap")]
        p = subprocess.run([sys.executable, CLI, "--paf"] + pafs + ["--region", "40:560", "--report", names[0], "--pairs", names[1],
                            "--haplotypes", names[2], "--min-minor-fraction", "0.1", "--device", dev],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        files[dev] = [open(n, "rb").read() for n in names]
    assert files["0"] == files["cpu"] and files["0"][0].count(b"\n") == 2 * 16 + 1
