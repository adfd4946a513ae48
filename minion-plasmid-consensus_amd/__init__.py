"""MI355X-native pileup + consensus: drop-in for the `consensus` rule of
scottdbrown/minion-plasmid-consensus (src/mapped_paf_read_parser.py).

Modules
  ingest   Steps 1-3 (FASTA / PAF ingest, flanks) -> packed per-read arrays
  _native  the ctypes prototype of every function of include/*.h, applied when a
           library is loaded; the tools' shared device plumbing
  engine   libmpc.so (include/mpc.h): its loading rules + torch device buffers
  writers  Step 7 output files
  synth    seeded synthetic cs-tagged data (tests / bench)
  dist     multi-GPU read sharding over RCCL (torch.distributed)
  verify   exact alignment of consensus files with the expected plasmid (K_vscan)
  coverage per-position depth / deletion / mismatch / insertion profile from the PAF (K_covparse)
  linkage  per-read alleles at variable sites and their pairwise co-occurrence (K_lnkparse, K_lnkpair)
  align    exact read-to-assembly alignment to a cs-tagged PAF (K_arevcomp, K_vscan, K_atrace)
  handoff  a launch's edit scripts as the pileup's inputs, in memory (K_acslen, K_acswrite)
  draft    the sense / antisense assembly from the first reads: seed, align, vote, call (K_dvote, K_dcall)
  _cli     what the command-line tools below share: status lines, banner, argparse types, error line,
           output files, verdict and exit status (standard library only; not imported here)
  mapped_paf_read_parser  the drop-in CLI
  verify_consensus        the "Check the results" CLI
  coverage_qc             the coverage criterion CLI
  linkage_qc              the sub-population (linked minor alleles) CLI
  align_reads             the final_alignment_paf CLI (reads + assembly -> PAF)
  draft_assembly          the canu_denovo_assembly CLI (reads -> sense / antisense assembly)
  reads_consensus         reads + assemblies -> consensus files in one run (final_alignment_paf + consensus)
"""
from . import _build, ingest, writers, synth  # noqa: F401
from . import engine  # noqa: F401
from . import verify  # noqa: F401
from . import coverage  # noqa: F401
from . import linkage  # noqa: F401
from . import align  # noqa: F401
from . import draft  # noqa: F401
from . import handoff  # noqa: F401

__all__ = ["ingest", "engine", "writers", "synth", "verify", "coverage", "linkage", "align", "draft", "handoff"]
