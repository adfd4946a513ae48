// paf_driver.cpp -- stand-alone driver of the two PAF readers that sit on
// csrc/host_file.h besides the ingest (which tests/native/ingest_driver.cpp
// drives): mpc_coverage_ingest / _free and mpc_pseudopair, with 1 and with 16
// threads, on every file named.  Built with -fsanitize=address,undefined by
// tests/test_paf_sanitized.py; prints what it read, one line per call.
//
//   paf_driver <pairs output path> <paf>...
#include <cstdio>
#include <initializer_list>

#include "mpc_coverage.h"
#include "mpc_ingest.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  for (int i = 2; i < argc; ++i) {
    for (int threads : {1, 16}) {
      mpc_coverage_paf paf;
      const int rc = mpc_coverage_ingest(argv[i], 1, threads, &paf);
      long long cs_sum = 0;  // every cs byte is read: an offset past the buffer is a report
      for (long long k = 0; rc == 0 && k < paf.cs_off[paf.n_records]; ++k) cs_sum += paf.cs[k];
      printf("cov %d threads %d rc %d records %lld lines %lld targets %lld cs_sum %lld message %s\n", i - 2, threads, rc,
             (long long)paf.n_records, (long long)paf.n_lines, (long long)paf.n_targets, cs_sum, paf.message);
      mpc_coverage_ingest_free(&paf);
      mpc_pseudopair_stats st;
      const int prc = mpc_pseudopair(argv[i], 7, 1, argv[1], threads, &st);
      printf("pp %d threads %d rc %d fwd %lld rev %lld kept %lld %lld pairs %lld message %s\n", i - 2, threads, prc,
             (long long)st.n_fwd, (long long)st.n_rev, (long long)st.n_fwd_kept, (long long)st.n_rev_kept,
             (long long)st.n_pairs, st.message);
    }
  }
  return 0;
}
