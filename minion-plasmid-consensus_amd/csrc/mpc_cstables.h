// mpc_cstables.h -- the one validation of the sample and site tables of
// include/mpc_coverage.h and mpc_linkage.h, shared by the host entry points
// (coverage.cpp, linkage.cpp) and the device ones (mpc_cov.hip, mpc_link.hip,
// on their read-back of the tables).  Host-only, plain C++17: g++ and hipcc
// both compile it.  Each check returns an empty string, or what is wrong, to go
// behind the caller's "<entry point>: ".
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace mpc_host {

// rows of sample s: "" or what is wrong with pos_off[s .. s + 1]
inline std::string check_sample_rows(const int64_t* pos_off, size_t s) {
  if (pos_off[s + 1] - pos_off[s] - 1 < 0) return "pos_off is not increasing";
  if (pos_off[s + 1] > INT32_MAX) return "n_pos is not below 2^31";
  return "";
}

// pos_off[S + 1] and, unless null, region[S][2]
inline std::string check_samples(const int64_t* pos_off, const int64_t* region, size_t S) {
  if (pos_off[0] != 0) return "pos_off[0] != 0";
  for (size_t s = 0; s < S; ++s) {
    std::string bad = check_sample_rows(pos_off, s);
    if (bad.empty() && region) {
      const int64_t L = pos_off[s + 1] - pos_off[s] - 1, lo = region[2 * s], hi = region[2 * s + 1];
      if (lo < 0 || lo > hi || hi > L)
        bad = "region [" + std::to_string(lo) + ", " + std::to_string(hi) + ") is outside [0, " + std::to_string(L) + ")";
    }
    if (!bad.empty()) return "sample " + std::to_string(s) + ": " + bad;
  }
  return "";
}

// pos_off[S + 1], site_off[S + 1] and site_key[K]
inline std::string check_sites(const int64_t* pos_off, const int64_t* site_off, const int64_t* site_key, size_t S,
                               int64_t K) {
  if (pos_off[0] != 0) return "pos_off[0] != 0";
  if (site_off[0] != 0 || site_off[S] != K) return "site_off does not run from 0 to n_sites";
  for (size_t s = 0; s < S; ++s) {
    const int64_t L = pos_off[s + 1] - pos_off[s] - 1;
    std::string bad = check_sample_rows(pos_off, s);
    if (bad.empty() && (site_off[s + 1] < site_off[s] || site_off[s + 1] > K)) bad = "site_off is not monotone";
    for (int64_t k = site_off[s]; bad.empty() && k < site_off[s + 1]; ++k) {
      const int64_t key = site_key[k];
      if (key < 0 || key > 2 * L || ((key & 1) && key > 2 * L - 1))
        bad = "site key " + std::to_string(key) + " is outside a target of " + std::to_string(L) + " bases";
      else if (k > site_off[s] && key <= site_key[k - 1]) bad = "site keys are not strictly increasing";
    }
    if (!bad.empty()) return "sample " + std::to_string(s) + ": " + bad;
  }
  return "";
}

}  // namespace mpc_host
