// linkage.cpp -- host half of linkage_qc (include/mpc_linkage.h):
//   mpc_linkage_host        plain scalar walk over the definition, one token at
//                           a time, then the pair counts: the CPU checker of
//                           K_lnkparse / K_lnkplanes / K_lnkpair, the timing
//                           baseline, --device cpu
//   mpc_linkage_pairs_host  the pair counts of a given allele matrix
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "host_file.h"
#include "host_threads.h"
#include "mpc_coverage.h"
#include "mpc_cstables.h"
#include "mpc_cswalk_host.h"
#include "mpc_linkage.h"

namespace {

constexpr int kOk = 0;  // MPC_OK of mpc.h

thread_local mpc_host::LastError g_lerr;

using mpc_host::parallel;

inline uint8_t sub_code(uint8_t y) {
  switch (y | 32) {
    case 'a': return 2;
    case 'c': return 3;
    case 'g': return 4;
    case 't': return 5;
  }
  return 6;
}

// what a token does to the record's allele row (the effects policy of cs_walk,
// mpc_cswalk_host.h).  key[0, nk): the sample's site keys, row[0, nk): its
// allele codes (zero on entry)
struct SiteFx {
  const int64_t* key;
  int64_t nk;
  uint8_t* row;
  void mark(int64_t want, uint8_t code) {
    const int64_t* it = std::lower_bound(key, key + nk, want);
    if (it != key + nk && *it == want) row[it - key] = code;
  }
  void match(int64_t, int64_t) {}
  void mismatch(int64_t p, uint8_t y) { mark(2 * p + 1, sub_code(y)); }
  void deletion(int64_t p, int64_t n) {
    for (const int64_t* it = std::lower_bound(key, key + nk, 2 * p + 1); it != key + nk && *it < 2 * (p + n); ++it)
      if (*it & 1) row[it - key] = 7;
  }
  void insertion(int64_t p, int64_t) { mark(2 * p, 7); }
  // after a walk of [ts, end] that returned MPC_COV_OK: covered ? max(code, 1) : 0
  void finish(int64_t ts, int64_t end) {
    for (int64_t i = 0; i < nk; ++i) {
      const int64_t s = key[i] >> 1;
      const bool covered = s >= ts && ((key[i] & 1) ? s < end : s <= end);
      row[i] = covered ? std::max<uint8_t>(row[i], 1) : 0;
    }
  }
};

// pair[i][j][a][b] over the records: every thread counts the upper triangle of
// its cut of the records into a table of its own, then the tables are summed
// and mirrored
void count_pairs(const uint8_t* alleles, int64_t N, int K, uint32_t* pair, int threads) {
  const size_t cells = (size_t)K * K * 64;
  std::fill(pair, pair + cells, 0u);
  const int T = mpc_host::clamp_threads(threads, N / 1024 + 1);
  std::vector<std::vector<uint32_t>> priv((size_t)T);
  parallel(T, [&](int t) {
    uint32_t* my = pair;
    if (t > 0) {
      priv[(size_t)t].assign(cells, 0u);
      my = priv[(size_t)t].data();
    }
    const int64_t a = N * t / T, b = N * (t + 1) / T;
    for (int64_t r = a; r < b; ++r) {
      const uint8_t* row = alleles + r * K;
      for (int i = 0; i < K; ++i) {
        uint32_t* base = my + ((size_t)i * K) * 64 + (size_t)(row[i] & 7) * 8;
        for (int j = i; j < K; ++j) ++base[(size_t)j * 64 + (row[j] & 7)];
      }
    }
  });
  for (int t = 1; t < T; ++t)
    for (size_t c = 0; c < cells; ++c) pair[c] += priv[(size_t)t][c];
  for (int i = 0; i < K; ++i)
    for (int j = i + 1; j < K; ++j)
      for (int a = 0; a < 8; ++a)
        for (int b = 0; b < 8; ++b) pair[(((size_t)j * K + i) * 8 + b) * 8 + a] = pair[(((size_t)i * K + j) * 8 + a) * 8 + b];
}

}  // namespace

extern "C" {

const char* mpc_linkage_last_error(void) { return g_lerr.msg.c_str(); }

int mpc_linkage_pairs_host(const uint8_t* alleles, int64_t n_records, int32_t n_sites, uint32_t* pair, int threads) {
  if (n_records < 0 || n_records > INT32_MAX) return g_lerr.fail("mpc_linkage_pairs_host: n_records outside [0, 2^31)");
  if (n_sites < 1 || n_sites > MPC_LNK_MAX_SITES)
    return g_lerr.fail("mpc_linkage_pairs_host: n_sites outside [1, " + std::to_string(MPC_LNK_MAX_SITES) + "]");
  if (!pair || (n_records > 0 && !alleles)) return g_lerr.fail("mpc_linkage_pairs_host: null pointer");
  count_pairs(alleles, n_records, n_sites, pair, threads);
  return kOk;
}

int mpc_linkage_host(const uint8_t* cs, const int64_t* cs_off, const int64_t* tstart, const int32_t* rec_sample,
                     int64_t n_records, const int64_t* pos_off, int32_t n_samples, const int64_t* site_off,
                     const int64_t* site_key, int32_t n_sites, uint8_t* alleles, uint32_t* pair, int32_t* status,
                     int threads) {
  const std::string fn = "mpc_linkage_host: ";
  if (n_records < 0 || n_records > INT32_MAX) return g_lerr.fail(fn + "n_records outside [0, 2^31)");
  if (n_samples < 1) return g_lerr.fail(fn + "n_samples < 1");
  if (n_sites < 1 || n_sites > MPC_LNK_MAX_SITES)
    return g_lerr.fail(fn + "n_sites outside [1, " + std::to_string(MPC_LNK_MAX_SITES) + "]");
  if (!pos_off || !site_off || !site_key || !pair || !status || !cs_off ||
      (n_records > 0 && (!cs || !tstart || !rec_sample || !alleles)))
    return g_lerr.fail(fn + "null pointer");
  const size_t S = (size_t)n_samples;
  const int64_t K = n_sites;
  const std::string bad = mpc_host::check_sites(pos_off, site_off, site_key, S, K);
  if (!bad.empty()) return g_lerr.fail(fn + bad);
  status[0] = status[1] = 0;
  if (n_records > 0) std::memset(alleles, 0, (size_t)n_records * (size_t)K);

  const int T = mpc_host::clamp_threads(threads, n_records);
  mpc_host::walk_records(n_records, T, status, [&](int) {
    return [=](int64_t r) {
      const int32_t s = rec_sample[r];
      if (s < 0 || s >= n_samples) return (int)MPC_COV_RANGE;
      SiteFx fx = {site_key + site_off[s], site_off[s + 1] - site_off[s], alleles + r * K + site_off[s]};
      const int64_t ts = tstart[r];
      int64_t end = 0;
      const int code = mpc_host::cs_walk(cs + cs_off[r], cs_off[r + 1] - cs_off[r], ts, pos_off[s + 1] - pos_off[s] - 1, fx, &end);
      if (code == MPC_COV_OK) fx.finish(ts, end);
      return code;
    };
  });
  count_pairs(alleles, n_records, n_sites, pair, threads);
  return kOk;
}

}  // extern "C"
