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
#include <thread>
#include <vector>

#include "host_threads.h"
#include "mpc_coverage.h"
#include "mpc_linkage.h"

namespace {

constexpr int kOk = 0, kArg = -1;  // MPC_OK, MPC_E_ARG of mpc.h

thread_local std::string g_lerr;
int lfail(const std::string& msg) {
  g_lerr = msg;
  return kArg;
}

template <class F>
void parallel(int T, F f) {
  if (T <= 1) { f(0); return; }
  std::vector<std::thread> th;
  th.reserve((size_t)T);
  for (int k = 0; k < T; ++k) th.emplace_back(f, k);
  for (auto& t : th) t.join();
}

inline bool is_letter(uint8_t c) { return (uint8_t)((c | 32) - 'a') < 26; }
inline bool is_digit(uint8_t c) { return (uint8_t)(c - '0') < 10; }

inline uint8_t sub_code(uint8_t y) {
  switch (y | 32) {
    case 'a': return 2;
    case 'c': return 3;
    case 'g': return 4;
    case 't': return 5;
  }
  return 6;
}

// One record, straight from the definition.  key[0, nk): the sample's site
// keys, row[0, nk): its allele codes (zero on entry).  Returns MPC_COV_*;
// malformed wins over out of range, so the grammar is followed to the end of
// the cs even once p has left the target.
int walk(const uint8_t* q, int64_t len, int64_t ts, int64_t L, const int64_t* key, int64_t nk, uint8_t* row) {
  if (len < 0) return MPC_COV_MALFORMED;
  if (len >= 2 && q[0] == 'Z' && q[1] == ':') { q += 2; len -= 2; }
  bool oor = ts < 0 || ts > L;
  int64_t p = ts, k = 0;
  auto mark = [&](int64_t want, uint8_t code) {
    const int64_t* it = std::lower_bound(key, key + nk, want);
    if (it != key + nk && *it == want) row[it - key] = code;
  };
  while (k < len) {
    const uint8_t op = q[k++];
    const int64_t a = k;
    if (op == ':') {
      int64_t n = 0;
      while (k < len && is_digit(q[k])) {
        if (k - a == 9) return MPC_COV_MALFORMED;  // a tenth digit
        n = n * 10 + (q[k++] - '0');
      }
      if (k == a) return MPC_COV_MALFORMED;
      if (!oor && p + n <= L) p += n;
      else oor = true;
    } else if (op == '*') {
      if (len - k < 2 || !is_letter(q[k]) || !is_letter(q[k + 1])) return MPC_COV_MALFORMED;
      k += 2;
      if (k < len && is_letter(q[k])) return MPC_COV_MALFORMED;
      if (!oor && p < L) {
        mark(2 * p + 1, sub_code(q[k - 1]));
        ++p;
      } else oor = true;
    } else if (op == '-' || op == '+') {
      while (k < len && is_letter(q[k])) ++k;
      const int64_t n = k - a;
      if (n == 0) return MPC_COV_MALFORMED;
      if (op == '-') {
        if (!oor && p + n <= L) {
          for (const int64_t* it = std::lower_bound(key, key + nk, 2 * p + 1); it != key + nk && *it < 2 * (p + n); ++it)
            if (*it & 1) row[it - key] = 7;
          p += n;
        } else oor = true;
      } else {
        if (!oor && p <= L) mark(2 * p, 7);
        else oor = true;
      }
    } else {
      return MPC_COV_MALFORMED;
    }
  }
  if (oor) return MPC_COV_RANGE;
  for (int64_t i = 0; i < nk; ++i) {
    const int64_t s = key[i] >> 1;
    const bool covered = s >= ts && ((key[i] & 1) ? s < p : s <= p);
    row[i] = covered ? std::max<uint8_t>(row[i], 1) : 0;
  }
  return MPC_COV_OK;
}

// pair[i][j][a][b] over the records: every thread counts the upper triangle of
// its cut of the records into a table of its own, then the tables are summed
// and mirrored
void count_pairs(const uint8_t* alleles, int64_t N, int K, uint32_t* pair, int threads) {
  const size_t cells = (size_t)K * K * 64;
  std::fill(pair, pair + cells, 0u);
  int T = threads > 0 ? threads : mpc_host::host_threads();
  T = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)T, N / 1024 + 1));
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

const char* mpc_linkage_last_error(void) { return g_lerr.c_str(); }

int mpc_linkage_pairs_host(const uint8_t* alleles, int64_t n_records, int32_t n_sites, uint32_t* pair, int threads) {
  if (n_records < 0 || n_records > INT32_MAX) return lfail("mpc_linkage_pairs_host: n_records outside [0, 2^31)");
  if (n_sites < 1 || n_sites > MPC_LNK_MAX_SITES)
    return lfail("mpc_linkage_pairs_host: n_sites outside [1, " + std::to_string(MPC_LNK_MAX_SITES) + "]");
  if (!pair || (n_records > 0 && !alleles)) return lfail("mpc_linkage_pairs_host: null pointer");
  count_pairs(alleles, n_records, n_sites, pair, threads);
  return kOk;
}

int mpc_linkage_host(const uint8_t* cs, const int64_t* cs_off, const int64_t* tstart, const int32_t* rec_sample,
                     int64_t n_records, const int64_t* pos_off, int32_t n_samples, const int64_t* site_off,
                     const int64_t* site_key, int32_t n_sites, uint8_t* alleles, uint32_t* pair, int32_t* status,
                     int threads) {
  const std::string fn = "mpc_linkage_host: ";
  if (n_records < 0 || n_records > INT32_MAX) return lfail(fn + "n_records outside [0, 2^31)");
  if (n_samples < 1) return lfail(fn + "n_samples < 1");
  if (n_sites < 1 || n_sites > MPC_LNK_MAX_SITES)
    return lfail(fn + "n_sites outside [1, " + std::to_string(MPC_LNK_MAX_SITES) + "]");
  if (!pos_off || !site_off || !site_key || !pair || !status || !cs_off ||
      (n_records > 0 && (!cs || !tstart || !rec_sample || !alleles)))
    return lfail(fn + "null pointer");
  const size_t S = (size_t)n_samples;
  const int64_t K = n_sites;
  if (pos_off[0] != 0) return lfail(fn + "pos_off[0] != 0");
  if (site_off[0] != 0 || site_off[S] != K) return lfail(fn + "site_off does not run from 0 to n_sites");
  for (size_t s = 0; s < S; ++s) {
    const int64_t L = pos_off[s + 1] - pos_off[s] - 1;
    const std::string who = fn + "sample " + std::to_string(s) + ": ";
    if (L < 0) return lfail(who + "pos_off is not increasing");
    if (pos_off[s + 1] > INT32_MAX) return lfail(who + "n_pos is not below 2^31");
    if (site_off[s + 1] < site_off[s] || site_off[s + 1] > K) return lfail(who + "site_off is not monotone");
    for (int64_t k = site_off[s]; k < site_off[s + 1]; ++k) {
      const int64_t key = site_key[k];
      if (key < 0 || key > 2 * L || ((key & 1) && key > 2 * L - 1))
        return lfail(who + "site key " + std::to_string(key) + " is outside a target of " + std::to_string(L) + " bases");
      if (k > site_off[s] && key <= site_key[k - 1]) return lfail(who + "site keys are not strictly increasing");
    }
  }
  status[0] = status[1] = 0;
  if (n_records > 0) std::memset(alleles, 0, (size_t)n_records * (size_t)K);

  int T = threads > 0 ? threads : mpc_host::host_threads();
  T = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)T, n_records));
  std::vector<int64_t> first_bad((size_t)T, INT64_MAX);
  std::vector<int> first_code((size_t)T, 0);
  parallel(T, [&](int t) {
    const int64_t a = n_records * t / T, b = n_records * (t + 1) / T;
    for (int64_t r = a; r < b; ++r) {
      const int32_t s = rec_sample[r];
      int code = MPC_COV_RANGE;
      if (s >= 0 && s < n_samples)
        code = walk(cs + cs_off[r], cs_off[r + 1] - cs_off[r], tstart[r], pos_off[s + 1] - pos_off[s] - 1,
                    site_key + site_off[s], site_off[s + 1] - site_off[s], alleles + r * K + site_off[s]);
      if (code != MPC_COV_OK && first_bad[(size_t)t] == INT64_MAX) {
        first_bad[(size_t)t] = r;
        first_code[(size_t)t] = code;
      }
    }
  });
  for (int t = 0; t < T; ++t)
    if (first_bad[(size_t)t] != INT64_MAX && status[0] == 0) {  // (cuts are in record order)
      status[0] = first_code[(size_t)t];
      status[1] = (int32_t)first_bad[(size_t)t];
    }
  count_pairs(alleles, n_records, n_sites, pair, threads);
  return kOk;
}

}  // extern "C"
