// verify.cpp -- host half of verify_consensus (include/mpc_verify.h):
//   mpc_verify_scan_host  plain scalar Sellers DP, the definition itself: the CPU
//                         checker of K_vscan, the timing baseline, --device cpu
//   mpc_verify_script     banded DP + canonical traceback once (distance, end)
//                         are known
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "host_threads.h"
#include "mpc_verify.h"

namespace {

constexpr int kOk = 0, kArg = -1;  // MPC_OK, MPC_E_ARG of mpc.h

thread_local std::string g_verr;
int vfail(const std::string& msg) {
  g_verr = msg;
  return kArg;
}

// A C G T -> 0..3 after upper-casing; any other byte -> `other` (4 on the query
// side, 5 on the text side: equal to nothing)
inline uint8_t vcode(uint8_t c, uint8_t other) {
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
  }
  return other;
}

std::vector<uint8_t> encode(const uint8_t* s, int64_t len, uint8_t other) {
  std::vector<uint8_t> v((size_t)len);
  for (int64_t i = 0; i < len; ++i) v[(size_t)i] = vcode(s[i], other);
  return v;
}

const char* check_lengths(int64_t m, int64_t n) {
  if (m < 1) return "empty query";
  if (m > MPC_VERIFY_MAX_QUERY) return "query longer than MPC_VERIFY_MAX_QUERY (65536)";
  if (n < 0 || n > INT32_MAX) return "text length outside [0, 2^31)";
  return nullptr;
}

// one pair: column j of D over all rows, text column by text column
void scan_pair(const uint8_t* q, int64_t m, const uint8_t* t, int64_t n, int32_t* out) {
  const std::vector<uint8_t> qc = encode(q, m, 4);
  std::vector<int32_t> col((size_t)m + 1);
  for (int64_t i = 0; i <= m; ++i) col[(size_t)i] = (int32_t)i;  // D[i][0] = i
  int32_t best = (int32_t)m, best_end = 0;
  // Rows in chunks that stay in L1; per chunk two passes over column j - 1: the
  // diagonal and left moves (no dependence between rows), then the up moves
  // (the serial chain, one add and one min per cell).
  constexpr int64_t kChunk = 2048;
  int32_t part[kChunk];
  int32_t* c = col.data();
  const uint8_t* qq = qc.data();
  for (int64_t j = 1; j <= n; ++j) {
    const uint8_t tc = vcode(t[j - 1], 5);
    int32_t diag0 = 0, up = 0;  // D[0][j-1], D[0][j]
    for (int64_t a = 1; a <= m; a += kChunk) {
      const int64_t b = std::min(a + kChunk, m + 1);
      const int32_t next_diag0 = c[b - 1];  // D[b-1][j-1], before this chunk overwrites it
      part[0] = std::min(diag0 + (qq[a - 1] != tc), c[a] + 1);
      for (int64_t i = a + 1; i < b; ++i) part[i - a] = std::min(c[i - 1] + (qq[i - 1] != tc), c[i] + 1);
      for (int64_t i = a; i < b; ++i) {
        up = std::min(part[i - a], up + 1);
        c[i] = up;
      }
      diag0 = next_diag0;
    }
    if (up < best) {  // strict: the smallest end wins
      best = up;
      best_end = (int32_t)j;
    }
  }
  out[0] = best;
  out[1] = best_end;
}

void put_run(std::string& s, int64_t len, char op) {
  if (len > 0) {
    s += std::to_string(len);
    s += op;
  }
}

}  // namespace

extern "C" const char* mpc_verify_last_error(void) { return g_verr.c_str(); }

extern "C" int mpc_verify_scan_host(const uint8_t* seq, const int64_t* pairs, int32_t n_pairs, int32_t* out,
                                    int threads) {
  if (n_pairs < 0) return vfail("mpc_verify_scan_host: n_pairs < 0");
  if (n_pairs == 0) return kOk;
  if (!seq || !pairs || !out) return vfail("mpc_verify_scan_host: null pointer");
  for (int32_t p = 0; p < n_pairs; ++p) {
    const int64_t* r = pairs + 4 * (int64_t)p;
    const char* bad = check_lengths(r[1], r[3]);
    if (!bad && (r[0] < 0 || r[2] < 0)) bad = "negative offset";
    if (bad) return vfail("mpc_verify_scan_host: pair " + std::to_string(p) + ": " + bad);
  }
  int nt = threads > 0 ? threads : mpc_host::host_threads();
  nt = std::max(1, std::min(nt, (int)n_pairs));
  std::atomic<int32_t> next{0};
  auto work = [&]() {
    for (int32_t p; (p = next.fetch_add(1)) < n_pairs;) {
      const int64_t* r = pairs + 4 * (int64_t)p;
      scan_pair(seq + r[0], r[1], seq + r[2], r[3], out + 2 * (int64_t)p);
    }
  };
  std::vector<std::thread> pool;
  for (int k = 1; k < nt; ++k) pool.emplace_back(work);
  work();
  for (auto& th : pool) th.join();
  return kOk;
}

extern "C" int mpc_verify_script(const uint8_t* q, int64_t m, const uint8_t* t, int64_t n, int32_t distance,
                                 int32_t end, int32_t* start, int32_t counts[4], char* cigar, size_t cigar_cap) {
  if (!start || !counts || !cigar || !q || (!t && n > 0)) return vfail("mpc_verify_script: null pointer");
  if (const char* bad = check_lengths(m, n)) return vfail(std::string("mpc_verify_script: ") + bad);
  if (distance < 0 || distance > m || end < 0 || end > n)
    return vfail("mpc_verify_script: (distance, end) outside the matrix");
  if (distance > MPC_VERIFY_MAX_EDITS) {
    if (cigar_cap < 2) return vfail("mpc_verify_script: cigar buffer too small");
    *start = -1;
    for (int k = 0; k < 4; ++k) counts[k] = -1;
    std::strcpy(cigar, "*");
    return kOk;
  }
  // Band: row i holds columns j = i + d0 - dist + b, b in [0, W).  Every optimal
  // path to (m, end) stays inside it; cells outside count as infinite.
  const int64_t dist = distance, d0 = (int64_t)end - m, W = 2 * dist + 1;
  const int32_t INF = INT32_MAX / 2;
  const std::vector<uint8_t> qc = encode(q, m, 4), tc = encode(t, n, 5);
  enum : uint8_t { kDiag = 1, kUp = 2, kMatch = 4 };
  std::vector<uint8_t> flags;  // per band cell: which traceback moves reproduce its value
  try {
    flags.assign((size_t)((m + 1) * W), 0);
  } catch (const std::bad_alloc&) {
    return vfail("mpc_verify_script: out of memory for the band");
  }
  // prev[b + 1] = D[i-1][.] at band slot b, with an infinite cell on either side
  std::vector<int32_t> prev((size_t)W + 2, INF), cur((size_t)W + 2, INF);
  for (int64_t b = 0; b < W; ++b) {
    const int64_t j = d0 - dist + b;
    if (j >= 0 && j <= n) prev[(size_t)b + 1] = 0;  // D[0][j] = 0
  }
  for (int64_t i = 1; i <= m; ++i) {
    const uint8_t qi = qc[(size_t)i - 1];
    uint8_t* f = &flags[(size_t)(i * W)];
    cur[0] = INF;
    for (int64_t b = 0; b < W; ++b) {
      const int64_t j = i + d0 - dist + b;
      int32_t v = INF;
      uint8_t fl = 0;
      if (j >= 0 && j <= n) {
        // same column, row i - 1: band slot b + 1; column j - 1, row i - 1: slot b; column j - 1, row i: slot b - 1
        const int32_t up = prev[(size_t)b + 2] + 1;
        if (j == 0) {
          v = (int32_t)i;  // D[i][0] = i (== up when row i - 1 holds column 0)
          fl = kUp;
        } else {
          const bool eq = qi == tc[(size_t)j - 1];
          const int32_t dg = prev[(size_t)b + 1] + (eq ? 0 : 1);
          const int32_t left = cur[(size_t)b] + 1;
          v = std::min(dg, std::min(up, left));
          if (dg == v) fl |= kDiag;
          if (up == v) fl |= kUp;
          if (eq) fl |= kMatch;
        }
        if (v > INF) v = INF;
      }
      cur[(size_t)b + 1] = v;
      f[b] = fl;
    }
    cur[(size_t)W + 1] = INF;
    prev.swap(cur);
  }
  // (m, end) sits on diagonal d0: band slot dist
  if (prev[(size_t)dist + 1] != distance)
    return vfail("mpc_verify_script: the band gives " + std::to_string(prev[(size_t)dist + 1]) + " at (m, end), the scan " +
                 std::to_string(distance));
  std::string ops;  // end -> start
  int64_t i = m, j = end;
  int32_t cnt[4] = {0, 0, 0, 0};
  while (i > 0) {
    const int64_t b = j - i - d0 + dist;
    if (b < 0 || b >= W) return vfail("mpc_verify_script: traceback left the band");
    const uint8_t fl = flags[(size_t)(i * W + b)];
    if (j > 0 && (fl & kDiag)) {
      const bool eq = fl & kMatch;
      ops += eq ? '=' : 'X';
      ++cnt[eq ? 0 : 1];
      --i;
      --j;
    } else if (fl & kUp) {
      ops += 'D';
      ++cnt[3];
      --i;
    } else {
      ops += 'I';
      ++cnt[2];
      --j;
    }
  }
  std::string cg;
  int64_t run = 0;
  char op = 0;
  for (size_t k = ops.size(); k-- > 0;) {
    if (ops[k] != op) {
      put_run(cg, run, op);
      op = ops[k];
      run = 0;
    }
    ++run;
  }
  put_run(cg, run, op);
  if (cg.size() + 1 > cigar_cap) return vfail("mpc_verify_script: cigar buffer too small");
  std::memcpy(cigar, cg.c_str(), cg.size() + 1);
  *start = (int32_t)j;
  for (int k = 0; k < 4; ++k) counts[k] = cnt[k];
  return kOk;
}
