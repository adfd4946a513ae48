// verify.cpp -- host half of verify_consensus (include/mpc_verify.h):
//   mpc_verify_scan_host  plain scalar Sellers DP, the definition itself: the CPU
//                         checker of K_vscan, the timing baseline, --device cpu
//   mpc_verify_script     the band trace of mpc_bandtrace.h once (distance, end)
//                         are known, its runs written as a CIGAR
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "host_file.h"
#include "host_threads.h"
#include "mpc_bandtrace.h"
#include "mpc_verify.h"

namespace {
using namespace mpc_band;

constexpr int kOk = 0;  // MPC_OK of mpc.h

thread_local mpc_host::LastError g_verr;

// one pair: column j of D over all rows, text column by text column
void scan_pair(const uint8_t* q, int64_t m, const uint8_t* t, int64_t n, int32_t* out) {
  std::vector<uint8_t> qc((size_t)m);
  for (int64_t i = 0; i < m; ++i) qc[(size_t)i] = (uint8_t)vcode(q[i], 4);
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
    const uint8_t tc = (uint8_t)vcode(t[j - 1], 5);
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

}  // namespace

extern "C" const char* mpc_verify_last_error(void) { return g_verr.msg.c_str(); }

extern "C" int mpc_verify_scan_host(const uint8_t* seq, const int64_t* pairs, int32_t n_pairs, int32_t* out,
                                    int threads) {
  if (n_pairs < 0) return g_verr.fail("mpc_verify_scan_host: n_pairs < 0");
  if (n_pairs == 0) return kOk;
  if (!seq || !pairs || !out) return g_verr.fail("mpc_verify_scan_host: null pointer");
  for (int32_t p = 0; p < n_pairs; ++p)
    if (const int bad = check_pair(pairs + 4 * (int64_t)p))
      return g_verr.fail("mpc_verify_scan_host: pair " + std::to_string(p) + ": " + fault_text(bad));
  std::atomic<int32_t> next{0};
  mpc_host::parallel(mpc_host::clamp_threads(threads, n_pairs), [&](int) {
    for (int32_t p; (p = next.fetch_add(1)) < n_pairs;) {
      const int64_t* r = pairs + 4 * (int64_t)p;
      scan_pair(seq + r[0], r[1], seq + r[2], r[3], out + 2 * (int64_t)p);
    }
  });
  return kOk;
}

extern "C" int mpc_verify_script(const uint8_t* q, int64_t m, const uint8_t* t, int64_t n, int32_t distance,
                                 int32_t end, int32_t* start, int32_t counts[4], char* cigar, size_t cigar_cap) {
  if (!start || !counts || !cigar || !q || (!t && n > 0)) return g_verr.fail("mpc_verify_script: null pointer");
  if (const int bad = check_lengths(m, n)) return g_verr.fail(std::string("mpc_verify_script: ") + fault_text(bad));
  if (distance < 0 || distance > m || end < 0 || end > n)
    return g_verr.fail("mpc_verify_script: (distance, end) outside the matrix");
  if (distance > MPC_VERIFY_MAX_EDITS) {
    if (cigar_cap < 2) return g_verr.fail("mpc_verify_script: cigar buffer too small");
    *start = -1;
    for (int k = 0; k < 4; ++k) counts[k] = -1;
    std::strcpy(cigar, "*");
    return kOk;
  }
  // the band trace of mpc_bandtrace.h; its runs are end -> start
  int32_t o[8];
  std::vector<int32_t> runs;
  try {
    Band band;
    runs.resize(2 * (size_t)distance + 1);
    band_trace(q, m, t, n, distance, end, o, runs.data(), band);
  } catch (const std::bad_alloc&) {
    return g_verr.fail("mpc_verify_script: out of memory for the band");
  }
  if (o[0] != MPC_ALIGN_OK) return g_verr.fail("mpc_verify_script: the band does not give the scan's distance at (m, end)");
  std::string cg;
  for (int32_t k = o[6]; k-- > 0;) {
    cg += std::to_string(run_len(runs[(size_t)k]));
    cg += "=XID"[run_op(runs[(size_t)k])];
  }
  if (cg.size() + 1 > cigar_cap) return g_verr.fail("mpc_verify_script: cigar buffer too small");
  std::memcpy(cigar, cg.c_str(), cg.size() + 1);
  *start = o[1];
  for (int k = 0; k < 4; ++k) counts[k] = o[2 + k];
  return kOk;
}
