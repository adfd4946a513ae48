// mpc_bandtrace.h -- what verify_consensus and align_reads must agree on, each
// written once: the symbol codes, the band's geometry and flag bits, the run
// packing (host and device, MPC_HD), the rules of the pair, revcomp and job
// tables (host entry points, and device entry points on their read-back; the
// guards of K_vscan, K_arevcomp and K_atrace restate them in place, so that
// their code stays what it was), and the one host band DP + canonical
// traceback (mpc_verify_script, mpc_align_trace_host).  No HIP header: g++ and
// hipcc both compile it.
//
// The band (include/mpc_align.h): given the scan's (d, end), row i (1 <= i <= m)
// holds columns j = i + (end - m) - d + b, 0 <= b < W = 2 d + 1; every optimal
// path to (m, end) stays inside it, cells with j < 0 or j > n are infinite, and
// the value at (m, end) -- slot d of row m -- must be d.  Each cell leaves one
// flag byte: which traceback moves reproduce its value.  The traceback from
// (m, end) takes the diagonal first, then up, then left (mpc_verify.h).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "mpc_align.h"

#ifndef MPC_HD
#if defined(__HIPCC__)
#define MPC_HD __host__ __device__
#else
#define MPC_HD
#endif
#endif

namespace mpc_band {

// A C G T -> 0..3 after upper-casing; any other byte -> `other` (4 on the query
// side, 5 on the text side: equal to nothing)
MPC_HD inline uint32_t vcode(uint32_t c, uint32_t other) {
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
  }
  return other;
}

MPC_HD inline uint32_t complement(uint32_t c) {
  switch (c) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
    case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
  }
  return c;
}

// bytes of one flag row: W rounded up to the 64 lanes of a store
MPC_HD inline int64_t row_pitch(int64_t d) { return (2 * d + 1 + 63) / 64 * 64; }

enum : uint32_t { kDiag = 1, kUp = 2, kMatch = 4 };              // flag bits of a band cell
enum : int32_t { kOpEq = 0, kOpX = 1, kOpI = 2, kOpD = 3 };      // verify's letters = X I D
MPC_HD inline int32_t pack_run(int32_t len, int32_t op) { return (len << 2) | op; }
MPC_HD inline int32_t run_len(int32_t run) { return run >> 2; }
MPC_HD inline int32_t run_op(int32_t run) { return run & 3; }

// ---- the table rules (host): 0, or why the row is refused --------------------
enum Fault : int {
  kFine = 0, kQueryEmpty, kQueryLong, kTextLen, kOffset, kSpan, kReadLen, kTargetLen, kDistance, kEnd, kSeq, kRuns, kFlags
};

// behind the caller's "<entry point>: read N: " / "pair N: " (kFine: null)
inline const char* fault_text(int f) {
  switch (f) {
    case kQueryEmpty: return "empty query";
    case kQueryLong: return "query longer than MPC_VERIFY_MAX_QUERY (65536)";
    case kTextLen: return "text length outside [0, 2^31)";
    case kOffset: return "negative offset";
    case kSpan: return "span outside the blob or overlapping";
    case kReadLen: return "read length outside [1, MPC_VERIFY_MAX_QUERY]";
    case kTargetLen: return "target length outside [1, 2^31)";
    case kDistance: return "distance outside [0, MPC_ALIGN_MAX_EDITS]";
    case kEnd: return "end outside [0, n]";
    case kSeq: return "sequence outside the blob";
    case kRuns: return "runs outside the run buffer";
    case kFlags: return "flag rows outside the workspace or not ascending";
  }
  return nullptr;
}

// the limits of mpc_verify.h
inline int check_lengths(int64_t m, int64_t n) {
  if (m < 1) return kQueryEmpty;
  if (m > MPC_VERIFY_MAX_QUERY) return kQueryLong;
  if (n < 0 || n > INT32_MAX) return kTextLen;
  return kFine;
}

// pair row of the scan: {q_off, q_len, t_off, t_len}
inline int check_pair(const int64_t* r) {
  if (const int bad = check_lengths(r[1], r[3])) return bad;
  return r[0] < 0 || r[2] < 0 ? kOffset : kFine;
}

// revcomp row: {src_off, len, dst_off}, both spans inside the blob and apart
inline int check_revcomp(const int64_t* r, int64_t seq_bytes) {
  const int64_t src = r[0], len = r[1], dst = r[2];
  if (len < 0 || src < 0 || dst < 0 || src > seq_bytes - len || dst > seq_bytes - len) return kSpan;
  return len > 0 && src < dst + len && dst < src + len ? kSpan : kFine;
}

// job row, what host and device share: lengths, d, end, sequences inside the
// blob, runs inside the run buffer
inline int check_job(const int64_t* j, int64_t seq_bytes, int64_t runs_cap) {
  const int64_t q_off = j[0], m = j[1], t_off = j[2], n = j[3], d = j[4], end = j[5], run_off = j[7];
  if (m < 1 || m > MPC_VERIFY_MAX_QUERY) return kReadLen;
  if (n < 1 || n > INT32_MAX) return kTargetLen;
  if (d < 0 || d > MPC_ALIGN_MAX_EDITS) return kDistance;
  if (end < 0 || end > n) return kEnd;
  if (q_off < 0 || q_off > seq_bytes - m || t_off < 0 || t_off > seq_bytes - n) return kSeq;
  if (run_off < 0 || run_off > runs_cap - (2 * d + 1)) return kRuns;
  return kFine;
}

// job row, device entry point only (after check_job): its flag rows inside the
// workspace, at or behind flag_next (the end of the previous job's rows)
inline int check_job_flags(const int64_t* j, int64_t flags_bytes, int64_t flag_next) {
  return j[6] < flag_next || j[6] > flags_bytes - j[1] * row_pitch(j[4]) ? kFlags : kFine;
}

// ---- the host band trace -----------------------------------------------------
struct Band {  // one thread's scratch, grown as needed
  std::vector<uint8_t> flags, tc;
  std::vector<int32_t> row;
};

// One pair (1 <= m, 0 <= n, 0 <= d, 0 <= end <= n): the band DP (one row of
// values kept in place, m x row_pitch(d) flag bytes), the traceback from
// (m, end) and its runs, end -> start, into runs[2 d + 1].  o[8] is the out
// row of mpc_align.h: {status, start, n_eq, n_x, n_i, n_d, n_runs, 0}, all 0
// behind a status of MPC_ALIGN_BAD_SCAN.  Throws std::bad_alloc.
inline void band_trace(const uint8_t* q, int64_t m, const uint8_t* t, int64_t n, int64_t d, int64_t end, int32_t* o,
                       int32_t* runs, Band& s) {
  const int64_t W = 2 * d + 1, P = row_pitch(d), d0 = end - m;
  const int32_t INF = 1 << 20;  // above every reachable value (<= 65,536 + 8,193)
  for (int k = 0; k < 8; ++k) o[k] = 0;
  s.flags.resize((size_t)(m * P));
  s.row.resize((size_t)W + 1);
  // the target bytes any band cell can touch: columns [jlo, jhi]
  const int64_t jlo = std::max<int64_t>(1, 1 + d0 - d), jhi = std::min<int64_t>(n, end + d);
  s.tc.resize((size_t)std::max<int64_t>(0, jhi - jlo + 1));
  for (int64_t j = jlo; j <= jhi; ++j) s.tc[(size_t)(j - jlo)] = (uint8_t)vcode(t[j - 1], 5);
  int32_t* row = s.row.data();
  for (int64_t b = 0; b < W; ++b) {
    const int64_t j = d0 - d + b;
    row[b] = (j >= 0 && j <= n) ? 0 : INF;  // D[0][j] = 0
  }
  row[W] = INF;
  for (int64_t i = 1; i <= m; ++i) {
    const uint8_t qi = (uint8_t)vcode(q[i - 1], 4);
    uint8_t* f = &s.flags[(size_t)((i - 1) * P)];
    int32_t left = INF;  // D[i][j - 1]
    for (int64_t b = 0; b < W; ++b) {
      const int64_t j = i + d0 - d + b;
      int32_t v = INF;
      uint8_t fl = 0;
      if (j >= 0 && j <= n) {
        // row i - 1: column j - 1 is slot b, column j is slot b + 1
        const int32_t up = row[b + 1] + 1;
        if (j == 0) {
          v = (int32_t)i;  // D[i][0] = i
          fl = kUp;
        } else {
          const bool eq = qi == s.tc[(size_t)(j - jlo)];
          const int32_t dg = row[b] + (eq ? 0 : 1);
          v = std::min(dg, std::min(up, left + 1));
          if (dg == v) fl |= kDiag;
          if (up == v) fl |= kUp;
          if (eq) fl |= kMatch;
        }
        if (v > INF) v = INF;
      }
      row[b] = v;
      left = v;
      f[b] = fl;
    }
  }
  if (row[d] != (int32_t)d) {  // (m, end) sits on diagonal d0: slot d
    o[0] = MPC_ALIGN_BAD_SCAN;
    return;
  }
  int64_t i = m, j = end;
  int32_t cnt[4] = {0, 0, 0, 0}, n_runs = 0, op = -1, len = 0;
  const int32_t cap = (int32_t)W;
  bool bad = false;
  auto flush = [&]() {
    if (len > 0) {
      if (n_runs < cap) runs[n_runs] = pack_run(len, op);
      else bad = true;
      ++n_runs;
    }
  };
  while (i > 0) {
    const int64_t b = j - i - d0 + d;
    if (b < 0 || b >= W) { bad = true; break; }
    const uint8_t fl = s.flags[(size_t)((i - 1) * P + b)];
    int32_t now;
    if (j > 0 && (fl & kDiag)) { now = (fl & kMatch) ? kOpEq : kOpX; --i; --j; }
    else if (fl & kUp) { now = kOpD; --i; }
    else if (j > 0) { now = kOpI; --j; }
    else { bad = true; break; }
    if (now != op) { flush(); op = now; len = 0; }
    ++len;
    ++cnt[now];
  }
  flush();
  if (bad) {
    o[0] = MPC_ALIGN_BAD_SCAN;
    return;
  }
  o[1] = (int32_t)j;
  for (int k = 0; k < 4; ++k) o[2 + k] = cnt[k];
  o[6] = n_runs;
}

}  // namespace mpc_band
