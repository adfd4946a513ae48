// mpc_bandtrace.h -- what verify_consensus and align_reads must agree on, each
// written once: the symbol codes, the band's geometry and flag bits, the run
// packing (host and device, MPC_HD), the rules of the pair, revcomp and job
// tables (host entry points, and device entry points on their read-back; the
// guards of K_vscan, K_arevcomp and K_atrace restate them in place, so that
// their code stays what it was), and the one host band DP + canonical
// traceback (mpc_verify_script, mpc_align_trace_host), and the end rule of
// align_reads with the cs bytes of a run (host and device: render_one, the
// handoff's host twins, K_acslen and K_acswrite).  No HIP header: g++ and hipcc
// both compile it.
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

// ---- the end rule and the cs bytes of a run (host and device) -----------------
// What one run moves and writes: read bases, target bases, and its bytes in the
// short-form cs ('=' ":<len>", 'X' "*tq" per base, 'D' an insertion "+<read
// bases>", 'I' a deletion "-<target bases>").
MPC_HD inline int32_t dec_digits(int64_t v) {
  int32_t k = 1;
  while (v >= 10) { v /= 10; ++k; }
  return k;
}
MPC_HD inline int64_t run_read_bases(int32_t run) { return run_op(run) != kOpI ? run_len(run) : 0; }
MPC_HD inline int64_t run_target_bases(int32_t run) { return run_op(run) != kOpD ? run_len(run) : 0; }
MPC_HD inline int64_t run_cs_bytes(int32_t run) {
  const int64_t len = run_len(run);
  switch (run_op(run)) {
    case kOpEq: return 1 + dec_digits(len);
    case kOpX: return 3 * len;
  }
  return 1 + len;
}
MPC_HD inline uint8_t lower_ascii(uint8_t c) { return (uint8_t)((c >= 'A' && c <= 'Z') ? c + 32 : c); }
MPC_HD inline uint8_t upper_ascii(uint8_t c) { return (uint8_t)((c >= 'a' && c <= 'z') ? c - 32 : c); }

// The kept span of a read's runs (traceback order, end -> start): [first, last]
// between the outermost '=' runs; what the dropped ops consumed: a_q / a_t the
// leading read / target bases (runs behind last), b_q / b_t the trailing ones
// (runs before first); and the sums over the kept span.  kept is false, and
// nothing else is set, for a read with no '=' run.  The wave of K_acslen takes
// the same sums 64 runs at a time from the same per-run functions.
struct EndRule {
  int32_t first, last;
  int64_t a_q, a_t, b_q, b_t;
  int64_t cs_bytes, n_eq, n_ops;  // of the kept span (cs_bytes without the "Z:")
};
MPC_HD inline bool end_rule(const int32_t* runs, int32_t n_runs, EndRule& e) {
  e = EndRule{0, n_runs - 1, 0, 0, 0, 0, 0, 0, 0};
  while (e.first < n_runs && run_op(runs[e.first]) != kOpEq) {
    e.b_q += run_read_bases(runs[e.first]);
    e.b_t += run_target_bases(runs[e.first]);
    ++e.first;
  }
  if (e.first >= n_runs) return false;
  while (run_op(runs[e.last]) != kOpEq) {
    e.a_q += run_read_bases(runs[e.last]);
    e.a_t += run_target_bases(runs[e.last]);
    --e.last;
  }
  for (int32_t k = e.first; k <= e.last; ++k) {
    e.n_ops += run_len(runs[k]);
    if (run_op(runs[k]) == kOpEq) e.n_eq += run_len(runs[k]);
    e.cs_bytes += run_cs_bytes(runs[k]);
  }
  return true;
}

// One run's cs bytes at dst (run_cs_bytes(run) of them), read at q[i ..] and
// target at t[j ..]; one lane of K_acswrite, one step of the host loops.
MPC_HD inline void put_run_cs(uint8_t* dst, int32_t run, const uint8_t* q, int64_t i, const uint8_t* t, int64_t j) {
  const int32_t len = run_len(run);
  q += i;
  t += j;
  switch (run_op(run)) {
    case kOpEq: {
      int32_t k = dec_digits(len);
      dst[0] = ':';
      for (int32_t v = len; k > 0; --k, v /= 10) dst[k] = (uint8_t)('0' + v % 10);
      break;
    }
    case kOpX:
      for (int32_t x = 0; x < len; ++x) {
        dst[3 * x] = '*';
        dst[3 * x + 1] = lower_ascii(t[x]);
        dst[3 * x + 2] = lower_ascii(q[x]);
      }
      break;
    case kOpD:  // a read base missing from the target: an insertion
      dst[0] = '+';
      for (int32_t x = 0; x < len; ++x) dst[1 + x] = lower_ascii(q[x]);
      break;
    default:  // an extra target base: a deletion
      dst[0] = '-';
      for (int32_t x = 0; x < len; ++x) dst[1 + x] = lower_ascii(t[x]);
  }
}

// ---- the table rules (host): 0, or why the row is refused --------------------
enum Fault : int {
  kFine = 0, kQueryEmpty, kQueryLong, kTextLen, kOffset, kSpan, kReadLen, kTargetLen, kDistance, kEnd, kSeq, kRuns, kFlags,
  kTrace, kWalk, kSizes, kPlace
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
    case kTrace: return "trace output outside its bounds or status not MPC_ALIGN_OK";
    case kWalk: return "runs do not span the read";
    case kSizes: return "size row does not agree with the job";
    case kPlace: return "place outside its buffer, overlapping or not ascending";
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

// out row of a traced read against its job: status, run count and start inside their bounds
inline int check_traced(const int64_t* j, const int32_t* o) {
  return o[0] != MPC_ALIGN_OK || o[6] < 0 || o[6] > 2 * j[4] + 1 || o[1] < 0 || o[1] > j[5] ? kTrace : kFine;
}

// the runs of a traced read walk exactly its m read bases and its target span [start, end)
inline int check_walk(const int64_t* j, const int32_t* o, const int32_t* runs) {
  int64_t qn = 0, tn = 0;
  for (int32_t k = 0; k < o[6]; ++k) {
    if (run_len(runs[k]) < 1) return kWalk;
    qn += run_read_bases(runs[k]);
    tn += run_target_bases(runs[k]);
  }
  return qn != j[1] || tn != j[5] - o[1] ? kWalk : kFine;
}

// The handoff's size row {kept, cs_len, up_len, down_len, tstart, tend, n_eq,
// n_ops} against its job and its place {cs_off, up_off, down_off} in buffers of
// cap[3] bytes, at or behind next[3] (the ends of the previous read's slots,
// which the call moves on): what mpc_align_cs_write[_host] checks before it
// writes.  A read that is not kept owns no bytes.
inline int check_place(const int64_t* j, const int64_t* z, const int64_t* place, const int64_t* cap, int64_t* next) {
  const int64_t m = j[1], n = j[3];
  if (z[0] != 0 && z[0] != 1) return kSizes;
  if (z[0] == 0) return z[1] | z[2] | z[3] ? kSizes : kFine;
  if (z[1] < 4 || z[2] < 0 || z[3] < 0 || z[2] > m - z[3] || z[4] < 0 || z[5] < z[4] || z[5] > n) return kSizes;
  const int64_t len[3] = {z[1], z[2], z[3]};
  for (int k = 0; k < 3; ++k) {
    if (place[k] < next[k] || place[k] > cap[k] - len[k]) return kPlace;
    next[k] = place[k] + len[k];
  }
  return kFine;
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
