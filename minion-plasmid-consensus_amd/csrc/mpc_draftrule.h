// mpc_draftrule.h -- what the host and the device half of draft_assembly must
// agree on, each written once (include/mpc_draft.h has the definition): the
// words of a tally row, the rule of the vote's tables, and the call of one
// column from its row and its prefix sums (MPC_HD: K_dcall and
// mpc_draft_call_host run the same code).  No HIP header: g++ and hipcc both
// compile it.
#pragma once
#include <cstdint>

#include "mpc_bandtrace.h"
#include "mpc_draft.h"

namespace mpc_draft {

enum : int { kStarts = 0, kEnds = 1, kEqOn = 2, kEqOff = 3, kDelOn = 4, kDelOff = 5, kSub = 8, kIns = 16 };

// ---- the vote's tables (host entry points, device entry point on its read-back) ----
// 0, or why the call is refused
inline const char* vote_sizes_fault(int64_t n, int64_t seq_bytes, int64_t runs_cap) {
  if (n < 1 || n > MPC_DRAFT_MAX_LEN) return "target length outside [1, MPC_DRAFT_MAX_LEN]";
  if (seq_bytes < 0 || runs_cap < 0) return "negative size";
  return nullptr;
}

// one read: the job rule of mpc_bandtrace.h, the tallies' n, and an out row that indexes its runs
inline const char* vote_row_fault(const int64_t* j, const int32_t* o, int64_t seq_bytes, int64_t runs_cap, int64_t n) {
  if (const int bad = mpc_band::check_job(j, seq_bytes, runs_cap)) return mpc_band::fault_text(bad);
  if (j[3] != n) return "target length is not the tallies' n";
  if (o[0] == MPC_ALIGN_OK && (o[6] < 0 || o[6] > 2 * j[4] + 1 || o[1] < 0 || o[1] > j[5])) return "trace output outside its bounds";
  return nullptr;
}

// ---- the call of one column ----------------------------------------------------
struct Emit {
  uint64_t ins;    // the bytes emitted from the insertion slots, first in the low byte
  int32_t n_ins;   // 0 .. MPC_DRAFT_SLOTS
  int32_t col;     // the column's byte, or -1
  bool changed, dropped;
};

// 'A' 'C' 'G' 'T' of codes 0-3 (one constant: no table in memory on the device)
MPC_HD inline uint32_t acgt(uint32_t code) { return (0x54474341u >> (8 * code)) & 0xffu; }

MPC_HD inline uint32_t smallest_max4(const int64_t* v) {
  uint32_t best = 0;
  for (uint32_t c = 1; c < 4; ++c)
    if (v[c] > v[best]) best = c;
  return best;
}

// row: the MPC_DRAFT_ROW words of column j; cov, eq, del: its prefix sums;
// with_ins: j > lo (the slots in front of the first kept column are not emitted)
MPC_HD inline Emit call_column(const uint32_t* row, uint32_t draft_byte, int64_t cov, int64_t eq, int64_t del, bool with_ins) {
  Emit e{0, 0, -1, false, false};
  if (with_ins) {
    const int64_t gcov = cov - (int64_t)row[kStarts];
    for (int s = 0; s < MPC_DRAFT_SLOTS; ++s) {
      int64_t v[4];
      for (int c = 0; c < 4; ++c) v[c] = row[kIns + 4 * s + c];
      if (!(2 * (v[0] + v[1] + v[2] + v[3]) > gcov)) break;
      e.ins |= (uint64_t)acgt(smallest_max4(v)) << (8 * e.n_ins);
      ++e.n_ins;
    }
  }
  const uint32_t dc = mpc_band::vcode(draft_byte, 5);
  int64_t b[4];
  for (uint32_t c = 0; c < 4; ++c) b[c] = (int64_t)row[kSub + c] + (c == dc ? eq : 0);
  if (b[0] + b[1] + b[2] + b[3] == 0) {
    e.col = (int32_t)draft_byte;
  } else if (2 * del > cov) {
    e.dropped = true;
  } else {
    uint32_t code = smallest_max4(b);
    if (dc < 4 && b[dc] == b[code]) code = dc;
    e.col = (int32_t)acgt(code);
    e.changed = code != dc;
  }
  return e;
}

}  // namespace mpc_draft
