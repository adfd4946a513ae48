// draft.cpp -- host half of draft_assembly (include/mpc_draft.h):
//   mpc_draft_vote_host  the votes of a launch's traced reads: the CPU checker
//                        of K_dvote, the timing baseline, --device cpu
//   mpc_draft_call_host  the new draft from the tallies: the same for K_dcall
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "host_file.h"
#include "host_threads.h"
#include "mpc_bandtrace.h"
#include "mpc_draft.h"
#include "mpc_draftrule.h"

namespace {
using namespace mpc_band;
using namespace mpc_draft;
using mpc_host::clamp_threads;

constexpr int kOk = 0;  // MPC_OK of mpc.h

thread_local mpc_host::LastError g_derr;

// One read's votes into t (rows 0 .. n); its vote status.
int32_t vote_one(const uint8_t* q, const int64_t* job, const int32_t* o, const int32_t* runs, uint32_t* t) {
  if (o[0] != MPC_ALIGN_OK) return MPC_DRAFT_NOT_TRACED;
  const int64_t m = job[1], end = job[5];
  const int32_t n_runs = o[6];
  // the runs must walk exactly the read and [start, end): every index below then stays inside both
  int64_t qn = 0, tn = 0;
  int32_t first = -1, last = -1;  // the outermost '=' runs, in alignment order a = n_runs - 1 - k
  for (int32_t a = 0; a < n_runs; ++a) {
    const int32_t run = runs[n_runs - 1 - a];
    const int64_t len = run_len(run), op = run_op(run);
    if (len < 1) return MPC_DRAFT_BAD_RUNS;
    if (op != kOpI) qn += len;
    if (op != kOpD) tn += len;
    if (op == kOpEq) {
      if (first < 0) first = a;
      last = a;
    }
  }
  if (qn != m || tn != end - o[1]) return MPC_DRAFT_BAD_RUNS;
  if (first < 0) return MPC_DRAFT_NO_MATCH;
  int64_t i = 0, j = o[1];
  for (int32_t a = 0; a <= last; ++a) {
    const int32_t run = runs[n_runs - 1 - a];
    const int64_t len = run_len(run), op = run_op(run);
    if (a >= first) {
      uint32_t* row = t + j * MPC_DRAFT_ROW;
      if (a == first) ++row[kStarts];
      switch (op) {
        case kOpEq:
          ++row[kEqOn];
          ++row[len * MPC_DRAFT_ROW + kEqOff];
          break;
        case kOpX:
          for (int64_t x = 0; x < len; ++x) {
            const uint32_t c = vcode(q[i + x], 4);
            if (c < 4) ++row[x * MPC_DRAFT_ROW + kSub + c];
          }
          break;
        case kOpI:  // an extra target base: a deletion
          ++row[kDelOn];
          ++row[len * MPC_DRAFT_ROW + kDelOff];
          break;
        default:  // a read base missing from the target: an insertion in front of column j
          for (int64_t s = 0; s < std::min<int64_t>(len, MPC_DRAFT_SLOTS); ++s) {
            const uint32_t c = vcode(q[i + s], 4);
            if (c < 4) ++row[kIns + 4 * s + c];
          }
      }
      if (a == last) ++t[(j + len) * MPC_DRAFT_ROW + kEnds];  // ('=': consumes len columns)
    }
    if (op != kOpI) i += len;
    if (op != kOpD) j += len;
  }
  return MPC_DRAFT_VOTED;
}

}  // namespace

extern "C" const char* mpc_draft_last_error(void) { return g_derr.msg.c_str(); }

extern "C" int mpc_draft_vote_host(const uint8_t* seq, int64_t seq_bytes, const int64_t* jobs, int32_t n_jobs,
                                   const int32_t* out, const int32_t* runs, int64_t runs_cap, uint32_t* tally, int64_t n,
                                   int32_t* status, int threads) {
  const std::string fn = "mpc_draft_vote_host: ";
  if (n_jobs < 0) return g_derr.fail(fn + "n_jobs < 0");
  if (n_jobs == 0) return kOk;
  if (!seq || !jobs || !out || !runs || !tally || !status) return g_derr.fail(fn + "null pointer");
  if (const char* bad = vote_sizes_fault(n, seq_bytes, runs_cap)) return g_derr.fail(fn + bad);
  for (int32_t r = 0; r < n_jobs; ++r)
    if (const char* bad = vote_row_fault(jobs + 8 * (int64_t)r, out + 8 * (int64_t)r, seq_bytes, runs_cap, n))
      return g_derr.fail(fn + "read " + std::to_string(r) + ": " + bad);
  const size_t words = (size_t)(n + 1) * MPC_DRAFT_ROW;
  // contiguous shares of reads per thread, each with tallies of its own (thread 0: the caller's)
  const int nt = clamp_threads(threads, (n_jobs + 63) / 64);
  std::vector<std::vector<uint32_t>> part((size_t)nt);
  try {
    for (int k = 1; k < nt; ++k) part[(size_t)k].assign(words, 0);
  } catch (const std::bad_alloc&) {
    return g_derr.fail(fn + "out of memory for the threads' tallies");
  }
  mpc_host::parallel(nt, [&](int k) {
    uint32_t* t = k == 0 ? tally : part[(size_t)k].data();
    const int32_t r0 = (int32_t)((int64_t)n_jobs * k / nt), r1 = (int32_t)((int64_t)n_jobs * (k + 1) / nt);
    for (int32_t r = r0; r < r1; ++r) {
      const int64_t* j = jobs + 8 * (int64_t)r;
      status[r] = vote_one(seq + j[0], j, out + 8 * (int64_t)r, runs + j[7], t);
    }
  });
  if (nt > 1)
    mpc_host::parallel(nt, [&](int k) {
      const size_t w0 = words * (size_t)k / (size_t)nt, w1 = words * (size_t)(k + 1) / (size_t)nt;
      for (int p = 1; p < nt; ++p) {
        const uint32_t* src = part[(size_t)p].data();
        for (size_t w = w0; w < w1; ++w) tally[w] += src[w];
      }
    });
  for (int32_t r = 0; r < n_jobs; ++r)
    if (status[r] == MPC_DRAFT_BAD_RUNS)
      return g_derr.fail(fn + "read " + std::to_string(r) + ": the runs do not walk the read and its target span", MPC_DRAFT_E_RUNS);
  return kOk;
}

extern "C" int mpc_draft_call_host(const uint32_t* tally, const uint8_t* draft, int64_t n, uint8_t* new_draft,
                                   int64_t new_cap, int32_t* info) {
  const std::string fn = "mpc_draft_call_host: ";
  if (!info) return g_derr.fail(fn + "null pointer");
  for (int k = 0; k < 8; ++k) info[k] = 0;
  if (!tally || !draft || (!new_draft && new_cap > 0)) return g_derr.fail(fn + "null pointer");
  if (n < 1 || n > MPC_DRAFT_MAX_LEN || new_cap < 0) return g_derr.fail(fn + "draft length outside [1, MPC_DRAFT_MAX_LEN]");
  std::vector<int32_t> cov, eq, del;
  try {
    cov.resize((size_t)n); eq.resize((size_t)n); del.resize((size_t)n);
  } catch (const std::bad_alloc&) {
    return g_derr.fail(fn + "out of memory");
  }
  // 32-bit prefix sums that wrap as K_dcall's do (exact below 2^30 voted reads)
  uint32_t c = 0, e = 0, d = 0;
  int32_t maxcov = 0;
  for (int64_t j = 0; j < n; ++j) {
    const uint32_t* row = tally + j * MPC_DRAFT_ROW;
    c += row[kStarts] - row[kEnds];
    e += row[kEqOn] - row[kEqOff];
    d += row[kDelOn] - row[kDelOff];
    cov[(size_t)j] = (int32_t)c; eq[(size_t)j] = (int32_t)e; del[(size_t)j] = (int32_t)d;
    maxcov = std::max(maxcov, (int32_t)c);
  }
  info[4] = maxcov;
  if (maxcov == 0) {
    info[0] = MPC_DRAFT_EMPTY;
    return g_derr.fail(fn + "no read mapped (the largest coverage is 0)", MPC_DRAFT_E_EMPTY);
  }
  int64_t lo = n, hi = 0;
  for (int64_t j = 0; j < n; ++j)
    if (2 * (int64_t)cov[(size_t)j] >= maxcov) {
      lo = std::min(lo, j);
      hi = j + 1;
    }
  int64_t at = 0;
  int32_t changed = 0, dropped = 0, inserted = 0;
  for (int64_t j = lo; j < hi; ++j) {
    const Emit em = call_column(tally + j * MPC_DRAFT_ROW, draft[j], cov[(size_t)j], eq[(size_t)j], del[(size_t)j], j > lo);
    for (int s = 0; s < em.n_ins; ++s, ++at)
      if (at < new_cap) new_draft[at] = (uint8_t)(em.ins >> (8 * s));
    if (em.col >= 0) {
      if (at < new_cap) new_draft[at] = (uint8_t)em.col;
      ++at;
    }
    inserted += em.n_ins; changed += em.changed; dropped += em.dropped;
  }
  info[1] = (int32_t)at; info[2] = (int32_t)lo; info[3] = (int32_t)hi;
  info[5] = changed; info[6] = dropped; info[7] = inserted;
  if (at > MPC_DRAFT_MAX_LEN) {
    info[0] = MPC_DRAFT_LONG;
    return g_derr.fail(fn + "the new draft holds " + std::to_string(at) + " bases (at most 131072 supported)", MPC_DRAFT_E_LONG);
  }
  if (at > new_cap) return g_derr.fail(fn + "the buffer holds " + std::to_string(new_cap) + " bytes, the new draft needs " + std::to_string(at));
  return kOk;
}
