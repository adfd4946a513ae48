// mpc_draft.hip -- the device half of draft_assembly on gfx950 (include/mpc_draft.h;
// DESIGN.md "draft_assembly").
//
//   K_dvote  the votes of a launch's traced reads, one wave64 per read
//   K_dcall  the new draft from the tallies, ONE workgroup of 1024 threads
//
// K_dvote reads a read's runs 64 at a time from the LAST run (the alignment's
// start), one run per lane, twice.  The first pass sums what the runs consume
// and finds the outermost '=' runs by ballot: runs that do not walk exactly the
// read and [start, end) give a status and add nothing, so in the second pass
// every index is inside the read and rows 0 .. n by construction (each lane
// checks it again).  The second pass gives every lane its (i, j) from a wave
// scan of the read and target advances plus one carry per chunk, and the lane
// makes its run's adds: two for a '=' or deletion run whatever its length
// (difference arrays), one per base of a substitution run, at most 8 for an
// insertion run.  The adds are uint32 global atomics whose results are not
// used (no return, no wait), so the tallies do not depend on their order.
//
// K_dcall runs once per round on at most 131,073 rows: three block prefix sums
// and the maximum, the trim bounds, then per tile of 1024 columns the emitted
// length of every column (mpc_draftrule.h call_column), a block exclusive scan
// and the write.  One workgroup, so that the carries are registers and no
// second launch or grid-wide scan is needed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "mpc.h"
#include "mpc_bandtrace.h"
#include "mpc_device.h"
#include "mpc_draft.h"
#include "mpc_draftrule.h"
#include "mpc_launch.h"

namespace {
using namespace mpc;
using namespace mpc_band;
using namespace mpc_draft;

constexpr int kCallThreads = 1024;

__device__ __forceinline__ void add1(uint32_t* p) { atomicAdd(p, 1u); }

// grid: one 64-thread workgroup per read
__global__ __launch_bounds__(64) void K_dvote(const uint8_t* __restrict__ seq, const int64_t seq_bytes,
                                              const int64_t* __restrict__ jobs, const int32_t* __restrict__ out,
                                              const int32_t* __restrict__ runs, const int64_t runs_cap,
                                              uint32_t* __restrict__ tally, const int64_t n_target, int32_t* __restrict__ status) {
  const int ln = lane();
  const int64_t r = blockIdx.x;
  const int64_t* jb = jobs + 8 * r;
  const int32_t* o = out + 8 * r;
  const int64_t q_off = jb[0], m64 = jb[1], n64 = jb[3], d64 = jb[4], end64 = jb[5], run_off = jb[7];
  const int32_t st = o[0], start = o[1], n_runs = o[6];
  if (st != MPC_ALIGN_OK) {
    if (ln == 0) status[r] = MPC_DRAFT_NOT_TRACED;
    return;
  }
  // restates vote_row_fault (mpc_draftrule.h), which the host applies before the launch
  bool ok = m64 >= 1 && m64 <= MPC_VERIFY_MAX_QUERY && n64 == n_target && n64 >= 1 && n64 <= MPC_DRAFT_MAX_LEN && d64 >= 0 &&
            d64 <= MPC_ALIGN_MAX_EDITS && end64 >= 0 && end64 <= n64;
  ok = ok && q_off >= 0 && q_off <= seq_bytes - m64 && run_off >= 0 && run_off <= runs_cap - (2 * d64 + 1);
  ok = ok && n_runs >= 0 && n_runs <= 2 * d64 + 1 && start >= 0 && start <= end64;
  if (!ok) {
    if (ln == 0) status[r] = MPC_DRAFT_BAD_RUNS;
    return;
  }
  const int m = (int)m64, n = (int)n64, end = (int)end64;
  const uint8_t* q = seq + q_off;
  const int32_t* rn = runs + run_off;

  // pass 1: what the runs consume, and the outermost '=' runs in alignment order a = n_runs - 1 - k
  int64_t qn = 0, tn = 0;
  bool bad = false;
  int first = -1, last = -1;
  for (int a0 = 0; a0 < n_runs; a0 += 64) {
    const int a = a0 + ln;
    const bool in = a < n_runs;
    const int32_t run = in ? rn[n_runs - 1 - a] : 0;
    const int len = run_len(run), op = run_op(run);
    bad |= in && len < 1;
    if (in && op != kOpI) qn += len;
    if (in && op != kOpD) tn += len;
    const uint64_t eqs = ballot(in && op == kOpEq);
    if (eqs) {
      if (first < 0) first = a0 + __ffsll((unsigned long long)eqs) - 1;
      last = a0 + 63 - __clzll((long long)eqs);
    }
  }
  qn = wave_sum(qn);
  tn = wave_sum(tn);
  if (ballot(bad) != 0 || qn != m || tn != (int64_t)end - start) {
    if (ln == 0) status[r] = MPC_DRAFT_BAD_RUNS;
    return;
  }
  if (ln == 0) status[r] = first < 0 ? MPC_DRAFT_NO_MATCH : MPC_DRAFT_VOTED;
  if (first < 0) return;

  // pass 2: (i, j) of every run, then its adds
  int ci = 0, cj = start;  // the carries: where the chunk's first run begins
  for (int a0 = 0; a0 <= last; a0 += 64) {
    const int a = a0 + ln;
    const bool in = a < n_runs;
    const int32_t run = in ? rn[n_runs - 1 - a] : 0;
    const int len = run_len(run), op = run_op(run);
    const int qa = (in && op != kOpI) ? len : 0, ta = (in && op != kOpD) ? len : 0;
    const int qs = wave_scan_i32(qa), ts = wave_scan_i32(ta);
    const int i = ci + qs - qa, j = cj + ts - ta;
    ci += wave_last_i32(qs);
    cj += wave_last_i32(ts);
    // the lane's own check of what pass 1 established for the whole read
    if (!(in && a >= first && a <= last && len >= 1 && i >= 0 && j >= 0 && (int64_t)j + ta <= n && (int64_t)i + qa <= m)) continue;
    uint32_t* row = tally + (int64_t)j * MPC_DRAFT_ROW;
    if (a == first) add1(row + kStarts);
    if (op == kOpEq) {
      add1(row + kEqOn);
      add1(row + (int64_t)len * MPC_DRAFT_ROW + kEqOff);
      if (a == last) add1(row + (int64_t)len * MPC_DRAFT_ROW + kEnds);
    } else if (op == kOpX) {
      for (int x = 0; x < len; ++x) {
        const uint32_t c = vcode(q[i + x], 4);
        if (c < 4) add1(row + (int64_t)x * MPC_DRAFT_ROW + kSub + c);
      }
    } else if (op == kOpI) {  // an extra target base: a deletion
      add1(row + kDelOn);
      add1(row + (int64_t)len * MPC_DRAFT_ROW + kDelOff);
    } else {  // a read base missing from the target: an insertion in front of column j
      const int k = min(len, MPC_DRAFT_SLOTS);
      for (int s = 0; s < k; ++s) {
        const uint32_t c = vcode(q[i + s], 4);
        if (c < 4) add1(row + kIns + 4 * s + c);
      }
    }
  }
}

// grid: ONE 1024-thread workgroup
__global__ __launch_bounds__(kCallThreads) void K_dcall(const uint32_t* __restrict__ tally, const uint8_t* __restrict__ draft,
                                                        const int n, uint8_t* __restrict__ fresh, const int64_t fresh_cap,
                                                        int32_t* __restrict__ work, int32_t* __restrict__ info) {
  constexpr int NW = kCallThreads / 64;
  __shared__ int32_t s_w[3][NW];  // block_scan's wave totals, then the reductions' (a barrier between any two uses)
  const int tid = (int)threadIdx.x;
  int32_t* cov = work;
  int32_t* eq = work + (n + 1);
  int32_t* del = work + 2 * (int64_t)(n + 1);

  // the three prefix sums (32-bit, wrapping) and the largest coverage
  int c_cov = 0, c_eq = 0, c_del = 0, mx = 0;
  for (int j0 = 0; j0 < n; j0 += kCallThreads) {
    const int j = j0 + tid;
    int v[3] = {0, 0, 0}, inc[3], tot[3];
    if (j < n) {
      const uint32_t* row = tally + (int64_t)j * MPC_DRAFT_ROW;
      v[0] = (int)(row[kStarts] - row[kEnds]);
      v[1] = (int)(row[kEqOn] - row[kEqOff]);
      v[2] = (int)(row[kDelOn] - row[kDelOff]);
    }
    block_scan<NW, 3>(v, inc, tot, s_w);
    if (j < n) {
      cov[j] = c_cov + inc[0]; eq[j] = c_eq + inc[1]; del[j] = c_del + inc[2];
      mx = max(mx, c_cov + inc[0]);
    }
    c_cov += tot[0]; c_eq += tot[1]; c_del += tot[2];
    __syncthreads();  // s_w: the next pass, the maximum below
  }
  mx = wave_max(mx);
  if (lane() == 0) s_w[0][tid >> 6] = mx;
  __syncthreads();
  int maxcov = 0;
  for (int k = 0; k < NW; ++k) maxcov = max(maxcov, s_w[0][k]);
  if (maxcov == 0) {
    if (tid < 8) info[tid] = tid == 0 ? MPC_DRAFT_EMPTY : 0;
    return;
  }

  // the trim: first and last column with 2 cov >= maxcov (each thread reads back what it wrote)
  int lo = n, hi = 0;
  for (int j = tid; j < n; j += kCallThreads)
    if (2 * (int64_t)cov[j] >= maxcov) {
      lo = min(lo, j);
      hi = max(hi, j + 1);
    }
  lo = -wave_max(-lo);
  hi = wave_max(hi);
  __syncthreads();
  if (lane() == 0) { s_w[1][tid >> 6] = lo; s_w[2][tid >> 6] = hi; }
  __syncthreads();
  for (int k = 0; k < NW; ++k) { lo = min(lo, s_w[1][k]); hi = max(hi, s_w[2][k]); }

  // the columns, a tile of 1024 at a time: emitted length, exclusive scan, write
  int at = 0, changed = 0, dropped = 0, inserted = 0;
  for (int j0 = lo; j0 < hi; j0 += kCallThreads) {
    const int j = j0 + tid;
    Emit em{0, 0, -1, false, false};
    if (j < hi) em = call_column(tally + (int64_t)j * MPC_DRAFT_ROW, draft[j], cov[j], eq[j], del[j], j > lo);
    const int cnt = em.n_ins + (em.col >= 0 ? 1 : 0);
    int total;
    __syncthreads();  // s_w: the pass before (the first: lo / hi above share its rows 1, 2 only)
    int64_t p = (int64_t)at + block_scan(cnt, total, s_w[0]) - cnt;
    at += total;
    for (int s = 0; s < em.n_ins; ++s, ++p)
      if (p < fresh_cap) fresh[p] = (uint8_t)(em.ins >> (8 * s));
    if (em.col >= 0 && p < fresh_cap) fresh[p] = (uint8_t)em.col;
    changed += em.changed; dropped += em.dropped; inserted += em.n_ins;
  }
  const int v[3] = {changed, dropped, inserted};
  int inc[3], tot[3];
  __syncthreads();  // s_w: the last pass, lo / hi
  block_scan<NW, 3>(v, inc, tot, s_w);
  if (tid == 0) {
    info[0] = at > MPC_DRAFT_MAX_LEN ? MPC_DRAFT_LONG : MPC_DRAFT_CALLED;
    info[1] = at; info[2] = lo; info[3] = hi; info[4] = maxcov; info[5] = tot[0]; info[6] = tot[1]; info[7] = tot[2];
  }
}

using mpc_launch::hip_fail;
using mpc_launch::read_back;

}  // namespace

extern "C" int mpc_draft_vote(const uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_jobs, int32_t n_jobs,
                              const int32_t* d_out, const int32_t* d_runs, int64_t runs_cap, uint32_t* d_tally, int64_t n,
                              int32_t* d_status, void* stream) {
  const char* fn = "mpc_draft_vote";
  if (n_jobs < 0) return mpc_fail_(MPC_E_ARG, "mpc_draft_vote: n_jobs < 0");
  if (n_jobs == 0) return MPC_OK;
  if (!d_seq || !d_jobs || !d_out || !d_runs || !d_tally || !d_status) return mpc_fail_(MPC_E_ARG, "mpc_draft_vote: null pointer");
  if (const char* bad = vote_sizes_fault(n, seq_bytes, runs_cap)) return mpc_fail_(MPC_E_ARG, (std::string(fn) + ": " + bad).c_str());
  hipStream_t st = (hipStream_t)stream;
  std::vector<int64_t> hj;
  std::vector<int32_t> ho;
  if (const int rc = read_back<int64_t>(st, {{d_jobs, (size_t)n_jobs * 8}}, hj, fn, "job table")) return rc;
  if (const int rc = read_back<int32_t>(st, {{d_out, (size_t)n_jobs * 8}}, ho, fn, "out table")) return rc;
  for (int32_t r = 0; r < n_jobs; ++r)
    if (const char* bad = vote_row_fault(&hj[(size_t)r * 8], &ho[(size_t)r * 8], seq_bytes, runs_cap, n))
      return mpc_fail_(MPC_E_ARG, (std::string(fn) + ": read " + std::to_string(r) + ": " + bad).c_str());
  hipLaunchKernelGGL(K_dvote, dim3((unsigned)n_jobs), dim3(64), 0, st, d_seq, seq_bytes, d_jobs, d_out, d_runs, runs_cap,
                     d_tally, n, d_status);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(fn, "K_dvote", e);
  std::vector<int32_t> hs;
  if (const int rc = read_back<int32_t>(st, {{d_status, (size_t)n_jobs}}, hs, fn, "K_dvote")) return rc;
  for (int32_t r = 0; r < n_jobs; ++r)
    if (hs[(size_t)r] == MPC_DRAFT_BAD_RUNS)
      return mpc_fail_(MPC_DRAFT_E_RUNS, (std::string(fn) + ": read " + std::to_string(r) + ": the runs do not walk the read and its target span").c_str());
  return MPC_OK;
}

extern "C" int mpc_draft_call(const uint32_t* d_tally, const uint8_t* d_draft, int64_t n, uint8_t* d_new, int64_t new_cap,
                              int32_t* d_work, int32_t* d_info, void* stream) {
  const char* fn = "mpc_draft_call";
  if (!d_tally || !d_draft || !d_work || !d_info || (!d_new && new_cap > 0)) return mpc_fail_(MPC_E_ARG, "mpc_draft_call: null pointer");
  if (n < 1 || n > MPC_DRAFT_MAX_LEN || new_cap < 0) return mpc_fail_(MPC_E_ARG, "mpc_draft_call: draft length outside [1, MPC_DRAFT_MAX_LEN]");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(K_dcall, dim3(1), dim3(kCallThreads), 0, st, d_tally, d_draft, (int)n, d_new, new_cap, d_work, d_info);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(fn, "K_dcall", e);
  std::vector<int32_t> hi;
  if (const int rc = read_back<int32_t>(st, {{d_info, 8}}, hi, fn, "K_dcall")) return rc;
  if (hi[0] == MPC_DRAFT_EMPTY) return mpc_fail_(MPC_DRAFT_E_EMPTY, "mpc_draft_call: no read mapped (the largest coverage is 0)");
  if (hi[0] == MPC_DRAFT_LONG)
    return mpc_fail_(MPC_DRAFT_E_LONG, ("mpc_draft_call: the new draft holds " + std::to_string(hi[1]) + " bases (at most 131072 supported)").c_str());
  if (hi[1] > new_cap)
    return mpc_fail_(MPC_E_ARG, ("mpc_draft_call: the buffer holds " + std::to_string(new_cap) + " bytes, the new draft needs " + std::to_string(hi[1])).c_str());
  return MPC_OK;
}
