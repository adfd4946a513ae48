// mpc_align.hip -- the device half of align_reads on gfx950 (include/mpc_align.h;
// DESIGN.md "align_reads").
//
//   K_arevcomp  the reverse complements of a batch's reads, one workgroup per read
//   K_atrace    the band trace of mpc_bandtrace.h (which describes the band, its
//               flag bytes and the traceback), one wave64 per read
//   K_acslen    the handoff to the pileup: what cs, flanks and target start of a
//               traced read measure, one wave64 per read
//   K_acswrite  "Z:" + cs and the upper-cased flanks of a kept read at its place,
//               one wave64 per read
//
// K_atrace keeps ONE row of band values in LDS (W + 1 ints, updated in place:
// row i - 1's column j - 1 is slot b, its column j is slot b + 1).  The lanes
// sit across 64 consecutive slots of the row; the left-move chain
// D[i][b] = min_k<=b x[k] + (b - k) is a DPP prefix maximum of BIAS - (x[k] - k)
// plus one carried value per 64 slots.  Each cell leaves one flag byte (which
// moves reproduce its value) in the read's workspace rows, 64 coalesced bytes
// per store.  The traceback reads those flags back in tiles of 64 rows x 64
// slots staged through LDS (64 independent loads, one wait), not one dependent
// global load per step.  Every index follows from the job's own m, n, d, end,
// which the kernel checks again: a wrong d gives a status, never an access
// outside the read's rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "mpc.h"
#include "mpc_align.h"
#include "mpc_bandtrace.h"
#include "mpc_device.h"
#include "mpc_launch.h"

namespace {
using namespace mpc;
using namespace mpc_band;

constexpr int kInf = 1 << 20;   // above every reachable value (<= 65,536 + 8,193)
constexpr int kBias = 1 << 21;  // keeps BIAS - (x - lane) positive for the max-scan
constexpr int kTile = 64;       // traceback tile: 64 rows x 64 slots

// grid: one 256-thread workgroup per read
__global__ __launch_bounds__(256) void K_arevcomp(uint8_t* __restrict__ seq, const int64_t seq_bytes,
                                                  const int64_t* __restrict__ tab) {
  const int64_t r = blockIdx.x;
  const int64_t src = tab[3 * r], len = tab[3 * r + 1], dst = tab[3 * r + 2];
  // restates the bounds of check_revcomp (mpc_bandtrace.h), which the host applies before the launch
  if (len < 0 || src < 0 || dst < 0 || src > seq_bytes - len || dst > seq_bytes - len) return;
  for (int64_t x = threadIdx.x; x < len; x += 256) seq[dst + x] = (uint8_t)complement(seq[src + len - 1 - x]);
}

// One wave per workgroup: its LDS accesses execute in program order, so lanes
// that read what other lanes wrote need no barrier, only that the compiler
// keeps the order -- and no wait for the flag stores still in flight, which a
// __syncthreads() would add to every 64 cells.
__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// grid: one 64-thread workgroup per read; dynamic LDS: the flag tile, row_cap ints, row_cap + 64 target codes
__global__ __launch_bounds__(64) void K_atrace(const uint8_t* __restrict__ seq, const int64_t seq_bytes,
                                               const int64_t* __restrict__ jobs, uint8_t* __restrict__ flags,
                                               const int64_t flags_bytes, int32_t* __restrict__ out,
                                               int32_t* __restrict__ runs, const int64_t runs_cap, const int32_t row_cap) {
  extern __shared__ int32_t lds[];
  uint8_t* tile = (uint8_t*)lds;            // kTile x 64 bytes
  int32_t* row = lds + kTile * 64 / 4;      // W + 1 ints
  uint8_t* tw = (uint8_t*)(row + row_cap);  // W + 63 target codes
  const int ln = lane();
  const int64_t r = blockIdx.x;
  const int64_t* jb = jobs + 8 * r;
  const int64_t q_off = jb[0], m64 = jb[1], t_off = jb[2], n64 = jb[3], d64 = jb[4], end64 = jb[5], flag_off = jb[6],
                run_off = jb[7];
  int32_t* o = out + 8 * r;
  // restates check_job and check_job_flags (flag_next 0) of mpc_bandtrace.h, which the host applies before
  // the launch, and adds the row_cap the launch was sized by
  bool ok = m64 >= 1 && m64 <= MPC_VERIFY_MAX_QUERY && n64 >= 1 && n64 <= INT32_MAX && d64 >= 0 &&
            d64 <= MPC_ALIGN_MAX_EDITS && end64 >= 0 && end64 <= n64;
  ok = ok && q_off >= 0 && q_off <= seq_bytes - m64 && t_off >= 0 && t_off <= seq_bytes - n64;
  ok = ok && 2 * d64 + 2 <= row_cap && run_off >= 0 && run_off <= runs_cap - (2 * d64 + 1);
  ok = ok && flag_off >= 0 && flag_off <= flags_bytes - m64 * row_pitch(d64);
  if (!ok) {
    if (ln < 8) o[ln] = ln == 0 ? MPC_ALIGN_BAD_JOB : 0;
    return;
  }
  const int m = (int)m64, n = (int)n64, d = (int)d64, end = (int)end64;
  const int W = 2 * d + 1, P = (int)row_pitch(d), d0 = end - m;
  const uint8_t* q = seq + q_off;
  const uint8_t* t = seq + t_off;
  uint8_t* F = flags + flag_off;  // row i at (i - 1) * P
  int32_t* rn = runs + run_off;

  for (int b = ln; b <= W; b += 64) {
    const int j = d0 - d + b;
    row[b] = (b < W && j >= 0 && j <= n) ? 0 : kInf;  // D[0][j] = 0; slot W stays infinite
  }

  for (int i0 = 1; i0 <= m; i0 += 64) {
    // 64 rows at a time: their query codes in one register, the W + 63 target codes they meet in LDS
    lds_fence();  // the previous rows no longer read tw
    const int tb = i0 + d0 - d - 1;  // target index of row i0's slot 0
    for (int x = ln; x < W + 63; x += 64) {
      const int jj = tb + x;
      tw[x] = (jj >= 0 && jj < n) ? (uint8_t)vcode(t[jj], 5) : (uint8_t)5;
    }
    const int qr = i0 - 1 + ln;
    const uint32_t qv = qr < m ? vcode(q[qr], 4) : 4;
    lds_fence();
    const int i1 = min(m, i0 + 63);
    for (int i = i0; i <= i1; ++i) {
      const uint32_t qi = (uint32_t)__builtin_amdgcn_readlane((int)qv, i - i0);
      const int jbase = i + d0 - d;
      uint8_t* f = F + (int64_t)(i - 1) * P;
      int carry = kInf;  // D[i][.] at the slot left of this chunk
      for (int c0 = 0; c0 < W; c0 += 64) {
        const int b = c0 + ln, j = jbase + b;
        const bool in = b < W && j >= 0 && j <= n;
        int x = kInf, dg = kInf, up = kInf;
        bool eq = false;
        if (in) {
          up = row[b + 1] + 1;
          if (j == 0) {
            x = i;  // D[i][0] = i
          } else {
            eq = qi == tw[i - i0 + b];
            dg = row[b] + (eq ? 0 : 1);
            x = min(dg, up);
          }
        }
        // left moves inside the chunk, then the one entering it
        const int pm = wave_scan_max_i32(kBias - (x - ln));
        int v = min(ln + kBias - pm, carry + 1 + ln);
        uint32_t fl = 0;
        if (in) {
          if (j == 0) fl = kUp;
          else fl = (dg == v ? kDiag : 0u) | (up == v ? kUp : 0u) | (eq ? kMatch : 0u);
        }
        v = in ? min(v, kInf) : kInf;
        carry = __builtin_amdgcn_readlane(v, 63);
        lds_fence();  // every lane has read row[b], row[b + 1]
        if (b < W) row[b] = v;
        f[b] = (uint8_t)fl;  // b < P: the pad holds 0; not waited for
        lds_fence();
      }
    }
  }
  __syncthreads();  // the flag stores are done before the tiles read them back

  if (uniform_i32(row[d]) != d) {  // (m, end) sits on diagonal d0: slot d
    if (ln < 8) o[ln] = ln == 0 ? MPC_ALIGN_BAD_SCAN : 0;
    return;
  }

  int i = m, j = end, op = -1, len = 0, n_runs = 0;
  int c_eq = 0, c_x = 0, c_i = 0, c_d = 0;
  bool bad = false;
  while (i > 0 && !bad) {
    const int b = j - i - d0 + d;
    if (b < 0 || b >= W) { bad = true; break; }
    const int ws = min(max(b - 32, 0), P - 64), i0 = i;
    __syncthreads();  // the previous tile is no longer read
#pragma unroll 8
    for (int k = 0; k < kTile; ++k) {
      const int rr = i0 - k;
      if (rr >= 1) tile[k * 64 + ln] = F[(int64_t)(rr - 1) * P + ws + ln];
    }
    __syncthreads();
    while (i > 0 && i > i0 - kTile) {
      const int bb = j - i - d0 + d - ws;
      if (bb < 0 || bb >= 64 || bb + ws >= W) break;  // next tile (or, outside the band, the check above)
      const uint32_t fl = (uint32_t)uniform_i32(tile[(i0 - i) * 64 + bb]);  // (every lane walks the same path)
      int now;
      if (j > 0 && (fl & kDiag)) {
        now = (fl & kMatch) ? kOpEq : kOpX;
        --i; --j;
      } else if (fl & kUp) {
        now = kOpD;
        --i;
      } else if (j > 0) {
        now = kOpI;
        --j;
      } else {
        bad = true;
        break;
      }
      if (now != op) {
        if (len > 0) {
          if (n_runs < W) { if (ln == 0) rn[n_runs] = pack_run(len, op); }
          else bad = true;
          ++n_runs;
        }
        op = now;
        len = 0;
      }
      ++len;
      c_eq += now == kOpEq; c_x += now == kOpX; c_i += now == kOpI; c_d += now == kOpD;
    }
  }
  if (len > 0) {
    if (n_runs < W) { if (ln == 0) rn[n_runs] = pack_run(len, op); }
    else bad = true;
    ++n_runs;
  }
  if (bad) {
    if (ln < 8) o[ln] = ln == 0 ? MPC_ALIGN_BAD_SCAN : 0;
    return;
  }
  if (ln == 0) {
    o[0] = MPC_ALIGN_OK; o[1] = j; o[2] = c_eq; o[3] = c_x; o[4] = c_i; o[5] = c_d; o[6] = n_runs; o[7] = 0;
  }
}

// ---- the handoff to the pileup (include/mpc_align.h) ----------------------------
// What a wave learns of one traced read before anything is sized or written:
// the job and the out row checked again, the end rule and the sums of the kept
// span.  The lanes sit across 64 runs at a time (traceback order); a ballot
// finds the first and the last '=' of a chunk, and DPP prefix sums of what each
// run moves and writes (run_read_bases, run_target_bases, run_cs_bytes of
// mpc_bandtrace.h) give the sums before the first '=' (the dropped trailing
// ops), behind the last one (the dropped leading ops) and over everything.  A
// run of a checked trace is at most MPC_VERIFY_MAX_QUERY long (m <= 65,536,
// deletions <= d), so every sum of at most 2 d + 1 = 8,193 runs fits 31 bits.
struct CsMeasure {
  int ok, kept, first, last;  // ok 0: the job, the out row or the runs are refused
  int m, n, cs_len, up_len, down_len, tstart, tend, n_eq, n_ops;
  int64_t q_off, t_off, run_off;
};

__device__ __forceinline__ CsMeasure cs_measure(const int64_t* __restrict__ jb, const int32_t* __restrict__ o,
                                                const int32_t* __restrict__ runs, const int64_t runs_cap,
                                                const int64_t seq_bytes) {
  const int ln = lane();
  CsMeasure M = {};
  const int64_t q_off = jb[0], m64 = jb[1], t_off = jb[2], n64 = jb[3], d64 = jb[4], end64 = jb[5], run_off = jb[7];
  // restates check_job and check_traced of mpc_bandtrace.h, which the host applies before the launch
  bool ok = m64 >= 1 && m64 <= MPC_VERIFY_MAX_QUERY && n64 >= 1 && n64 <= INT32_MAX && d64 >= 0 &&
            d64 <= MPC_ALIGN_MAX_EDITS && end64 >= 0 && end64 <= n64;
  ok = ok && q_off >= 0 && q_off <= seq_bytes - m64 && t_off >= 0 && t_off <= seq_bytes - n64;
  ok = ok && run_off >= 0 && run_off <= runs_cap - (2 * d64 + 1);
  const int status = o[0], start = o[1], n_runs = o[6];
  ok = ok && status == MPC_ALIGN_OK && n_runs >= 0 && n_runs <= 2 * d64 + 1 && start >= 0 && start <= end64;
  if (!ok) return M;
  const int32_t* rn = runs + run_off;
  int all_q = 0, all_t = 0, all_b = 0, all_l = 0;  // every run
  int bef_q = 0, bef_t = 0, bef_b = 0, bef_l = 0;  // the runs before the first '='
  int beh_q = 0, beh_t = 0, beh_b = 0, beh_l = 0;  // the runs behind the last '=' so far
  int n_eq = 0, first = 0, last = -1;
  bool found = false, bad = false;
  for (int c0 = 0; c0 < n_runs; c0 += 64) {
    const int k = c0 + ln;
    const bool valid = k < n_runs;
    const int32_t run = valid ? rn[k] : 0;
    const bool fits = run_len(run) >= 1 && run_len(run) <= MPC_VERIFY_MAX_QUERY;
    bad = bad || ballot(valid && !fits) != 0;
    const bool use = valid && fits;
    const int vq = use ? (int)run_read_bases(run) : 0, vt = use ? (int)run_target_bases(run) : 0;
    const int vb = use ? (int)run_cs_bytes(run) : 0, vl = use ? run_len(run) : 0;
    const bool eq = use && run_op(run) == kOpEq;
    const uint64_t em = ballot(eq);
    const int sq = wave_scan_i32(vq), st = wave_scan_i32(vt), sb = wave_scan_i32(vb), sl = wave_scan_i32(vl);
    const int tq = wave_last_i32(sq), tt = wave_last_i32(st), tb = wave_last_i32(sb), tl = wave_last_i32(sl);
    n_eq += wave_sum(eq ? vl : 0);
    if (em != 0) {
      const int f = __ffsll((unsigned long long)em) - 1, l = 63 - __clzll((long long)em);
      if (!found) {  // exclusive sums at lane f
        bef_q += __shfl(sq - vq, f, 64); bef_t += __shfl(st - vt, f, 64);
        bef_b += __shfl(sb - vb, f, 64); bef_l += __shfl(sl - vl, f, 64);
        first = c0 + f;
        found = true;
      }
      last = c0 + l;
      beh_q = tq - __shfl(sq, l, 64); beh_t = tt - __shfl(st, l, 64);
      beh_b = tb - __shfl(sb, l, 64); beh_l = tl - __shfl(sl, l, 64);
    } else if (!found) {
      bef_q += tq; bef_t += tt; bef_b += tb; bef_l += tl;
    } else {
      beh_q += tq; beh_t += tt; beh_b += tb; beh_l += tl;
    }
    all_q += tq; all_t += tt; all_b += tb; all_l += tl;
  }
  // the runs walk exactly the read and the target span (check_walk)
  if (bad || all_q != (int)m64 || all_t != (int)end64 - start) return M;
  M.ok = 1;
  M.m = (int)m64; M.n = (int)n64; M.q_off = q_off; M.t_off = t_off; M.run_off = run_off;
  if (!found) return M;
  M.kept = 1; M.first = first; M.last = last;
  M.cs_len = 2 + all_b - bef_b - beh_b;
  M.up_len = beh_q; M.down_len = bef_q;
  M.tstart = start + beh_t; M.tend = (int)end64 - bef_t;
  M.n_eq = n_eq; M.n_ops = all_l - bef_l - beh_l;
  return M;
}

// lane k < 8 holds column k of the read's size row
__device__ __forceinline__ int64_t size_column(const CsMeasure& M, int k) {
  const int v[8] = {M.kept, M.cs_len, M.up_len, M.down_len, M.tstart, M.tend, M.n_eq, M.n_ops};
  int x = v[0];
#pragma unroll
  for (int c = 1; c < 8; ++c) x = k == c ? v[c] : x;
  return x;
}

// grid: one 64-thread workgroup per read
__global__ __launch_bounds__(64) void K_acslen(const int64_t* __restrict__ jobs, const int64_t seq_bytes,
                                               const int32_t* __restrict__ out, const int32_t* __restrict__ runs,
                                               const int64_t runs_cap, int64_t* __restrict__ sizes) {
  const int64_t r = blockIdx.x;
  const CsMeasure M = cs_measure(jobs + 8 * r, out + 8 * r, runs, runs_cap, seq_bytes);
  const int ln = lane();
  if (ln < 8) sizes[8 * r + ln] = M.ok ? size_column(M, ln) : (ln == 0 ? -1 : 0);
}

// grid: one 64-thread workgroup per read.  The wave measures the read again,
// and writes only when that gives the size row it was handed and the place
// holds it.  Then it walks the kept runs forward (last -> first), one lane per
// run: the prefix sums of (cs bytes, read bases, target bases), carried from
// chunk to chunk, give each run its byte offset and its (i, j); the lane writes
// its run's bytes (put_run_cs), plain byte stores; the flanks are copied by the
// whole wave, 64 bytes at a time.
__global__ __launch_bounds__(64) void K_acswrite(const uint8_t* __restrict__ seq, const int64_t seq_bytes,
                                                 const int64_t* __restrict__ jobs, const int32_t* __restrict__ out,
                                                 const int32_t* __restrict__ runs, const int64_t runs_cap,
                                                 const int64_t* __restrict__ sizes, const int64_t* __restrict__ place,
                                                 uint8_t* __restrict__ cs, const int64_t cs_bytes,
                                                 uint8_t* __restrict__ up, const int64_t up_bytes,
                                                 uint8_t* __restrict__ down, const int64_t down_bytes,
                                                 int32_t* __restrict__ status) {
  const int64_t r = blockIdx.x;
  const int ln = lane();
  const CsMeasure M = cs_measure(jobs + 8 * r, out + 8 * r, runs, runs_cap, seq_bytes);
  const int64_t* z = sizes + 8 * r;
  const int64_t cs_off = place[3 * r], up_off = place[3 * r + 1], down_off = place[3 * r + 2];
  bool agree = M.ok != 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) agree = agree && z[c] == size_column(M, c);
  // restates the bounds of check_place (mpc_bandtrace.h)
  if (agree && M.kept)
    agree = cs_off >= 0 && cs_off <= cs_bytes - M.cs_len && up_off >= 0 && up_off <= up_bytes - M.up_len &&
            down_off >= 0 && down_off <= down_bytes - M.down_len && M.up_len <= M.m - M.down_len;
  if (ln == 0) status[r] = agree ? MPC_ALIGN_OK : MPC_ALIGN_BAD_JOB;
  if (!agree || !M.kept) return;
  const uint8_t* q = seq + M.q_off;
  const uint8_t* t = seq + M.t_off;
  const int32_t* rn = runs + M.run_off;
  uint8_t* dst = cs + cs_off;
  if (ln == 0) { dst[0] = 'Z'; dst[1] = ':'; }
  int bo = 2, qi = M.up_len, tj = M.tstart;
  const int total = M.last - M.first + 1;
  for (int p0 = 0; p0 < total; p0 += 64) {
    const int pos = p0 + ln;
    const bool valid = pos < total;
    const int32_t run = valid ? rn[M.last - pos] : 0;
    const int vb = valid ? (int)run_cs_bytes(run) : 0, vq = valid ? (int)run_read_bases(run) : 0,
              vt = valid ? (int)run_target_bases(run) : 0;
    const int sb = wave_scan_i32(vb), sq = wave_scan_i32(vq), st = wave_scan_i32(vt);
    const int at = bo + sb - vb, i = qi + sq - vq, j = tj + st - vt;
    // what the lane indexes, checked again: its bytes inside the read's slot, its bases inside the read and the target
    if (valid && at >= 2 && at + vb <= M.cs_len && i >= 0 && i + vq <= M.m && j >= 0 && j + vt <= M.n)
      put_run_cs(dst + at, run, q, i, t, j);
    bo += wave_last_i32(sb); qi += wave_last_i32(sq); tj += wave_last_i32(st);
  }
  for (int x = ln; x < M.up_len; x += 64) up[up_off + x] = upper_ascii(q[x]);
  const uint8_t* tail = q + (M.m - M.down_len);
  for (int x = ln; x < M.down_len; x += 64) down[down_off + x] = upper_ascii(tail[x]);
}

using mpc_launch::hip_fail;
using mpc_launch::read_back;

// "<fn>: read r: <why>" as MPC_E_ARG
int refuse_read(const char* fn, int32_t r, const char* why) {
  return mpc_fail_(MPC_E_ARG, (std::string(fn) + ": read " + std::to_string(r) + ": " + why).c_str());
}

}  // namespace

extern "C" int mpc_align_revcomp(uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_tab, int32_t n_reads, void* stream) {
  if (n_reads < 0) return mpc_fail_(MPC_E_ARG, "mpc_align_revcomp: n_reads < 0");
  if (n_reads == 0) return MPC_OK;
  if (!d_seq || !d_tab || seq_bytes < 0) return mpc_fail_(MPC_E_ARG, "mpc_align_revcomp: null pointer");
  hipStream_t st = (hipStream_t)stream;
  std::vector<int64_t> h;
  if (const int rc = read_back<int64_t>(st, {{d_tab, (size_t)n_reads * 3}}, h, "mpc_align_revcomp", "read table")) return rc;
  for (int32_t r = 0; r < n_reads; ++r)
    if (const int bad = check_revcomp(&h[(size_t)r * 3], seq_bytes))
      return mpc_fail_(MPC_E_ARG, ("mpc_align_revcomp: read " + std::to_string(r) + ": " + fault_text(bad)).c_str());
  hipLaunchKernelGGL(K_arevcomp, dim3((unsigned)n_reads), dim3(256), 0, st, d_seq, seq_bytes, d_tab);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("mpc_align_revcomp", "K_arevcomp", e);
  return MPC_OK;
}

extern "C" int mpc_align_trace(const uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_jobs, int32_t n_jobs,
                               uint8_t* d_flags, int64_t flags_bytes, int32_t* d_out, int32_t* d_runs, int64_t runs_cap,
                               void* stream) {
  if (n_jobs < 0) return mpc_fail_(MPC_E_ARG, "mpc_align_trace: n_jobs < 0");
  if (n_jobs == 0) return MPC_OK;
  if (!d_seq || !d_jobs || !d_flags || !d_out || !d_runs || seq_bytes < 0 || flags_bytes < 0 || runs_cap < 0)
    return mpc_fail_(MPC_E_ARG, "mpc_align_trace: null pointer or negative size");
  hipStream_t st = (hipStream_t)stream;
  const char* fn = "mpc_align_trace";
  std::vector<int64_t> h;
  if (const int rc = read_back<int64_t>(st, {{d_jobs, (size_t)n_jobs * 8}}, h, fn, "job table")) return rc;
  int64_t flag_next = 0, d_max = 0;
  for (int32_t r = 0; r < n_jobs; ++r) {
    const int64_t* j = &h[(size_t)r * 8];
    int bad = check_job(j, seq_bytes, runs_cap);
    if (!bad) bad = check_job_flags(j, flags_bytes, flag_next);
    if (bad) return mpc_fail_(MPC_E_ARG, ("mpc_align_trace: read " + std::to_string(r) + ": " + fault_text(bad)).c_str());
    flag_next = j[6] + j[1] * row_pitch(j[4]);
    d_max = j[4] > d_max ? j[4] : d_max;
  }
  const int32_t row_cap = (int32_t)((2 * d_max + 2 + 63) / 64 * 64);
  const size_t lds_bytes = (size_t)kTile * 64 + (size_t)row_cap * sizeof(int32_t) + (size_t)row_cap + 64;
  hipLaunchKernelGGL(K_atrace, dim3((unsigned)n_jobs), dim3(64), lds_bytes, st, d_seq, seq_bytes, d_jobs, d_flags,
                     flags_bytes, d_out, d_runs, runs_cap, row_cap);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(fn, "K_atrace", e);
  std::vector<int32_t> ho;
  if (const int rc = read_back<int32_t>(st, {{d_out, (size_t)n_jobs * 8}}, ho, fn, "K_atrace")) return rc;
  for (int32_t r = 0; r < n_jobs; ++r)
    if (ho[(size_t)r * 8] != MPC_ALIGN_OK)
      return mpc_fail_(MPC_ALIGN_E_SCAN, ("mpc_align_trace: read " + std::to_string(r) + ": status " +
                                          std::to_string(ho[(size_t)r * 8]) + ": the band does not give the scan's distance at (m, end)").c_str());
  return MPC_OK;
}

extern "C" int mpc_align_cs_sizes(const int64_t* d_jobs, int32_t n_jobs, int64_t seq_bytes, const int32_t* d_out,
                                  const int32_t* d_runs, int64_t runs_cap, int64_t* d_sizes, void* stream) {
  const char* fn = "mpc_align_cs_sizes";
  if (n_jobs < 0) return mpc_fail_(MPC_E_ARG, "mpc_align_cs_sizes: n_jobs < 0");
  if (n_jobs == 0) return MPC_OK;
  if (!d_jobs || !d_out || !d_runs || !d_sizes || seq_bytes < 0 || runs_cap < 0)
    return mpc_fail_(MPC_E_ARG, "mpc_align_cs_sizes: null pointer or negative size");
  hipStream_t st = (hipStream_t)stream;
  std::vector<int64_t> h;
  std::vector<int32_t> ho;
  if (const int rc = read_back<int64_t>(st, {{d_jobs, (size_t)n_jobs * 8}}, h, fn, "job table")) return rc;
  if (const int rc = read_back<int32_t>(st, {{d_out, (size_t)n_jobs * 8}}, ho, fn, "trace output")) return rc;
  for (int32_t r = 0; r < n_jobs; ++r) {
    int bad = check_job(&h[(size_t)r * 8], seq_bytes, runs_cap);
    if (!bad) bad = check_traced(&h[(size_t)r * 8], &ho[(size_t)r * 8]);
    if (bad) return refuse_read(fn, r, fault_text(bad));
  }
  hipLaunchKernelGGL(K_acslen, dim3((unsigned)n_jobs), dim3(64), 0, st, d_jobs, seq_bytes, d_out, d_runs, runs_cap, d_sizes);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(fn, "K_acslen", e);
  if (const int rc = read_back<int64_t>(st, {{d_sizes, (size_t)n_jobs * 8}}, h, fn, "K_acslen")) return rc;
  for (int32_t r = 0; r < n_jobs; ++r)
    if (h[(size_t)r * 8] < 0) return refuse_read(fn, r, fault_text(kWalk));
  return MPC_OK;
}

extern "C" int mpc_align_cs_write(const uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_jobs, int32_t n_jobs,
                                  const int32_t* d_out, const int32_t* d_runs, int64_t runs_cap, const int64_t* d_sizes,
                                  const int64_t* d_place, uint8_t* d_cs, int64_t cs_bytes, uint8_t* d_up, int64_t up_bytes,
                                  uint8_t* d_down, int64_t down_bytes, int32_t* d_status, void* stream) {
  const char* fn = "mpc_align_cs_write";
  if (n_jobs < 0) return mpc_fail_(MPC_E_ARG, "mpc_align_cs_write: n_jobs < 0");
  if (n_jobs == 0) return MPC_OK;
  if (!d_seq || !d_jobs || !d_out || !d_runs || !d_sizes || !d_place || !d_status || seq_bytes < 0 || runs_cap < 0 ||
      cs_bytes < 0 || up_bytes < 0 || down_bytes < 0 || (!d_cs && cs_bytes > 0) || (!d_up && up_bytes > 0) ||
      (!d_down && down_bytes > 0))
    return mpc_fail_(MPC_E_ARG, "mpc_align_cs_write: null pointer or negative size");
  hipStream_t st = (hipStream_t)stream;
  std::vector<int64_t> h;
  std::vector<int32_t> ho;
  const size_t J = (size_t)n_jobs;
  if (const int rc = read_back<int64_t>(st, {{d_jobs, J * 8}, {d_sizes, J * 8}, {d_place, J * 3}}, h, fn, "tables")) return rc;
  if (const int rc = read_back<int32_t>(st, {{d_out, J * 8}}, ho, fn, "trace output")) return rc;
  const int64_t cap[3] = {cs_bytes, up_bytes, down_bytes};
  int64_t at[3] = {0, 0, 0};
  for (int32_t r = 0; r < n_jobs; ++r) {
    const int64_t* j = &h[(size_t)r * 8];
    int bad = check_job(j, seq_bytes, runs_cap);
    if (!bad) bad = check_traced(j, &ho[(size_t)r * 8]);
    if (!bad) bad = check_place(j, &h[J * 8 + (size_t)r * 8], &h[J * 16 + (size_t)r * 3], cap, at);
    if (bad) return refuse_read(fn, r, fault_text(bad));
  }
  hipLaunchKernelGGL(K_acswrite, dim3((unsigned)n_jobs), dim3(64), 0, st, d_seq, seq_bytes, d_jobs, d_out, d_runs, runs_cap,
                     d_sizes, d_place, d_cs, cs_bytes, d_up, up_bytes, d_down, down_bytes, d_status);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(fn, "K_acswrite", e);
  if (const int rc = read_back<int32_t>(st, {{d_status, J}}, ho, fn, "K_acswrite")) return rc;
  for (int32_t r = 0; r < n_jobs; ++r)
    if (ho[(size_t)r] != MPC_ALIGN_OK) return refuse_read(fn, r, fault_text(kSizes));
  return MPC_OK;
}
