// mpc_cov.hip -- coverage_qc on gfx950 (include/mpc_coverage.h; DESIGN.md
// "coverage_qc"): K_covparse walks every record's cs tag, K_covfinish turns
// the difference columns into depths and reduces the region statistics.
//
// K_covparse: one wave64 per record, workgroups of 16 waves over a contiguous
// cut of the records.  The cs is taken in tiles of 64 x kCovK bytes (kCovK
// non-temporal byte loads per lane in flight), one 64-byte chunk at a time,
// by the tokenizer K_lnkparse shares (cs_chunk, mpc_cswalk.h): it gives every
// token its p; what a token does to the pileup is CovFx below.  A '-' run that
// crosses a chunk is emitted in pieces; ':' and '*' take effect where they close.
//
// What is written: aligned u deleted of a record is exactly [tstart, final p),
// so the depth column takes ONE +1 / -1 pair per record (its span) and the
// deleted column one pair per deletion piece; K_covfinish computes
// depth = prefix(span) - prefix(deleted).  u32 wraparound keeps that exact.
// Mismatches and insertions are point increments.  All of it goes through a
// workgroup's LDS slice of its sample's rows (the first and the last kCovHalf
// rows: every read of a plasmid starts near 0 and ends near L) and reaches HBM
// once per workgroup and touched word; rows between the halves of a longer
// target, and records of another sample than the workgroup's first, take
// device atomics directly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "mpc.h"
#include "mpc_coverage.h"
#include "mpc_cstables.h"
#include "mpc_cswalk.h"
#include "mpc_device.h"
#include "mpc_launch.h"

namespace {
using namespace mpc;

typedef long long i64;
typedef unsigned long long u64;

constexpr int kCovK = kCsK, kCovTile = kCsTile;  // the tile of the shared walk
constexpr int kCovWaves = 16;
constexpr int kCovThreads = 64 * kCovWaves;
constexpr int kCovHalf = 2048;            // LDS slice: rows [0, kCovHalf) and the last kCovHalf rows
constexpr int kCovSlots = 2 * kCovHalf;   // x 4 columns x 4 bytes = 64 KiB
constexpr int kCovMaxWgs = 256;           // one workgroup per CU
constexpr int kErrSlot = 15;              // stats[0][15]: the status key between the two kernels

// the sample a workgroup's LDS slice stands for
struct Slice {
  uint32_t* tab;
  int32_t sample;
  i64 nrows;
};

__device__ __forceinline__ int slice_slot(i64 r, i64 nrows) {
  if (nrows <= kCovSlots || r < kCovHalf) return (int)r;
  const i64 top = nrows - kCovHalf;
  return r >= top ? (int)(kCovHalf + (r - top)) : -1;
}

// where a record's effects go: rows of its sample, through the slice when it is the slice's sample
struct Sink {
  uint32_t* rows;  // the sample's first row
  uint32_t* tab;   // the slice, or nullptr
  i64 nrows;
  __device__ __forceinline__ void add(uint32_t r, int col, uint32_t delta) const {
    const int sl = tab ? slice_slot(r, nrows) : -1;
    if (sl >= 0) __hip_atomic_fetch_add(&tab[sl * 4 + col], delta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_add(&rows[(i64)r * 4 + col], delta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// per-lane partial counts of ONE record (slots 1-6; a record's cs is shorter than 2^31 bytes)
struct Counts {
  uint32_t match, mism, insev, insb, delev, delb;
};

// what a token does to the pileup (the effects policy of cs_chunk, mpc_cswalk.h)
struct CovFx {
  static constexpr bool kBase = false;
  const Sink& out;
  Counts& t;
  __device__ __forceinline__ void carried_match(uint32_t num) const { if (lane() == 0) t.match += num; }
  __device__ __forceinline__ void carried_sub() const { ++t.mism; }
  __device__ __forceinline__ void carried_sub_at(uint32_t p) const { out.add(p, 2, 1u); }
  __device__ __forceinline__ void count(bool num_close, uint32_t v, bool hit, bool k_del, bool k_ins, int cnt, bool isop) const {
    t.match += num_close ? v : 0u;
    t.mism += hit;
    t.delb += k_del ? (uint32_t)cnt : 0u;
    t.delev += k_del && isop;
    t.insb += k_ins ? (uint32_t)cnt : 0u;
    t.insev += k_ins && isop;
  }
  __device__ __forceinline__ bool look(i64, i64) const { return true; }
  __device__ __forceinline__ void emit(bool hit, bool del_piece, uint32_t pos, uint32_t reach, uint32_t) const {
    out.add(pos, hit ? 2 : del_piece ? 1 : 3, 1u);
    if (del_piece) out.add(reach, 1, ~0u);
  }
};

// grid: workgroups over contiguous cuts of per_wg records; wave w of a workgroup takes every 16th.
// A wave reads the tables of its next 64 records lane-parallel (lane j: record j of them), then
// walks them one by one, the first tile of the next record in flight behind the current one.
__global__ __launch_bounds__(kCovThreads) void K_covparse(
    const uint8_t* __restrict__ cs, const int64_t* __restrict__ cs_off, const int64_t* __restrict__ tstart,
    const int32_t* __restrict__ rec_sample, const i64 n_records, const i64 per_wg,
    const int64_t* __restrict__ pos_off, const int32_t n_samples, uint32_t* __restrict__ rows,
    uint64_t* __restrict__ stats) {
  __shared__ uint32_t tab[kCovSlots * 4];
  __shared__ u64 acc[8];
  const int tid = (int)threadIdx.x, ln = lane(), wave = tid >> 6;
  const uint64_t lemask = (2ull << ln) - 1ull;  // lanes at or below this one
  for (int i = tid; i < kCovSlots * 4; i += kCovThreads) tab[i] = 0;
  if (tid < 8) acc[tid] = 0;

  const i64 r0 = (i64)blockIdx.x * per_wg;
  const i64 r1 = r0 + per_wg < n_records ? r0 + per_wg : n_records;
  Slice sl = {tab, -1, 0};
  i64 sl_base = 0;
  if (r0 < r1) {
    const int32_t s0 = rec_sample[r0];
    if (s0 >= 0 && s0 < n_samples) {
      sl.sample = s0;
      sl_base = pos_off[s0];
      sl.nrows = pos_off[s0 + 1] - sl_base;
    }
  }
  __syncthreads();

  u64 mine[7] = {0, 0, 0, 0, 0, 0, 0};  // slots 0-6 of the slice's sample, per lane (slot 0: lane 0 counts)
  for (i64 rb = r0 + wave; rb < r1; rb += (i64)kCovWaves * 64) {
    const i64 rj = rb + (i64)kCovWaves * ln;
    int32_t m_s = -1, m_len = -1;
    i64 m_a = 0, m_ts = 0, m_base = 0, m_nrows = 0;
    if (rj < r1) {
      m_s = rec_sample[rj];
      m_a = cs_off[rj];
      const i64 len = cs_off[rj + 1] - m_a;
      m_ts = tstart[rj];
      if (m_s >= 0 && m_s < n_samples) {
        m_base = pos_off[m_s];
        m_nrows = pos_off[m_s + 1] - m_base;
      } else m_s = -1;
      if (len >= 0 && len <= INT32_MAX) {
        m_len = (int32_t)len;
        if (len >= 2 && cs[m_a] == 'Z' && cs[m_a + 1] == ':') { m_a += 2; m_len -= 2; }
      }
    }
    const i64 left = (r1 - rb + kCovWaves - 1) / kCovWaves;
    const int count = left < 64 ? (int)left : 64;
    uint32_t nb[kCovK];
    const uint8_t* q = cs + rl64(m_a, 0);
    int len = (int32_t)rl((uint32_t)m_len, 0);
    cs_load_tile(nb, q, len, 0);
    for (int j = 0; j < count; ++j) {
      const i64 r = rb + (i64)kCovWaves * j;
      const int32_t s = (int32_t)rl((uint32_t)m_s, j);
      const i64 ts = rl64(m_ts, j), base = rl64(m_base, j), nrows = rl64(m_nrows, j);
      const uint8_t* const cq = q;
      const int clen = len;
      uint32_t bt[kCovK];
#pragma unroll
      for (int k = 0; k < kCovK; ++k) bt[k] = nb[k];
      if (j + 1 < count) {
        q = cs + rl64(m_a, j + 1);
        len = (int32_t)rl((uint32_t)m_len, j + 1);
        cs_load_tile(nb, q, len, 0);
      }
      if (s < 0) {
        if (ln == 0) cs_report((u64*)&stats[kErrSlot], r, MPC_COV_RANGE);
        continue;
      }
      const uint32_t L = (uint32_t)(nrows - 1);
      Walk w = {ts, 0u, 0, 0, clen < 0, ts < 0 || ts > (i64)L};
      const Sink out = {rows + base * 4, s == sl.sample ? tab : nullptr, nrows};
      Counts t = {0, 0, 0, 0, 0, 0};
      CovFx fx = {out, t};
      for (int t0 = 0; t0 < clen && !w.bad; t0 += kCovTile) {
        if (t0 > 0) cs_load_tile(bt, cq, clen, t0);
#pragma unroll
        for (int k = 0; k < kCovK; ++k) {
          const int cb = t0 + k * 64;
          if (cb < clen && !w.bad) cs_chunk(bt[k], clen - cb < 64 ? clen - cb : 64, cb + 64 >= clen, L, lemask, fx, w);
        }
      }
      if (w.bad || w.oor) {
        if (ln == 0) cs_report((u64*)&stats[kErrSlot], r, w.bad ? MPC_COV_MALFORMED : MPC_COV_RANGE);
        continue;
      }
      if (ln == 0 && w.p > ts) {  // the span: aligned + deleted
        out.add((uint32_t)ts, 0, 1u);
        out.add((uint32_t)w.p, 0, ~0u);
      }
      if (s == sl.sample) {
        mine[0] += ln == 0;
        mine[1] += t.match; mine[2] += t.mism; mine[3] += t.insev; mine[4] += t.insb; mine[5] += t.delev; mine[6] += t.delb;
      } else {
        const u64 v[6] = {wave_sum((u64)t.match), wave_sum((u64)t.mism), wave_sum((u64)t.insev), wave_sum((u64)t.insb),
                          wave_sum((u64)t.delev), wave_sum((u64)t.delb)};
        if (ln == 0) {
          uint64_t* st = stats + (i64)s * MPC_COV_STATS;
          __hip_atomic_fetch_add((u64*)&st[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          for (int k = 0; k < 6; ++k)
            if (v[k]) __hip_atomic_fetch_add((u64*)&st[1 + k], v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }

  for (int k = 0; k < 7; ++k) {
    const u64 v = wave_sum(mine[k]);
    if (ln == 0 && v) __hip_atomic_fetch_add(&acc[k], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  if (sl.sample < 0) return;
  if (tid < 7 && acc[tid])
    __hip_atomic_fetch_add((u64*)&stats[(i64)sl.sample * MPC_COV_STATS + tid], acc[tid], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  // the slice: one device atomic per touched word
  uint32_t* srows = rows + sl_base * 4;
  const bool whole = sl.nrows <= kCovSlots;
  for (int i = tid; i < kCovSlots * 4; i += kCovThreads) {
    const uint32_t v = tab[i];
    if (!v) continue;
    const int slot = i >> 2;
    const i64 r = whole || slot < kCovHalf ? (i64)slot : sl.nrows - kCovHalf + (slot - kCovHalf);
    if (r < sl.nrows) __hip_atomic_fetch_add(&srows[r * 4 + (i & 3)], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// grid: one workgroup per sample.  Prefix-sums the span and deletion differences
// in place into depth and deleted, 1024 rows per step, and reduces slots 7-12
// over the region in the same pass.  Workgroup 0 also decodes the status key.
__global__ __launch_bounds__(kCovThreads) void K_covfinish(
    uint32_t* __restrict__ rows, const int64_t* __restrict__ pos_off, const int64_t* __restrict__ region,
    const uint32_t min_depth, uint64_t* __restrict__ stats, int32_t* __restrict__ status) {
  __shared__ uint32_t wtot[2][kCovWaves];
  __shared__ u64 red[4][kCovWaves];
  __shared__ uint32_t redm[2][kCovWaves];
  const int tid = (int)threadIdx.x, ln = lane(), wave = tid >> 6;
  const i64 s = blockIdx.x;
  const i64 base = pos_off[s], nrows = pos_off[s + 1] - base;
  const i64 lo = region[2 * s], hi = region[2 * s + 1];
  uint32_t carry_sp = 0, carry_dl = 0;
  u64 sum = 0, sq = 0, sdel = 0, nbelow = 0;
  uint32_t mn = UINT32_MAX, mx = 0;
  for (i64 t0 = 0; t0 < nrows; t0 += kCovThreads) {
    const i64 i = t0 + tid;
    const bool in = i < nrows;
    uint32_t* row = rows + (base + (in ? i : 0)) * 4;
    const uint32_t isp = wave_incl_scan<uint32_t>(in ? row[0] : 0u);
    const uint32_t idl = wave_incl_scan<uint32_t>(in ? row[1] : 0u);
    if (ln == 63) { wtot[0][wave] = isp; wtot[1][wave] = idl; }
    __syncthreads();
    uint32_t pre_sp = carry_sp, pre_dl = carry_dl;
#pragma unroll
    for (int k = 0; k < kCovWaves; ++k) {
      const uint32_t x = wtot[0][k], y = wtot[1][k];
      if (k < wave) { pre_sp += x; pre_dl += y; }
      carry_sp += x;
      carry_dl += y;
    }
    const uint32_t del = pre_dl + idl, depth = pre_sp + isp - del;
    if (in) {
      row[0] = depth;
      row[1] = del;
      if (i >= lo && i < hi) {
        sum += depth;
        sq += (u64)depth * depth;
        sdel += del;
        nbelow += depth < min_depth;
        mn = depth < mn ? depth : mn;
        mx = depth > mx ? depth : mx;
      }
    }
    __syncthreads();
  }
  sum = wave_sum(sum); sq = wave_sum(sq); sdel = wave_sum(sdel); nbelow = wave_sum(nbelow);
  mx = wave_max(mx);
  mn = ~wave_max(~mn);
  if (ln == 0) {
    red[0][wave] = sum; red[1][wave] = sq; red[2][wave] = sdel; red[3][wave] = nbelow;
    redm[0][wave] = mn; redm[1][wave] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    u64 a = 0, b = 0, c = 0, d = 0;
    uint32_t m0 = UINT32_MAX, m1 = 0;
    for (int k = 0; k < kCovWaves; ++k) {
      a += red[0][k]; b += red[1][k]; c += red[2][k]; d += red[3][k];
      m0 = redm[0][k] < m0 ? redm[0][k] : m0;
      m1 = redm[1][k] > m1 ? redm[1][k] : m1;
    }
    uint64_t* st = stats + s * MPC_COV_STATS;
    st[7] = a; st[8] = b; st[9] = hi > lo ? m0 : 0; st[10] = m1; st[11] = d; st[12] = c;
    if (s == 0) {
      const u64 key = st[kErrSlot];
      if (key) {
        cs_status(key, status);
        st[kErrSlot] = 0;
      }
    }
  }
}

}  // namespace

extern "C" int mpc_coverage_tile_bytes(void) { return kCovTile; }

extern "C" int mpc_coverage_run(const uint8_t* d_cs, const int64_t* d_cs_off, const int64_t* d_tstart,
                                const int32_t* d_rec_sample, int64_t n_records, const int64_t* d_pos_off,
                                const int64_t* d_region, int32_t n_samples, uint32_t min_depth, uint32_t* d_rows,
                                uint64_t* d_stats, int32_t* d_status, void* stream) {
  using namespace mpc_launch;
  const char* fn = "mpc_coverage_run";
  if (n_records < 0 || n_records > INT32_MAX) return mpc_fail_(MPC_E_ARG, "mpc_coverage_run: n_records outside [0, 2^31)");
  if (n_samples < 1) return mpc_fail_(MPC_E_ARG, "mpc_coverage_run: n_samples < 1");
  if (!d_pos_off || !d_region || !d_rows || !d_stats || !d_status || !d_cs_off ||
      (n_records > 0 && (!d_cs || !d_tstart || !d_rec_sample)))
    return mpc_fail_(MPC_E_ARG, "mpc_coverage_run: null pointer");
  if (((uintptr_t)d_stats & 7) != 0) return mpc_fail_(MPC_E_ARG, "mpc_coverage_run: d_stats is not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t S = (size_t)n_samples;
  std::vector<int64_t> h;
  if (const int rc = read_back<int64_t>(st, {{d_pos_off, S + 1}, {d_region, 2 * S}}, h, fn, "sample tables")) return rc;
  const std::string bad = mpc_host::check_samples(h.data(), h.data() + S + 1, S);
  if (!bad.empty()) return mpc_fail_(MPC_E_ARG, ("mpc_coverage_run: " + bad).c_str());
  const int64_t n_pos = h[S];
  hipError_t e = hipMemsetAsync(d_rows, 0, (size_t)n_pos * 4 * sizeof(uint32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(d_stats, 0, S * MPC_COV_STATS * sizeof(uint64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(d_status, 0, 2 * sizeof(int32_t), st);
  if (e != hipSuccess) return hip_fail(fn, "clearing the outputs", e);
  if (n_records > 0) {
    const RecordGrid g = record_grid(n_records, kCovWaves, kCovMaxWgs);
    hipLaunchKernelGGL(K_covparse, dim3((unsigned)g.wgs), dim3(kCovThreads), 0, st, d_cs, d_cs_off, d_tstart, d_rec_sample,
                       (i64)n_records, (i64)g.per_wg, d_pos_off, n_samples, d_rows, d_stats);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(fn, "K_covparse", e);
  }
  hipLaunchKernelGGL(K_covfinish, dim3((unsigned)n_samples), dim3(kCovThreads), 0, st, d_rows, d_pos_off, d_region,
                     min_depth, d_stats, d_status);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(fn, "K_covfinish", e);
  return MPC_OK;
}
