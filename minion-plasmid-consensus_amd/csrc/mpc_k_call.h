// The consensus phase (mpc_consensus; Steps 5-6, :332-439): K_call is the
// per-slot top / second / tie / N rule (:363-439) with the samples' max depth,
// K_select the threshold test and the ordered compaction of the calls.
#pragma once

#include "mpc_k_common.h"

namespace {

__device__ __forceinline__ int sample_of_row(const Dev& d, int64_t row) {
  int lo = 0, hi = d.S - 1;  // last sample whose first row <= row
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d.srow[mid] <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// first row of every sample in LDS (kSmpLds samples; beyond that the global search)
constexpr int kSmpLds = 512;
__device__ __forceinline__ void load_sample_rows(const Dev& d, int32_t* srow) {
  for (int s = threadIdx.x; s < d.S && s < kSmpLds; s += blockDim.x) srow[s] = d.srow[s];
}
__device__ __forceinline__ int sample_of_row_lds(const Dev& d, const int32_t* srow, int64_t row) {
  if (d.S > kSmpLds) return sample_of_row(d, row);
  int lo = 0, hi = d.S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (srow[mid] <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// rows per thread of K_call: 1 while the grid is small (the kernel is
// latency-bound: more blocks), kCRBig for large pileups, where every block's
// max-depth atomic on the few maxdepth words serializes (C5: 5.7k blocks)
constexpr int kCRBig = 8;
constexpr int64_t kCallBlocksMax = 512;  // (the 70 kb parity case takes the kCRBig path)

// per slot: sorted(tuples in dict order, key=count)[::-1] -> top / second / tie -> N (:363-423).
// The stable descending sort of the reverse-dict-ordered (base, count) list
// is a descending sort of the keys count << 2 | dict index; bases with count
// 0 are not in the list (they sort last, and no positive count ties them).
// Branch-free: a 5-exchange sorting network (no register-indexed arrays: the
// insertion sort put them in scratch, K_call<8> spilled 18 VGPRs).
__device__ __forceinline__ uint4 call_slot(uint4 cv, double gtf, uint32_t* total_out) {
  const uint32_t total = cv.x + cv.y + cv.z + cv.w;  // A, T, C, G
  *total_out = total;
  if (total == 0) return make_uint4(0, 0, 0, 0);
  uint64_t k0 = ((uint64_t)cv.x << 2) | 0u, k1 = ((uint64_t)cv.y << 2) | 1u;
  uint64_t k2 = ((uint64_t)cv.z << 2) | 2u, k3 = ((uint64_t)cv.w << 2) | 3u;
  auto cx = [](uint64_t& a, uint64_t& b) {  // a >= b after
    const uint64_t hi = a > b ? a : b, lo = a > b ? b : a;
    a = hi; b = lo;
  };
  cx(k0, k1); cx(k2, k3); cx(k0, k2); cx(k1, k3); cx(k1, k2);
  const uint32_t c0 = (uint32_t)(k0 >> 2), c1 = (uint32_t)(k1 >> 2), c2 = (uint32_t)(k2 >> 2), c3 = (uint32_t)(k3 >> 2);
  // 'A' 'T' 'C' 'G' by dict index
  auto name = [](uint64_t k) -> uint32_t { return (0x47435441u >> (8 * (uint32_t)(k & 3u))) & 0xffu; };
  const uint32_t m = (c0 > 0) + (c1 > 0) + (c2 > 0) + (c3 > 0);  // c0 > 0 (total > 0)
  // ties of the first / second count (every tied count is positive: c0 > 0, and c1 is tested only when m >= 2)
  const uint32_t tie0 = c0 * (1u + (c1 == c0) + (c2 == c0) + (c3 == c0));
  const uint32_t tie1 = c1 * ((c0 == c1) + 1u + (c2 == c1) + (c3 == c1));
  const bool one = m == 1 || c0 > c1;
  uint32_t base = one ? name(k0) : 'N';
  const uint32_t count = one ? c0 : tie0;
  const bool two = m == 2 || c1 > c2;
  const uint32_t base2 = m <= 1 ? 'X' : (two ? name(k1) : 'N');
  const uint32_t count2 = m <= 1 ? 0u : (two ? c1 : tie1);
  const uint32_t chrom1 = base;
  if ((double)count < gtf * (double)count2) base = 'N';   // :421
  return make_uint4(base | (chrom1 << 8) | (base2 << 16) | (1u << 24), count, count2, total);
}

// calls of every row + max depth over slot 0 (:332-341); rows t + 256 k of the block
template <int kCR>  // (kCR rows in flight per thread: up to 128 VGPRs, no spills)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kCR > 1 ? 4 : 8))) void K_call(Dev d, int64_t R) {
  constexpr int kCB = 256 * kCR;  // rows per block
  __shared__ int32_t srow[kSmpLds];
  __shared__ int32_t s_blk[2], s_w[4];
  const bool cap = (d.status[MPC_ST_FLAGS] & DE_CAP) != 0;
  const int64_t need0 = cap ? 0 : (int64_t)d.status[MPC_ST_ROWS_NEEDED];
  const int64_t need = need0 < R ? need0 : R;
  load_sample_rows(d, srow);
  const int64_t b0 = (int64_t)blockIdx.x * kCB;
  __syncthreads();
  if (threadIdx.x < 2) {
    const int64_t rr = threadIdx.x == 0 ? b0 : (b0 + kCB < need ? b0 + kCB : need) - 1;
    s_blk[threadIdx.x] = rr >= 0 ? sample_of_row_lds(d, srow, rr) : 0;
  }
  uint4 cv[kCR];
  uint8_t mt[kCR];
#pragma unroll
  for (int k = 0; k < kCR; ++k) {  // all loads first (in bounds: rows < R), in parallel with the status word
    const int64_t row = b0 + threadIdx.x + 256 * k;
    cv[k] = row < R ? reinterpret_cast<const uint4*>(d.rows)[row] : make_uint4(0, 0, 0, 0);
    mt[k] = row < R ? d.meta[row] : 0;
  }
#pragma unroll
  for (int k = 0; k < kCR; ++k)
    if (b0 + threadIdx.x + 256 * k >= need) { cv[k] = make_uint4(0, 0, 0, 0); mt[k] = 0; }
  __syncthreads();
  int32_t dep[kCR];  // slot-0 depth of the row (:336), -1: none
#pragma unroll
  for (int k = 0; k < kCR; ++k) {
    const int64_t row = b0 + threadIdx.x + 256 * k;
    uint32_t total = 0;
    const uint4 out = call_slot(cv[k], d.gtf, &total);
    if (row < R) reinterpret_cast<uint4*>(d.res)[row] = out;
    dep[k] = (total > 0 && (mt[k] & 2u)) ? (int32_t)total : -1;
  }
  // one atomic per (block, sample): atomics on the few maxdepth words serialize
  for (int sb = s_blk[0]; sb <= s_blk[1]; ++sb) {  // block-uniform
    int32_t mx = -1;
#pragma unroll
    for (int k = 0; k < kCR; ++k) {
      const int64_t row = b0 + threadIdx.x + 256 * k;
      if (dep[k] > mx && (s_blk[0] == s_blk[1] || sample_of_row_lds(d, srow, row) == sb)) mx = dep[k];
    }
    mx = wave_max(mx);
    __syncthreads();
    if (lane() == 0) s_w[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int32_t m = max(max(s_w[0], s_w[1]), max(s_w[2], s_w[3]));
      // skip the atomic when a value of this run already covers m (the maxima
      // only grow; a cached read is never above the true one): all blocks'
      // atomics on the few maxdepth words serialize (C5: 6k blocks)
      if (m >= 0 && (uint32_t)m > __hip_atomic_load(d.maxdepth + sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(d.maxdepth + sb, (uint32_t)m);
    }
  }
}

// keep[row] = emitted (:428) and the ordered compaction of the kept calls in
// ONE launch: every block publishes its kept count, then chains the counts of
// the blocks before it by a decoupled look-back (one 64-bit status word per
// block, {flag, launch epoch, value}: flag 1 = the block's own count, 2 = its
// inclusive prefix; wave 0 reads 64 predecessors per step and stops at the
// nearest prefix).  Blocks are dispatched in index order, so a block only ever
// waits on blocks that are already running or done; the spin is bounded anyway
// (DE_INTERNAL instead of a hang).  Replaces K_keep + K_emit (two launches and
// a read of every block count by every block).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void K_select(Dev d, int64_t R, uint32_t epoch) {
  __shared__ int32_t srow[kSmpLds];
  __shared__ uint32_t smd[kSmpLds];
  __shared__ int32_t s_w[1][4];
  __shared__ int64_t s_pre[1];
  load_sample_rows(d, srow);
  for (int s = threadIdx.x; s < d.S && s < kSmpLds; s += blockDim.x) smd[s] = d.maxdepth[s];
  const int64_t b = blockIdx.x;
  const int64_t nb = (R + kKB - 1) / kKB;
  const int64_t base = b * kKB + 4 * threadIdx.x;
  uint4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = base + k < R ? reinterpret_cast<const uint4*>(d.res)[base + k] : make_uint4(0, 0, 0, 0);
  __syncthreads();
  int c = 0;
  uint32_t bits = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (v[k].x >> 24) {
      const int s = sample_of_row_lds(d, srow, base + k);
      const double thr = (double)(s < kSmpLds ? smd[s] : d.maxdepth[s]) * d.mdf;  // :338
      if ((double)v[k].y > thr) { ++c; bits |= 1u << k; }  // :428
    }
  }
  const int cv[1] = {c};
  int inc[1], bt[1];
  int64_t pre[1];
  chain_scan<4, 1>(reinterpret_cast<uint64_t*>(d.ksum), b, epoch, cv, inc, bt, pre, s_w, s_pre, &d.status[MPC_ST_FLAGS]);
  int64_t pos = pre[0] + inc[0] - c;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (bits & (1u << k)) {
      const uint4 x = v[k];
      reinterpret_cast<uint4*>(d.calls)[pos++] = make_uint4(x.x & 0xffffffu, x.y, x.z, x.w);
    }
  // ncalls[s] = calls before the first row of sample s; ncalls[S] = all
  const int64_t b0 = b * kKB, all = pre[0] + bt[0];
  for (int s = 0; s < d.S; ++s) {
    const int64_t rb = s < kSmpLds ? srow[s] : d.srow[s];
    if (rb >= b0 && rb < b0 + kKB && (rb - b0) / 4 == threadIdx.x) {
      int64_t q = pre[0] + inc[0] - c;
      for (int k = 0; k < (int)((rb - b0) & 3); ++k) q += (bits >> k) & 1u;
      d.ncalls[s] = (int32_t)q;
    }
    if (b == nb - 1 && threadIdx.x == 0 && rb >= nb * kKB) d.ncalls[s] = (int32_t)all;
  }
  if (b == nb - 1 && threadIdx.x == 0) d.ncalls[d.S] = (int32_t)all;
}

}  // namespace
