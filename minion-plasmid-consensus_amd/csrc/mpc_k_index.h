// The index and runs phases (mpc_index, mpc_runs): the order in which the
// reference meets a gap's strings (:37-72 depend on it) as a sort of the RIGHT
// events and a global run index space (the kernels: mpc_kernels.hip's overview),
// and what K_left / K_ins / K_flank read them with (run_left, load_unit, unit_page).
#pragma once

#include <algorithm>

#include "mpc_k_common.h"

namespace {

// ---------------------------------------------------------------------------
// Downstream (RIGHT) events.  A gap holding only RIGHT events needs only its
// longest downstream flank (slot bi = base bi, :64-72).  Gaps that also hold a
// LEFT event ("mixed") need the RIGHT events in read order -> sort keys.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool has_left(const uint32_t* bm, int64_t g) { return (bm[g >> 5] >> (g & 31)) & 1u; }

__device__ __forceinline__ bool l_is(int j) { return lane() == j; }
__device__ __forceinline__ void rsplit_block(const Dev& d, int64_t b) {
  __shared__ int64_t s_key;
  __shared__ int32_t s_val;
  __shared__ int32_t s_w[kRS / 64];
  const int64_t r = b * blockDim.x + threadIdx.x;
  const bool in = r < d.N;
  int64_t g = -1;
  int32_t len = 0;
  bool mixed = false;
  const int64_t rg = d.read_offset + r;
  if (in) {
    const int s = d.sample[r];
    const int64_t n = d.n_of[s];
    const int64_t ie = d.i_end[r];
    const int64_t L = d.down_off[r + 1] - d.down_off[r];
    len = L > 0x7fffffff ? 0x7fffffff : (int32_t)L;
    if (len > 0 && ie <= n) {
      g = d.gbase[s] + ie;
      mixed = has_left(d.hasleft, g);
    }
    d.rlen[rg] = len;
  }
  // block-local stable compaction of the mixed events (read order), for K_rsort
  int bt;
  const int inc = block_scan(mixed ? 1 : 0, bt, s_w);
  if (mixed) {
    const int64_t o = b * blockDim.x + inc - 1;
    d.keys_in[o] = (uint32_t)g;
    d.vals_in[o] = (int32_t)rg;
  }
  if (d.gcnt) {  // multi-workgroup sort: the event's slot within its gap (any order), one atomic per gap per wave
    for (uint64_t act = ballot(mixed); act;) {
      const int lead = __ffsll((unsigned long long)act) - 1;
      const int32_t gl = __builtin_amdgcn_readlane((int)g, lead);
      const uint64_t same = ballot(mixed && (int32_t)g == gl);
      int32_t base = 0;
      if (l_is(lead)) base = atomicAdd(d.gcnt + gl, __popcll(same));
      base = __builtin_amdgcn_readlane(base, lead);
      if (mixed && (int32_t)g == gl) d.kslot[b * blockDim.x + inc - 1] = base + lanes_below(same);
      act &= ~same;
    }
  }
  if (threadIdx.x == 0) d.bcnt[b] = bt;
  block_atomic_max(d.maxR, g < 0 ? 0 : g, len, in && g >= 0 && !mixed, &s_key, &s_val);
}

// ---------------------------------------------------------------------------
// K_rsort: the mixed RIGHT events (partial reads ending at gaps that also hold
// LEFT events: few) sorted by (gap, read).  One workgroup: gather the per-block
// lists of K_rsplit (in read order), then a stable LSD radix sort on the gap
// (8-bit digits, a contiguous segment per wave, wave multi-split ranks) -- in
// LDS when the list fits, else ping-ponging through HBM (same code, generic
// pointers).
// ---------------------------------------------------------------------------
constexpr int kSortLds = 8192;
constexpr int kRsuLds = 2;  // K_rsort chunks in flight in LDS (measured 1/2/4/8 at C1/C2/C4: 2)
constexpr int kGatherLds = 2048;  // source blocks whose prefix stays in LDS (entry-parallel gather)

// One stable LSD pass of K_rsort over digit (key >> sh) & 255: wave w owns the
// contiguous segment [s0, s1) of the list (read order); per-wave digit
// histograms, one scan -> per (wave, digit) start, then every wave walks ITS
// segment in order, 64 entries at a time: stable ranks by wave multi-split,
// the digit's cursor in the wave's own LDS row (no barrier inside the walk:
// 4 per pass).  Force-inlined at call sites whose buffers are all LDS or all
// HBM, so the accesses compile to ds_* / global_* instead of flat.
template <int U>  // chunks of 64 entries in flight per wave (HBM: latency; LDS: few)
__device__ __forceinline__ void rsort_pass(const uint32_t* sk, const int32_t* sv, uint32_t* dk, int32_t* dv, int sh,
                                           int64_t s0, int64_t s1, int32_t (*wc)[256], int32_t* hb) {
  constexpr int NW = kRS / 64;
  const int tid = threadIdx.x, l = lane(), w = tid >> 6;
  const uint64_t lt = (1ull << l) - 1ull;
  for (int k = l; k < 256; k += 64) wc[w][k] = 0;
  for (int64_t i0 = s0; i0 < s1; i0 += U * 64) {
    uint32_t kk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + 64 * u + l;
      kk[u] = i < s1 ? sk[i] : ~0u;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (kk[u] != ~0u) atomicAdd(&wc[w][(kk[u] >> sh) & 255u], 1);
  }
  __syncthreads();
  if (tid < 256) {
    int t = 0;
    for (int k = 0; k < NW; ++k) t += wc[k][tid];
    hb[tid] = t;
  }
  __syncthreads();
  if (tid < 64) {  // exclusive scan of the 256 digit totals (4 per lane)
    const int x0 = hb[4 * tid], x1 = hb[4 * tid + 1], x2 = hb[4 * tid + 2], x3 = hb[4 * tid + 3];
    const int t4 = x0 + x1 + x2 + x3;
    const int e = wave_scan_i32(t4) - t4;
    hb[4 * tid] = e; hb[4 * tid + 1] = e + x0; hb[4 * tid + 2] = e + x0 + x1; hb[4 * tid + 3] = e + x0 + x1 + x2;
  }
  __syncthreads();
  if (tid < 256) {  // per (wave, digit) start: digit start + the digit's entries in lower waves
    int run = hb[tid];
    for (int k = 0; k < NW; ++k) { const int c = wc[k][tid]; wc[k][tid] = run; run += c; }
  }
  __syncthreads();
  for (int64_t i0 = s0; i0 < s1; i0 += U * 64) {
    uint32_t kk[U];
    int32_t vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + 64 * u + l;
      kk[u] = i < s1 ? sk[i] : 0u;
      vv[u] = i < s1 ? sv[i] : 0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool v = i0 + 64 * u + l < s1;
      const uint32_t dg = (kk[u] >> sh) & 255u;
      uint64_t m = ballot(v);
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const uint64_t bb = ballot(((dg >> bit) & 1u) != 0);
        m &= ((dg >> bit) & 1u) ? bb : ~bb;
      }
      const int rank = __popcll(m & lt);
      const int base = v ? wc[w][dg] : 0;
      if (v) { dk[base + rank] = kk[u]; dv[base + rank] = vv[u]; }
      if (v && rank == 0) wc[w][dg] = base + __popcll(m);  // after every lane's read (in order: one wave)
    }
  }
  __syncthreads();
}

// Register path of K_rsort (more entries than the LDS path holds, up to
// kRS * kRegE): an entry is ONE word, gap << sb | its index in read order (sb
// bits), so the stable gap passes keep read order and need one LDS buffer: the
// entries of a pass's source order sit in VGPRs (wave w: positions s0 + 64 u +
// lane), the scatter writes the new order into LDS, and every wave reloads its
// positions from there.  The values (global reads) wait in HBM at their index.
constexpr int kRegE = 32;
__device__ __forceinline__ void rsort_reg_pass(uint32_t (&e)[kRegE], int64_t s0, int64_t s1, int sh, uint32_t* buf,
                                               int32_t (*wc)[256], int32_t* hb, bool reload) {
  constexpr int NW = kRS / 64;
  const int tid = threadIdx.x, l = lane(), w = tid >> 6;
  const uint64_t lt = (1ull << l) - 1ull;
  for (int k = l; k < 256; k += 64) wc[w][k] = 0;
#pragma unroll
  for (int u = 0; u < kRegE; ++u)
    if (s0 + 64 * u + l < s1) atomicAdd(&wc[w][(e[u] >> sh) & 255u], 1);
  __syncthreads();
  if (tid < 256) {
    int t = 0;
    for (int k = 0; k < NW; ++k) t += wc[k][tid];
    hb[tid] = t;
  }
  __syncthreads();
  if (tid < 64) {
    const int x0 = hb[4 * tid], x1 = hb[4 * tid + 1], x2 = hb[4 * tid + 2], x3 = hb[4 * tid + 3];
    const int t4 = x0 + x1 + x2 + x3;
    const int ex = wave_scan_i32(t4) - t4;
    hb[4 * tid] = ex; hb[4 * tid + 1] = ex + x0; hb[4 * tid + 2] = ex + x0 + x1; hb[4 * tid + 3] = ex + x0 + x1 + x2;
  }
  __syncthreads();
  if (tid < 256) {
    int run = hb[tid];
    for (int k = 0; k < NW; ++k) { const int c = wc[k][tid]; wc[k][tid] = run; run += c; }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kRegE; ++u) {
    const bool v = s0 + 64 * u + l < s1;
    if (ballot(v) == 0) break;  // (wave-uniform) the wave's positions are used up
    const uint32_t dg = (e[u] >> sh) & 255u;
    uint64_t m = ballot(v);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const uint64_t bb = ballot(((dg >> bit) & 1u) != 0);
      m &= ((dg >> bit) & 1u) ? bb : ~bb;
    }
    const int rank = __popcll(m & lt);
    const int base = v ? wc[w][dg] : 0;
    if (v) buf[base + rank] = e[u];
    if (v && rank == 0) wc[w][dg] = base + __popcll(m);
  }
  __syncthreads();
  if (reload) {
#pragma unroll
    for (int u = 0; u < kRegE; ++u)
      if (s0 + 64 * u + l < s1) e[u] = buf[s0 + 64 * u + l];
  }
}

__global__ __launch_bounds__(kRS) void K_rsort(Dev d, int32_t nblocks, int32_t end_bit) {
  if (d.rsflag && d.rsflag[0] == 1) return;  // the multi-workgroup path sorted them
  __shared__ uint32_t pool[4 * kSortLds];  // LDS path: keys and values, two buffers each; register path: one buffer
  uint32_t (*lk)[kSortLds] = reinterpret_cast<uint32_t (*)[kSortLds]>(pool);
  int32_t (*lv)[kSortLds] = reinterpret_cast<int32_t (*)[kSortLds]>(pool + 2 * kSortLds);
  __shared__ int32_t wc[kRS / 64][256];
  __shared__ int32_t hb[256];
  __shared__ int32_t s_w[kRS / 64];
  __shared__ int32_t s_bpre[kGatherLds + 1];
  const int tid = threadIdx.x, l = lane(), w = tid >> 6;
  const bool pre_lds = nblocks <= kGatherLds;
  // exclusive prefix of the per-block counts -> bpre[0..nblocks]
  int carry = 0;
  for (int c0 = 0; c0 < nblocks; c0 += kRS) {
    const int b = c0 + tid;
    const int v = b < nblocks ? d.bcnt[b] : 0;
    int tot;
    const int pre = carry + block_scan(v, tot, s_w) - v;
    carry += tot;
    if (b < nblocks) {
      d.bpre[b] = pre;
      if (pre_lds) s_bpre[b] = pre;
    }
    __syncthreads();  // s_w: the next pass
  }
  const int64_t M = carry;
  if (tid == 0) { d.bpre[nblocks] = (int32_t)M; d.status[MPC_ST_MIXED] = (uint32_t)M; }
  if (M == 0) return;
  const int passes = (end_bit + 7) / 8;
  const bool in_lds = M <= kSortLds;
  const int sb = 32 - __clz((uint32_t)(M - 1) | 1u);  // bits of an entry index (register path)
  if (!in_lds && M <= (int64_t)kRS * kRegE && end_bit + sb <= 32) {
    // ---- register path: gather gap << sb | index into LDS (values to HBM), one source block per thread ----
    for (int b = tid; b < nblocks; b += kRS) {
      const int c = d.bcnt[b];
      const int o = d.bpre[b];
      const uint32_t* ks = d.keys_in + (int64_t)b * kRS;
      const int32_t* vs = d.vals_in + (int64_t)b * kRS;
      for (int j0 = 0; j0 < c; j0 += 8) {
        uint32_t kk[8];
        int32_t vv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = j0 + u < c ? j0 + u : c - 1;
          kk[u] = ks[j];
          vv[u] = vs[j];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (j0 + u < c) { pool[o + j0 + u] = kk[u] << sb | (uint32_t)(o + j0 + u); d.vals_tmp[o + j0 + u] = vv[u]; }
      }
    }
    __syncthreads();
    constexpr int NW = kRS / 64;
    const int64_t s0 = M * w / NW, s1 = M * (w + 1) / NW;  // <= 64 kRegE positions per wave
    uint32_t e[kRegE];
#pragma unroll
    for (int u = 0; u < kRegE; ++u) e[u] = s0 + 64 * u + l < s1 ? pool[s0 + 64 * u + l] : 0u;
    __syncthreads();  // every wave holds its entries before the first scatter
    for (int p = 0; p < passes; ++p) rsort_reg_pass(e, s0, s1, sb + 8 * p, pool, wc, hb, p + 1 < passes);
    const uint32_t im = (1u << sb) - 1u;  // (sb <= 15 here)
    for (int64_t i0 = 0; i0 < M; i0 += 4 * kRS) {
      uint32_t x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const int64_t i = i0 + tid + u * kRS; x[u] = i < M ? pool[i] : 0u; }
      int32_t vv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const int64_t i = i0 + tid + u * kRS; vv[u] = i < M ? d.vals_tmp[x[u] & im] : 0; }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + tid + u * kRS;
        if (i < M) { d.keys_out[i] = x[u] >> sb; d.vals_out[i] = vv[u]; }
      }
    }
    return;
  }
  uint32_t* kb[2];
  int32_t* vb[2];
  if (in_lds) { kb[0] = lk[0]; kb[1] = lk[1]; vb[0] = lv[0]; vb[1] = lv[1]; }
  else {
    kb[passes & 1] = d.keys_out; vb[passes & 1] = d.vals_out;
    kb[(passes + 1) & 1] = d.keys_tmp; vb[(passes + 1) & 1] = d.vals_tmp;
  }
  __syncthreads();
  // gather (read order) into buffer 0.  Few source blocks: entry-parallel, the
  // source block of entry i by a search of the LDS prefix, 8 loads in flight
  // per thread; else one source block per thread, 8 loads in flight per batch
  // (the copies are independent; a serial loop would wait a full memory
  // latency per entry)
  for (int64_t i0 = 0; pre_lds && i0 < M; i0 += 8 * kRS) {
    uint32_t kk[8];
    int32_t vv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t i = i0 + tid + (int64_t)u * kRS;
      kk[u] = 0u; vv[u] = 0;
      if (i < M) {
        int lo = 0, hi = nblocks - 1;  // last block with s_bpre <= i (it holds >= 1 entry)
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (s_bpre[mid] <= i) lo = mid; else hi = mid - 1;
        }
        const int64_t src = (int64_t)lo * kRS + (i - s_bpre[lo]);
        kk[u] = d.keys_in[src];
        vv[u] = d.vals_in[src];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t i = i0 + tid + (int64_t)u * kRS;
      if (i < M) {
        if (in_lds) { lk[0][i] = kk[u]; lv[0][i] = vv[u]; }
        else { kb[0][i] = kk[u]; vb[0][i] = vv[u]; }
      }
    }
  }
  for (int b = tid; !pre_lds && b < nblocks; b += kRS) {
    const int c = d.bcnt[b];
    const int o = d.bpre[b];
    const uint32_t* ks = d.keys_in + (int64_t)b * kRS;
    const int32_t* vs = d.vals_in + (int64_t)b * kRS;
    for (int j0 = 0; j0 < c; j0 += 8) {
      uint32_t kk[8];
      int32_t vv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 + u < c ? j0 + u : c - 1;
        kk[u] = ks[j];
        vv[u] = vs[j];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (j0 + u < c) { kb[0][o + j0 + u] = kk[u]; vb[0][o + j0 + u] = vv[u]; }
    }
  }
  __syncthreads();
  constexpr int NW = kRS / 64;
  const int64_t s0 = M * w / NW, s1 = M * (w + 1) / NW;
  if (in_lds) {  // LDS -> LDS passes, the last one LDS -> HBM
    for (int p = 0; p + 1 < passes; ++p) rsort_pass<kRsuLds>(lk[p & 1], lv[p & 1], lk[(p + 1) & 1], lv[(p + 1) & 1], 8 * p, s0, s1, wc, hb);
    rsort_pass<kRsuLds>(lk[(passes - 1) & 1], lv[(passes - 1) & 1], d.keys_out, d.vals_out, 8 * (passes - 1), s0, s1, wc, hb);
  } else {
    for (int p = 0; p < passes; ++p) {  // buffer (passes - p) & 1 is keys_out / vals_out: the last pass lands there
      const bool src_out = ((passes - p) & 1) == 0;
      rsort_pass<8>(src_out ? d.keys_out : d.keys_tmp, src_out ? d.vals_out : d.vals_tmp, src_out ? d.keys_tmp : d.keys_out,
                 src_out ? d.vals_tmp : d.vals_out, 8 * p, s0, s1, wc, hb);
    }
  }
}

// ---------------------------------------------------------------------------
// Multi-workgroup sort of the mixed RIGHT events (many reads: K_rsort's one
// workgroup took 88 us at C3's 19k events, all of it latency).  K_rsplit gave
// every event a slot within its gap (atomics: any order); K_rscan scans the
// per-gap counts (two launches: block sums, then block scans with the sum of
// the blocks before), K_rscatter puts every event at rsl[gap] + slot, and
// K_rsegsort restores read order inside each gap (a wave's bitonic sort of up
// to 64 reads).  A gap with more than 64 events, or few events overall, sends
// the launch to K_rsort instead (path word rsflag[0]: 1 = this path).
// ---------------------------------------------------------------------------
// (kRsortMultiBlocks, kScanPer, kScanBlk: mpc_geometry.h)
constexpr int kSegMax = 64;

__global__ __launch_bounds__(1024) void K_rscan1(Dev d) {
  __shared__ int32_t s_s[16], s_m[16];
  const int64_t g0 = (int64_t)blockIdx.x * kScanBlk + (int64_t)threadIdx.x * kScanPer;
  int32_t sum = 0, mx = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    const int32_t c = g0 + k <= d.G ? d.gcnt[g0 + k] : 0;
    sum += c;
    mx = c > mx ? c : mx;
  }
  sum = wave_sum(sum);
  mx = wave_max(mx);
  const int w = threadIdx.x >> 6;
  if (lane() == 0) { s_s[w] = sum; s_m[w] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t t = 0, m = 0;
    for (int k = 0; k < 16; ++k) { t += s_s[k]; m = s_m[k] > m ? s_m[k] : m; }
    d.rsflag[4 + 2 * blockIdx.x] = t;
    d.rsflag[5 + 2 * blockIdx.x] = m;
  }
}

__global__ __launch_bounds__(1024) void K_rscan2(Dev d, int32_t nblk_scan) {
  __shared__ int32_t s_w[16];
  __shared__ int32_t s_pre, s_tot, s_max;
  const int tid = threadIdx.x;
  if (tid < 64) {  // blocks before this one, and the totals
    int32_t pre = 0, tot = 0, mx = 0;
    for (int k = tid; k < nblk_scan; k += 64) {
      const int32_t c = d.rsflag[4 + 2 * k], m = d.rsflag[5 + 2 * k];
      tot += c;
      if (k < (int)blockIdx.x) pre += c;
      mx = m > mx ? m : mx;
    }
    pre = wave_sum(pre);
    tot = wave_sum(tot);
    mx = wave_max(mx);
    if (tid == 0) { s_pre = pre; s_tot = tot; s_max = mx; }
  }
  __syncthreads();
  const int64_t g0 = (int64_t)blockIdx.x * kScanBlk + (int64_t)tid * kScanPer;
  int32_t c[kScanPer], sum = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) { c[k] = g0 + k <= d.G ? d.gcnt[g0 + k] : 0; sum += c[k]; }
  int bt;
  int32_t run = s_pre + block_scan(sum, bt, s_w) - sum;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    if (g0 + k <= d.G) d.rsl[g0 + k] = run;  // (K_rstart writes the same values again)
    run += c[k];
  }
  if (blockIdx.x == 0 && tid == 0) {
    const bool multi = s_tot > kSortLds && s_max <= kSegMax;
    d.rsflag[0] = multi ? 1 : 0;
    d.status[MPC_ST_RSORT_PATH] = multi ? 1u : 2u;
    if (multi) d.status[MPC_ST_MIXED] = (uint32_t)s_tot;
  }
}

__global__ __launch_bounds__(kRS) void K_rscatter(Dev d) {
  if (d.rsflag[0] != 1) return;
  const int64_t b = blockIdx.x;
  const int c = d.bcnt[b];
  if ((int)threadIdx.x >= c) return;
  const int64_t o = b * kRS + threadIdx.x;
  const uint32_t g = d.keys_in[o];
  const int64_t pos = (int64_t)d.rsl[g] + d.kslot[o];
  d.keys_out[pos] = g;
  d.vals_out[pos] = d.vals_in[o];
}

// one wave per gap: its (<= 64) reads in ascending order, bitonic over the lanes
__global__ __launch_bounds__(256) void K_rsegsort(Dev d) {
  if (d.rsflag[0] != 1) return;
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g > d.G) return;
  const int32_t c = d.gcnt[g];
  if (c < 2) return;  // (wave-uniform)
  const int l = lane();
  const int64_t a0 = d.rsl[g];
  int32_t v = l < c ? d.vals_out[a0 + l] : INT32_MAX;
  for (int k = 2; k <= 64; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int32_t y = __shfl_xor(v, j, 64);
      const bool up = (l & k) == 0, low = (l & j) == 0;
      v = (low == up) ? (v < y ? v : y) : (v > y ? v : y);
    }
  }
  if (l < c) d.vals_out[a0 + l] = v;
}

// rsl[g] = #mixed RIGHT events of this shard with gap < g; rpos[local read] =
// its position in the shard's sorted list (so consumers need no search).  One
// shard: right_start = rsl, roff = 0, and the RIGHT length of run t + g (the run
// that this event closes) is filled here.  Several: per-gap counts for the
// exchange (K_runs / K_runR).
__global__ __launch_bounds__(256) void K_rstart(Dev d) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t M = d.status[MPC_ST_MIXED];
  if (t <= d.G) {
    const int32_t v = (int32_t)lower_bound_u32(d.keys_out, 0, M, (uint32_t)t);
    d.rsl[t] = v;
    if (d.n_shards == 1) { d.right_start[t] = v; d.roff[t] = 0; }
    if (t < d.G) d.rcnt[t] = (int32_t)lower_bound_u32(d.keys_out, 0, M, (uint32_t)t + 1) - v;
  }
  if (t < M) {
    const uint32_t g = d.keys_out[t];
    const int64_t rg = d.vals_out[t];
    const int64_t lr = rg - d.read_offset;
    if (lr >= 0 && lr < d.N) d.rpos[lr] = (int32_t)t;
    if (d.n_shards == 1) d.runR[t + g] = d.rlen[rg];
  }
}

// Several shards: global right_start and roff from all shards' per-gap counts:
// 1024 gaps per block, the blocks' sums chained by a decoupled look-back
// (K_layout's status words, which it re-tags with its own epoch later in the
// step; one workgroup over all gaps took C2 x 8 shards 18 us)
constexpr int kRunsGB = 1024;
__global__ __launch_bounds__(kRunsGB) void K_runs(Dev d, uint32_t epoch) {
  __shared__ int32_t s_w[1][kRunsGB / 64];
  __shared__ int64_t s_pre[1];
  const int64_t b = blockIdx.x;
  const int64_t g = b * kRunsGB + threadIdx.x;
  int32_t tot = 0, below = 0;
  if (g < d.G)
    for (int k = 0; k < d.n_shards; ++k) {
      const int32_t c = d.rcnt_all[(int64_t)k * d.G + g];
      tot += c;
      below += k < d.shard ? c : 0;
    }
  const int v[1] = {tot};
  int inc[1], bt[1];
  int64_t pre[1];
  chain_scan<kRunsGB / 64, 1>(reinterpret_cast<uint64_t*>(d.bsum), b, epoch, v, inc, bt, pre, s_w, s_pre,
                              &d.status[MPC_ST_FLAGS]);
  if (g <= d.G) {
    d.right_start[g] = (int32_t)(pre[0] + inc[0] - tot);
    d.roff[g] = below;
  }
}

// Several shards: RIGHT length of the run each of this shard's mixed RIGHT
// events closes, in the global run index space (exchange: MAX over shards).
__global__ __launch_bounds__(256) void K_runR(Dev d) {
  const int64_t nml = d.rsl[d.G];
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nml; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = d.keys_out[t];
    const int64_t run = (int64_t)d.right_start[g] + g + d.roff[g] + (t - d.rsl[g]);
    d.runR[run] = d.rlen[d.vals_out[t]];
  }
}

// Global run index of a LEFT event of (this shard's) global read rg at global
// gap g: runs of gap g are [right_start[g] + g, right_start[g+1] + g + 1); run
// k precedes the k-th mixed RIGHT event of the gap, k = RIGHT events of lower
// shards + this shard's RIGHT events of earlier reads.
__device__ __forceinline__ int64_t run_left(const int32_t* rs, const int32_t* rsl, const int32_t* roff,
                                            const int32_t* vals_out, int64_t g, int64_t rg) {
  const int64_t a = rsl[g], b = rsl[g + 1];
  int64_t k = roff[g];
  if (b > a) k += lower_bound_i32(vals_out, a, b, (int32_t)rg) - a;
  return rs[g] + g + k;
}

// ---------------------------------------------------------------------------
// Bucketed event work units.  K_parse leaves, per parse workgroup, its
// insertion events counting-sorted into buckets of 16 gaps.  Entries of the
// host table `bc` are (sample, bucket, chunk of <= 256 parse workgroups);
// K_units cuts every entry's events into units of <= kUnit events (hot
// buckets become many units) and appends them to one list.
// ---------------------------------------------------------------------------
constexpr int kLeftVals = 4096;       // mixed RIGHT reads of a bucket staged in K_left's LDS
constexpr int kUnit = kUB * kEPT;     // events per work unit (K_left<kUB>; K_left<512>: half)

struct UnitArgs {
  const int4* bc;  // {sample, bucket, pw0, pw1}
  const int32_t* n_of; const int32_t* gbase;
  const int32_t* bk_cnt; int4* units; uint32_t* status;  // units: 2 int4 per unit (see load_unit)
  int64_t n_bc, units_cap;
  int32_t nbs;
  int32_t unit;  // pages per work unit (K_left's threads x kEPT / 64: one page per wave and step)
};

// kUE consecutive table entries per wave (one wave per entry at a time), one
// add to the unit counter per block: a single counter word serializes its
// atomics (~90 per us), and C5 has 45k entries
constexpr int kUE = 4;
constexpr int kUnitEntriesPerBlock = (kRS / 64) * kUE;
__device__ __forceinline__ void units_block(const UnitArgs& a, int64_t blk) {
  __shared__ int32_t s_wu[kRS / 64];
  __shared__ uint32_t s_ubase;
  const int l = lane(), w = threadIdx.x >> 6;
  const int64_t ent0 = blk * kUnitEntriesPerBlock + (int64_t)w * kUE;
  int ts[kUE], nus[kUE], wsum = 0;
  int4 bcs[kUE];
#pragma unroll
  for (int e = 0; e < kUE; ++e) {
    const int64_t ent = ent0 + e;
    int t = 0;
    bcs[e] = make_int4(0, 0, 0, 0);
    if (ent < a.n_bc) {  // wave-uniform
      const int4 bc = a.bc[ent];
      bcs[e] = bc;
      for (int pw = bc.z + l; pw < bc.w; pw += 64) t += (a.bk_cnt[(int64_t)pw * a.nbs + bc.y] + kPgEv - 1) / kPgEv;
      t = wave_sum(t);  // the entry's pages
    }
    ts[e] = t;
    nus[e] = (t + a.unit - 1) / a.unit;
    wsum += nus[e];
  }
  if (l == 0) s_wu[w] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int k = 0; k < kRS / 64; ++k) { const int v = s_wu[k]; s_wu[k] = tot; tot += v; }
    s_ubase = tot ? atomicAdd(&a.status[MPC_ST_UNITS], (uint32_t)tot) : 0u;
  }
  __syncthreads();
  int64_t u0 = (int64_t)s_ubase + s_wu[w];
#pragma unroll
  for (int e = 0; e < kUE; ++e) {
    const int nu = nus[e];
    if (nu == 0) continue;
    if (u0 + nu > a.units_cap) {
      if (l == 0) atomicOr(&a.status[MPC_ST_FLAGS], DE_INTERNAL);
      return;
    }
    const int n = a.n_of[bcs[e].x], gb = a.gbase[bcs[e].x];
    for (int i = l; i < nu; i += 64) {
      const int e0 = i * a.unit;
      a.units[2 * (u0 + i)] = bcs[e];
      a.units[2 * (u0 + i) + 1] = make_int4(e0, ts[e] - e0 < a.unit ? ts[e] - e0 : a.unit, n, gb);
    }
    u0 += nu;
  }
}

// One launch for two independent jobs after the parse: blocks [0, nrb) split
// the RIGHT events (one read per thread), the rest cut the insertion work
// units (one table entry per wave).  Block-uniform branch.
__global__ __launch_bounds__(kRS) void K_rsplit_units(Dev d, UnitArgs ua, int32_t nrb) {
  if ((int32_t)blockIdx.x < nrb) rsplit_block(d, blockIdx.x);
  else units_block(ua, (int64_t)blockIdx.x - nrb);
}

struct UnitView { int smp, bucket, p0, np, n, gb, g0, gl, nsl; };
// A unit record (2 int4, written by units_block): {sample, bucket, pw0, pw1},
// {p0, np, n, gbase}: pages [p0, p0 + np) of the entry's page sequence (its
// slices -- parse workgroups pw0.. -- in order, each slice's pages as its list
// in pg_list holds them: global page numbers, all full but the last).  One
// round trip loads, per slice, its events, its list base and its workgroup's
// first read, and the bucket's per-gap tables (global run range, this shard's
// sorted-RIGHT range); a block scan gives the slices' first pages (s_ppre).
// Wave w then takes the unit's pages w, w + NW, ... (unit_page: the slice of a
// wave-uniform page by a search of s_ppre, its global page from pg_list), one
// event per lane.
__device__ __forceinline__ UnitView load_unit(const int4* units, int64_t u, const int32_t* bk_cnt,
                                              const int32_t* bk_off, const int64_t* rbase, int nbs,
                                              const int32_t* right_start, const int32_t* rsl, const int32_t* roff,
                                              const int4* pwork, int32_t* s_ppre, int32_t* s_cnt, int64_t* s_src,
                                              int32_t* s_r0, int32_t* s_wsum, int32_t* s_rs, int32_t* s_rsl,
                                              int32_t* s_roff) {
  const int4 ua = units[2 * u], ub = units[2 * u + 1];
  UnitView v;
  v.smp = ua.x; v.bucket = ua.y; v.p0 = ub.x; v.np = ub.y; v.n = ub.z; v.gb = ub.w; v.nsl = ua.w - ua.z;
  v.g0 = v.bucket * kBW;
  v.gl = v.g0 + kBW - 1 < v.n ? v.g0 + kBW - 1 : v.n;  // last gap of the bucket
  const int l = lane(), w = threadIdx.x >> 6;
  const int tid = (int)threadIdx.x;
  int cnt = 0, r0 = 0;
  int64_t src = 0;
  if (tid < 256) {  // <= 256 slices (parse workgroups) per table entry
    const int pw = ua.z + tid;
    if (pw < ua.w) {
      const int64_t slot = (int64_t)pw * nbs + v.bucket;
      cnt = bk_cnt[slot];
      src = rbase[pw] + bk_off[slot];  // the slice's page list in pg_list
      r0 = pwork[pw].y;
    }
  }
  const int64_t gg = (int64_t)v.gb + v.g0 + tid;
  if (tid <= v.gl + 1 - v.g0) { s_rs[tid] = right_start[gg]; s_rsl[tid] = rsl[gg]; s_roff[tid] = roff[gg]; }
  const int npg = (cnt + kPgEv - 1) / kPgEv;
  if (tid < 256) {
    const int inc = wave_scan_i32(npg);
    if (l == 63) s_wsum[w] = inc;
    s_ppre[tid] = inc - npg;
    s_cnt[tid] = cnt;
    s_src[tid] = src;
    s_r0[tid] = r0;
  }
  __syncthreads();
  if (tid < 256) {
    int wpre = 0;
    for (int k = 0; k < w; ++k) wpre += s_wsum[k];
    s_ppre[tid] += wpre;
  }
  __syncthreads();
  return v;
}
// page P of the unit's entry: its global page, events and slice's first read
struct UnitPage { uint32_t page; int cnt, r0; };
__device__ __forceinline__ UnitPage unit_page(const uint32_t* pg_list, const int32_t* s_ppre, const int32_t* s_cnt,
                                              const int64_t* s_src, const int32_t* s_r0, int P) {
  int j = 0;
#pragma unroll
  for (int h = 128; h >= 1; h >>= 1) j = s_ppre[j + h] <= P ? j + h : j;
  const int k = P - s_ppre[j];
  UnitPage r;
  r.page = pg_list[s_src[j] + k];
  r.cnt = min(kPgEv, s_cnt[j] - kPgEv * k);
  r.r0 = s_r0[j];
  return r;
}

}  // namespace

// Host side: the unit-cutting arguments and the sort launches
static UnitArgs unit_args(const mpc_plan* p, const Dev& d) {
  UnitArgs a;
  a.bc = at<const int4>(p, mpc_plan::B_WBC); a.bk_cnt = at<int32_t>(p, mpc_plan::B_BKCNT);
  a.units = at<int4>(p, mpc_plan::B_UNITS); a.status = d.status;
  a.n_of = d.n_of; a.gbase = d.gbase;
  a.n_bc = p->n_bc; a.units_cap = p->units_cap; a.nbs = p->nbmax; a.unit = p->left_ub * kEPT / kPgEv;

  return a;
}

// the mixed RIGHT events sorted by (gap, read): the multi-workgroup chain when
// the plan has many reads (it falls back to K_rsort by itself), else K_rsort
static void launch_rsort(const mpc_plan* p, const Dev& d, hipStream_t st) {
  const int32_t nrb = (int32_t)((p->N + kRS - 1) / kRS);
  if (p->rsort_multi) {
    const int32_t ns = (int32_t)((p->G + 1 + kScanBlk - 1) / kScanBlk);
    hipLaunchKernelGGL(K_rscan1, dim3(ns), dim3(1024), 0, st, d);
    hipLaunchKernelGGL(K_rscan2, dim3(ns), dim3(1024), 0, st, d, ns);
    hipLaunchKernelGGL(K_rscatter, dim3(nrb), dim3(kRS), 0, st, d);
    hipLaunchKernelGGL(K_rsegsort, dim3((unsigned)((p->G + 1 + 3) / 4)), dim3(256), 0, st, d);
  }
  hipLaunchKernelGGL(K_rsort, dim3(1), dim3(kRS), 0, st, d, nrb, (int32_t)p->end_bit);
}
