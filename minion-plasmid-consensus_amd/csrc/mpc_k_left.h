// The tally phase (mpc_tally): what processBaseString_leftIndel (:37-62) needs
// of the LEFT strings before the slot layout can be replayed.
// K_left: LEFT events -> per-run max length M (the slot layout's input; the
// bases themselves are tallied on rows once the layout is known).
//  * insertions: persistent workgroups over the work units; a unit's events
//    all lie in one kBW-gap bucket, so its (gap, run) maxima live in LDS (runs
//    k < kKMax; rarer runs go to HBM) and are flushed with atomics
//  * long insertions and upstream flanks (one per read, LEFT at gap tstart,
//    :303): grid-stride, wave-aggregated atomicMax (most reads share gap 0)
#pragma once

#include <algorithm>

#include "mpc_k_common.h"
#include "mpc_k_index.h"  // run_left, load_unit, unit_page

namespace {

struct LeftArgs {
  const int64_t* up_off; const int32_t* sample; const int32_t* tstart;
  const int32_t* n_of; const int32_t* gbase;
  const int4* bc; const int4* units; const uint32_t* status;
  const uint32_t* ins_sorted; const uint32_t* pg_list; const int32_t* bk_cnt; const int32_t* bk_off;
  const int64_t* rbase;
  const int4* pwork;  // parse work table {sample, r0, r1, 0}: a slice's first read
  int64_t N, read_offset, ovf_cap;
  int32_t nbs;
  const int32_t* right_start; const int32_t* rsl; const int32_t* roff; const int32_t* vals_out;
  int32_t* M; uint32_t* runt;
  const Ovf* ovf; const uint32_t* ovf_cnt;
};

// Resident blocks per CU, so that the per-unit latency chains overlap:
// UB = 1024 at most 64 VGPRs, two 16-wave blocks (LDS ~57 KB each; C3 K_left
// 312 -> 227 us, C4 387 -> 286 us; 5 VGPRs spill); UB = 512 at most 80 VGPRs
// and a smaller RIGHT-read stage, three 8-wave blocks (C5 285 -> 218 us)
template <int UB>  // threads per block; work units of UB * kEPT events
__global__ __launch_bounds__(UB) __attribute__((amdgpu_waves_per_eu(UB == 1024 ? 8 : 6))) void K_left(LeftArgs a) {
  __shared__ int64_t s_key;
  __shared__ int32_t s_val;
  // strides padded to odd word counts: every gap of the bucket starts on a
  // different bank (unpadded, all gaps' run-0 counters shared 16 banks)
  constexpr int kMs = kKMax + 1, kTs = kKMax * 16 + 1;
  __shared__ uint32_t Ml[kBW * kMs];
  __shared__ int32_t s_rs[kBW + 1], s_rsl[kBW + 1], s_roff[kBW + 1];  // per gap of the bucket (K_left)
  __shared__ int32_t s_ppre[257], s_cnt[256], s_r0[256], s_wsum[4];   // per slice: first page, events, first read
  __shared__ int64_t s_src[256];                                      // ... and its page list in pg_list
  // 1024-thread blocks (C1-C4: few, large units) stage the unit's pages once,
  // all threads in parallel (one barrier); 512-thread blocks (C5: many small
  // units) look each page up in the wave that takes it (no barrier)
  constexpr bool kStage = UB == 1024;
  constexpr int kUP = kStage ? UB * kEPT / kPgEv : 1;
  __shared__ uint4 s_pe[kUP];             // staged: {global page, events, first read, 0}
  __shared__ uint32_t Tl[kBW * kTs];  // per (gap, run): inline bases [bi from the 3' end][code]
  // 512-thread blocks: a smaller stage, so three blocks fit a CU's LDS
  constexpr int kLV = UB == 512 ? 3072 : kLeftVals;
  __shared__ int32_t s_vals[kLV];         // the bucket's mixed RIGHT reads (vals_out), searched per event
  // (K_units raises DE_INTERNAL instead of overrunning the unit list)
#ifdef MPC_STAMPS_LEFT
  uint64_t st_acc[kStampSeg] = {0, 0, 0, 0, 0, 0, 0, 0}, st_prev;
  MPC_STAMP(st_prev);
#endif
  const int64_t nunits = (a.status[MPC_ST_FLAGS] & DE_INTERNAL) ? 0 : a.status[MPC_ST_UNITS];
  // 512-thread blocks (plans with many small buckets, C5): the tallies are
  // zeroed once and every unit flushes (and re-zeroes) only the runs it can
  // touch (s_kn), and short slices are searched for all events at once -- C5
  // K_left 215 -> 189 us; on the 1024-thread plans (C2-C4) the same code was
  // slower (profiles/r04_experiments/k_left_variants.txt: l_kfpa)
  constexpr bool kLean = UB == 512;
  __shared__ int32_t s_kn;
  if constexpr (kLean) {
    for (int k = threadIdx.x; k < kBW * kMs; k += blockDim.x) Ml[k] = 0;
    for (int k = threadIdx.x; k < kBW * kTs; k += blockDim.x) Tl[k] = 0;
  }
  for (int64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
    if constexpr (kLean) {
      if (threadIdx.x == 0) s_kn = 0;  // ordered before its atomics by load_unit's barriers
    } else {
      for (int k = threadIdx.x; k < kBW * kMs; k += blockDim.x) Ml[k] = 0;
      for (int k = threadIdx.x; k < kBW * kTs; k += blockDim.x) Tl[k] = 0;
    }
    MPC_LSEG(0);
    const UnitView uv = load_unit(a.units, u, a.bk_cnt, a.bk_off, a.rbase, a.nbs, a.right_start, a.rsl, a.roff,
                                  a.pwork, s_ppre, s_cnt, s_src, s_r0, s_wsum, s_rs, s_rsl, s_roff);
    MPC_LSEG(1);
    const int n = uv.n;
    const int gb = uv.gb;
    const int g0 = uv.g0;
    uint32_t evs[kEPT];
    int32_t r0q[kEPT];  // the first read of each event's parse workgroup
    // all loads first (latency), then the tallies: wave w takes the unit's
    // pages w, w + NW, ... (wave-uniform: their slice searches and page numbers
    // are uniform), lane l the page's event l
    constexpr int NW = UB / 64;
    const int wv = uniform_i32((int)(threadIdx.x >> 6)), ln = lane();
    if constexpr (kStage) {
      for (int t = threadIdx.x; t < min(uv.np, kUP); t += UB) {
        const UnitPage pg = unit_page(a.pg_list, s_ppre, s_cnt, s_src, s_r0, uv.p0 + t);
        s_pe[t] = make_uint4(pg.page, (uint32_t)pg.cnt, (uint32_t)pg.r0, 0u);
      }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < kEPT; ++q) {
      const int t = wv + NW * q;
      evs[q] = ~0u;
      r0q[q] = 0;
      if (t < uv.np) {
        UnitPage pg;
        if constexpr (kStage) {
          const uint4 e = s_pe[t];
          pg.page = e.x; pg.cnt = (int)e.y; pg.r0 = (int)e.z;
        } else {
          pg = unit_page(a.pg_list, s_ppre, s_cnt, s_src, s_r0, uv.p0 + t);
        }
        r0q[q] = __builtin_amdgcn_readfirstlane(pg.r0);  // wave-uniform: SGPRs (K_left<1024> spilled 12 VGPRs)
        if (ln < pg.cnt) evs[q] = a.ins_sorted[(int64_t)pg.page * kPgEv + ln];
      }
    }
    // the run of an event at a mixed gap is a search of the gap's RIGHT reads:
    // stage the bucket's (contiguous in vals_out) in LDS, so no event waits on
    // a chain of dependent global loads
    const int32_t v0 = s_rsl[0], vn = s_rsl[uv.gl + 1 - g0] - v0;
    const bool vl = vn <= kLV;
    for (int k = threadIdx.x; vl && k < vn; k += blockDim.x) s_vals[k] = a.vals_out[v0 + k];
    if constexpr (kLean) {
      // LDS runs this unit can touch: an event at gap p has run k in
      // [roff, roff + its mixed RIGHT reads]; the flush covers runs < s_kn
      if (threadIdx.x < kBW && (int)threadIdx.x <= uv.gl - g0) {
        const int p = (int)threadIdx.x;
        atomicMax(&s_kn, min(s_rsl[p + 1] - s_rsl[p], kKMax - 1) + 1);
      }
    }
    MPC_LSEG(2);
    __syncthreads();
    MPC_LSEG(3);
#pragma unroll
    for (int q = 0; q < kEPT; ++q) {
      const uint32_t ev = evs[q];
      if (ev == ~0u) continue;
      const int gap = g0 + (int)((ev >> 10) & (kBW - 1));
      const int64_t g = (int64_t)gb + gap;
      const int32_t rg = (int32_t)a.read_offset + r0q[q] + (int32_t)(ev >> 16);  // global reads < 2^30
      const int L = (int)((ev >> 8) & 3u) + 1;
      const int p = gap - g0;
      // run of the event within its gap: this shard's runs of the gap start at
      // roff (the RIGHT events of lower shards); k counts from there
      const int32_t la = s_rsl[p], lb = s_rsl[p + 1];
      int32_t k = 0;
      if (lb > la) {
        if (vl) {  // 32-bit search of the staged RIGHT reads
          int lo = la - v0, hi = lb - v0;
          const int l0 = lo;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_vals[mid] < rg) lo = mid + 1; else hi = mid;
          }
          k += lo - l0;
        } else {
          k += lower_bound_i32(a.vals_out, la, lb, rg) - la;
        }
      }
      // the bases too, run-relative (LEFT: base bi from the 3' end lands on the
      // run's slot hi_run - 1 - bi, :37-62): K_ins maps them to rows after the layout
      // LDS slots: the shard's runs of the gap (as many as on one GPU); the
      // global run is s_rs[p] + g + roff + k
      if (k < kKMax) {
        // the run's longest LEFT string: UB = 1024 takes it from the highest
        // slot holding a base at the flush (one LDS atomic less per event: C4
        // K_left 230 -> 220 us); UB = 512 (C5: +5 us that way) per event
        if constexpr (kLean) atomicMax(&Ml[p * kMs + k], (uint32_t)L);
        uint32_t* tp = Tl + p * kTs + k * 16;
#pragma unroll
        for (int j = 0; j < kInsInline; ++j)  // straight-line: bases j < L
          if (j < L) atomicAdd(tp + 4 * (L - 1 - j) + (int)((ev >> (2 * j)) & 3u), 1u);
      } else {
        const int64_t run = s_rs[p] + g + (int64_t)s_roff[p] + k;
        atomicMax(a.M + run, L);
        uint32_t* rt = a.runt + run * 16;
        for (int j = 0; j < L; ++j) atomicAdd(rt + 4 * (L - 1 - j) + (int)((ev >> (2 * j)) & 3u), 1u);
      }
    }
    MPC_LSEG(4);
    __syncthreads();
    MPC_LSEG(5);
    if constexpr (kLean) {  // runs k < s_kn of every gap (k-major), read and re-zeroed
      const int kn = s_kn;
      for (int q = threadIdx.x; q < kBW * kn; q += blockDim.x) {
        const int p = q & (kBW - 1), k = q / kBW;
        const uint32_t m = Ml[p * kMs + k];
        if (m) {
          atomicMax(a.M + s_rs[p] + (int64_t)gb + g0 + p + s_roff[p] + k, (int32_t)m);
          Ml[p * kMs + k] = 0;
        }
      }
      for (int q = threadIdx.x; q < kBW * kn * 16; q += blockDim.x) {  // contiguous per (gap, run)
        const int p = (q >> 4) & (kBW - 1), k = q / (kBW * 16);
        const uint32_t v = Tl[p * kTs + k * 16 + (q & 15)];
        if (v) {
          atomicAdd(a.runt + (s_rs[p] + (int64_t)gb + g0 + p + s_roff[p] + k) * 16 + (q & 15), v);
          Tl[p * kTs + k * 16 + (q & 15)] = 0;
        }
      }
      __syncthreads();
      MPC_LSEG(6);
      continue;
    }
    for (int q = threadIdx.x; q < kBW * kKMax * 16; q += blockDim.x) {  // contiguous per (gap, run)
      const int k = (q >> 4) % kKMax, p = (q >> 4) / kKMax;
      const uint32_t v = Tl[p * kTs + k * 16 + (q & 15)];
      if (v) {
        atomicAdd(a.runt + (s_rs[p] + (int64_t)gb + g0 + p + s_roff[p] + k) * 16 + (q & 15), v);
        atomicMax(&Ml[p * kMs + k], (uint32_t)((q & 15) >> 2) + 1u);  // slot bi holds a base: M > bi
      }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < kBW * kKMax; q += blockDim.x) {
      const int k = q % kKMax, p = q / kKMax;
      const uint32_t m = Ml[p * kMs + k];
      if (m) atomicMax(a.M + s_rs[p] + (int64_t)gb + g0 + p + s_roff[p] + k, (int32_t)m);
    }
    __syncthreads();
    MPC_LSEG(6);
  }
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  // the per-read parts start at the first block that had no unit (rotated
  // block index), so they run beside the unit blocks instead of after them
  const int64_t fb = ((int64_t)blockIdx.x + gridDim.x - nunits % gridDim.x) % gridDim.x;
  const int64_t tid = fb * blockDim.x + threadIdx.x;
  // long insertions
  const int64_t nov = *a.ovf_cnt < (uint32_t)a.ovf_cap ? *a.ovf_cnt : a.ovf_cap;
  for (int64_t t = tid; t < nov; t += nthreads) {
    const Ovf o = a.ovf[t];
    const int64_t g = (int64_t)a.gbase[a.sample[o.read]] + o.gap;
    atomicMax(a.M + run_left(a.right_start, a.rsl, a.roff, a.vals_out, g, a.read_offset + o.read), o.len);
  }
  // upstream flanks (block-uniform trips: block_atomic_max synchronizes the block)
  for (int64_t r0 = fb * blockDim.x; r0 < a.N; r0 += nthreads) {
    const int64_t r = r0 + threadIdx.x;
    int64_t run = 0;
    int32_t L = 0;
    bool ok = false;
    if (r < a.N) {
      const int64_t ul = a.up_off[r + 1] - a.up_off[r];
      const int s = a.sample[r];
      const int ts = a.tstart[r];
      if (ul > 0 && ts >= 0 && ts <= a.n_of[s]) {
        const int64_t g = (int64_t)a.gbase[s] + ts;
        run = a.right_start[g + 1] > a.right_start[g]
                  ? run_left(a.right_start, a.rsl, a.roff, a.vals_out, g, a.read_offset + r)
                  : (int64_t)a.right_start[g] + g;
        L = ul > 0x7fffffff ? 0x7fffffff : (int32_t)ul;
        ok = true;
      }
    }
    block_atomic_max(a.M, run, L, ok, &s_key, &s_val);
  }
#ifdef MPC_STAMPS_LEFT
  MPC_LSEG(7);
  const int64_t gw = (int64_t)blockIdx.x * (UB / 64) + (threadIdx.x >> 6);
  if (lane() < kStampSeg && gw < kStampWaves) {
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < kStampSeg; ++k) v = lane() == k ? st_acc[k] : v;
    g_stamps[gw * kStampSeg + lane()] = v;
  }
#endif
}

}  // namespace

// Host side: K_left's arguments, geometry and launch
static LeftArgs left_args(const mpc_plan* p, const Dev& d) {
  LeftArgs a;
  a.up_off = d.up_off; a.sample = d.sample; a.tstart = d.tstart; a.n_of = d.n_of; a.gbase = d.gbase;
  a.bc = at<const int4>(p, mpc_plan::B_WBC); a.units = at<const int4>(p, mpc_plan::B_UNITS); a.status = d.status;
  a.ins_sorted = at<uint32_t>(p, mpc_plan::B_INSSORT); a.pg_list = at<uint32_t>(p, mpc_plan::B_PGLIST);
  a.bk_cnt = at<int32_t>(p, mpc_plan::B_BKCNT); a.bk_off = at<int32_t>(p, mpc_plan::B_BKOFF);
  a.rbase = at<int64_t>(p, mpc_plan::B_RBASE); a.pwork = at<const int4>(p, mpc_plan::B_WPARSE);
  a.N = d.N; a.read_offset = d.read_offset; a.ovf_cap = d.ovf_cap; a.nbs = p->nbmax;
  a.right_start = d.right_start; a.rsl = d.rsl; a.roff = d.roff; a.vals_out = d.vals_out; a.M = d.M; a.runt = d.runt;
  a.ovf = d.ovf; a.ovf_cnt = d.ovf_cnt;
  return a;
}

// K_left's geometry (planner: left_ub):
// two (1024-thread) or three (512-thread) resident blocks per CU
static int64_t left_grid(const mpc_plan* p) {
  return std::max<int64_t>(1, std::min<int64_t>(p->units_cap, p->left_ub == 512 ? 768 : 512));
}
static void launch_left(const mpc_plan* p, const Dev& d, hipStream_t st) {
  if (p->left_ub == 512) hipLaunchKernelGGL(K_left<512>, dim3(left_grid(p)), dim3(512), 0, st, left_args(p, d));
  else hipLaunchKernelGGL(K_left<kUB>, dim3(left_grid(p)), dim3(kUB), 0, st, left_args(p, d));
}
