// What every stage of the pileup path (mpc_k_*.h, one translation unit:
// mpc_kernels.hip) shares: the error flags, the 32-bit coordinate caps, the
// decoupled look-back and the chained scan of K_runs / K_layout / K_select, the
// insertion event word, Dev
// (the device-side views of a plan) with its host filler plan_dev, the codes of
// a written cs byte, wave idioms and the stamp macros of the diagnostic builds.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mpc.h"
#include "mpc_device.h"
#include "mpc_geometry.h"
#include "mpc_plan.h"

// (one translation unit: every stage header sees these through this one)
using namespace mpc;
using namespace mpc_geom;

namespace {

constexpr uint32_t DE_OP = MPC_DE_OP, DE_VALUE = MPC_DE_VALUE, DE_INDEX = MPC_DE_INDEX,
                   DE_KEY = MPC_DE_KEY, DE_CAP = MPC_DE_CAPACITY, DE_INTERNAL = MPC_DE_INTERNAL,
                   DE_UNSUP = MPC_DE_UNSUPPORTED;

constexpr int kBlk = 1024;          // cs bytes staged per wave iteration (64 lanes x 16 B)
constexpr int kInsInline = 4;       // insertions up to this length travel as one event word
// 32-bit coordinates: a unit's advances are clamped at kAdvCap > n (a clamped
// advance still leaves i past the end).  An advance of 2^22 takes at least 8 cs
// bytes (':' + 7 digits; a '-' advances by its operand bytes), so a window's
// prefix of advances stays below (WIN / 8) * 2^22 <= 2^30 at the largest
// window, and a coordinate (a read base <= kICap plus that prefix plus one
// unit's advance) below 2^31 (static_assert below).  The insertion event word
// holds the gap in 22 bits (kNullGap).  Hence kMaxRefLen (mpc_geometry.h).
constexpr int kAdvCap = 1 << 22;    // > any reference length: a clamped advance keeps i past the end
constexpr int kICap = 1 << 28;      // saturation of the running coordinate i
constexpr int kMaxWin = 2048;       // largest parse window (bytes)
static_assert((int64_t)kICap + (int64_t)(kMaxWin / 8) * kAdvCap + 2 * (int64_t)kAdvCap < (int64_t)INT32_MAX,
              "32-bit coordinates: read base + window prefix of advances + one unit");
static_assert((int64_t)MPC_TSTART_MIN - (int64_t)(kMaxWin / 8) * kAdvCap > (int64_t)INT32_MIN,
              "32-bit coordinates below 0 (negative target starts)");
constexpr int kKMax = 8;            // runs per gap tallied in K_left's LDS (others go to HBM)
constexpr uint32_t kNullGap = 0x3fffffu;
// decoupled look-back status words (K_layout, K_select): flag in bits 62-63
// (1 = a block's own sum, 2 = its inclusive prefix), the launch epoch in bits
// 32-61, the 32-bit value below
constexpr uint64_t kSelAgg = 1ull << 62, kSelPre = 2ull << 62, kSelTag = 0x3fffffffull << 32;

// Decoupled look-back, called by ONE wave of block b: publishes the block's NV
// values (own[k], flag 1), sums its predecessors' values back to the nearest
// inclusive prefix, publishes its own inclusive prefix (flag 2) and returns the
// exclusive prefixes in pre[k].  Block b's NV words are st[NV*b .. NV*b+NV-1]; a
// predecessor counts once all its words carry this launch's tag and the same
// flag.  Each step reads 64 predecessors, one per lane (wider steps measured
// the same: DESIGN.md §7, dropped variants).  Blocks are dispatched in index
// order, so the blocks waited on are running or done; the spin is bounded
// anyway (DE_INTERNAL).
template <int NV>
__device__ void lookback(uint64_t* st, int64_t b, uint64_t tag, const int32_t* own, int64_t* pre, uint32_t* flags) {
  const int l = lane();
  if (l == 0)
    for (int k = NV - 1; k >= 0; --k)
      __hip_atomic_store(st + NV * b + k, (b == 0 ? kSelPre : kSelAgg) | tag | (uint32_t)own[k], __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  int64_t acc[NV];
  for (int k = 0; k < NV; ++k) acc[k] = 0;
  int spins = 0;
  for (int64_t j0 = b - 1; j0 >= 0;) {
    uint64_t x[NV];
    const int64_t j = j0 - l;  // distance l; before block 0: prefixes of 0
#pragma unroll
    for (int k = 0; k < NV; ++k)
      x[k] = j >= 0 ? __hip_atomic_load(st + NV * j + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (kSelPre | tag);
    // every predecessor up to the nearest prefix must be ready
    bool ready = (x[0] & kSelTag) == tag && (x[0] >> 62) != 0;
#pragma unroll
    for (int k = 1; k < NV; ++k) ready = ready && (x[k] & kSelTag) == tag && (x[k] >> 62) == (x[0] >> 62);
    const bool is_pre = (x[0] >> 62) == 2;
    const uint64_t rdy = ballot(ready), pfx = ballot(ready && is_pre);
    const uint64_t need = pfx ? (pfx & (0 - pfx)) * 2 - 1 : ~0ull;
    if ((rdy & need) != need) {
      if (++spins > (1 << 22)) {  // never expected: in-order dispatch
        if (l == 0) atomicOr(flags, (uint32_t)MPC_DE_INTERNAL);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] += wave_sum(((need >> l) & 1ull) ? (int32_t)(uint32_t)x[k] : 0);
    if (pfx != 0) break;
    j0 -= 64;
  }
  if (l == 0 && b > 0)
    for (int k = NV - 1; k >= 0; --k)
      __hip_atomic_store(st + NV * b + k, kSelPre | tag | (uint32_t)(int32_t)(acc[k] + own[k]), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  for (int k = 0; k < NV; ++k) pre[k] = acc[k];
}

// The chained scan of K_runs, K_layout and K_select, called by every thread of
// block b: block_scan, then wave 0 chains the block's totals (lookback, tagged
// with the launch epoch) and broadcasts the exclusive prefixes through s_pre
// (NV words of LDS).  Per value: incl = the thread's inclusive prefix within the
// block, total = the block's sum, pre = the sum of the blocks before.  Two
// barriers; s_w and s_pre as block_scan's s_w (one call per launch today).
template <int NW, int NV>
__device__ __forceinline__ void chain_scan(uint64_t* st, int64_t b, uint32_t epoch, const int (&v)[NV], int (&incl)[NV],
                                           int (&total)[NV], int64_t (&pre)[NV], int32_t (*s_w)[NW], int64_t* s_pre,
                                           uint32_t* flags) {
  block_scan<NW, NV>(v, incl, total, s_w);
  if (threadIdx.x < 64) {
    int64_t p[NV];
    lookback<NV>(st, b, (uint64_t)(epoch & 0x3fffffffu) << 32, total, p, flags);
    if (lane() == 0)
      for (int k = 0; k < NV; ++k) s_pre[k] = p[k];
  }
  __syncthreads();
  for (int k = 0; k < NV; ++k) pre[k] = s_pre[k];
}

// WoEv.type of a string in a wrapped odd position (the records: mpc_geometry.h)
enum { kWoUp = 0, kWoIns = 1, kWoDown = 2 };  // (order within one read: upstream, cs, downstream)

// Insertion events (what K_left reads): 4 bytes, bases (8 bits, 2 per base in
// string order) | (len-1) << 8 | gap within its kBW-gap bucket << 10 | read
// relative to the parse workgroup's first read << 16 (< 2^15: wg_reads_cap);
// bit 31 clear.  The bucket and the workgroup are implied by the PAGE the
// event lies in: K_parse places every event once, into 64-event pages of its
// (workgroup, bucket), allocated as they fill (parse_place_event); the
// epilogue lists every bucket's pages, all full but the last (pg_list).
// (kPgEv events per page, parse_page_base: mpc_geometry.h)
constexpr int kPgBits = 12;                  // bucket word: page << 12 | fill
constexpr uint32_t kPgNone = 0xFFFFFu;       // page field of a bucket with no page yet
constexpr uint32_t kPgOvf = kPgNone - 1u;    // ... of a bucket whose workgroup ran out of pages (DE_INTERNAL)
constexpr uint32_t kPgInit = (kPgNone << kPgBits) | (uint32_t)kPgEv;  // first event opens a page
constexpr uint32_t kPgMark = 0xFFFFFFFFu;    // pg_own of a bucket's last page (placed by the epilogue)
static_assert(kPgEv + 1024 < (1 << kPgBits), "fill field: a full page plus every thread of a block waiting");
__device__ __forceinline__ uint32_t ins_word(int gap, int len, uint32_t bases, int rel_read) {
  return bases | ((uint32_t)(len - 1) << 8) | (((uint32_t)gap % (uint32_t)kBW) << 10) | ((uint32_t)rel_read << 16);
}

struct Dev {  // device-side views of the plan for the small kernels (passed by value)
  const uint8_t* ref; const int64_t* ref_off;
  const uint8_t* cs; const int64_t* cs_off;
  const int32_t* tstart;
  const uint8_t* up; const int64_t* up_off;
  const uint8_t* down; const int64_t* down_off;
  const int32_t* sample;
  int64_t N, Ng, read_offset, cs_base;
  int32_t S, G;
  const int32_t* n_of; const int32_t* gbase;
  uint32_t* status;
  int32_t* i_end;
  Ovf* ovf; uint32_t* ovf_cnt; int64_t ovf_cap;
  uint32_t* hasleft;                 // bitmap over gaps
  int32_t* maxR;
  uint32_t* keys_in; int32_t* vals_in; uint32_t* keys_out; int32_t* vals_out;
  uint32_t* keys_tmp; int32_t* vals_tmp; int32_t* bcnt; int32_t* bpre;  // K_rsplit -> K_rsort
  int32_t* gcnt; int32_t* kslot;     // multi-workgroup sort: [G+1] mixed events per gap, [N] slot in its gap
  int32_t* rsflag;                   // [4] its path word, scan partials follow (K_rscan)
  int32_t* rlen;                     // [Ng] downstream length by global read
  int32_t* rpos;                     // [N] local read -> position of its mixed RIGHT event in the sorted list
  int32_t* right_start;              // [G+1] mixed RIGHT events (all shards) with gap < g
  int32_t* rsl;                      // [G+1] the same over this shard's sorted list (== right_start on 1 GPU)
  int32_t* roff;                     // [G+1] mixed RIGHT events at gap g on lower shards
  int32_t* rcnt;                     // [G] this shard's mixed RIGHT events per gap (exchange)
  const int32_t* rcnt_all;           // [n_shards][G] all shards' counts (exchange)
  int32_t shard, n_shards;
  int32_t* diff;                     // [G]
  uint32_t* sub;                     // [G][4]
  int32_t* M;                        // [Ng+G] per run: longest LEFT string
  int32_t* runR;                     // [Ng+G] per run: length of the RIGHT string closing it
  int32_t* hiR; int32_t* loR;        // [Ng+G] per run: hi seen by its LEFT events, lo seen by its RIGHT event
  int32_t* lo_f; int32_t* rowcnt; int32_t* row_base;
  int32_t* bsum;                     // [2 * ceil(G / kGB)] x 8 B: K_layout's look-back words (rows, diff)
  uint32_t* rows; uint8_t* meta; int64_t row_cap;
  uint32_t* runt;                    // [Ng+G][4][4] per run: inline insertion bases by slot from the right end
  uint32_t* res; int32_t* keep; int32_t* ksum; uint32_t* calls; int32_t* ncalls; uint32_t* maxdepth;
  int32_t* srow;                     // [S] first row of every sample (K_layout)
  // strings in wrapped odd positions (negative starts; wo_cap 0: none planned)
  WoEv* wo; uint64_t* wo_key; uint32_t* wo_idx; int32_t* wo_erun; WoPos* wo_pos; WoRun* wo_run;
  int64_t wo_cap;                    // list capacity
  // n_shards > 1 with negative starts (else null): the three exchange buffers
  // (wo_rec, wo_all, wo_cov below), laid out one after the other.  ONE pointer,
  // in the place of a size no kernel read: Dev keeps its size and offsets, so
  // the kernels that know nothing of this are compiled to what they were.
  uint8_t* wo_x;
  double mdf, gtf;
};
static_assert(sizeof(void*) == sizeof(int64_t), "Dev layout");
// the three exchange buffers behind wo_x (each starts 256-byte aligned: wo_a256)
__device__ __forceinline__ WoRec* wo_rec(const Dev& d) { return reinterpret_cast<WoRec*>(d.wo_x); }
__device__ __forceinline__ const WoRec* wo_all(const Dev& d) {
  return reinterpret_cast<const WoRec*>(d.wo_x + wo_a256(d.wo_cap * (int64_t)sizeof(WoRec)));
}
__device__ __forceinline__ int32_t* wo_cov(const Dev& d) {
  return reinterpret_cast<int32_t*>(d.wo_x + wo_a256(d.wo_cap * (int64_t)sizeof(WoRec)) +
                                    wo_a256((d.wo_cap + 1) * (int64_t)sizeof(WoRec)));
}

// Dict code of a written base after .upper() (:87, :96): A0 T1 C2 G3, -1 if not ACGT.
// (c|0x20) maps exactly {A,a}->a, {C,c}->c, {G,g}->g, {T,t}->t; h=(lc>>1)&3 is a
// perfect hash a0 c1 t2 g3, bit-swapped into dict order.
__device__ __forceinline__ int code_upper(uint32_t c) {
  const uint32_t lc = c | 0x20u;
  const uint32_t h = (lc >> 1) & 3u;
  const uint32_t expect = (0x67746361u >> (8 * h)) & 0xffu;
  const int code = (int)(((h & 1u) << 1) | (h >> 1));
  return lc == expect ? code : -1;
}

// special-character bits of a lane's 16 staged bytes, restricted to [lo, hi)
__device__ __forceinline__ uint32_t special_mask16(uint4 v, int lo, int hi) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    const bool sp = (c == 0x3Au) | (c == 0x5Au) | (((c - 0x2Au) <= 3u) & (c != 0x2Cu));  // : Z * + -
    m |= (uint32_t)sp << k;
  }
  hi = hi < 0 ? 0 : (hi > 16 ? 16 : hi);
  lo = lo < 0 ? 0 : (lo > 16 ? 16 : lo);
  return m & ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// x * 2561 (= 2^11 + 2^9 + 1) as two full-rate shift-adds; the compiler would
// fold the shifts back into the quarter-rate v_mul_lo_u32
__device__ __forceinline__ uint32_t mul2561(uint32_t x) {
  uint32_t y, z;
  asm("v_lshl_add_u32 %0, %1, 9, %1" : "=v"(y) : "v"(x));
  asm("v_lshl_add_u32 %0, %1, 11, %2" : "=v"(z) : "v"(x), "v"(y));
  return z;
}

__device__ __forceinline__ int64_t readlane64(int64_t x, int j) {
  const int lo = __builtin_amdgcn_readlane((int)(uint32_t)x, j);
  const int hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)x >> 32), j);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int lanes_below(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Diagnostic build only (-DMPC_STAMPS, scripts/kparse_stamps.py): s_memtime
// stamps around K_parse's segments, summed per wave in scalar registers and
// stored once per wave into g_stamps (nothing else reads them).  The product
// build compiles none of this.
// -DMPC_STAMPS_LEFT: the same stamps around K_left's segments instead
// (scripts/kleft_stamps.py).
#if defined(MPC_STAMPS) || defined(MPC_STAMPS_LEFT)
constexpr int kStampSeg = 8, kStampWaves = 1 << 16;
__device__ uint64_t g_stamps[kStampWaves * kStampSeg];
#define MPC_STAMP(t)                                                                   \
  do {                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                               \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");        \
    __builtin_amdgcn_sched_barrier(0);                                               \
  } while (0)
#define MPC_SEG_ALWAYS(k)           \
  do {                              \
    uint64_t t_;                    \
    MPC_STAMP(t_);                  \
    st_acc[k] += t_ - st_prev;      \
    st_prev = t_;                   \
  } while (0)
#endif
#ifdef MPC_STAMPS
#define MPC_SEG(k) MPC_SEG_ALWAYS(k)
#else
#define MPC_SEG(k) do {} while (0)
#endif
#ifdef MPC_STAMPS_LEFT
#define MPC_LSEG(k) MPC_SEG_ALWAYS(k)
#else
#define MPC_LSEG(k) do {} while (0)
#endif

}  // namespace

// Host side: the buffers of a bound plan (mpc_plan.h)
template <class T>
static T* at(const mpc_plan* p, int b) { return reinterpret_cast<T*>(p->ws + p->off[b]); }

// the device-side views of a bound plan
static Dev plan_dev(const mpc_plan* p) {
  using P = mpc_plan;
  const mpc_input& in = p->in;
  Dev d{};
  d.ref = in.ref; d.ref_off = in.ref_off; d.cs = in.cs; d.cs_off = in.cs_off; d.tstart = in.tstart;
  d.up = in.up; d.up_off = in.up_off; d.down = in.down; d.down_off = in.down_off; d.sample = in.sample;
  d.N = p->N; d.Ng = p->Ng; d.read_offset = in.read_offset; d.cs_base = in.cs_base; d.S = p->S; d.G = (int32_t)p->G;
  d.n_of = at<int32_t>(p, P::B_NOF); d.gbase = at<int32_t>(p, P::B_GBASE);
  d.status = at<uint32_t>(p, P::B_STATUS); d.i_end = at<int32_t>(p, P::B_IEND);
  d.ovf = at<Ovf>(p, P::B_OVF); d.ovf_cnt = at<uint32_t>(p, P::B_OVFCNT); d.ovf_cap = p->ovf_cap;
  d.hasleft = at<uint32_t>(p, P::B_HASLEFT); d.maxR = at<int32_t>(p, P::B_MAXR);
  d.keys_in = at<uint32_t>(p, P::B_KIN); d.vals_in = at<int32_t>(p, P::B_VIN);
  d.keys_out = at<uint32_t>(p, P::B_KOUT); d.vals_out = at<int32_t>(p, P::B_VOUT);
  d.keys_tmp = at<uint32_t>(p, P::B_KTMP); d.vals_tmp = at<int32_t>(p, P::B_VTMP);
  d.bcnt = at<int32_t>(p, P::B_BCNT); d.bpre = at<int32_t>(p, P::B_BPRE);
  d.gcnt = p->rsort_multi ? at<int32_t>(p, P::B_GCNT) : nullptr;
  d.kslot = p->rsort_multi ? at<int32_t>(p, P::B_KSLOT) : nullptr;
  d.rsflag = p->rsort_multi ? at<int32_t>(p, P::B_RSFLAG) : nullptr;
  d.rlen = at<int32_t>(p, P::B_RLEN); d.rpos = at<int32_t>(p, P::B_RPOS); d.right_start = at<int32_t>(p, P::B_RSTART);
  d.rsl = at<int32_t>(p, P::B_RSLOC); d.roff = at<int32_t>(p, P::B_ROFF); d.rcnt = at<int32_t>(p, P::B_RCNT);
  d.rcnt_all = at<int32_t>(p, P::B_RCNTALL); d.shard = p->shard; d.n_shards = p->n_shards;
  d.diff = at<int32_t>(p, P::B_DIFF); d.sub = at<uint32_t>(p, P::B_SUB);
  d.M = at<int32_t>(p, P::B_M); d.runR = at<int32_t>(p, P::B_RUNR); d.runt = at<uint32_t>(p, P::B_RUNT);
  d.hiR = at<int32_t>(p, P::B_HIR); d.loR = at<int32_t>(p, P::B_LOR);
  d.lo_f = at<int32_t>(p, P::B_LOF); d.rowcnt = at<int32_t>(p, P::B_ROWCNT); d.row_base = at<int32_t>(p, P::B_ROWBASE);
  d.bsum = at<int32_t>(p, P::B_BSUM);
  d.rows = at<uint32_t>(p, P::B_ROWS); d.meta = at<uint8_t>(p, P::B_META);
  d.row_cap = p->row_cap;
  d.res = at<uint32_t>(p, P::B_RES); d.keep = at<int32_t>(p, P::B_KEEP); d.ksum = at<int32_t>(p, P::B_KSUM);
  d.calls = at<uint32_t>(p, P::B_CALLS); d.ncalls = at<int32_t>(p, P::B_NCALLS); d.maxdepth = at<uint32_t>(p, P::B_MAXD);
  d.srow = at<int32_t>(p, P::B_SROW);
  d.wo = at<WoEv>(p, P::B_WOEV); d.wo_key = at<uint64_t>(p, P::B_WOKEY); d.wo_idx = at<uint32_t>(p, P::B_WOIDX);
  d.wo_erun = at<int32_t>(p, P::B_WOERUN); d.wo_pos = at<WoPos>(p, P::B_WOPOS); d.wo_run = at<WoRun>(p, P::B_WORUN);
  d.wo_cap = p->wo_cap;
  if (p->n_shards > 1 && p->wo_cap > 0) d.wo_x = at<uint8_t>(p, P::B_WOREC);  // (B_WOALL, B_WOCOV follow: wo_all(), wo_cov())
  return d;
}

static inline unsigned nblk(int64_t n, int b = 256) {
  int64_t g = (n + b - 1) / b;
  if (g < 1) g = 1;
  if (g > 65535 * 16) g = 65535 * 16;
  return (unsigned)g;
}
