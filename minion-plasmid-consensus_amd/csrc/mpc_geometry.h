// The contract between the host planner (mpc_plan.cpp) and the kernels
// (mpc_k_*.h, compiled as mpc_kernels.hip): the constants, sizing functions and plain structs both
// sides must agree on.  What a plan depends on is all here; the kernels keep
// what only they use.  No HIP header: this compiles under plain g++ as well as
// under hipcc.
#pragma once

#include <cstdint>

#include "mpc.h"

#if defined(__HIPCC__)
#define MPC_HD __host__ __device__
#else
#define MPC_HD
#endif

namespace mpc_geom {

// 32-bit coordinates and the 22-bit gap of the insertion event word bound the
// reference (mpc_k_common.h: kAdvCap, kNullGap)
constexpr int kMaxRefLen = (1 << 22) - 2;
constexpr int kBW = 64;             // gaps per insertion bucket (K_left workgroup)
static_assert(kBW <= 64 && (kBW & (kBW - 1)) == 0, "sorted insertion events hold the gap within its bucket in 6 bits");

struct Ovf {  // long insertion (len > kInsInline), tallied by K_flank
  int64_t off;  // absolute byte offset of the inserted bases in cs
  int32_t read;
  int32_t gap;  // local gap index (i), sample implied by read
  int32_t len;
  int32_t pad[3];
};

// A string Python's negative index wrap writes into an ODD position: with i in
// [-n, 0), obsarr[2 i] is obsarr[2 (n + i) + 1], the reference base n + i.  An
// upstream flank at tstart = i (:303) or a '+' at i (:81-87) is a LEFT string
// there, the downstream flank of a read ending at i (:323) a RIGHT string.
// K_parse lists them (rare: minimap2 never writes a negative start); the
// position's slot list is then replayed like a gap's (K_woprep, K_wocover,
// K_layout<true>, K_worows).
struct WoEv {
  int32_t g;     // global index of the odd position: gbase[s] + (n + i)
  int32_t read;  // local read
  int32_t len;   // '+': operand bytes (flanks: from the read's offsets)
  int32_t type;  // kWo*
  int64_t src;   // '+': absolute cs offset of the operand
};
struct WoPos {   // one odd position holding such strings
  int32_t g, beg, end;  // its events [beg, end) in the sorted list
  int32_t run0, nrun;   // its runs (LEFT events between consecutive RIGHT ones)
  int32_t lo, F, row0;  // replayed lo, slots, first row (K_layout<true>)
};
struct WoRun {
  int32_t M, R;         // longest LEFT string of the run / RIGHT string closing it
  int32_t hiR, loR;     // replayed hi seen by its LEFT events / lo seen by its RIGHT event
  uint32_t C[4];        // one-base LEFT writes of the reads covering the position (:79, :96)
};
constexpr int64_t kWoCapMax = 1 << 22;  // event list bound (the single-workgroup sort)
// What a shard sends of a WoEv (n_shards > 1, K_wopack): nothing in it points
// into the owner's buffers.  A flank's length comes from the owner's up_off /
// down_off, which no other shard holds, so it travels here.  Record 0 of the
// gathered list is a header: its g is the number of records behind it.
struct WoRec {
  int32_t g;      // as WoEv
  int32_t gread;  // global read: read_offset + local read (< 2^30)
  int32_t len;    // string length (flanks included)
  int32_t type;   // kWo*
  int32_t shard;  // the owner
  int32_t ev;     // index in the owner's WoEv list
};
static_assert(sizeof(WoRec) == 24, "exchanged as 6 int32 (mpc.h MPC_BUF_WRAP_REC)");
// this shard's records; all shards' records behind a header; per run "some
// read of this shard has a one-base write" (each starts 256-byte aligned)
MPC_HD inline int64_t wo_a256(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

constexpr int kPgEv = 64;                    // insertion events per page (256 B)
// page base (in pages) of parse workgroup wg: its events are at most half its
// cs bytes plus 3 per read (an insertion takes >= 2 cs bytes), i.e. at most
// bytes / 128 + 3 reads / 64 full pages, plus one partial page per bucket
MPC_HD inline int64_t parse_page_base(int64_t cs_rel, int64_t r, int64_t wg, int nbs) {
  return cs_rel / 128 + (3 * r) / 64 + wg * (int64_t)(nbs + 4);
}

// ---------------------------------------------------------------------------
// K_parse
// ---------------------------------------------------------------------------
constexpr int kSlots = 64;              // reads touching a window (slot 0 = read carried in)
constexpr int kMaxPW = 16;              // waves per workgroup (runtime: blockDim.x / 64)
constexpr int kMaxCh = MPC_PARSE_CHUNKS;  // read chunks per parse workgroup, taken dynamically by its waves

// units per window (tok list capacity): a 2 KiB window is cut early when it
// would hold more (LDS budget), smaller windows never hold more than WIN
template <int WIN> constexpr int tok_cap() { return WIN <= 1024 ? WIN : 1024; }

// Deferred placement (K_parse DP): insertion events are queued per wave in LDS
// (kDefQ entries) and placed 64 at a time, one per lane, instead of in every
// round that holds one (2 KiB windows, tally modes 1 and 3 with one
// substitution window, when the queues fit the LDS budget).
constexpr int kDefQ = 128;  // queue entries per wave (a power of 2, >= 127)
MPC_HD constexpr int defer_bytes(int nw) { return nw * kDefQ * 8; }
// Tally modes (bit TM) whose rounds find a unit's read base by an LDS round trip
// (slot base written by the read's start lane, read back by every lane) instead
// of a scalar pass over the round's read starts: short reads (C1 / C2) start
// several reads per round
#ifndef MPC_LDS_BASE_MODES
#define MPC_LDS_BASE_MODES 0x07
#endif
MPC_HD constexpr bool lds_base_rt(int tm) { return (MPC_LDS_BASE_MODES >> tm) & 1; }

template <int WIN, bool SV>              // SV: the read-base slots (lds_base modes)
struct alignas(16) WaveLds {            // per-wave LDS of K_parse
  int32_t s_val[SV ? kSlots : 0];       // read base: i = s_val + window prefix of advances
  int32_t s_ts[kSlots];                 // tstart (clamped to [MPC_TSTART_MIN, kICap])
  int32_t s_read[kSlots];               // local read index
  int32_t s_iend[kSlots];               // i_end | bit 30: read has a downstream flank
  int64_t s_end[kSlots];                // cs offset of the read's end
  uint8_t stage[WIN + 16];              // window bytes (+16: word reads past the end)
  uint8_t ra[WIN / 8];                  // read-start bits, bit = byte
  uint16_t tok[tok_cap<WIN>() + 2 + 64];  // unit starts in [P, C), then the sentinel C; bits 12-14: ':' prefix
                                        // operand length, bit 15: read start (+64: unconditional loads)
};

// Substitution events (tally mode 3, references too long for LDS substitution
// tallies): position within a kSubWin-position window << 2 | code, per wave and
// window in the wave's region [(cs_off[ra] - cs_base) / kSubEvBytes + 2 ra, ...)
// of window w's slice; K_subs tallies them per window in LDS.  A '*' token takes
// at least 2 cs bytes ('*' and the base it writes, :96 -- minimap2 writes 3,
// "*ag", but "*a" is valid: round 5 sized the regions by 3 bytes, which two-byte
// tokens overran)
constexpr int kSubWinBits = 14, kSubWin = 1 << kSubWinBits, kMaxSubWins = 4;
constexpr int kSubEvBytes = 2;
constexpr int kSubsWG = 32;  // parse workgroups per K_subs block, at most

MPC_HD inline int parse_hl_words(int n) { return (n + 1 + 31) / 32; }
// the chunk table (cs offset, read), the chunk counter and the page counter
MPC_HD constexpr int parse_misc_bytes() { return (kMaxCh + 2) * 8 + (kMaxCh + 4) * 4 + 16; }
static_assert(parse_misc_bytes() % 16 == 0 && kMaxCh % 4 == 0, "parse LDS misc area alignment");
template <int WIN>
// position tallies of K_parse: 0 = global atomics, 4 = global atomics AND the
// LEFT bitmap / insertion-bucket counters / event-sort cursors in HBM (references
// too long for any LDS mode, up to kMaxRefLen), 1 = LDS, 12 B per position
// (sub 4 x u16, depth decrements | increments u16), 2 = LDS, 10 B per position
// (the depth difference as one biased 16-bit half), 3 = depth differences in
// LDS (2 B per position), substitutions global: references up to ~40 kb
MPC_HD inline int parse_lds_bytes(int n_max, int tm, int nbmax, int nw) {
  const int wl = lds_base_rt(tm) ? (int)sizeof(WaveLds<WIN, true>) : (int)sizeof(WaveLds<WIN, false>);
  if (tm == 4) return nw * wl + parse_misc_bytes();  // per-gap state in HBM
  const int tallies = tm == 0 ? 0 : tm == 1 ? 12 * (n_max + 1) : tm == 2 ? 8 * (n_max + 1) + 4 * ((n_max + 2) / 2)
                                                                 : 4 * ((n_max + 2) / 2);
  const int buckets = 16 * nbmax + 4;  // epilogue: counts, cursors, chunk counts, chunk offsets
  return nw * wl + parse_misc_bytes() + 4 * parse_hl_words(n_max) + 4 * nbmax +
         (tallies > buckets ? tallies : buckets);
}

// reads per parse workgroup that keep the 16-bit LDS tallies exact: a read adds
// at most 2 to a position's depth counters; modes 2 / 3 keep the depth
// difference as one half biased by 0x8000 (|sum| <= 2 * 16383 < 0x8000),
// mode 1 keeps decrements and increments apart (2 * 32767 < 2^16)
MPC_HD constexpr int64_t wg_reads_cap(int tm) { return tm == 2 || tm == 3 ? 16383 : 32767; }

// ---------------------------------------------------------------------------
// The kernels behind the parse: block shapes the planner sizes buffers by
// ---------------------------------------------------------------------------
constexpr int kRS = 1024;                       // threads (= reads) of a K_rsplit / K_rsort block
constexpr int64_t kRsortMultiBlocks = 512;      // K_rsplit blocks (of 1024 reads) above which the plan takes the
                                                // multi-workgroup sort (K_rscan / K_rscatter / K_rsegsort)
constexpr int kScanPer = 8;                     // gaps per thread of K_rscan
constexpr int kScanBlk = 1024 * kScanPer;       // gaps per K_rscan block
constexpr int kUB = 1024;             // threads of K_ins and of K_left's default geometry
constexpr int kEPT = 16;         // events per thread per unit (loads batched)
#ifndef MPC_LAYOUT_GAPS
#define MPC_LAYOUT_GAPS 256
#endif
constexpr int kGB = MPC_LAYOUT_GAPS;  // gaps per K_layout block (fewer blocks: a shorter look-back chain)
constexpr int kKB = 1024;  // rows per K_select block (4 per thread)

}  // namespace mpc_geom
