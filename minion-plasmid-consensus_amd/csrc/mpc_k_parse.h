// The parse phase (mpc_parse): K_parse replaces Step 4 of the reference (the
// cs tokenizer :285-323 and processOperation :74-104); what it leaves behind:
// mpc_kernels.hip's overview.  K_subs / K_subsum (tally mode 3): substitution
// events -> tallies.
#pragma once

#include <type_traits>

#include "mpc_k_common.h"

namespace {

// (kSlots, kMaxPW, kMaxCh, tok_cap, WaveLds and the LDS sizing: mpc_geometry.h)
constexpr uint32_t kFar = 0x7fffu;      // sentinel: the window's only token ends beyond the window

// Every round tries the fast decode first, in every tally mode (the empty
// tokens "Z" ":" that start each read decode as no-ops on it).
// Tally mode 3 with ONE substitution window (references up to 16384 bases:
// C3, C4): the K_parse<3, WIN, NK, true> instantiation takes the round's
// substitution slots from a wave-uniform count -- no loop over windows, no
// count kept in a VGPR lane (C3 -1.3 to -1.9 %, C4 -2.2 %); plans with more
// windows (C5) keep the loop, in a kernel that compiles nothing else.
// Deferred placement (K_parse DP, kDefQ) and the tally modes that find a
// unit's read base by an LDS round trip (MPC_LDS_BASE_MODES): mpc_geometry.h.
// The variants measured against these and dropped: DESIGN.md §7.
template <int TM> constexpr bool lds_base() { return (MPC_LDS_BASE_MODES >> TM) & 1; }

struct ParseArgs {  // slim argument block (no SGPR spills)
  const uint8_t* cs; const int64_t* cs_off; const int32_t* tstart;
  const int64_t* up_off; const int64_t* down_off; const int32_t* n_of; const int32_t* gbase;
  const int4* work;  // per workgroup: {sample, first read, end read, chunks}
  const int32_t* wave_tab;  // per workgroup: kMaxCh + 1 read boundaries of its chunks (planner: by cs bytes)
  int64_t cs_base, ovf_cap, read_offset, n_reads;
  int32_t nbs;       // bucket slots per parse workgroup (max buckets)
  int32_t* i_end; uint32_t* ins_sorted; uint32_t* pg_own; uint32_t* pg_list; int32_t* bk_cnt; int32_t* bk_off;
  int64_t* rbase;
  uint32_t* bk_cur;  // tally mode 4 only: per (workgroup, bucket) page words in HBM
  Ovf* ovf; uint32_t* ovf_cnt; uint32_t* hasleft; uint32_t* status;
  int32_t* diff; uint32_t* sub;
  // tally mode 3: substitutions as 2-byte events per (wave, position window),
  // tallied by K_subs (0 windows: global atomics)
  uint16_t* subev; uint32_t* subev_cnt; int64_t subev_cap; int32_t sub_wins;
  WoEv* wo; int64_t wo_cap;  // strings written into wrapped odd positions (negative starts only)
  int32_t defer_off;  // deferred placement (K_parse DP): LDS byte offset of the per-wave event queues
};

// (substitution events, the tally modes' LDS bytes and the reads-per-workgroup
// cap of the 16-bit tallies: mpc_geometry.h)

struct TokInfo { int adv; int kind; uint32_t pay; uint32_t err; };

// Semantics of one token that do not depend on its coordinate, operand read
// from HBM: the slow path for rare tokens (a token longer than the window,
// long insertions / substitution operands, ':' operands that are not 1-4 plain digits).
__device__ __noinline__ TokInfo analyze_long(const uint8_t* cs, int64_t s, int64_t e, bool is_last) {
  TokInfo r{0, 0, 0u, 0u};
  const uint32_t op = cs[s];
  if (!is_special(op)) { r.err = DE_OP; return r; }
  const int64_t olen = e - s - 1;
  if (!(olen > 0 || is_last)) return r;
  if (op == ':') {
    int64_t vv = 0;
    if (!py_int(cs + s + 1, olen, &vv)) r.err |= DE_VALUE;
    else r.adv = vv <= 0 ? 0 : (vv < kAdvCap ? (int)vv : kAdvCap);
    r.kind = r.adv > 0 ? 1 : 0;
  } else if (op == '*') {
    if (olen == 0) { r.err |= DE_INDEX; return r; }
    const int cd = code_upper(cs[e - 1]);
    if (cd < 0) r.err |= DE_KEY;
    r.pay = (uint32_t)(cd & 3); r.adv = 1; r.kind = 2;
  } else if (op == '+') {
    if (olen == 0) return r;
    bool ok = true;
    for (int64_t x = s + 1; x < e; ++x) {
      const int cd = code_upper(cs[x]);
      ok &= cd >= 0;
      // an inline insertion (<= kInsInline bases) travels with its bases in the
      // event word, base k at bits 2k (the window decode's pk): a short '+'
      // gets here behind a ':' prefix that is not plain digits (": 12+ac")
      if (x - s - 1 < kInsInline) r.pay |= (uint32_t)(cd & 3) << (2 * (x - s - 1));
    }
    if (!ok) r.err |= DE_KEY;
    r.kind = 3;
  } else if (op == '-') {
    r.adv = olen < kAdvCap ? (int)olen : kAdvCap;
    r.kind = olen > 0 ? 4 : 0;
  }
  return r;
}

// first special character in cs[x0, bound) (x0 16-aligned), else bound: all lanes, 1 KiB per step.
// Inlined: a call in the window loop pins the values live across it to the
// callee-saved registers (K_parse<3, 2048> 127 -> 120 VGPRs inlined)
__device__ __forceinline__ int64_t scan_special_wave(const uint8_t* cs, int64_t x0, int64_t bound) {
  for (int64_t x = x0; x < bound; x += 1024) {
    const int64_t y = x + 16 * lane();
    uint32_t m = 0;
    if (y < bound) {
      const uint4 v = *reinterpret_cast<const uint4*>(cs + y);
      const int64_t lim = bound - y;
      m = special_mask16(v, 0, lim > 16 ? 16 : (int)lim);
    }
    const uint64_t b = ballot(m != 0);
    if (b) {
      const int f = __ffsll((unsigned long long)b) - 1;
      const uint32_t mf = (uint32_t)__builtin_amdgcn_readlane((int)m, f);
      return x + 16 * f + __ffs(mf) - 1;
    }
  }
  return bound;
}

__device__ __forceinline__ void push_ovf(const ParseArgs& a, int64_t off, int64_t r, int gap, int len) {
  const uint32_t slot = atomicAdd(a.ovf_cnt, 1u);
  if ((int64_t)slot < a.ovf_cap) {
    Ovf o; o.off = off; o.read = (int32_t)r; o.gap = gap; o.len = len;
    o.pad[0] = o.pad[1] = o.pad[2] = 0;
    a.ovf[slot] = o;
  } else {
    atomicOr(&a.status[MPC_ST_FLAGS], DE_INTERNAL);
  }
}

// a string into a wrapped odd position (WoEv); returns the data error to flag:
// none, or DE_UNSUP when the plan has no room (declared no negative starts,
// several shards)
__device__ __forceinline__ uint32_t push_wo(const ParseArgs& a, int g, int64_t r, int type, int len, int64_t src) {
  if (a.wo_cap <= 0) return DE_UNSUP;
  const uint32_t slot = atomicAdd(&a.status[MPC_ST_WRAP_EVENTS], 1u);
  if ((int64_t)slot >= a.wo_cap) return DE_UNSUP;
  WoEv e;
  e.g = g; e.read = (int32_t)r; e.len = len; e.type = type; e.src = src;
  a.wo[slot] = e;
  return 0u;
}

__device__ __forceinline__ void flag_read(const ParseArgs& a, uint32_t err, int64_t r) {
  atomicOr(&a.status[MPC_ST_FLAGS], err);
  atomicMin(&a.status[MPC_ST_FIRST_READ], (uint32_t)r);
}

// Per-byte character classes of a lane's staged bytes, SWAR per 32-bit word
// (no per-byte compares: those pin 2 SGPRs per byte): bit k of sp = byte k is
// special (: Z * + -), of cm = ':'.  The ops that may follow a ':' prefix in
// one unit are sp & ~cm ('Z' included: a unit ':n' + 'Z' decodes as the two
// tokens it is, so only two masks are compacted per word).
__device__ __forceinline__ uint32_t byte_hits(uint32_t w, uint32_t pat) {  // bit 7 of byte k: byte k == pat's
  const uint32_t t = w ^ pat;
  return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
}
__device__ __forceinline__ uint32_t hit_nibble(uint32_t z) {  // bits 7, 15, 23, 31 -> bits 0..3
  z >>= 7;
  z |= z >> 7;
  z |= z >> 14;
  return z & 0xfu;
}
// Special bytes by two v_perm table lookups per word: a byte c = (hi, lo) is
// special iff lo >= 8, c < 0x80 and bit hi of T1[lo & 7] is set -- T1[2] (lo
// 0xA) = {2, 3, 5} for '*' ':' 'Z', T1[3] (lo 0xB) = {2} for '+', T1[5] (lo
// 0xD) = {2} for '-' -- i.e. T1[lo & 7] & (1 << hi) != 0, the second lookup
// giving 1 << (hi & 7).  That AND is 8 exactly for ':' (hi 3), so both masks
// come from one pair of lookups.
template <int NW>
__device__ __forceinline__ void word_classes(const uint32_t* w, uint32_t* sp, uint32_t* cm) {
  uint32_t s_ = 0, c_ = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const uint32_t c = w[i];
    const uint32_t t1 = __builtin_amdgcn_perm(0x00000400u, 0x042C0000u, c & 0x07070707u);
    const uint32_t t2 = __builtin_amdgcn_perm(0x80402010u, 0x08040201u, (c >> 4) & 0x07070707u);
    const uint32_t y = t1 & t2;                   // per byte: 0, or the single bit 1 << hi (<= 0x20)
    const uint32_t ok = (c << 4) & ~c;            // bit 7 of a byte: lo >= 8 and c < 0x80
    const uint32_t zs = (y + 0x7F7F7F7Fu) & ok & 0x80808080u;  // bit 7: y != 0 (no carry out: y <= 0x20)
    const uint32_t zc = (y << 4) & ok & 0x80808080u;           // bit 7: y == 8 (':')
    s_ |= hit_nibble(zs) << (4 * i);
    c_ |= hit_nibble(zc) << (4 * i);
  }
  *sp = s_;
  *cm = c_;
}
struct alignas(16) U8x32 { uint4 a, b; };  // a lane's 32 bytes of a 2 KiB window
__device__ __forceinline__ void chunk_classes(uint2 v, uint32_t* sp, uint32_t* cm) {
  const uint32_t w[2] = {v.x, v.y};
  word_classes<2>(w, sp, cm);
}
__device__ __forceinline__ void chunk_classes(uint4 v, uint32_t* sp, uint32_t* cm) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  word_classes<4>(w, sp, cm);
}
__device__ __forceinline__ void chunk_classes(U8x32 v, uint32_t* sp, uint32_t* cm) {
  const uint32_t w[8] = {v.a.x, v.a.y, v.a.z, v.a.w, v.b.x, v.b.y, v.b.z, v.b.w};
  word_classes<8>(w, sp, cm);
}
// bits [0, x) set, x in [0, 32]
__device__ __forceinline__ uint32_t lowmask(int x) { return x >= 32 ? 0xffffffffu : (1u << x) - 1u; }
// a lane's CH boundary / read-start bits in the per-wave LDS bit arrays
template <int CH>
__device__ __forceinline__ void put_lane_bits(uint8_t* arr, int l, uint32_t v) {
  if (CH == 32) reinterpret_cast<uint32_t*>(arr)[l] = v;
  else if (CH == 16) reinterpret_cast<uint16_t*>(arr)[l] = (uint16_t)v;
  else arr[l] = (uint8_t)v;
}
template <int CH>
__device__ __forceinline__ uint32_t get_lane_bits(const uint8_t* arr, int l) {
  if (CH == 32) return reinterpret_cast<const uint32_t*>(arr)[l];
  if (CH == 16) return reinterpret_cast<const uint16_t*>(arr)[l];
  return arr[l];
}
// lane l gets x of lane l-1 (0 on lane 0) / of lane l+1 (0 on lane 63)
__device__ __forceinline__ uint32_t from_lane_below(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138, 0xf, 0xf, true);  // wave_shr:1
}
__device__ __forceinline__ uint32_t from_lane_above(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x130, 0xf, 0xf, true);  // wave_shl:1
}


// One window's prefetched inputs: WIN/64 cs bytes per lane and the offsets /
// tstart of reads rs0 + lane.
template <int CH> struct Chunk;
template <> struct Chunk<16> { using T = uint4; };
template <> struct Chunk<8> { using T = uint2; };
template <> struct Chunk<32> { using T = U8x32; };
template <int CH>
struct WinIn {
  typename Chunk<CH>::T d;
  int64_t o;
  uint32_t uo, dno;  // low words of the flank offsets: only the lengths' signs are needed
  int32_t ts;
};
// A lane's cs bytes of a window.  The cs stream is read exactly once, so it is
// loaded non-temporally (evict-first in the caches) and does not push the
// insertion pages being filled out of L2 before their lines are whole.
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint4 nt_load16(const uint8_t* p) {
  const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}
template <int CH>
__device__ __forceinline__ typename Chunk<CH>::T cs_load(const uint8_t* p) {
  if constexpr (CH == 32) {
    U8x32 v;
    v.a = nt_load16(p);
    v.b = nt_load16(p + 16);
    return v;
  } else if constexpr (CH == 16) {
    return nt_load16(p);
  } else {
    const u32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p));
    return make_uint2(v.x, v.y);
  }
}
template <int CH>
__device__ __forceinline__ WinIn<CH> fetch_window(const ParseArgs& a, int64_t P, int64_t rs0, int l) {
  WinIn<CH> f;
  const int64_t A = P & ~(int64_t)15;
  f.d = cs_load<CH>(a.cs + A + CH * l);
  const int64_t r = rs0 + l;
  const bool ok = r <= a.n_reads;
  f.o = ok ? a.cs_off[r] : INT64_MAX;
  f.uo = ok ? reinterpret_cast<const uint32_t*>(a.up_off)[2 * r] : 0u;
  f.dno = ok ? reinterpret_cast<const uint32_t*>(a.down_off)[2 * r] : 0u;
  f.ts = r < a.n_reads ? a.tstart[r] : 0;
  return f;
}
__device__ __forceinline__ void chunk_load(const uint8_t* p, uint4& v) { v = *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void chunk_load(const uint8_t* p, uint2& v) { v = *reinterpret_cast<const uint2*>(p); }
__device__ __forceinline__ void chunk_load(const uint8_t* p, U8x32& v) {
  v.a = reinterpret_cast<const uint4*>(p)[0];
  v.b = reinterpret_cast<const uint4*>(p)[1];
}
__device__ __forceinline__ void chunk_store(uint8_t* p, uint4 v) { *reinterpret_cast<uint4*>(p) = v; }
__device__ __forceinline__ void chunk_store(uint8_t* p, uint2 v) { *reinterpret_cast<uint2*>(p) = v; }
__device__ __forceinline__ void chunk_store(uint8_t* p, U8x32 v) {
  reinterpret_cast<uint4*>(p)[0] = v.a;
  reinterpret_cast<uint4*>(p)[1] = v.b;
}

// One insertion event into its (workgroup, bucket) page (every lane with an
// event calls it; wave-uniform loop).  The bucket word W = page << 12 | fill:
// a returning add takes slot `fill`; the lane that takes slot 64 of a full page
// opens the next one (page counter npg, owner pg_own) and publishes it with
// fill 1 (its own event in slot 0); lanes that found the page full meanwhile
// (slot > 64, their adds are discarded by the publish) wait for the new page
// and try again.  W lives in LDS (tally modes 0-3) or HBM (mode 4).  Every
// wave reaches the loop's end: an opener never waits.
template <bool GLOBAL_W>
__device__ __forceinline__ void parse_place_event(const ParseArgs& a, bool has, uint32_t* W, uint32_t* npg,
                                                  int64_t pbase, uint32_t* pg0, uint32_t pcap, int b, uint32_t word) {
  // common case straight-line: the add gives a slot of the current page
  // (pg0 = the workgroup's first page: 32-bit offsets from a scalar base)
  uint32_t old = has ? atomicAdd(W, 1u) : 0u;
  const bool fast = has && (old & ((1u << kPgBits) - 1u)) < (uint32_t)kPgEv;
  if (fast) pg0[(old >> kPgBits) * kPgEv + (old & ((1u << kPgBits) - 1u))] = word;
  bool need = has && !fast;
  if (!ballot(need)) return;
  // the page is full: open the next one, or wait for its opener.  A waiting
  // lane looks at W once per pass of the wave-uniform loop, so an opener lane
  // of the SAME wave (whose branch the compiler may place after the waiting
  // lanes' code in one pass) has published before the next look
  bool waiting = false, first = true;
  uint32_t wpg = 0;
  int spins = 0;
  while (ballot(need)) {
    if (need && waiting) {
      const uint32_t cur = GLOBAL_W ? __hip_atomic_load(W, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                    : __hip_atomic_load(W, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      waiting = (cur >> kPgBits) == wpg;
      if (waiting && ++spins > (1 << 22)) {  // bounded: never expected
        atomicOr(&a.status[MPC_ST_FLAGS], DE_INTERNAL);
        need = false;
      }
    }
    if (need && !waiting) {
      if (!first) old = atomicAdd(W, 1u);
      first = false;
      const uint32_t slot = old & ((1u << kPgBits) - 1u), pg = old >> kPgBits;
      if (pg == kPgOvf && slot > (uint32_t)kPgEv) {
        // the region ran out of pages (flagged by the opener): the event is
        // dropped, and the word reset so its fill never carries into the page field
        atomicExch(W, (kPgOvf << kPgBits) | (uint32_t)kPgEv);
        need = false;
      } else if (slot < (uint32_t)kPgEv) {
        pg0[pg * kPgEv + slot] = word;
        need = false;
      } else if (slot == (uint32_t)kPgEv) {
        const uint32_t np = atomicAdd(npg, 1u);
        if (np >= pcap) {  // never expected: the page region bound (parse_page_base)
          // publish the overflow page, so waiting lanes leave (dropping their events)
          atomicOr(&a.status[MPC_ST_FLAGS], DE_INTERNAL);
          atomicExch(W, (kPgOvf << kPgBits) | (uint32_t)kPgEv);
        } else {
          a.pg_own[pbase + np] = (uint32_t)b;
          pg0[np * kPgEv] = word;
          atomicExch(W, (np << kPgBits) | 1u);
        }
        need = false;
      } else {
        waiting = true;  // the page filled meanwhile: wait for its opener
        wpg = pg;
      }
    }
  }
}

// End of a parse workgroup: flush the LDS position tallies and the LEFT-gap
// bitmap with contiguous atomics (tally modes 1-3), then list every bucket's
// pages: bk_cnt = its events, bk_off = where its page list starts in
// pg_list[pbase ...] -- the pages (global page numbers) in any order but the bucket's current
// (possibly partial) page LAST, so event e of the bucket is in page
// pg_list[pbase + bk_off + e / 64] at slot e % 64.  W (page words), cnt and cur
// are LDS for modes 0-3 (cnt, cur alias the flushed tallies) and HBM for mode 4
// (W = bk_cur, cnt = bk_cnt zeroed by K_clear, cur = bk_cur once read).  Every
// thread of the block calls it.
template <int TM>
__device__ void parse_epilogue(const ParseArgs& a, int n, int gb, int nbk, uint32_t* hl, uint32_t* W, uint32_t* uni,
                               const uint32_t* npg, int64_t pbase, uint32_t pcap) {
  constexpr bool big = TM == 4;
  constexpr bool fused = TM >= 1 && TM <= 3;
  constexpr bool lds_sub = TM == 1 || TM == 2;
  constexpr bool packed = TM == 2 || TM == 3;
  const int l = lane();
  const int nsub = lds_sub ? 2 * (n + 1) : 0;
  const uint32_t* sub_l = uni;
  const uint32_t* del_l = uni + nsub;
  // ---- flush LDS tallies and the LEFT-gap bitmap ----
  if (fused) {
    // one word per lane, consecutive lanes on consecutive words: a wave's
    // atomics cover contiguous bytes (memory-side atomics run at full rate
    // only on contiguous segments)
    for (int p = threadIdx.x; p <= n; p += blockDim.x) {
      int32_t dv;
      if (packed) dv = (int32_t)((del_l[p >> 1] >> (16 * (p & 1))) & 0xffffu) - 0x8000;
      else { const uint32_t dl = del_l[p]; dv = (int32_t)(dl >> 16) - (int32_t)(dl & 0xffffu); }
      if (dv) atomicAdd(a.diff + gb + p, dv);
    }
    uint32_t* sg = a.sub + (int64_t)gb * 4;
    for (int k = threadIdx.x; lds_sub && k < 4 * (n + 1); k += blockDim.x) {  // word k = position k/4, code k%4
      const uint32_t w2 = sub_l[2 * (k >> 2) + ((k >> 1) & 1)];
      const uint32_t v = (k & 1) ? (w2 >> 16) : (w2 & 0xffffu);
      if (v) atomicAdd(sg + k, v);
    }
  }
  for (int k = threadIdx.x; !big && k < parse_hl_words(n); k += blockDim.x) {
    const uint32_t v = hl[k];
    if (!v) continue;
    const int g0 = gb + 32 * k;  // global bit of local bit 0 of this word
    atomicOr(a.hasleft + (g0 >> 5), v << (g0 & 31));
    if (g0 & 31) atomicOr(a.hasleft + (g0 >> 5) + 1, v >> (32 - (g0 & 31)));
  }
  const int64_t wgb = (int64_t)blockIdx.x * a.nbs;
  uint32_t* cnt = big ? reinterpret_cast<uint32_t*>(a.bk_cnt) + wgb : uni;       // non-last pages per bucket
  uint32_t* cur = big ? a.bk_cur + wgb : uni + nbk;                               // list cursors
  auto wload = [&](int b) -> uint32_t {
    return big ? __hip_atomic_load(W + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : W[b];
  };
  __syncthreads();  // (LDS tallies flushed: cnt / cur may alias them)
  const uint32_t np_all = min(*npg, pcap);  // (the counter runs past pcap only after DE_INTERNAL)
  // A: mark every bucket's last page (it goes to the end of the bucket's list)
  for (int b = threadIdx.x; b < nbk; b += blockDim.x) {
    const uint32_t w = wload(b);
    if ((w >> kPgBits) < pcap) a.pg_own[pbase + (w >> kPgBits)] = kPgMark;
    if (!big) cnt[b] = 0;
  }
  __syncthreads();
  // B: the other pages per bucket
  for (uint32_t p = threadIdx.x; p < np_all; p += blockDim.x) {
    const uint32_t b = a.pg_own[pbase + p];
    if (b != kPgMark) atomicAdd(cnt + b, 1u);
  }
  __syncthreads();
  // C: one wave -- list offsets (exclusive scan of the page counts), event
  // counts, the last page at the end of each list, the list cursors
  if (threadIdx.x < 64) {
    int carry = 0;
    for (int c0 = 0; c0 < nbk; c0 += 64) {
      const int b = c0 + l;
      uint32_t w = kPgInit, c = 0;
      if (b < nbk) {
        w = wload(b);
        c = big ? (uint32_t)__hip_atomic_load(cnt + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : cnt[b];
      }
      const bool has = (w >> kPgBits) < pcap;  // (not kPgNone, not kPgOvf)
      const int np = (int)c + (has ? 1 : 0);
      const int inc = wave_scan_i32(np);
      const int off = carry + inc - np;
      if (b < nbk) {
        a.bk_cnt[wgb + b] = has ? (int32_t)(c * kPgEv + (w & ((1u << kPgBits) - 1u))) : 0;
        a.bk_off[wgb + b] = off;
        if (has) a.pg_list[pbase + off + np - 1] = (uint32_t)(pbase + (w >> kPgBits));
        if (big) __hip_atomic_store(cur + b, (uint32_t)off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else cur[b] = (uint32_t)off;
      }
      carry += wave_last_i32(inc);
    }
  }
  if (threadIdx.x == 0) a.rbase[blockIdx.x] = pbase;
  __syncthreads();
  // D: place the other pages
  for (uint32_t p = threadIdx.x; p < np_all; p += blockDim.x) {
    const uint32_t b = a.pg_own[pbase + p];
    if (b != kPgMark) a.pg_list[pbase + atomicAdd(cur + b, 1u)] = (uint32_t)(pbase + p);
  }
}

// Workgroup = contiguous reads of ONE sample (host work table); wave w takes
// the w-th part of them and streams their cs bytes in windows of WIN bytes
// (WIN/64 per lane, coalesced).  Token boundaries (special characters and read starts) are bits
// of an LDS mask.  A window is cut at its LAST boundary C, so every token in
// [P, C) ends inside the window (no lookahead halo); the next window starts at
// C.  The token starts are compacted into a list of UNITS -- a ':' token
// with 1-4 digits and the op token right after it in the same read form one
// unit (minimap2's short cs alternates them, so this halves the list) -- and
// processed ONE UNIT PER LANE, 64 per round: branch-free SWAR decode of the
// operand words, one DPP scan of the advances for the coordinates i (reads
// are segments: per-read bases in a slot table), ballot/mbcnt for the read
// slot.  Effects: substitution / deletion / span tallies (LDS in tally modes
// 1-3), insertion events placed once into 64-event pages of their (workgroup,
// bucket) (parse_place_event), LEFT-gap bits (LDS bitmap).  Epilogue: flush
// the tallies, list every bucket's pages (parse_epilogue).
// NK: the plan holds reads with a negative tstart (mpc_input.neg_reads): the
// kernel carries the rounds of Python's negative index wrap (NEG below),
// taken by the workgroups that hold such a read; without NK nothing of it is
// compiled in (its registers would bound every plan's kernel), and a negative
// tstart is MPC_DE_UNSUPPORTED (parsed from 0, never an out-of-range write).
// S1: tally mode 3 with one substitution window; DP: deferred placement
// (both described at kDefQ above).
template <int TM, int WIN, bool NK, bool S1 = false, bool DP = false>
__global__ __launch_bounds__(kMaxPW * 64) void K_parse(ParseArgs a) {
  static_assert(!S1 || TM == 3, "one substitution window: tally mode 3 only");
  static_assert(!DP || TM != 4, "deferred placement: bucket words in LDS");
  constexpr int CH = WIN / 64;
  static_assert(WIN <= kMaxWin, "coordinate bound (kMaxWin)");
  using WL = WaveLds<WIN, lds_base<TM>()>;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int l = lane();
  const int nw = (int)(blockDim.x >> 6);
  const int w = uniform_i32((int)(threadIdx.x >> 6));
  WL& W = *reinterpret_cast<WL*>(lds + w * (int)sizeof(WL));
  int64_t* cbo = reinterpret_cast<int64_t*>(lds + nw * (int)sizeof(WL));        // [kMaxCh + 1] chunk bounds: cs offset
  int32_t* cbr = reinterpret_cast<int32_t*>(cbo + kMaxCh + 2);                  // [kMaxCh + 1] ... and read
  uint32_t* cnext = reinterpret_cast<uint32_t*>(cbr + kMaxCh + 4);              // next chunk to take
  uint32_t* hl = cnext + 4;                                                      // LEFT gaps bitmap
  const int4 wk = a.work[blockIdx.x];
#ifdef MPC_STAMPS
  uint64_t st_acc[kStampSeg] = {0, 0, 0, 0, 0, 0, 0, 0}, st_prev;
  MPC_STAMP(st_prev);
#endif
  const int smp = wk.x;
  const int64_t r0 = wk.y, r1 = wk.z;
  const int n = a.n_of[smp];
  const int gb = a.gbase[smp];
  const int nbk = (n + 1 + kBW - 1) / kBW;  // insertion buckets
  constexpr bool big = TM == 4;             // per-gap state (LEFT bitmap, bucket page words) in HBM
  // [nbk] page word of every insertion bucket (page << 12 | fill, parse_place_event)
  uint32_t* bkw = big ? a.bk_cur + (int64_t)blockIdx.x * a.nbs : hl + parse_hl_words(n);
  uint32_t* uni = hl + parse_hl_words(n) + nbk;
  uint32_t* npg = cnext + 1;                // pages opened by the workgroup
  // the workgroup's page region [pbase, pnext) (parse_page_base)
  const int64_t pbase = parse_page_base(a.cs_off[r0] - a.cs_base, r0, blockIdx.x, a.nbs);
  const int64_t pnext = parse_page_base(a.cs_off[r1] - a.cs_base, r1, blockIdx.x + 1, a.nbs);
  const uint32_t pcap = (uint32_t)min(pnext - pbase, (int64_t)kPgOvf);
  uint32_t* const pg0 = a.ins_sorted + pbase * kPgEv;  // the region's first event slot
  constexpr bool fused = TM >= 1 && TM <= 3;  // depth differences in LDS (one address space per instantiation)
  constexpr bool lds_sub = TM == 1 || TM == 2;  // substitution tallies in LDS too
  constexpr bool packed = TM == 2 || TM == 3;
  const int nsub = lds_sub ? 2 * (n + 1) : 0;
  uint32_t* sub_l = uni;                    // [2 (n+1)] (TM 1, 2): A | T << 16, C | G << 16
  // TM 1:    [n+1] depth-decrement count | depth-increment count << 16
  // TM 2, 3: [(n+2)/2] depth difference of position p in half p&1 of word p>>1,
  //          biased by 0x8000: at most 16383 reads per workgroup and 2 per read and
  //          position keep every partial sum inside (0, 0xffff): no carry across halves
  uint32_t* del_l = uni + nsub;
  for (int k = threadIdx.x; !big && k < parse_hl_words(n); k += blockDim.x) hl[k] = 0;
  for (int k = threadIdx.x; !big && k < nbk; k += blockDim.x) bkw[k] = kPgInit;  // (mode 4: K_clear)
  // chunks 0..nw-1 go to waves 0..nw-1 (the counter runs in units of 64: take_chunk)
  if (threadIdx.x == 0) { *cnext = (uint32_t)nw * 64u; *npg = 0u; cnext[2] = 0u; }
  const int nch = wk.w;
  for (int k = threadIdx.x; k <= nch; k += blockDim.x) {
    const int32_t r = a.wave_tab[(int64_t)blockIdx.x * (kMaxCh + 1) + k];
    cbr[k] = r;
    cbo[k] = a.cs_off[r];
  }
  if (fused)
    for (int k = threadIdx.x; k < nsub + (packed ? (n + 2) / 2 : n + 1); k += blockDim.x)
      uni[k] = (packed && k >= nsub) ? 0x80008000u : 0u;
  // a read with a negative tstart in the workgroup: its chunks take the rounds
  // that follow Python's negative index wrap (NEG below; the others compile
  // none of it)
  // (an OR through cnext[2], not __syncthreads_or: that one takes static LDS
  // the planner's budget does not hold)
  bool wg_neg = false;
  if constexpr (NK) {
    bool has_neg = false;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) has_neg |= a.tstart[r] < 0;
    __syncthreads();
    if (ballot(has_neg) && lane() == 0) atomicOr(cnext + 2, 1u);
    __syncthreads();
    wg_neg = uniform_i32((int)cnext[2]) != 0;
  } else {
    __syncthreads();  // the chunk table, counters and cleared tallies above are in place
  }

  auto odd_sub = [&](int pos, int code) {
    if (lds_sub) atomicAdd(sub_l + 2 * pos + (code >> 1), 1u << (16 * (code & 1)));
    else atomicAdd(a.sub + (int64_t)(gb + pos) * 4 + code, 1u);
  };
  auto depth_dec = [&](int pos) {  // diff[pos] -= 1
    if (packed) atomicSub(del_l + (pos >> 1), 1u << (16 * (pos & 1)));
    else if (fused) atomicAdd(del_l + pos, 1u);
    else atomicAdd(a.diff + gb + pos, -1);
  };
  auto depth_inc = [&](int pos) {  // diff[pos] += 1
    if (packed) atomicAdd(del_l + (pos >> 1), 1u << (16 * (pos & 1)));
    else if (fused) atomicAdd(del_l + pos, 1u << 16);
    else atomicAdd(a.diff + gb + pos, 1);
  };

  auto left_bit = [&](int pos) {  // gap pos holds a LEFT event
    if (big) atomicOr(a.hasleft + ((gb + pos) >> 5), 1u << ((gb + pos) & 31));
    else atomicOr(hl + (pos >> 5), 1u << (pos & 31));
  };
  // The workgroup's reads come in chunks (planner: contiguous, by cs bytes,
  // 5/8 of the bytes in the first nw chunks, smaller ones after); wave w
  // starts on chunk w and takes the next free one when it is done, so all
  // waves reach the epilogue barrier within about one small chunk of each
  // other (a static share per wave left them waiting there ~20 % of their
  // time: profiles/r03_stamps).  The chunk table sits in LDS (one load per
  // chunk bound per workgroup).  A chunk is a stream of its own: event
  // regions, i_end.
  // take the next chunk: every lane of the wave adds 1, so the counter runs in
  // units of 64 (the wave is whole here: blocks are whole waves, and the chunk
  // loop is wave-uniform).  No divergent region guards the atomic (a
  // lane-0-only atomic in the loop head was compiled into a loop exit that
  // only lane 0 took: the wave never left), and the value added is uniform: a
  // per-lane value (lane 0 one, the others zero) was compiled into a scalar
  // loop over all 64 lanes, ~500 instructions per chunk taken, where this is
  // one lane count and one add
  auto take_chunk = [&]() {
    const uint32_t v = atomicAdd(cnext, 1u);
    return uniform_i32((int)(v >> 6));  // (the first lane's: the counter before the add)
  };
  // deferred placement: the wave's queue of (bucket, event word) in LDS, a ring
  // of kDefQ entries between dq_tail and dq_head (wave-uniform counters); a
  // round appends its events, and 64 at a time are placed after it (<= 63 wait
  // before a round, <= 127 after one)
  uint2* const dq = DP ? reinterpret_cast<uint2*>(lds + a.defer_off) + w * kDefQ : nullptr;
  uint32_t dq_head = 0, dq_tail = 0;
  auto defer_flush = [&](const int cnt) {  // the cnt (<= 64) oldest events, one per lane
    wave_sync_lds();
    const bool has = l < cnt;
    const uint2 e = has ? dq[(dq_tail + l) & (kDefQ - 1)] : make_uint2(0u, 0u);
    parse_place_event<big>(a, has, bkw + e.x, npg, pbase, pg0, pcap, (int)e.x, e.y);
    dq_tail += (uint32_t)cnt;
  };
  auto chunks = [&](auto negc) {
  constexpr bool NEG = decltype(negc)::value;
  for (int chk = w < nch ? w : nch; chk < nch; chk = take_chunk()) {
  const int64_t ra = uniform_i32(cbr[chk]), rb = uniform_i32(cbr[chk + 1]);
  const int64_t wend = readlane64(cbo[chk + 1], 0);
  int64_t P = readlane64(cbo[chk], 0);
  const int64_t sev_base = (P - a.cs_base) / kSubEvBytes + 2 * ra;  // ... and its substitution-event regions (TM 3)
  uint32_t nsub_v = 0;                                    // lane k: substitution events of window k
  uint32_t nsub_s = 0;                                    // ... of the only window (S1, wave-uniform)
  int64_t rs0 = ra;         // first read whose cs starts at or after P
  bool carry = false;       // slot 0 holds a read continuing into this window
  int32_t c_base = 0;       // ... and its coordinate base (wave-uniform): i = base + window prefix of advances
  WinIn<CH> cur = fetch_window<CH>(a, P, rs0, l);
  while (P < wend) {
    const int64_t A = P & ~(int64_t)15;
    // ---- window: at most 63 read starts in [P, E) ----
    int64_t E = A + WIN < wend ? A + WIN : wend;
    const int64_t o63 = readlane64(cur.o, 63);
    if (o63 < E) E = o63;
    MPC_SEG(0);
    // the next read's offsets (lane l + 1, by DPP; lane 63 is never a read of the window)
    const int64_t o_nx = (int64_t)(((uint64_t)from_lane_above((uint32_t)((uint64_t)cur.o >> 32)) << 32) |
                                   from_lane_above((uint32_t)cur.o));
    const uint32_t uo_nx = from_lane_above(cur.uo);
    const uint32_t dno_nx = from_lane_above(cur.dno);
    if (E <= P) {
      // reads rs0 .. rs0+62 all start at P: 63 empty cs (processOperation('', ''))
      if (l < 63) {
        flag_read(a, DE_OP, rs0 + l);
        a.i_end[rs0 + l] = cur.ts < 0 ? 0 : (cur.ts > n ? n + 1 : cur.ts);
      }
      rs0 += 63;
      cur = fetch_window<CH>(a, P, rs0, l);  // (same P)
      continue;
    }
    // ---- stage bytes, boundary bits ----
    chunk_store(W.stage + CH * l, cur.d);
    uint32_t spm, cm_own;
    chunk_classes(cur.d, &spm, &cm_own);
    const uint32_t om_own = spm & ~cm_own;
    put_lane_bits<CH>(W.ra, l, 0u);
    wave_sync_lds();
    {  // read-start bits of every read starting inside the window (incl. E)
      const int64_t rel = cur.o - A;
      if (rel >= 0 && rel < WIN) atomicOr(reinterpret_cast<uint32_t*>(W.ra) + (rel >> 5), 1u << (rel & 31));
    }
    wave_sync_lds();
    const int64_t cA = A + CH * l;
    const uint32_t ra_own = get_lane_bits<CH>(W.ra, l);
    const uint32_t em_own = spm | ra_own;  // boundaries: special characters and read starts
    // ---- cut C: E if E is a boundary (a read start), else the last boundary in (P, E) ----
    const bool e_rs = (E == wend) || (E == o63);
    int64_t C;
    bool c_rs;
    bool far = false;
    if (e_rs) { C = E; c_rs = true; }
    else {
      int lo = (int)(P + 1 - cA), hi = (int)(E - cA);
      lo = lo < 0 ? 0 : (lo > CH ? CH : lo);
      hi = hi < 0 ? 0 : (hi > CH ? CH : hi);
      const uint32_t m = em_own & lowmask(hi) & ~lowmask(lo);
      const uint64_t b = ballot(m != 0);
      if (b) {
        const int f = 63 - __clzll((long long)b);
        const uint32_t mf = (uint32_t)__builtin_amdgcn_readlane((int)m, f);
        const uint32_t rf = (uint32_t)__builtin_amdgcn_readlane((int)ra_own, f);
        const int k = 31 - __clz(mf);
        C = A + CH * f + k;
        c_rs = (rf >> k) & 1u;
      } else {
        // one token runs past the window: its end is the next special character
        // or the next read start (the first read start after P)
        const uint64_t bn = ballot(cur.o > P);
        const int fo = bn ? __ffsll((unsigned long long)bn) - 1 : 63;
        const int64_t bound = readlane64(cur.o, fo) < wend ? readlane64(cur.o, fo) : wend;
        C = scan_special_wave(a.cs, A + WIN, bound);
        c_rs = C == bound;
        far = true;
      }
    }
    if (WIN > tok_cap<WIN>() && !far) {
      // more than tok_cap tokens in [P, C): cut at the tok_cap-th boundary after P
      int lo = (int)(P - cA), hi = (int)(C - cA);
      lo = lo < 0 ? 0 : (lo > CH ? CH : lo);
      hi = hi < 0 ? 0 : (hi > CH ? CH : hi);
      const uint32_t m = em_own & lowmask(hi) & ~lowmask(lo);
      const int cb = __popc(m);
      // at most tok_cap / 64 boundaries in every lane: no cut (the usual case, no scan)
      const bool may = ballot(cb > tok_cap<WIN>() / 64) != 0;
      const int inc = may ? wave_scan_i32(cb) : 0;
      if (may && wave_last_i32(inc) > tok_cap<WIN>()) {
        const int f = __ffsll((unsigned long long)ballot(inc > tok_cap<WIN>())) - 1;
        uint32_t mf = (uint32_t)__builtin_amdgcn_readlane((int)m, f);
        const int j = tok_cap<WIN>() - (__builtin_amdgcn_readlane(inc, f) - __builtin_amdgcn_readlane(cb, f));
        for (int u = 0; u < j; ++u) mf &= mf - 1;  // drop the j lowest boundaries of lane f
        const int k = __ffs(mf) - 1;
        C = A + CH * f + k;
        c_rs = (((uint32_t)__builtin_amdgcn_readlane((int)ra_own, f)) >> k) & 1u;
      }
    }
    const bool inwin = l < 63 && cur.o < C;  // read rs0+l starts in [P, C)
    const int nst = __popcll(ballot(inwin));
    // ---- per-read slots ----
    if (inwin) {
      const int q = l + 1;
      const bool up = uo_nx != cur.uo, dn = dno_nx != cur.dno;  // flank lengths < 2^32
      uint32_t derr = 0;
      // (a kernel without the negative rounds parses a negative start from 0, flagged)
      const int ts = !NEG && cur.ts < 0 ? 0 : cur.ts;
      if (!NEG && cur.ts < 0) derr |= DE_UNSUP;
      // obsarr[2 tstart] (:303) with Python's negative wrap: below -n past the
      // front (IndexError), in [-n, 0) a LEFT string at the wrapped ODD
      // position n + tstart (listed; only NEG chunks see a negative tstart)
      if (up && ts < 0) {
        if (ts + n < 0) derr |= DE_INDEX;
        else if constexpr (NEG) derr |= push_wo(a, gb + ts + n, rs0 + l, kWoUp, 0, 0);
        else derr |= DE_INTERNAL;
      }
      if (ts < MPC_TSTART_MIN) derr |= DE_UNSUP;
      if (up && ts > n) derr |= DE_INDEX;             // leftIndel(2*i) past the end
      if (o_nx <= cur.o) derr |= DE_OP;               // processOperation('', '')
      if (derr) flag_read(a, derr, rs0 + l);
      if (up && ts >= 0 && ts <= n) left_bit(ts);  // upstream flank: LEFT at gap tstart
      W.s_end[q] = o_nx;
      W.s_ts[q] = ts < MPC_TSTART_MIN ? MPC_TSTART_MIN : (ts > kICap ? kICap : ts);
      W.s_read[q] = (int32_t)(rs0 + l);
      W.s_iend[q] = (ts < 0 ? 0 : (ts > n ? n + 1 : ts)) | (dn ? 1 << 30 : 0);
    }
    // ---- the next window starts at C (its bytes and read records load after
    // this window's rounds: holding them across the rounds costs VGPRs) ----
    const int64_t Pn = C, rsn = rs0 + nst;
    // ---- token list: starts in [P, C) (bit 15 = read start), then the sentinel ----
    int T;
    {
      int tlo = (int)(P - cA), thi = (int)(C - cA);
      tlo = tlo < 0 ? 0 : (tlo > CH ? CH : tlo);
      thi = thi < 0 ? 0 : (thi > CH ? CH : thi);
      const uint32_t rng = lowmask(thi) & ~lowmask(tlo);
      const uint32_t tm = em_own & rng;
      // Units: a ':' token with 1-4 operand bytes and the op token right after
      // it in the same read, both in [P, C), are ONE list entry (bits 12-14: the
      // ':' operand length); every other token is its own entry.  Bit-parallel
      // on 32-bit masks: bit k of at(m, d) = bit k + d of this lane's mask m
      // continued by the next lane's, so a ':' at k has operand length d - 1
      // when the first boundary after it is an op at k + d (d = 2..5).
      const uint32_t cmr = cm_own & rng, omr = om_own & ~ra_own & rng;
      const uint32_t em_nx = from_lane_above(em_own), om_nx = from_lane_above(omr);
      auto at = [&](uint32_t own, uint32_t nx, int d) -> uint32_t {
        if constexpr (CH == 32) return __builtin_amdgcn_alignbit(nx, own, (uint32_t)d);
        else return (own | (nx << CH)) >> d;
      };
      const uint32_t n1 = ~at(em_own, em_nx, 1), n2 = n1 & ~at(em_own, em_nx, 2);
      const uint32_t n3 = n2 & ~at(em_own, em_nx, 3), n4 = n3 & ~at(em_own, em_nx, 4);
      const uint32_t p2 = cmr & n1 & at(omr, om_nx, 2);  // ':' whose op is 2 bytes on
      const uint32_t p3 = cmr & n2 & at(omr, om_nx, 3);
      const uint32_t p4 = cmr & n3 & at(omr, om_nx, 4);
      const uint32_t p5 = cmr & n4 & at(omr, om_nx, 5);
      const uint32_t pl0 = p2 | p4, pl1 = p3 | p4;        // operand length d - 1 in 3 bit planes
      // the absorbed ops: here, or (carried) in the next lane
      uint32_t ab_own, ab_hi;
      if constexpr (CH == 32) {
        ab_own = (p2 << 2) | (p3 << 3) | (p4 << 4) | (p5 << 5);
        ab_hi = (p2 >> 30) | (p3 >> 29) | (p4 >> 28) | (p5 >> 27);
      } else {
        const uint32_t ab = (p2 << 2) | (p3 << 3) | (p4 << 4) | (p5 << 5);
        ab_own = ab & lowmask(CH);
        ab_hi = ab >> CH;
      }
      ab_own |= from_lane_below(ab_hi);
      const uint32_t tu = tm & ~ab_own;
      const int cnt = __popc(tu);
      const int incl = wave_scan_i32(cnt);
      T = wave_last_i32(incl);
      const int base = CH * l;
      auto entry = [&](int k) -> uint16_t {
        return (uint16_t)((uint32_t)(base + k) | (((pl0 >> k) & 1u) << 12) | (((pl1 >> k) & 1u) << 13) |
                          (((p5 >> k) & 1u) << 14) | (((ra_own >> k) & 1u) << 15));
      };
      uint32_t m = tu;
      int idx = incl - cnt;
      while (m) {
        const int k = __ffs(m) - 1;
        m &= m - 1;
        W.tok[idx++] = entry(k);
      }
      if (l == 0) W.tok[T] = far ? (uint16_t)(kFar | (c_rs ? 0x8000u : 0u)) : (uint16_t)((C - A) | (c_rs ? 0x8000u : 0u));
    }
    wave_sync_lds();
    MPC_SEG(1);

    // ---- rounds: one token per lane ----
    const int far_c = (int)(C - A < (1 << 30) ? C - A : (1 << 30));  // wave-uniform
    int32_t G = 0;  // advances of the window's earlier rounds
    int qc = 0;     // read starts of the window's earlier rounds
    int32_t cb = c_base;  // coordinate base of the open read (wave-uniform)
    // one round (64 units, one per lane): GEN = the general decode; without it
    // the fast decode, and false (nothing applied) when a unit is not canonical
    auto round = [&](const int t0, auto genc) -> bool {
      constexpr bool GEN = decltype(genc)::value;
      const int t = t0 + l;
      const bool v = t < T;
      const uint32_t t0r = W.tok[t], t1r = W.tok[t + 1];  // in bounds for every lane (+64 padding)
      const uint32_t e0 = v ? t0r : 0u, e1 = v ? t1r : 0u;
      const int s0 = (int)(e0 & 0xfffu);         // unit start
      const int pl = (int)((e0 >> 12) & 7u);     // ':' operand length of a unit's prefix (0: none)
      const int sx = pl ? s0 + pl + 1 : s0;      // the unit's main token
      const bool lfar = v && ((e1 & 0x7fffu) == kFar);
      // far: the token ends at C (beyond the window); 32-bit here (far_c saturates
      // at 2^30 > kAdvCap + the window), 64-bit only on the slow path
      const int ex32 = lfar ? far_c : (int)(e1 & 0xfffu);
      const int ex = ex32 - sx - 1 < kAdvCap ? ex32 : sx + 1 + kAdvCap;
      const bool is_rs = v && (e0 >> 15);
      const bool last = v && (e1 >> 15);
      const uint64_t brs = ballot(is_rs);
      const int q = qc + lanes_below(brs) + (is_rs ? 1 : 0);
      // the read's slot (tstart, read, i_end), loaded before the decode
      const int32_t q_ts = W.s_ts[q], q_read = W.s_read[q], q_iend = W.s_iend[q];
      // ---- decode.  Fast path: every unit of the round is canonical -- an
      // optional absorbed ':' prefix of 1-4 digits, then ':' + 1-4 digits, '*' +
      // 1-4 bytes ending in a base, '+' + 1-4 bases or '-' + 1-4 bytes, ending
      // inside the window -- so no data error can arise but the coordinate
      // checks; branch-free from two 8-byte LDS reads.  A round holding any
      // other unit ('Z', empty / long operands, non-digits, non-bases, a token
      // past the window, a read not starting with an operator) takes the
      // general decode below for all its lanes.
      const uint32_t* b32 = reinterpret_cast<const uint32_t*>(W.stage);
      int adv0, adv, kind, olen_e;
      uint32_t pay, err = 0u;
      bool fast = false;
      if constexpr (!GEN) {
        const uint32_t sh = (uint32_t)(sx & 3);
        uint32_t m0 = b32[sx >> 2], m1 = b32[(sx >> 2) + 1];  // bytes sx .. sx + 4 (sh + 4 <= 7)
        const int pa = (s0 + 1) >> 2;
        uint32_t p0 = b32[pa], p1 = b32[pa + 1];
        // (opaque: both 8-byte reads issue together, unconditionally -- the
        // compiler would otherwise sink the prefix read into a branch on pl)
        asm volatile("" : "+v"(m0), "+v"(m1), "+v"(p0), "+v"(p1));
        const uint32_t op = __builtin_amdgcn_alignbyte(m1, m0, sh) & 0xffu;
        const uint32_t ow = sh == 3u ? m1 : __builtin_amdgcn_alignbyte(m1, m0, sh + 1u);  // operand bytes
        const uint32_t pw = __builtin_amdgcn_alignbyte(p1, p0, (uint32_t)((s0 + 1) & 3));  // ':' prefix
        const int olen = ex32 - sx - 1;
        const int ol4 = olen < 0 ? 0 : (olen > 4 ? 4 : olen);
        const bool colon = op == ':', star = op == '*', plus = op == '+', minus = op == '-';
        const int cl = pl ? pl : (colon ? ol4 : 0);  // digits of the unit's ':' operand
        const uint32_t cw = pl ? pw : ow;
        const uint32_t cvm = cl == 4 ? 0xffffffffu : ((1u << (8 * cl)) - 1u);
        const uint32_t Tx = cw ^ 0x30303030u;
        const bool dig = ((((Tx & 0x7F7F7F7Fu) + 0x76767676u) | Tx) & 0x80808080u & cvm) == 0;
        uint32_t X = (Tx & cvm & 0x0F0F0F0Fu) << ((32 - 8 * cl) & 31);  // right-aligned digits (cl = 0: 0)
        X = mul2561(X) >> 8;
        X = ((X & 0x00FF00FFu) * 6553601u) >> 16;
        const int val = (int)(X & 0xffffu);
        //   bases: (c|0x20) must equal "acgt"[h] with h = (lc>>1)&3 (v_perm table lookup)
        const uint32_t lc = ow | 0x20202020u;
        const uint32_t hh = (lc >> 1) & 0x03030303u;
        const uint32_t bad = lc ^ __builtin_amdgcn_perm(0u, 0x67746361u, hh);
        const uint32_t codes = ((hh & 0x01010101u) << 1) | ((hh >> 1) & 0x01010101u);  // dict order A0 T1 C2 G3
        const uint32_t shl = 8u * (uint32_t)((ol4 - 1) & 3);
        const uint32_t vm = ol4 == 4 ? 0xffffffffu : ((1u << (8 * ol4)) - 1u);
        uint32_t pk = (codes | (codes >> 6)) & 0x000f000fu;
        pk = (pk | (pk >> 12)) & ((1u << (2 * ol4)) - 1u);
        // a special token with an empty operand that is not its read's last --
        // the 'Z' and ':' every read's cs starts with ("Z::12*ag") -- is a no-op
        // (:309: the operator is only applied to a non-empty operand); no prefix
        // can precede it ('Z' / ':' / '*' / '+' / '-' are never absorbed digits)
        const bool nop = (olen == 0) & !last & (pl == 0) & (colon | star | plus | minus | (op == 'Z'));
        fast = !v | (!lfar & ((olen >= 1) & (olen <= 4) & dig &
                              (colon | minus | (star & (((bad >> shl) & 0xffu) == 0u)) | (plus & ((bad & vm) == 0u))) |
                              nop));
        // branch-free: '*' 0x2A -> 2, '+' 0x2B -> 3, '-' 0x2D -> 4 from op & 7;
        // ':' -> 1 when it matches at least one base (:77); a no-op: 0
        const int mv = -(int)(v & !nop), mc = -(int)colon;
        const int o7 = (int)(op & 7u);
        kind = mv & ((mc & (int)(val > 0)) | (~mc & (o7 - (o7 >> 2))));
        adv = mv & ((mc & val) | (int)star | (-(int)minus & ol4));
        adv0 = mv & (-(int)(pl != 0)) & val;
        const uint32_t ms = 0u - (uint32_t)star;
        pay = (ms & ((codes >> shl) & 3u)) | (~ms & pk);
        olen_e = ol4;
        if (ballot(!fast)) return false;  // (before any effect: the round restarts on the general decode)
      }
      if constexpr (GEN) {  // general decode of the whole round
        const int a4 = sx >> 2;
        const uint32_t sh = (uint32_t)(sx & 3);
        const uint32_t d0 = b32[a4], d1 = b32[a4 + 1], d2 = b32[a4 + 2];
        const uint32_t x0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
        const uint32_t x1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
        const uint32_t op = x0 & 0xffu;
        const uint32_t w0 = __builtin_amdgcn_alignbyte(x1, x0, 1u);
        const int olen = ex - sx - 1;
        // branch-free decode: op class, 4 operand bytes at once (SWAR)
        const bool colon = op == ':', star = op == '*', plus = op == '+', minus = op == '-';
        const bool spec = colon | star | plus | minus | (op == 'Z');
        const bool act = v & spec & ((olen > 0) | last);  // empty operand: skipped unless last (:309, :320)
        const int ol4 = olen < 0 ? 0 : (olen > 4 ? 4 : olen);
        const uint32_t vm = ol4 == 4 ? 0xffffffffu : ((1u << (8 * ol4)) - 1u);  // operand bytes in w0
        //   the unit's ':' operand -- its prefix (pl bytes after s0) or the main
        //   token's own operand -- up to 4 digits: right-align, SWAR decimal
        const bool pre = pl != 0;
        const int pa = (s0 + 1) >> 2;
        const uint32_t pw = __builtin_amdgcn_alignbyte(b32[pa + 1], b32[pa], (uint32_t)((s0 + 1) & 3));
        const int cl = pre ? pl : (colon ? ol4 : 0);
        const uint32_t cw = pre ? pw : w0;
        const uint32_t cvm = cl == 4 ? 0xffffffffu : ((1u << (8 * cl)) - 1u);
        const uint32_t Tx = cw ^ 0x30303030u;
        const bool cdig = ((((Tx & 0x7F7F7F7Fu) + 0x76767676u) | Tx) & 0x80808080u & cvm) == 0;
        uint32_t X = cl == 0 ? 0u : (Tx & cvm & 0x0F0F0F0Fu) << (8 * (4 - cl));
        X = mul2561(X) >> 8;
        X = ((X & 0x00FF00FFu) * 6553601u) >> 16;
        const int adv_c = (int)(X & 0xffffu);
        adv0 = pre ? adv_c : 0;
        const bool dig_ok = (olen >= 1) & (olen <= 4) & cdig;  // main ':' token
        //   bases: (c|0x20) must equal "acgt"[h] with h = (lc>>1)&3 (v_perm table lookup)
        const uint32_t lc = w0 | 0x20202020u;
        const uint32_t hh = (lc >> 1) & 0x03030303u;
        const uint32_t bad = lc ^ __builtin_amdgcn_perm(0u, 0x67746361u, hh);
        const uint32_t codes = ((hh & 0x01010101u) << 1) | ((hh >> 1) & 0x01010101u);  // dict order A0 T1 C2 G3
        const int shl = 8 * ((olen - 1) & 3);
        const bool last_ok = ((bad >> shl) & 0xffu) == 0;  // '*': written base = operand[-1] (:96)
        uint32_t pk = codes;
        pk = (pk | (pk >> 6)) & 0x000f000fu;
        pk = (pk | (pk >> 12)) & 0xffu;
        const uint32_t mstar = 0u - (uint32_t)star;
        pay = (mstar & ((codes >> shl) & 3u)) | (~mstar & (pk & ((1u << (2 * ol4)) - 1u)));
        const bool slow = lfar | (pre & !cdig) | (act & ((colon & !dig_ok) | ((star | plus) & (olen > 4))));
        const int kop = ((int)star << 1) | ((int)plus * 3) | ((int)minus << 2);  // exclusive classes
        const int mcol = -(int)colon;
        kind = (-(int)act) & ((mcol & (int)(adv_c > 0)) | (~mcol & (-(int)(olen > 0) & kop)));
        adv = (-(int)(kind == 1) & adv_c) | (int)(kind == 2) | (-(int)(kind == 4) & (olen < kAdvCap ? olen : kAdvCap));
        err = (v & !spec) ? DE_OP : 0u;  // cs does not start with an operator (:100-102)
        if (act & star & (olen == 0)) err |= DE_INDEX;  // operand[-1] of '' (:96)
        if ((kind == 2) & !last_ok) err |= DE_KEY;
        if ((kind == 3) & ((bad & vm) != 0)) err |= DE_KEY;
        olen_e = olen;
        if (slow) {  // rare: decode from HBM
          const int64_t s = A + sx, e = A + (lfar ? C - A : (int64_t)(e1 & 0xfffu));
          const TokInfo ti = analyze_long(a.cs, s, e, last);
          adv = ti.adv; kind = ti.kind; pay = ti.pay; err = ti.err;
          olen_e = (int)(e - s - 1 < kAdvCap ? e - s - 1 : kAdvCap);
          if (pl) {
            const TokInfo tp = analyze_long(a.cs, A + s0, s, false);
            adv0 = tp.adv;
            err |= tp.err;
          }
        }
      }
      MPC_SEG(2);
      // ---- coordinates ----
      const int advu = adv0 + adv;            // unit advance <= 2^23: 64 lanes stay < 2^29
      const int ainc = wave_scan_i32(advu);
      const int aex = ainc - advu;
      const int atot = wave_last_i32(ainc);
      // read bases, i = base + G + aex: lanes before the round's first read
      // start continue the open read (base cb); a read starting at lane j has
      // base tstart - (G + aex_j) on lanes j.. up to the next start.  Tally
      // modes with short reads (lds_base: several starts per round) take the
      // base from the read's slot in LDS, written by its start lane; the
      // others make one scalar pass over the start lanes (about one per round:
      // reads hold tens to hundreds of units), with no LDS write, fence and
      // read back
      int bv = cb;
      if constexpr (lds_base<TM>()) {
        if (is_rs) W.s_val[q] = q_ts - (G + aex);
        wave_sync_lds();
        const int sv = W.s_val[q];
        bv = q == 0 ? cb : sv;  // slot 0: the read open since an earlier window
      } else {
        for (uint64_t m = brs; m; m &= m - 1) {
          const int j = __ffsll((unsigned long long)m) - 1;
          cb = __builtin_amdgcn_readlane(q_ts, j) - (G + __builtin_amdgcn_readlane(aex, j));
          bv = l >= j ? cb : bv;
        }
      }
      const int iu = bv + G + aex;  // coordinate at the unit start
      const int i = iu + adv0;                // ... and at its main token
      MPC_SEG(3);
      // ---- effects ----
      // data errors and effects as flat predicates (no nested exec-mask regions)
      // IndexError (refarr / obsarr past the end): a ':' prefix writes [iu, i),
      // ':' [i, i + adv), '*' [i, i + 1), '+' the gap i: every kind 1-3 needs
      // 0 <= i and i + adv <= n (adv = 1 for '*', 0 for '+'); sign of an OR
      bool bad_i = ((adv0 > 0) & ((iu | (n - i)) < 0)) | (((uint32_t)(kind - 1) <= 2u) & ((i | (n - adv - i)) < 0));
      // Negative coordinates (a negative tstart; chunks that hold one only):
      // refarr / obsarr take index x at len + x for x in [-(2n+1), 0)
      // (Python list indexing).  A ':' or '-' there writes nothing
      // (the wrapped refarr index is even: ''); a '*' at i < 0 writes its base
      // as a one-base LEFT string at gap n + 1 + i; a '+' at i in [-n, 0) is a
      // LEFT string at the wrapped ODD position n + i (listed, push_wo)
      bool wrap = false, unsup = false, wo_ins = false;
      int di = i, gi = i, li = olen_e;  // deletion start, LEFT gap and length
      if constexpr (NEG) {
        const bool mat = (kind == 1) | (kind == 2);
        bad_i = ((adv0 > 0) & (((iu + n + 1) | (n - i)) < 0)) | (mat & (((i + n + 1) | (n - adv - i)) < 0)) |
                ((kind == 3) & (((i + n) | (n - i)) < 0));
        // an advance clamped at kAdvCap from a negative coordinate (its true
        // end may still be <= n)
        unsup = ((adv0 >= kAdvCap) & (iu < 0)) | ((adv >= kAdvCap) & (i < 0) & ((kind == 1) | (kind == 4)));
        wo_ins = (kind == 3) & (i < 0) & (i + n >= 0);
        wrap = (kind == 2) & (i < 0);
        di = i < 0 ? 0 : i;
        gi = wrap ? i + n + 1 : i;
        li = wrap ? 1 : olen_e;
      }
      uint32_t te = err | (bad_i ? DE_INDEX : 0u) | (unsup ? DE_UNSUP : 0u);
      const int rl = q_read;
      if (NEG && wo_ins && te == 0) te |= push_wo(a, gb + i + n, rl, kWoIns, olen_e, A + sx + 1);
      const bool ok = te == 0 && !wo_ins;
      const bool ins_inline = ((kind == 3 && olen_e <= kInsInline) || wrap) && ok;
      const bool any_ins = ballot(ins_inline) != 0;  // (wave-uniform)
      if (ok & (kind == 2) & !wrap & (TM != 3 || (!S1 && a.sub_wins == 0))) odd_sub(i, (int)pay);  // (S1: one window)
      const bool del = NEG ? ok & (kind == 4) & (di < n) & (i + olen_e > di) : ok & (kind == 4) & (i >= 0) & (i < n);
      if (del) {
        depth_dec(di);
        depth_inc(i + olen_e < n ? i + olen_e : n);
      }
      if (ok & ((kind == 3) | wrap)) left_bit(gi);
      if (ok & (kind == 3) & (olen_e > kInsInline)) push_ovf(a, A + sx + 1, rl, i, olen_e);
      if (S1) {  // one substitution window: a wave-uniform count
        const bool sev = ok && kind == 2 && !wrap;
        const uint64_t bw = ballot(sev);
        const uint16_t ev = (uint16_t)(((uint32_t)i << 2) | pay);
        if (sev) a.subev[sev_base + nsub_s + lanes_below(bw)] = ev;
        nsub_s += (uint32_t)__popcll(bw);
      } else if (TM == 3 && a.sub_wins > 0) {  // substitution events, wave-aggregated per window
        const bool sev = ok && kind == 2 && !wrap;
        const int win = i >> kSubWinBits;
        uint16_t* wp = a.subev + sev_base;  // window ww's region of this wave
        for (int ww = 0; ww < a.sub_wins; ++ww, wp += a.subev_cap) {
          const bool mine = sev && win == ww;
          const uint64_t bw = ballot(mine);
          if (!bw) continue;
          const uint32_t n0 = (uint32_t)__builtin_amdgcn_readlane((int)nsub_v, ww);
          if (mine) wp[n0 + lanes_below(bw)] = (uint16_t)(((uint32_t)(i & (kSubWin - 1)) << 2) | pay);
          if (l == ww) nsub_v += (uint32_t)__popcll(bw);
        }
      }
      if (DP) {  // the event into the wave's queue
        const uint64_t bi = ballot(ins_inline);
        if (ins_inline)
          dq[(dq_head + lanes_below(bi)) & (kDefQ - 1)] = make_uint2((uint32_t)(gi / kBW), ins_word(gi, li, pay, rl - (int)r0));
        dq_head += (uint32_t)__popcll(bi);
      } else if (any_ins) {  // the event into its bucket's page (written once)
        parse_place_event<big>(a, ins_inline, bkw + gi / kBW, npg, pbase, pg0, pcap, gi / kBW,
                               ins_word(gi, li, pay, rl - (int)r0));
      }
      if (last) {  // the read's last operation: i_end, downstream check, span
        const int ia = i + adv;
        const int ie = ia < 0 ? 0 : (ia > n ? n + 1 : ia);
        const int dnf = q_iend & (1 << 30);
        if (dnf && ia > n) te |= DE_INDEX;   // rightIndel(2*i) past the end
        // ... or, wrapped, past the front, or a RIGHT string at the odd
        // position n + ia (listed; i_end n + 1: no gap row for it)
        int iw = ie;
        if (NEG && dnf && ia < 0) {
          if (ia + n < 0) te |= DE_INDEX;
          else { te |= push_wo(a, gb + ia + n, rl, kWoDown, 0, 0); iw = n + 1; }
        }
        W.s_iend[q] = iw | dnf;
        const int ts = NEG && q_ts < 0 ? 0 : q_ts;  // matches below 0 write nothing
        const int e2 = ie > n ? n : ie;
        if (ts < e2) { depth_inc(ts); depth_dec(e2); }
      }
      if (te) flag_read(a, te, rl);
      G += atot;
      qc += __popcll(brs);
      MPC_SEG(4);
      return true;
    };
    // canonical rounds take the fast decode; a round holding any other unit is
    // redone on the general decode (one loop: measured against a loop per kind
    // and against per-window canonical checks, profiles/r06_experiments/)
    for (int t0 = 0; t0 < T; t0 += 64) {
      if (!round(t0, std::false_type{})) round(t0, std::true_type{});
      if (DP && dq_head - dq_tail >= 64u) defer_flush(64);
    }
    wave_sync_lds();
    // ---- reads that ended in this window: i_end; carry the open one ----
    if (l <= nst && (l > 0 || carry) && W.s_end[l] <= C) a.i_end[W.s_read[l]] = W.s_iend[l] & ~(1 << 30);
    const bool cont = (nst > 0 || carry) && W.s_end[nst] > C;
    if constexpr (lds_base<TM>())
      if (nst > 0) cb = uniform_i32(W.s_val[nst]);  // the base of the window's last read start
    if (cont) {
      const int64_t v = (int64_t)cb + G;
      c_base = (int32_t)(v > kICap ? kICap : v);
    }
    if (cont && l == 0) {
      W.s_end[0] = W.s_end[nst];
      W.s_ts[0] = W.s_ts[nst];
      W.s_read[0] = W.s_read[nst];
      W.s_iend[0] = W.s_iend[nst];
    }
    carry = cont;
    wave_sync_lds();
    P = Pn;
    rs0 = rsn;
    if (Pn < wend) cur = fetch_window<CH>(a, Pn, rsn, l);
    MPC_SEG(5);
  }
  // reads starting at the range end have an empty cs
  for (int64_t r = rs0 + l; r < rb; r += 64) {
    const int ts = a.tstart[r];
    flag_read(a, DE_OP, r);
    a.i_end[r] = ts < 0 ? 0 : (ts > n ? n + 1 : ts);
  }
  if (TM == 3 && l < a.sub_wins)
    a.subev_cnt[((int64_t)blockIdx.x * kMaxCh + chk) * kMaxSubWins + l] = S1 ? nsub_s : nsub_v;
  }  // chunks
  };
  if constexpr (NK) {
    if (wg_neg) chunks(std::true_type{});
    else chunks(std::false_type{});
  } else {
    chunks(std::false_type{});
  }
  if (DP && dq_head != dq_tail) defer_flush((int)(dq_head - dq_tail));  // (<= 63)
  MPC_SEG(5);
  __syncthreads();
  MPC_SEG(6);
  parse_epilogue<TM>(a, n, gb, nbk, hl, bkw, uni, npg, pbase, pcap);
#ifdef MPC_STAMPS
  MPC_SEG(7);
  const int64_t gw = (int64_t)blockIdx.x * kMaxPW + w;
  if (l < kStampSeg && gw < kStampWaves) {
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < kStampSeg; ++k) v = l == k ? st_acc[k] : v;
    g_stamps[gw * kStampSeg + l] = v;
  }
#endif
}


// ---------------------------------------------------------------------------
// K_subs (tally mode 3): the substitution events of a sample's parse waves for
// one kSubWin-position window, tallied in LDS as 16-bit counters (the event
// word IS the counter index: position << 2 | code; a block's chunk holds at most
// 65535 reads, and a read substitutes a position at most once) and stored as
// the block's slab row.  One block
// per (sample, window, chunk of <= kSubsWG parse workgroups); wave v walks the
// chunk's regions v, v + 16, ... (8 loads in flight per lane).
// ---------------------------------------------------------------------------
// K_subs blocks store their 16-bit tallies in a slab row each, reduced per
// (sample, window) by K_subsum (instead of every block adding its ~4 n counters
// into the same words with global atomics)
struct SubsArgs {
  const int4* work;    // {sample, window, first parse workgroup, end}
  const int4* pwork;   // parse work table {sample, r0, r1, 0}
  const int32_t* wave_tab;  // the parse chunks' read ranges (kMaxCh + 1 boundaries per workgroup)
  const int64_t* cs_off; int64_t cs_base;
  const uint16_t* subev; const uint32_t* subev_cnt; int64_t subev_cap;
  const int32_t* n_of; const int32_t* gbase; uint32_t* sub;
  uint32_t* slab;  // [K_subs block][kSubWin * 2] packed tallies
  int32_t nw_parse;
};
__global__ __launch_bounds__(1024) void K_subs(SubsArgs a) {
  __shared__ uint32_t cnt[kSubWin * 2];  // (position, code pair): codes 2h | 2h+1 in the halves
  const int4 wk = a.work[blockIdx.x];
  const int smp = wk.x, win = wk.y, pw0 = wk.z, pw1 = wk.w;
  const int nreg = (pw1 - pw0) * kMaxCh, l = lane(), v = threadIdx.x >> 6, nv = blockDim.x >> 6;
  for (int k = threadIdx.x; k < kSubWin * 2; k += blockDim.x) cnt[k] = 0;
  __syncthreads();
  for (int rg = v; rg < nreg; rg += nv) {
    const int pw = pw0 + rg / kMaxCh, ww = rg % kMaxCh;  // parse workgroup, chunk
    if (ww >= a.pwork[pw].w) continue;
    const int64_t ra = a.wave_tab[(int64_t)pw * (kMaxCh + 1) + ww];  // the chunk's first read
    const int c = (int)a.subev_cnt[((int64_t)pw * kMaxCh + ww) * kMaxSubWins + win];
    const uint16_t* src = a.subev + (int64_t)win * a.subev_cap + (a.cs_off[ra] - a.cs_base) / kSubEvBytes + 2 * ra;
    auto tally = [&](uint32_t ev) { atomicAdd(&cnt[ev >> 1], 1u << (16 * (ev & 1u))); };
    // 16-byte loads (8 events per lane each, 4 in flight): the region's events up
    // to the first 16-byte boundary and after the last whole group one per lane
    const int head = min(c, (int)(((16u - ((uint32_t)(uintptr_t)src & 15u)) & 15u) >> 1));
    if (l < head) tally(src[l]);
    const uint4* body = reinterpret_cast<const uint4*>(src + head);
    const int ng = (c - head) >> 3;
    for (int q0 = 0; q0 < ng; q0 += 4 * 64) {
      uint4 g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = q0 + l + 64 * u;
        g[u] = q < ng ? body[q] : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (q0 + l + 64 * u >= ng) continue;
        const uint32_t w4[4] = {g[u].x, g[u].y, g[u].z, g[u].w};
#pragma unroll
        for (int h = 0; h < 4; ++h) { tally(w4[h] & 0xffffu); tally(w4[h] >> 16); }
      }
    }
    const int t0 = head + 8 * ng;
    if (t0 + l < c) tally(src[t0 + l]);  // (< 8 events)
  }
  __syncthreads();
  const int64_t p0 = (int64_t)win * kSubWin, n = a.n_of[smp];
  // the window's positions (< n), two words each, coalesced
  uint32_t* row = a.slab + (int64_t)blockIdx.x * (kSubWin * 2);
  const int nw2 = (int)(2 * (n - p0 < kSubWin ? n - p0 : kSubWin));
  for (int j = threadIdx.x; j < nw2; j += blockDim.x) row[j] = cnt[j];
}

// K_subsum: per (sample, window, 256 slab words): the sum over the window's
// K_subs blocks (4 groups of rows per thread column, 8 loads in flight each,
// LDS reduce), stored into the substitution tallies (the only writer of a mode-3
// window's words).  work: {sample, window, first block, end block}.
constexpr int kSumCols = 256;
template <int RG>  // row groups: 4 when windows have many slab rows (C3: 256), else 1 (C5: ~5)
__global__ __launch_bounds__(kSumCols * RG) void K_subsum(const int4* work, const uint32_t* slab, const int32_t* n_of,
                                                          const int32_t* gbase, uint32_t* sub) {
  __shared__ uint32_t part[RG][kSumCols][2];
  constexpr int kChunks = kSubWin * 2 / kSumCols;
  const int4 wk = work[blockIdx.x / kChunks];
  const int x = threadIdx.x & (kSumCols - 1), y = threadIdx.x / kSumCols;
  const int64_t p0 = (int64_t)wk.y * kSubWin, n = n_of[wk.x];
  const int nw2 = (int)(2 * (n - p0 < kSubWin ? n - p0 : kSubWin));
  const int j = (int)(blockIdx.x % kChunks) * kSumCols + x;
  uint32_t lo = 0, hi = 0;
  if (j < nw2) {
    for (int b0 = wk.z + y; b0 < wk.w; b0 += RG * 8) {
      uint32_t v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int b = b0 + RG * u;
        v[u] = b < wk.w ? slab[(int64_t)b * (kSubWin * 2) + j] : 0u;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) { lo += v[u] & 0xffffu; hi += v[u] >> 16; }
    }
  }
  part[y][x][0] = lo;
  part[y][x][1] = hi;
  __syncthreads();
  if (y == 0 && j < nw2) {
    lo = 0;
    hi = 0;
#pragma unroll
    for (int r = 0; r < RG; ++r) { lo += part[r][x][0]; hi += part[r][x][1]; }
    uint32_t* dst = sub + ((int64_t)gbase[wk.x] + p0) * 4 + 2 * j;  // word j: position j / 2, codes 2 (j & 1) + {0, 1}
    dst[0] = lo;
    dst[1] = hi;
  }
}

}  // namespace

// Host side: the parse launches
static ParseArgs parse_args(const mpc_plan* p, const Dev& d) {
  ParseArgs a;
  a.cs = d.cs; a.cs_off = d.cs_off; a.tstart = d.tstart; a.up_off = d.up_off; a.down_off = d.down_off;
  a.n_of = d.n_of; a.gbase = d.gbase;
  a.work = reinterpret_cast<const int4*>(p->ws + p->off[mpc_plan::B_WPARSE]);
  a.wave_tab = at<const int32_t>(p, mpc_plan::B_WWAVE);
  a.cs_base = d.cs_base; a.ovf_cap = d.ovf_cap; a.read_offset = d.read_offset; a.n_reads = d.N;
  a.nbs = p->nbmax;
  a.i_end = d.i_end;
  a.ins_sorted = at<uint32_t>(p, mpc_plan::B_INSSORT);
  a.pg_own = at<uint32_t>(p, mpc_plan::B_PGOWN); a.pg_list = at<uint32_t>(p, mpc_plan::B_PGLIST);
  a.bk_cnt = at<int32_t>(p, mpc_plan::B_BKCNT); a.bk_off = at<int32_t>(p, mpc_plan::B_BKOFF);
  a.rbase = at<int64_t>(p, mpc_plan::B_RBASE); a.bk_cur = at<uint32_t>(p, mpc_plan::B_BKCUR);
  a.ovf = d.ovf; a.ovf_cnt = d.ovf_cnt; a.hasleft = d.hasleft; a.status = d.status;
  a.diff = d.diff; a.sub = d.sub;
  a.subev = at<uint16_t>(p, mpc_plan::B_SUBEV); a.subev_cnt = at<uint32_t>(p, mpc_plan::B_SUBCNT);
  a.subev_cap = p->subev_cap; a.sub_wins = p->tally_mode == 3 ? p->sub_wins : 0;
  a.wo = d.wo; a.wo_cap = d.wo_cap;
  a.defer_off = p->defer_off;
  return a;
}

// instantiated (tally mode, window) pairs; packed modes only with 1 and 2 KiB windows
template <bool NK>
static const void* parse_kernel_t(int tm, int win, bool s1) {
  if (tm == 4) return (const void*)K_parse<4, 1024, NK>;
  if (tm == 2) return win == 1024 ? (const void*)K_parse<2, 1024, NK> : (const void*)K_parse<2, 2048, NK>;
  if (tm == 3 && s1)
    return win == 1024 ? (const void*)K_parse<3, 1024, NK, true> : (const void*)K_parse<3, 2048, NK, true>;
  if (tm == 3) return win == 1024 ? (const void*)K_parse<3, 1024, NK> : (const void*)K_parse<3, 2048, NK>;
  if (win == 512) return tm ? (const void*)K_parse<1, 512, NK> : (const void*)K_parse<0, 512, NK>;
  if (win == 2048) return tm ? (const void*)K_parse<1, 2048, NK> : (const void*)K_parse<0, 2048, NK>;
  return tm ? (const void*)K_parse<1, 1024, NK> : (const void*)K_parse<0, 1024, NK>;
}
// the plan's K_parse: with the negative-start rounds only when it holds such reads
static const void* parse_kernel(const mpc_plan* p) {
  const bool s1 = p->tally_mode == 3 && p->sub_wins == 1;
  if (p->defer_off > 0)  // (planner: 2 KiB windows, tally mode 1 or 3 with s1, no negative starts)
    return p->tally_mode == 1 ? (const void*)K_parse<1, 2048, false, false, true>
                              : (const void*)K_parse<3, 2048, false, true, true>;
  return p->in.neg_reads > 0 ? parse_kernel_t<true>(p->tally_mode, p->parse_win, s1)
                             : parse_kernel_t<false>(p->tally_mode, p->parse_win, s1);
}
static void launch_subs(const mpc_plan* p, const Dev& d, hipStream_t st) {
  if (p->work_sub.empty()) return;
  SubsArgs a;
  a.work = at<const int4>(p, mpc_plan::B_WSUB); a.pwork = at<const int4>(p, mpc_plan::B_WPARSE);
  a.cs_off = d.cs_off; a.cs_base = d.cs_base;
  a.subev = at<uint16_t>(p, mpc_plan::B_SUBEV); a.subev_cnt = at<uint32_t>(p, mpc_plan::B_SUBCNT);
  a.subev_cap = p->subev_cap; a.n_of = d.n_of; a.gbase = d.gbase; a.sub = d.sub; a.nw_parse = p->parse_nw;
  a.wave_tab = at<const int32_t>(p, mpc_plan::B_WWAVE);
  a.slab = at<uint32_t>(p, mpc_plan::B_SUBSLAB);
  hipLaunchKernelGGL(K_subs, dim3((unsigned)(p->work_sub.size() / 4)), dim3(1024), 0, st, a);
  const dim3 g((unsigned)(p->work_subsum.size() / 4 * (kSubWin * 2 / kSumCols)));
  if (p->subsum_rows > 8)
    hipLaunchKernelGGL(K_subsum<4>, g, dim3(4 * kSumCols), 0, st, at<const int4>(p, mpc_plan::B_WSUBSUM),
                       (const uint32_t*)a.slab, d.n_of, d.gbase, d.sub);
  else
    hipLaunchKernelGGL(K_subsum<1>, g, dim3(kSumCols), 0, st, at<const int4>(p, mpc_plan::B_WSUBSUM),
                       (const uint32_t*)a.slab, d.n_of, d.gbase, d.sub);
}
static void launch_parse(const mpc_plan* p, const Dev& d, hipStream_t st) {
  ParseArgs a = parse_args(p, d);
  void* args[] = {&a};
  (void)hipLaunchKernel(parse_kernel(p), dim3(p->n_parse_wg), dim3(p->parse_nw * 64), args, (size_t)p->parse_lds, st);
}
