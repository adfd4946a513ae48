// mpc_cswalk.h -- the one device tokenizer of the short-form cs grammar of
// include/mpc_coverage.h, shared by K_covparse (mpc_cov.hip) and K_lnkparse
// (mpc_link.hip).  One wave64 walks one record, one 64-byte chunk at a time:
// classify the byte per lane, ballot the operators, let every operator lane own
// its token (lane 0 owns the token still open from the chunk before), read the
// token's reference advance, prefix-scan the advances over the wave to give
// every token its p.  Carried from chunk to chunk (wave-uniform): p, the open
// operator, the number read so far and its digit count / the letters of an open
// run.  A '-' run that crosses a chunk is seen in pieces; ':' and '*' take
// effect where they close.
//
// What a token DOES is the effects policy Fx:
//   static constexpr bool kBase     the policy wants the substituted base of *xy
//                                   (then it has a member `uint32_t lastb`, the
//                                   last byte of the chunk before: a *xy whose
//                                   letters end a chunk and which is closed by an
//                                   operator in lane 0 has left the registers)
//   carried_match(num)              an open :N closed in lane 0 (all lanes call)
//   carried_sub()                   an open *xy closed in lane 0 (lane 0 calls) ...
//   carried_sub_at(p)               ... and where, when that is inside the target
//   count(...)                      per-lane tallies of the chunk's tokens
//   look(p0, p1)                    wave-uniform: can the chunk's reference range
//                                   [p0, p1] hold an effect at all
//   emit(hit, del, pos, reach, y)   one token's effect (divergent): a mismatch at
//                                   pos with read base y, a deletion piece
//                                   [pos, reach), else an insertion before pos
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpc_coverage.h"
#include "mpc_device.h"

namespace mpc {

typedef long long cs_i64;
typedef unsigned long long cs_u64;

constexpr int kCsK = 4;  // 64-byte chunks per tile
constexpr int kCsTile = 64 * kCsK;
constexpr int kCsFastAdv = 1 << 25;  // 32 tokens of a chunk x this stays inside 32 bits

// wave-uniform state of a record's walk
struct Walk {
  cs_i64 p;        // current position (at most L while !oor)
  uint32_t num;    // value of an open number
  int32_t op, cnt; // open operator (0: none) and its operand bytes so far
  bool bad, oor;
};

__device__ __forceinline__ uint32_t rl(uint32_t v, int j) { return (uint32_t)__builtin_amdgcn_readlane((int)v, j); }
__device__ __forceinline__ cs_i64 rl64(cs_i64 v, int j) {
  return (cs_i64)(((cs_u64)rl((uint32_t)((cs_u64)v >> 32), j) << 32) | rl((uint32_t)v, j));
}

// one 64-byte chunk: lane ln holds byte c (valid below nvalid); last: the cs ends in this chunk
template <class Fx>
__device__ __forceinline__ void cs_chunk(const uint32_t c, const int nvalid, const bool last, const uint32_t L,
                                         const uint64_t lemask, Fx& fx, Walk& w) {
  const int ln = lane();
  const bool valid = ln < nvalid;
  const uint32_t x = c - 0x2au;  // '*' 0, '+' 1, '-' 3, ':' 16
  const bool isop = valid && x <= 16u && ((0x1000bu >> x) & 1u);
  const bool isdig = (c - '0') < 10u;
  const bool islet = ((c | 32u) - 'a') < 26u;
  const uint64_t opm = ballot(isop);
  const uint64_t colons = ballot(isop && c == ':');
  bool lbad = false, loor = false;
  cs_i64 p0 = w.p;
  const cs_i64 p_in = p0;

  // the token left open by the chunk before ends at an operator in lane 0
  if ((opm & 1ull) && w.op) {
    if (w.op == ':') {
      if (w.cnt < 1) lbad = true;
      else { fx.carried_match(w.num); p0 += w.num; }
    } else if (w.op == '*') {
      if (w.cnt != 2) lbad = true;
      else {
        if (ln == 0) {
          fx.carried_sub();
          if (!w.oor) { if (p0 < (cs_i64)L) fx.carried_sub_at((uint32_t)p0); else loor = true; }
        }
        p0 += 1;
      }
    } else if (w.cnt < 1) lbad = true;
    if (p0 > (cs_i64)L) w.oor = true;
  }

  // the operator that governs this lane's byte: the highest operator at or below the lane, else the open one
  const uint64_t below = opm & lemask;
  const bool gov_colon = below ? (below & colons) > (below & ~colons) : w.op == ':';
  // (an operand byte before any operator has no governor)
  lbad |= valid && !isop && ((!below && !w.op) || (gov_colon ? !isdig : !islet));

  // token owners: operator lanes, and lane 0 for the open token when it continues here
  const bool own = isop || (ln == 0 && valid);
  const uint32_t kind = isop ? c : (uint32_t)w.op;
  const int s = isop ? ln + 1 : 0;                  // first operand lane
  const uint64_t above = s < 64 ? opm >> s : 0ull;  // operators from there on
  const int nx = above ? s + __ffsll((cs_i64)above) - 1 : nvalid;
  const int cnt = nx - s;                           // operand bytes in this chunk
  const bool closed = above != 0 || last;
  const int tot = (isop ? 0 : w.cnt) + cnt;
  const bool isnum = own && kind == ':' && tot <= 9;
  uint32_t v = isop ? 0u : w.num;
  for (int d = 0; d < 9; ++d) {
    if (!ballot(isnum && d < cnt)) break;
    const uint32_t dg = (uint32_t)__shfl((int)c, s + d < 63 ? s + d : 63, 64) - '0';
    if (isnum && d < cnt) v = (v << 3) + (v << 1) + dg;  // (shift-adds: v_mul_lo_u32 is quarter rate)
  }

  // what the token does, as selects: nested branches on the kind cost more than the arithmetic
  const bool k_num = own && kind == ':', k_sub = own && kind == '*', k_del = own && kind == '-', k_ins = own && kind == '+';
  lbad |= (k_num && (tot > 9 || (closed && tot < 1))) || (k_sub && (tot > 2 || (closed && tot != 2))) ||
          ((k_del || k_ins) && closed && tot < 1);
  const bool num_close = k_num && closed && tot >= 1 && tot <= 9;
  const bool hit = k_sub && closed && tot == 2;  // a mismatch closes here
  const int adv = num_close ? (int)v : hit ? 1 : k_del ? cnt : 0;
  fx.count(num_close, v, hit, k_del, k_ins, cnt, isop);
  if (!isnum) v = 0;

  // every token's p: a wave prefix scan of the advances (32-bit while no run is longer than 2^25)
  uint32_t pos;
  if (!ballot(adv > kCsFastAdv)) {
    const int incl = wave_scan_i32(adv);
    pos = (uint32_t)p0 + (uint32_t)(incl - adv);
    w.p = p0 + wave_last_i32(incl);
  } else {
    const cs_i64 incl = wave_incl_scan<cs_i64>((cs_i64)adv);
    const cs_i64 at = p0 + incl - adv;
    pos = at > (cs_i64)L ? 0x80000000u : (uint32_t)at;  // (past L: refused below whatever it is)
    w.p = p0 + rl64(incl, 63);
  }

  // at most two words per token: a point, or the two ends of a deletion piece
  const bool del_piece = k_del && cnt > 0, ins_at = k_ins && isop;
  const uint32_t reach = pos + (del_piece ? (uint32_t)cnt : 0u);
  const bool wants = hit || del_piece || ins_at;
  const bool fits = hit ? pos < L : reach <= L;
  loor = loor || (wants && !w.oor && !fits);
  uint32_t y = 0;
  if constexpr (Fx::kBase) {
    // the second letter of *xy: the token's last operand byte of this chunk (a closing *xy has one here)
    if (ballot(hit)) y = (uint32_t)__shfl((int)c, (s + cnt - 1) & 63, 64);
  }
  if (fx.look(p_in, w.p) && wants && fits && !w.oor) fx.emit(hit, del_piece, pos, reach, y);

  // what stays open
  if (nvalid > 0) {
    const int j = uniform_i32(opm ? 63 - __clzll((cs_i64)opm) : 0);
    if (opm) w.op = (int32_t)rl(c, j);
    w.cnt = (int32_t)rl((uint32_t)tot, j);
    w.num = rl(v, j);
    if constexpr (Fx::kBase) fx.lastb = rl(c, nvalid - 1);
  }
  w.bad |= ballot(lbad) != 0;
  w.oor |= ballot(loor) != 0 || w.p > (cs_i64)L;
}

__device__ __forceinline__ void cs_load_tile(uint32_t (&bt)[kCsK], const uint8_t* q, int len, int t0) {
#pragma unroll
  for (int k = 0; k < kCsK; ++k) {
    const int i = t0 + k * 64 + lane();
    bt[k] = i < len ? (uint32_t)__builtin_nontemporal_load(q + i) : 0u;
  }
}

// The status key both walks keep between their two kernels: record r failed with
// `code`.  The smallest record wins, malformed before out of range: the largest
// inverted key.
__device__ __forceinline__ void cs_report(cs_u64* key_slot, cs_i64 r, int code) {
  const cs_u64 key = ~((cs_u64)r * 2 + (code == MPC_COV_RANGE ? 1 : 0));
  __hip_atomic_fetch_max(key_slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ... and the decoding of a key that is not 0 (0: no record failed) into status = {code, record}
__device__ __forceinline__ void cs_status(cs_u64 key, int32_t* __restrict__ status) {
  const cs_u64 v = ~key;
  status[0] = (v & 1) ? MPC_COV_RANGE : MPC_COV_MALFORMED;
  status[1] = (int32_t)(v >> 1);
}

}  // namespace mpc
