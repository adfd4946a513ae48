// mpc_verify.hip -- K_vscan: batched, exact, score-only Sellers scan on gfx950
// (include/mpc_verify.h; DESIGN.md "verify_consensus").
//
// One wave64 per (query, text) pair, no LDS, no atomics, no cross-wave traffic.
// The query is cut into blocks of 64 rows held as Myers/Hyyro bit vectors; lane
// l owns the K consecutive blocks [l K, (l + 1) K).  The lanes form a systolic
// array over the text: in step s lane l runs text column s - l through its K
// blocks, top to bottom, and hands the horizontal delta leaving its last block
// together with the column's symbol to lane l + 1 (one DPP wave shift per step).
// Lane 0 enters every column with delta 0: the text start is free.  The lane
// that owns the query's last row follows D[m][j] and keeps its first minimum.
// Every loop bound follows from m and n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "mpc.h"
#include "mpc_bandtrace.h"
#include "mpc_device.h"
#include "mpc_launch.h"
#include "mpc_verify.h"

namespace {
using namespace mpc;
using namespace mpc_band;

constexpr uint32_t kNoColumn = 7;  // symbol slot of a step that carries no text column

// lane l reads lane l - 1 (wave_shr:1 over the 64 lanes; lane 0 reads 0).  Must
// run with every lane enabled: a disabled source lane reads as 0.
__device__ __forceinline__ uint32_t from_lane_below(uint32_t v) { return (uint32_t)dpp_i32<0x138>((int)v); }

__device__ __forceinline__ uint64_t splat(bool p) {
  const uint32_t w = 0u - (uint32_t)p;
  return ((uint64_t)w << 32) | w;
}

template <int K>
__device__ __forceinline__ void vscan_pair(const uint8_t* __restrict__ q, const int32_t m,
                                           const uint8_t* __restrict__ t, const int64_t n,
                                           int32_t* __restrict__ out) {
  const int ln = lane();
  const int nblk = (m + 63) >> 6;
  const int L = (nblk + K - 1) / K;                          // lanes in use
  const int last_k = ln == L - 1 ? nblk - 1 - ln * K : -1;   // this lane's block that holds row m
  const int top = (m - 1) & 63;                              // row m's bit in that block

  uint64_t Pv[K], Mv[K], Pa[K], Pc[K], Pg[K], Pt[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    Pv[k] = ~0ull;
    Mv[k] = 0;
    uint64_t a = 0, c = 0, g = 0, tt = 0;
    const int64_t r0 = ((int64_t)ln * K + k) * 64;
    for (int i = 0; i < 64; ++i) {
      const int64_t r = r0 + i;
      const uint32_t x = r < m ? vcode(q[r], 4) : 4;
      a |= (uint64_t)(x == 0) << i;
      c |= (uint64_t)(x == 1) << i;
      g |= (uint64_t)(x == 2) << i;
      tt |= (uint64_t)(x == 3) << i;
    }
    Pa[k] = a; Pc[k] = c; Pg[k] = g; Pt[k] = tt;
  }

  int32_t score = m, best = m, best_end = 0;  // D[m][0] = m; only a strictly smaller value moves the end
  uint32_t handed = kNoColumn << 2;           // what this lane left for lane l + 1: hp | hm << 1 | symbol << 2
  uint32_t tbuf = kNoColumn;                  // 64 text symbols, one per lane
  const int64_t steps = n > 0 ? n + L - 1 : 0;
  for (int64_t s = 0; s < steps; ++s) {
    if ((s & 63) == 0) {                      // next 64 text bytes, coalesced
      const int64_t j = s + ln;
      tbuf = j < n ? vcode(t[j], 5) : kNoColumn;
    }
    uint32_t in = from_lane_below(handed);
    const uint32_t head = (uint32_t)__builtin_amdgcn_readlane((int)tbuf, (int)(s & 63));
    if (ln == 0) in = head << 2;
    const uint32_t sym = in >> 2;
    handed = kNoColumn << 2;
    if (sym != kNoColumn && ln < L) {
      uint32_t hp = in & 1u, hm = (in >> 1) & 1u;  // incoming horizontal delta +1 / -1
      // all-ones for the column's base, all-zero otherwise (codes 4, 5: no match mask); masks, not
      // selects: the compiler turns a select chain over 64-bit values into branches
      const uint64_t sa = splat(sym == 0), sc = splat(sym == 1), sg = splat(sym == 2), st = splat(sym == 3);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        uint64_t Eq = (Pa[k] & sa) | (Pc[k] & sc) | (Pg[k] & sg) | (Pt[k] & st);
        const uint64_t pv = Pv[k], mv = Mv[k];
        const uint64_t Xv = Eq | mv;
        Eq |= (uint64_t)hm;
        const uint64_t Xh = (((Eq & pv) + pv) ^ pv) | Eq;
        uint64_t Ph = mv | ~(Xh | pv);
        uint64_t Mh = pv & Xh;
        if (k == last_k) score += (int32_t)((Ph >> top) & 1u) - (int32_t)((Mh >> top) & 1u);
        const uint32_t hp_out = (uint32_t)(Ph >> 63), hm_out = (uint32_t)(Mh >> 63);
        Ph = (Ph << 1) | hp;
        Mh = (Mh << 1) | hm;
        Pv[k] = Mh | ~(Xv | Ph);
        Mv[k] = Ph & Xv;
        hp = hp_out;
        hm = hm_out;
      }
      handed = hp | (hm << 1) | (sym << 2);
      if (last_k >= 0 && score < best) {
        best = score;
        best_end = (int32_t)(s - ln + 1);
      }
    }
  }
  if (ln == L - 1) {
    out[0] = best;
    out[1] = best_end;
  }
}

// grid: one 64-thread workgroup per pair
__global__ __launch_bounds__(64) void K_vscan(const uint8_t* __restrict__ seq, const int64_t* __restrict__ pairs,
                                              int32_t* __restrict__ out) {
  const int64_t p = blockIdx.x;
  const int64_t q_off = pairs[4 * p], m64 = pairs[4 * p + 1], t_off = pairs[4 * p + 2], n = pairs[4 * p + 3];
  int32_t* o = out + 2 * p;
  // restates check_pair of mpc_bandtrace.h, which the host applies before the launch (its n < 2^31 is not
  // needed here: every loop bound is 64-bit)
  if (m64 < 1 || m64 > MPC_VERIFY_MAX_QUERY || n < 0 || q_off < 0 || t_off < 0) {
    if (threadIdx.x == 0) { o[0] = -1; o[1] = -1; }
    return;
  }
  const int32_t m = (int32_t)m64;
  const uint8_t* q = seq + q_off;
  const uint8_t* t = seq + t_off;
  // the smallest K with 64 lanes x K blocks x 64 rows >= m
  if (m <= 4096) vscan_pair<1>(q, m, t, n, o);
  else if (m <= 8192) vscan_pair<2>(q, m, t, n, o);
  else if (m <= 16384) vscan_pair<4>(q, m, t, n, o);
  else if (m <= 32768) vscan_pair<8>(q, m, t, n, o);
  else vscan_pair<16>(q, m, t, n, o);
}

}  // namespace

extern "C" int mpc_verify_scan(const uint8_t* d_seq, const int64_t* d_pairs, int32_t n_pairs, int32_t* d_out,
                               void* stream) {
  if (n_pairs < 0) return mpc_fail_(MPC_E_ARG, "mpc_verify_scan: n_pairs < 0");
  if (n_pairs == 0) return MPC_OK;
  if (!d_seq || !d_pairs || !d_out) return mpc_fail_(MPC_E_ARG, "mpc_verify_scan: null pointer");
  hipStream_t st = (hipStream_t)stream;
  std::vector<int64_t> h;
  if (const int rc = mpc_launch::read_back<int64_t>(st, {{d_pairs, (size_t)n_pairs * 4}}, h, "mpc_verify_scan", "pair table"))
    return rc;
  for (int32_t p = 0; p < n_pairs; ++p)
    if (const int bad = check_pair(&h[(size_t)p * 4]))
      return mpc_fail_(MPC_E_ARG, ("mpc_verify_scan: pair " + std::to_string(p) + ": " + fault_text(bad)).c_str());
  hipLaunchKernelGGL(K_vscan, dim3((unsigned)n_pairs), dim3(64), 0, st, d_seq, d_pairs, d_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mpc_launch::hip_fail("mpc_verify_scan", "K_vscan", e);
  return MPC_OK;
}
