// The layout phase (mpc_layout): K_layout, the replay of the slot creation of
// processBaseString_leftIndel / _rightIndel (:37-72), then the row offsets.
// Per gap the list grows at the front (LEFT, right-justified) and at the back
// (RIGHT, left-justified).  State: lo = slots prepended, hi = slots appended.
//   LEFT  len L : base bi -> absolute hi-1-bi ; lo = max(lo, L-hi)
//   RIGHT len R : base bi -> absolute -lo+bi  ; hi = max(hi, R-lo)
// Within a run of LEFT events hi is constant, so only the run's longest LEFT
// string matters (M); run k is closed by the gap's k-th mixed RIGHT event
// (length runR).  One thread per gap replays its runs; the row counts and the
// depth difference array are then scanned in the same launch (K_layout, kGB
// gaps per block).
#pragma once

#include "mpc_k_common.h"
#include "mpc_k_wrap.h"  // wo_lower

namespace {

// K_layout = K_replay + K_assemble in ONE launch: the per-gap replay, then the
// row offsets and depths as block scans chained across blocks by a decoupled
// look-back (per block two 64-bit status words, rows and depth difference, each
// {flag, launch epoch, value}: flag 1 = the block's own sum, 2 = its inclusive
// prefix).  Blocks are dispatched in index order, so a block waits only on
// running or finished blocks; the spin is bounded (DE_INTERNAL, never a hang).
// The row capacity is checked per gap (rows that do not fit are not written);
// the last block sets ROWS_NEEDED and DE_CAP for the re-plan.
// WO: the plan lists wrapped odd positions (K_woprep); such a position after
// gap g is replayed here too and takes F rows instead of one.
template <bool WO>
__global__ __launch_bounds__(kGB) void K_layout(Dev d, uint32_t epoch) {
  __shared__ int32_t s_w[2][kGB / 64];
  __shared__ int64_t s_pre[2];
  const int64_t b = blockIdx.x;
  const int64_t nb = (d.G + kGB - 1) / kGB;
  const int64_t g = b * kGB + threadIdx.x;
  int32_t rc = 0, dv = 0;
  int32_t F = 1, wop = -1;  // rows of the odd position after the gap; its listed index
  int s = 0;
  int64_t p = 0;
  if (g < d.G) {
    const int64_t r0 = (int64_t)d.right_start[g] + g, r1 = (int64_t)d.right_start[g + 1] + g + 1;  // runs of gap g
    int32_t lo = 0, hi = 0;
    for (int64_t t = r0; t < r1; ++t) {
      d.hiR[t] = hi;                          // hi seen by the run's LEFT events
      const int32_t m = d.M[t];
      if (m - hi > lo) lo = m - hi;
      if (t + 1 < r1) {
        d.loR[t] = lo;                        // lo seen by the RIGHT event closing the run
        const int32_t R = d.runR[t];
        if (R - lo > hi) hi = R - lo;
      }
    }
    // RIGHT-only gaps: their flanks were not sorted; slot bi = base bi
    const int32_t mr = d.maxR[g];
    if (mr - lo > hi) hi = mr - lo;
    d.lo_f[g] = lo;
    int lo_s = 0, hi_s = d.S - 1;  // sample of gap g
    while (lo_s < hi_s) {
      const int mid = (lo_s + hi_s + 1) >> 1;
      if (d.gbase[mid] <= g) lo_s = mid; else hi_s = mid - 1;
    }
    s = lo_s;
    p = g - d.gbase[s];
    if constexpr (WO) {
      const int np = (int)d.status[MPC_ST_WRAP_POS];
      const int k = wo_lower(d.wo_pos, np, g);
      if (p < d.n_of[s] && k < np && d.wo_pos[k].g == g) {
        // lo / hi of the odd position over its runs; a run's one-base writes
        // are a LEFT string of length 1
        const WoPos P = d.wo_pos[k];
        int32_t wl = 0, wh = 0;
        for (int32_t j = 0; j < P.nrun; ++j) {
          WoRun& R = d.wo_run[P.run0 + j];
          const int32_t c1 = (R.C[0] | R.C[1] | R.C[2] | R.C[3]) != 0u ? 1 : 0;
          const int32_t m = R.M > c1 ? R.M : c1;
          R.hiR = wh;
          if (m - wh > wl) wl = m - wh;
          if (j + 1 < P.nrun) {
            R.loR = wl;
            if (R.R - wl > wh) wh = R.R - wl;
          }
        }
        F = wl + wh;
        wop = k;
        d.wo_pos[k].lo = wl;
        d.wo_pos[k].F = F;
      }
    }
    rc = lo + hi + (p < d.n_of[s] ? F : 0);  // rows of a gap = its slots + the odd position after it
    d.rowcnt[g] = rc;
    dv = d.diff[g];
  }
  // [2 nb] look-back words: block b's rows word, diff word
  const int v[2] = {rc, dv};
  int inc[2], bt[2];
  int64_t pre[2];
  chain_scan<kGB / 64, 2>(reinterpret_cast<uint64_t*>(d.bsum), b, epoch, v, inc, bt, pre, s_w, s_pre, &d.status[MPC_ST_FLAGS]);
  if (b == nb - 1 && threadIdx.x == 0) {
    const int64_t tot = pre[0] + bt[0];
    d.status[MPC_ST_ROWS_NEEDED] = (uint32_t)tot;
    if (tot > d.row_cap) atomicOr(&d.status[MPC_ST_FLAGS], DE_CAP);
  }
  if (g >= d.G) return;
  const int64_t rb = pre[0] + inc[0] - rc;  // exclusive
  const int64_t dep = pre[1] + inc[1];      // inclusive
  d.row_base[g] = (int32_t)rb;
  if (p == 0) d.srow[s] = (int32_t)rb;  // the consensus kernels' sample table (one load, no gbase chain)
  if (rb + rc > d.row_cap) return;      // does not fit: the last block flags DE_CAP (re-plan)
  const int64_t n = d.n_of[s];
  const int64_t nslots = (int64_t)rc - (p < n ? F : 0);
  if (nslots > 0) d.meta[rb] = 2;  // first slot of the gap
  if (p < n) {
    // each shard: its own reads' depth and substitutions (rows are summed over shards)
    // odd position p: depth = reads covering p with a match or substitution
    const uint32_t* sb = d.sub + g * 4;
    const uint32_t s0 = sb[0], s1 = sb[1], s2 = sb[2], s3 = sb[3];
    const int64_t match = dep - (int64_t)s0 - s1 - s2 - s3;
    uint32_t c[4] = {s0, s1, s2, s3};
    uint32_t fl = 0;
    if (match < 0) fl |= DE_INTERNAL;
    else if (match > 0) {
      const int rcode = base_code_exact(d.ref[d.ref_off[s] + p]);
      if (rcode < 0) fl |= DE_KEY;  // refarr base not in the dict (:61)
      else c[rcode] += (uint32_t)match;
    }
    if (fl) atomicOr(&d.status[MPC_ST_FLAGS], fl);
    if (WO && wop >= 0) d.wo_pos[wop].row0 = (int32_t)(rb + nslots);  // rows by K_worows
    else reinterpret_cast<uint4*>(d.rows)[rb + nslots] = make_uint4(c[0], c[1], c[2], c[3]);
    d.meta[rb + nslots] = 3;  // odd row, first slot of its position
  }
}

}  // namespace
