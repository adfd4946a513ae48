// The rows phase (mpc_rows): the bases of the strings of :37-72 onto the slot
// rows the layout gave them -- K_ins the insertions, K_flank the upstream and
// downstream flanks, K_worows the strings in wrapped odd positions.
#pragma once

#include <algorithm>

#include "mpc_k_common.h"
#include "mpc_k_index.h"  // run_left
#include "mpc_k_wrap.h"   // wo_listed, wo_lower, wo_len

namespace {

// ---------------------------------------------------------------------------
// Slot tallies of the even positions (:37-72 applied to insertion strings).
// A LEFT string's base bi (from the 3' end) lands on slot hi_run - 1 - bi of
// its gap, so K_left tallies the inline insertions per (run, bi, base) and
// K_ins maps every run onto its rows once the layout gives hi_run.  A
// grid-stride tail adds the long insertions (bases re-read from cs).
// ---------------------------------------------------------------------------

struct InsArgs {
  uint32_t* status; const int32_t* sample; const int32_t* gbase;
  int64_t read_offset, ovf_cap, G;
  const int32_t* right_start; const int32_t* rsl; const int32_t* roff; const int32_t* vals_out;
  const int32_t* row_base; const int32_t* lo_f; const int32_t* hiR;
  uint32_t* rows; const Ovf* ovf; const uint32_t* ovf_cnt; const uint8_t* cs;
  uint32_t* runt;
};

__global__ __launch_bounds__(kUB) void K_ins(InsArgs a) {
  const int l = lane();
  const int w = uniform_i32((int)(threadIdx.x >> 6));
  const bool cap = (a.status[MPC_ST_FLAGS] & DE_CAP) != 0;  // rows too small: only clear runt
  // inline insertions: K_left left their bases per run, indexed by the slot
  // from the run's right end; the layout gives the run's rows (one thread per
  // gap, over the gap's runs; LEFT base bi -> row row_base + lo_f + hi_run - 1 - bi)
  // wave-interleaved over the blocks (64 consecutive gaps per wave, consecutive
  // waves on different CUs): a few thousand gaps must not land on a few CUs
  // a gap with ONE run and no long insertions anywhere: its inline-insertion
  // rows get contributions from this thread only (rows are zero before K_ins;
  // K_flank adds after it), so a 16-byte store per non-empty slot replaces four
  // scattered atomics (C5: ~6 M atomics, 300 of K_ins' 330 us)
  const bool no_ovf = *a.ovf_cnt == 0;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t gw = (int64_t)w * gridDim.x + blockIdx.x; gw * 64 < a.G; gw += nwaves) {
    const int64_t g = gw * 64 + l;
    if (g >= a.G) continue;
    // this shard's runs of the gap (one GPU: all of them): a shard's LEFT
    // events fall into the runs its own reads span, [roff, roff + its mixed
    // RIGHT events of the gap]; K_left wrote nothing into the others
    const int64_t t0 = (int64_t)a.right_start[g] + g + a.roff[g], t1 = t0 + (a.rsl[g + 1] - a.rsl[g]) + 1;
    const int64_t top = (int64_t)a.row_base[g] + a.lo_f[g] - 1;
    const bool excl = no_ovf && t1 - t0 == 1;
    for (int64_t t = t0; t < t1; ++t) {
      uint4* rt = reinterpret_cast<uint4*>(a.runt + t * 16);
      uint4 v[4];
#pragma unroll
      for (int bi = 0; bi < 4; ++bi) v[bi] = rt[bi];
#pragma unroll
      for (int bi = 0; bi < 4; ++bi) rt[bi] = make_uint4(0u, 0u, 0u, 0u);  // runt is zero for the next K_left
      if (cap) continue;
      const int64_t rtop = top + a.hiR[t];
#pragma unroll
      for (int bi = 0; bi < 4; ++bi) {
        uint32_t* row = a.rows + (rtop - bi) * 4;
        if (excl) {
          if (v[bi].x | v[bi].y | v[bi].z | v[bi].w) *reinterpret_cast<uint4*>(row) = v[bi];
          continue;
        }
        if (v[bi].x) atomicAdd(row + 0, v[bi].x);
        if (v[bi].y) atomicAdd(row + 1, v[bi].y);
        if (v[bi].z) atomicAdd(row + 2, v[bi].z);
        if (v[bi].w) atomicAdd(row + 3, v[bi].w);
      }
    }
  }
  if (cap) return;
  // long insertions (grid-stride over waves, LEFT like the short ones)
  const int64_t nov = *a.ovf_cnt < (uint32_t)a.ovf_cap ? *a.ovf_cnt : a.ovf_cap;
  for (int64_t t = (int64_t)blockIdx.x * (kUB / 64) + w; t < nov; t += (int64_t)gridDim.x * (kUB / 64)) {
    const Ovf o = a.ovf[t];
    const int64_t g = a.gbase[a.sample[o.read]] + o.gap;
    const int64_t run = run_left(a.right_start, a.rsl, a.roff, a.vals_out, g, a.read_offset + o.read);
    const int64_t rb = (int64_t)a.row_base[g] + a.lo_f[g] + a.hiR[run] - 1;
    for (int64_t bi = l; bi < o.len; bi += 64) {
      const int c = code_upper(a.cs[o.off + o.len - 1 - bi]);
      atomicAdd(a.rows + (rb - bi) * 4 + (c < 0 ? 0 : c), 1u);
    }
  }
}

// ---------------------------------------------------------------------------
// Flank tallies.  Every read's upstream flank (LEFT at gap tstart, :303 ->
// :37-62) and downstream flank (RIGHT at gap i_end, :323 -> :64-72) map
// LINEARLY onto rows once the layout is known: byte j of the flank goes to row
// rowstart + j, with
//   upstream   rowstart = row_base + lo_f + hi_run - L
//   downstream rowstart = row_base + lo_f - lo_at
// (hi_run / lo_at = 0 unless the gap is mixed).  Each WAVE owns 64
// consecutive reads (one per lane: its record, its two row starts); their
// flank bytes are contiguous, so the wave stages them in its LDS with 16-byte
// loads (both sides before any tally) and walks them in 256-byte segments,
// consecutive lanes on consecutive bytes.  The owner of a byte needs no block
// barrier and no scan: a wave's non-empty flanks lie one after the other in
// lane order, so the owner of byte x is the k-th of them, k = the flank starts
// at or before x.  Per stage every such flank sets the bit of its start byte
// in the wave's LDS bitmap (one ds_or); per 64-byte group a ballot of the
// lanes' bits and a lane prefix count give k (a scalar popcount carries it
// over groups, segments and stages), and a table written once per side holds
// the k-th flank's row offset.  Rows of the hot gaps (voted per
// chunk of reads: for full-length reads gap 0 upstream, gap n downstream) are
// tallied in LDS windows, everything else with global atomics.  Block
// barriers: two per chunk (after its records load, which hands the vote the
// gaps and rows of three reads, and after the vote), and the flush (at the
// end, or when a block's chunk range crosses into another sample's gaps).
// ---------------------------------------------------------------------------
#ifndef MPC_FLANK_WAVES
#define MPC_FLANK_WAVES 8
#endif
constexpr int kFW = MPC_FLANK_WAVES;  // waves per block (64 reads each): C2's 200k reads fit one round of resident blocks
constexpr int kFWSmall = 2;     // ... when kFW-wave blocks would not give every CU one (C1)
constexpr int kWinRows = 256;   // LDS window rows per flank side
constexpr int kFSeg = 256;      // flank bytes per wave step (4 per lane)
constexpr int kFStageLd = 2;    // 16-byte loads per lane per staged side (2 KiB per wave)
constexpr int kFStageBytes = kFStageLd * 64 * 16;  // the stage itself
constexpr int kFStage = kFStageBytes - 16;  // flank bytes per side staged per wave (C3: 64 reads x 0-40 B, mean 1280)
constexpr int kFBitmap = kFStageBytes / 32;  // dwords of a wave's start bitmap: one bit per staged byte
static_assert(kFBitmap == 64, "one bitmap word per lane");
// K_flank blocks at most (two per CU): beyond, a block takes a contiguous range of
// chunks (C3: 1954 one-chunk blocks 135 us, 512 blocks of ~4 chunks 110 us)
#ifndef MPC_FLANK_BLOCKS_MAX
#define MPC_FLANK_BLOCKS_MAX 512
#endif
// 2-wave blocks only when 8-wave blocks would leave most CUs idle (C1's 20 k
// reads: 40 blocks); a C3 shard of 125 k reads (244 blocks of 8 waves) took
// 47.8 us in 2-wave blocks and 26.6 us in 8-wave ones (threshold 256 -> 128;
// C1, C2, C3 / 4 shards unchanged: profiles/r06_experiments/k_flank_small_blocks.txt)
#ifndef MPC_FLANK_SMALL_BELOW
#define MPC_FLANK_SMALL_BELOW 128
#endif

struct FlankArgs {
  uint32_t* status; const int32_t* sample; const int32_t* n_of; const int32_t* gbase;
  const int32_t* tstart; const int32_t* i_end;
  const int64_t* up_off; const uint8_t* up; const int64_t* down_off; const uint8_t* down;
  const int32_t* right_start; const int32_t* rsl; const int32_t* roff; const int32_t* vals_out; const int32_t* rpos;
  const int32_t* row_base; const int32_t* lo_f; const int32_t* hiR; const int32_t* loR;
  uint32_t* rows;
  int64_t N, read_offset;
};

// dict code of an exact-case base (flanks are upper-cased at ingest, :270):
// h = (c >> 1) & 3 is a perfect hash A0 C1 T2 G3 on "ACTG", bit-swapped to A0 T1 C2 G3
__device__ __forceinline__ int code_exact(uint32_t c) {
  const uint32_t h = (c >> 1) & 3u;
  const uint32_t expect = (0x47544341u >> (8 * h)) & 0xffu;
  const int code = (int)(((h & 1u) << 1) | (h >> 1));
  return c == expect ? code : -1;
}

template <int NW, bool MULTI>  // waves per block; blocks take several chunks (grid capped)
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(MULTI || NW < kFW ? 4 : 6))) void K_flank(FlankArgs a) {
  // row r, code c at word 5 r + c: consecutive rows (the bytes of one flank,
  // on consecutive lanes) fall on distinct banks
  __shared__ uint32_t win[2][kWinRows * 5];
  __shared__ uint32_t bm[NW][kFBitmap];  // per wave: one bit per staged byte, set where a non-empty flank starts
  __shared__ int32_t rkt[NW][64];        // per wave and side: the row offset of the k-th non-empty flank
  __shared__ __attribute__((aligned(16))) uint8_t stg[NW][2][kFStageBytes];  // per wave and side: staged flank bytes
  // the windows' first rows: placed, and voted for the chunk (by chunk parity: a
  // wave still comparing chunk k's vote never sees chunk k + 1's)
  __shared__ int64_t s_w0[2], s_wn[2][2];
  // per side: the three voters' gap and its first row (written before the chunk's
  // first barrier, read before its second: no parity needed)
  __shared__ int2 s_vote[2][3];
  if (a.status[MPC_ST_FLAGS] & (DE_CAP | DE_INTERNAL)) return;
  const int tid = threadIdx.x, l = lane();
  const int w = uniform_i32(tid >> 6);
  const int64_t tot = a.status[MPC_ST_ROWS_NEEDED];
  constexpr int64_t RB = NW * 64;
  for (int k = tid; k < 2 * kWinRows * 5; k += blockDim.x) (&win[0][0])[k] = 0;
  const int64_t nchunks = (a.N + RB - 1) / RB;
  // the block's chunks: a contiguous range (one sample's reads but at sample
  // boundaries), so its windows are flushed once per range, not per chunk --
  // every block's flush adds into the same hot rows (C3: 1954 one-chunk blocks)
  const int64_t cpb = MULTI ? (nchunks + gridDim.x - 1) / gridDim.x : 1;
  const int64_t ck0 = (int64_t)blockIdx.x * cpb, ck1 = ck0 + cpb < nchunks ? ck0 + cpb : nchunks;
  auto flush = [&]() {
    for (int side = 0; side < 2; ++side) {
      const int64_t w0 = s_w0[side];
      for (int k = tid; k < kWinRows * 4; k += blockDim.x) {
        const uint32_t v = win[side][(k >> 2) * 5 + (k & 3)];
        if (v) atomicAdd(a.rows + w0 * 4 + k, v);
      }
    }
  };
  uint32_t lerr = 0;
  int64_t lread = INT64_MAX;
  uint32_t* bm_w = bm[w];
  int32_t* rk_w = rkt[w];
#pragma unroll 1
  for (int64_t ck = ck0; ck < ck1; ++ck) {
    const int64_t rb = ck * RB + (int64_t)w * 64;  // the wave's first read
    const int64_t r = rb + l;
    const bool live = r < a.N;
    // per-read records: flank byte ranges and the row of byte 0 of each flank,
    // kept in 32 bits past this point (rows < 2^31; a flank longer than 2^31 - 1
    // bytes takes the HBM path below with its 64-bit offsets reloaded): fewer
    // VGPRs, more resident waves -- the other batches' kernels in flight get
    // the CUs K_flank does not hold
    int64_t off0 = 0, off1 = 0;
    int32_t L0 = 0, L1 = 0, rw0 = -1, rw1 = -1;
    int2 v0 = make_int2(-1, 0), v1 = make_int2(-1, 0);  // for the vote: each flank's gap (-1: empty flank or no row), the gap's first row
    if (live) {
      const int s = a.sample[r], ts = a.tstart[r], ie = a.i_end[r];
      off0 = a.up_off[r];
      off1 = a.down_off[r];
      const int64_t ul = a.up_off[r + 1] - off0, dl = a.down_off[r + 1] - off1;
      const int n = a.n_of[s];
      const int64_t gb = a.gbase[s];
      if (ul > 0 && ts >= 0 && ts <= n) {  // LEFT at gap tstart
        const int64_t g = gb + ts;
        int64_t hi = 0;
        if (a.right_start[g + 1] > a.right_start[g])
          hi = a.hiR[run_left(a.right_start, a.rsl, a.roff, a.vals_out, g, a.read_offset + r)];
        v0 = make_int2((int32_t)g, a.row_base[g]);
        const int64_t rs = (int64_t)v0.y + a.lo_f[g] + hi - ul;
        if (rs >= 0 && rs + ul > tot) lerr |= DE_INTERNAL;
        else rw0 = (int32_t)rs;
      }
      if (dl > 0 && ie >= 0 && ie <= n) {  // RIGHT at gap i_end
        const int64_t g = gb + ie;
        int64_t lo_at = 0;
        if (a.right_start[g + 1] > a.right_start[g]) {
          const int64_t t = a.rpos[r];
          lo_at = a.loR[(int64_t)a.right_start[g] + g + a.roff[g] + (t - a.rsl[g])];
        }
        v1 = make_int2((int32_t)g, a.row_base[g]);
        const int64_t rs = (int64_t)v1.y + a.lo_f[g] - lo_at;
        if (rs >= 0 && rs + dl > tot) lerr |= DE_INTERNAL;
        else rw1 = (int32_t)rs;
      }
      L0 = ul < INT32_MAX ? (int32_t)ul : INT32_MAX;
      L1 = dl < INT32_MAX ? (int32_t)dl : INT32_MAX;
    }
    {  // LDS window: rows of the gap most of the chunk's reads use.  A vote of 3
       // (the chunk's first, middle and last read): their lanes hold the gap and
       // its first row already, so the vote costs no global load of its own (on
       // two threads ahead of the records it was five dependent ones, off ->
       // sample -> tstart -> n_of / gbase -> row_base, that the block waited for)
      const int64_t c0 = ck * RB;
      const int64_t nr = a.N - c0 < RB ? a.N - c0 : RB;
      if (r == c0) { s_vote[0][0] = v0; s_vote[1][0] = v1; }
      if (r == c0 + nr / 2) { s_vote[0][1] = v0; s_vote[1][1] = v1; }
      if (r == c0 + nr - 1) { s_vote[0][2] = v0; s_vote[1][2] = v1; }
    }
    __syncthreads();  // the votes are in; every wave is done with the previous chunk
    if (tid < 2) {
      const int2 x = s_vote[tid][0], y = s_vote[tid][1], z = s_vote[tid][2];
      const int2 gw = (x.x == y.x || x.x == z.x) ? x : y;
      s_wn[ck & 1][tid] = gw.x >= 0 ? (int64_t)gw.y : (int64_t)INT32_MIN;
      if (ck == ck0) s_w0[tid] = s_wn[ck & 1][tid];  // the first placement (windows zeroed above)
    }
    __syncthreads();
    const int64_t* wn_ = s_wn[ck & 1];
    if (MULTI && (wn_[0] != s_w0[0] || wn_[1] != s_w0[1])) {  // (block-uniform) windows move: flush, clear, place
      flush();
      __syncthreads();
      for (int k = tid; k < 2 * kWinRows * 5; k += blockDim.x) (&win[0][0])[k] = 0;
      if (tid < 2) s_w0[tid] = wn_[tid];
      __syncthreads();
    }
    if (rb >= a.N) continue;
    const int last = a.N - 1 - rb < 63 ? (int)(a.N - 1 - rb) : 63;  // the wave's last read
    // the wave's flank bytes of both sides: [Bw, Bw + nb)
    const int64_t Bw0 = readlane64(off0, 0), nb0 = readlane64(off0 + L0, last) - Bw0;
    const int64_t Bw1 = readlane64(off1, 0), nb1 = readlane64(off1 + L1, last) - Bw1;
    // byte offsets in the wave's range (32-bit whenever the range is below 2^30)
    const int32_t xo0 = live ? (int32_t)(off0 - Bw0) : (int32_t)min(nb0, (int64_t)INT32_MAX);
    const int32_t xo1 = live ? (int32_t)(off1 - Bw1) : (int32_t)min(nb1, (int64_t)INT32_MAX);
    // stage [Bw + c0, Bw + c0 + kFStage) of a side in the wave's LDS (16-byte
    // loads from the aligned-down start).  The first stage of BOTH sides is
    // loaded before any tally: a load issued after a global atomic waits for
    // that atomic too (vmcnt retires in order), so loads between the atomics
    // serialized the wave on them)
    auto stage_load = [&](const uint8_t* src, int64_t B, int64_t nb, int64_t c0, uint4 (&v)[kFStageLd]) {
      const int64_t A = (B + c0) & ~(int64_t)15;
      const int64_t cnt = nb - c0 < kFStage ? nb - c0 : kFStage;
      const int n16 = (int)(((B + c0 - A) + cnt + 15) >> 4);
#pragma unroll
      for (int j = 0; j < kFStageLd; ++j)
        v[j] = l + 64 * j < n16 ? *reinterpret_cast<const uint4*>(src + A + 16 * (l + 64 * j)) : make_uint4(0u, 0u, 0u, 0u);
    };
    auto stage_store = [&](uint8_t* st, const uint4 (&v)[kFStageLd]) {
#pragma unroll
      for (int j = 0; j < kFStageLd; ++j) *reinterpret_cast<uint4*>(st + 16 * (l + 64 * j)) = v[j];
    };
    {
      uint4 v0[kFStageLd], v1[kFStageLd];
      if (nb0 > 0) stage_load(a.up, Bw0, nb0, 0, v0);
      if (nb1 > 0) stage_load(a.down, Bw1, nb1, 0, v1);
      if (nb0 > 0) stage_store(stg[w][0], v0);
      if (nb1 > 0) stage_store(stg[w][1], v1);
    }
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
      const uint8_t* src = side ? a.down : a.up;
      // (selects, not arrays indexed by side: a runtime index would put them in scratch)
      const int32_t L = side ? L1 : L0, frs = side ? rw1 : rw0, xo = side ? xo1 : xo0;
      const int64_t Bw = side ? Bw1 : Bw0, nb = side ? nb1 : nb0;
      if (nb <= 0) continue;
      const int32_t w032 = s_w0[side] >= 0 ? (int32_t)s_w0[side] : -(1 << 30);  // no window: never a hit
      uint32_t* wn = win[side];
      uint8_t* st = stg[w][side];
      if (nb >= (1 << 30)) {  // (huge flanks: every lane walks its own from HBM; rows < 2^31)
        int64_t fo = live ? (side ? a.down_off[r] : a.up_off[r]) : 0;
        int64_t fl = live ? (side ? a.down_off[r + 1] : a.up_off[r + 1]) - fo : 0;
        // (a use of both on every path from here: when a branch around the
        // loads' first use left them pending, the compiler waited for them --
        // vmcnt(0), so for every global atomic before it -- at the next write of
        // their registers, in each iteration of the segment loop below)
        asm volatile("" : "+v"(fo), "+v"(fl));
        for (int64_t j = 0; frs >= 0 && j < fl; ++j) {
          const int code = code_exact(src[fo + j]);
          if (code < 0) { lerr |= DE_KEY; lread = r < lread ? r : lread; continue; }
          const int32_t row = (int32_t)(frs + j);
          const uint32_t wr = (uint32_t)(row - w032);
          if (wr < (uint32_t)kWinRows) atomicAdd(wn + wr * 5 + code, 1u);
          else atomicAdd(a.rows + (int64_t)row * 4 + code, 1u);
        }
        continue;
      }
      // wave-relative byte x of lane l's flank: row = x + rowoff (rs + L <= tot < 2^31;
      // no row: rowoff = INT32_MIN, so every row of the flank is negative)
      const int32_t rowoff = (live && frs >= 0) ? frs - xo : INT32_MIN;
      const bool ne = live && L > 0;
      const int nb32 = (int)nb;
      // the side's non-empty flanks by rank (their order on the lanes): the
      // row offset of the k-th one at rk_w[k].  (The previous side's and
      // chunk's reads of the table are behind: LDS works a wave's
      // instructions in order.)
      const uint64_t nem = ballot(ne);
      if (ne) rk_w[lanes_below(nem)] = rowoff;
      uint32_t carry = 0;  // flanks starting before the byte group: the rank of its predecessor's owner
#pragma unroll 1
      for (int c0 = 0; c0 < nb32; c0 += kFStage) {
        if (c0 > 0) {  // (a wave with more than kFStage bytes on this side)
          uint4 v[kFStageLd];
          stage_load(src, Bw, nb, c0, v);
          stage_store(st, v);
        }
        const int sh = (int)((Bw + c0) & 15);
        const int c1 = nb32 - c0 < kFStage ? nb32 : c0 + kFStage;
        // the stage's start bitmap: bit x - c0 is set where a non-empty flank
        // starts on byte x (distinct bytes: one ds_or per flank, no return).
        // Only starts in this stage: the others count when their stage comes
        bm_w[l] = 0;
        if (ne && xo >= c0 && xo < c1) atomicOr(bm_w + ((xo - c0) >> 5), 1u << ((xo - c0) & 31));
        wave_sync_lds();
#pragma unroll 1
        for (int S = c0; S < c1; S += kFSeg) {
          // lane l takes bytes S + 64 k + l (k < 4): consecutive lanes on
          // consecutive bytes, so a flank's bytes (consecutive rows) leave as few
          // 64-B atomic requests as they can (4 bytes per lane put every lane's
          // row atomic in a segment of its own: C3 K_flank +30 %)
          // The four 64-byte groups of the segment go through each step
          // TOGETHER: their bitmap words and staged bytes in one batch of LDS
          // reads, four ranks (only the scalar carry links the groups), one
          // batch of table reads -- two LDS round trips per segment before
          // the tallies, nothing written per segment.  The byte reads are
          // unconditional, so their index stays inside the stage: only group
          // 3 of a full stage's last segment can pass it (dead lanes, x >= c1)
          static_assert(15 + (kFStage - 1) / kFSeg * kFSeg + 191 < kFStageBytes, "groups 0-2 read inside the stage");
          static_assert((kFStage - 1) / kFSeg * kFSeg + kFSeg <= 64 * 32, "a stage's segments stay inside the bitmap");
          const int bx = sh + (S - c0) + l;
          const uint32_t* bm_s = bm_w + ((S - c0) >> 5) + (l >> 5);  // the word of byte S + l; group k: + 2 k
          uint32_t bw[4], ch[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) bw[k] = bm_s[2 * k];
#pragma unroll
          for (int k = 0; k < 4; ++k) ch[k] = st[k < 3 ? bx + 64 * k : min(bx + 192, kFStageBytes - 1)];
          // (all eight are in registers here: none sinks to its use below)
          asm volatile("" : "+v"(bw[0]), "+v"(bw[1]), "+v"(bw[2]), "+v"(bw[3]), "+v"(ch[0]), "+v"(ch[1]), "+v"(ch[2]), "+v"(ch[3]));
          uint32_t rk[4];  // the rank of the byte's owner: flanks starting at or before it (0: none)
          int32_t q[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint32_t mine = (bw[k] >> (l & 31)) & 1u;
            const uint64_t m = ballot(mine != 0);  // the group's starts
            rk[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, carry + mine));
            carry += (uint32_t)__popcll(m);
            // the row offset of the byte's flank
            q[k] = rk_w[rk[k] > 0 ? rk[k] - 1 : 0];
          }
          asm volatile("" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]));
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int x = S + 64 * k + l;
            int32_t row = x + q[k];
            if (x >= c1 || rk[k] == 0) row = -1;  // past the wave's range
            int code = -1;
            if (row >= 0) {  // (< 0: also a flank without a row)
              code = code_exact(ch[k]);
              if (code < 0) {
                lerr |= DE_KEY;
                uint64_t m = nem;  // the lane of the rk-th non-empty flank
                for (uint32_t i = 1; i < rk[k]; ++i) m &= m - 1;
                const int64_t rr = rb + __builtin_ctzll(m);
                lread = rr < lread ? rr : lread;
              }
            }
            const uint32_t wr = (uint32_t)(row - w032);
            const bool hit = wr < (uint32_t)kWinRows;
            if (code >= 0 && hit) atomicAdd(wn + wr * 5 + code, 1u);
            if (code >= 0 && !hit) atomicAdd(a.rows + (int64_t)row * 4 + code, 1u);
          }
        }
        wave_sync_lds();  // (the stage is reloaded for the next kFStage bytes)
      }
    }
  }
  __syncthreads();
  if (ck1 > ck0) flush();
  if (lerr) {
    atomicOr(&a.status[MPC_ST_FLAGS], lerr);
    if (lread != INT64_MAX) atomicMin(&a.status[MPC_ST_FIRST_READ], (uint32_t)lread);
  }
}

// The rows of the listed wrapped odd positions (K_layout<true> placed them at
// row0, lo = the replayed slots prepended): a run's one-base writes go to slot
// lo + hiR - 1; a LEFT string's base bi from its 3' end to lo + hiR - 1 - bi
// (:55-61), a RIGHT string's base bi to lo - loR + bi (:67-71).  One wave per
// position (its runs) / per string (its bases on the lanes).
__global__ __launch_bounds__(256) void K_worows(Dev d) {
  const int np = (int)d.status[MPC_ST_WRAP_POS];
  if (np == 0 || (d.status[MPC_ST_FLAGS] & DE_CAP)) return;
  const int64_t n_ev = wo_listed(d);
  const int l = lane();
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t gw = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  for (int64_t p = gw; p < np; p += nwaves) {
    const WoPos P = d.wo_pos[p];
    for (int32_t j = l; j < P.nrun; j += 64) {
      const WoRun R = d.wo_run[P.run0 + j];
      uint32_t* row = d.rows + ((int64_t)P.row0 + P.lo + R.hiR - 1) * 4;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (R.C[c]) atomicAdd(row + c, R.C[c]);
    }
  }
  uint32_t err = 0;
  int64_t eread = INT64_MAX;
  for (int64_t e = gw; e < n_ev; e += nwaves) {
    int64_t own = d.wo_idx[e];
    if (d.wo_x) {  // only this shard's strings: their bytes are here, at the local index
      const WoRec rc = wo_all(d)[1 + own];
      if (rc.shard != d.shard) continue;
      own = rc.ev;
    }
    const WoEv ev = d.wo[own];
    const WoPos P = d.wo_pos[wo_lower(d.wo_pos, np, ev.g)];
    const WoRun R = d.wo_run[P.run0 + d.wo_erun[e]];
    const int64_t L = wo_len(d, ev);
    const uint8_t* src = ev.type == kWoIns ? d.cs + ev.src
                       : ev.type == kWoUp  ? d.up + d.up_off[ev.read]
                                           : d.down + d.down_off[ev.read];
    for (int64_t bi = l; bi < L; bi += 64) {
      int code;
      int64_t slot;
      if (ev.type == kWoDown) {
        code = code_exact(src[bi]);
        slot = (int64_t)P.lo - R.loR + bi;
      } else {
        const uint32_t c = src[L - 1 - bi];
        code = ev.type == kWoIns ? code_upper(c) : code_exact(c);
        slot = (int64_t)P.lo + R.hiR - 1 - bi;
      }
      if (code < 0) {  // KeyError (:61, :71); a '+' base K_parse flagged too
        err |= DE_KEY;
        eread = ev.read < eread ? ev.read : eread;
        continue;
      }
      atomicAdd(d.rows + ((int64_t)P.row0 + slot) * 4 + code, 1u);
    }
  }
  if (err) {
    atomicOr(&d.status[MPC_ST_FLAGS], err);
    atomicMin(&d.status[MPC_ST_FIRST_READ], (uint32_t)eread);
  }
}

}  // namespace

// Host side: the arguments, geometry and launch of K_ins and K_flank
static int64_t ins_grid(const mpc_plan* p) { return std::max<int64_t>(1, std::min<int64_t>(p->units_cap, 512)); }
static int flank_waves(const mpc_plan* p) {
  return (p->N + kFW * 64 - 1) / (kFW * 64) < MPC_FLANK_SMALL_BELOW ? kFWSmall : kFW;
}
// K_flank blocks: one per chunk of flank_waves * 64 reads, at most kFlankBlocksMax
constexpr int64_t kFlankBlocksMax = MPC_FLANK_BLOCKS_MAX;
static int64_t flank_grid(const mpc_plan* p) {
  const int64_t fr = flank_waves(p) * 64;
  return std::max<int64_t>(1, std::min<int64_t>(kFlankBlocksMax, (p->N + fr - 1) / fr));
}

static InsArgs ins_args(const mpc_plan* p, const Dev& d) {
  InsArgs a;
  a.status = d.status; a.sample = d.sample; a.gbase = d.gbase;
  a.read_offset = d.read_offset; a.ovf_cap = d.ovf_cap; a.G = p->G;
  a.right_start = d.right_start; a.rsl = d.rsl; a.roff = d.roff; a.vals_out = d.vals_out;
  a.row_base = d.row_base; a.lo_f = d.lo_f; a.hiR = d.hiR;
  a.rows = d.rows; a.ovf = d.ovf; a.ovf_cnt = d.ovf_cnt; a.cs = d.cs;
  a.runt = d.runt;
  return a;
}

static FlankArgs flank_args(const mpc_plan* p, const Dev& d) {
  (void)p;
  FlankArgs a;
  a.status = d.status; a.sample = d.sample; a.n_of = d.n_of; a.gbase = d.gbase;
  a.tstart = d.tstart; a.i_end = d.i_end;
  a.up_off = d.up_off; a.up = d.up; a.down_off = d.down_off; a.down = d.down;
  a.right_start = d.right_start; a.rsl = d.rsl; a.roff = d.roff; a.vals_out = d.vals_out; a.rpos = d.rpos;
  a.row_base = d.row_base; a.lo_f = d.lo_f; a.hiR = d.hiR; a.loR = d.loR;
  a.rows = d.rows; a.N = d.N; a.read_offset = d.read_offset;
  return a;
}
static void launch_flank(const mpc_plan* p, const Dev& d, hipStream_t st) {
  const int nw = flank_waves(p);
  const dim3 grid((unsigned)flank_grid(p)), block((unsigned)(nw * 64));
  const bool multi = flank_grid(p) < (p->N + nw * 64 - 1) / (nw * 64);  // blocks take chunk ranges
  const FlankArgs fa = flank_args(p, d);
  if (nw == kFWSmall) {
    if (multi) hipLaunchKernelGGL((K_flank<kFWSmall, true>), grid, block, 0, st, fa);
    else hipLaunchKernelGGL((K_flank<kFWSmall, false>), grid, block, 0, st, fa);
  } else {
    if (multi) hipLaunchKernelGGL((K_flank<kFW, true>), grid, block, 0, st, fa);
    else hipLaunchKernelGGL((K_flank<kFW, false>), grid, block, 0, st, fa);
  }
}
