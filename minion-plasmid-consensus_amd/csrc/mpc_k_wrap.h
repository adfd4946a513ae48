// The wrap phase (mpc_wrap; one shard: inside mpc_layout).
// Wrapped odd positions (negative target starts; WoEv).  An odd position that
// receives LEFT strings (upstream flanks :303, '+' insertions :81-87) or
// RIGHT strings (downstream flanks :323) through Python's negative index wrap
// grows a slot list like a gap's (:37-72), and its one-base writes -- the
// match or substitution of every read covering the reference base (:79, :96)
// -- are LEFT strings of length 1 in the same replay.  Its runs are split at
// its RIGHT strings in read order (a read's own LEFT strings there precede its
// RIGHT one; a read ending at n + i < 0 never reaches the base itself).
//   K_woprep       one workgroup: sorts the list by (position, read, kind);
//                  the positions, their runs, each string's run, the longest
//                  LEFT / the closing RIGHT string per run
//   K_wocover      one thread per read: walks its cs (:306-320) and counts its
//                  one-base write at every listed position it covers into the
//                  run it falls in
//   K_layout<true> replays each listed position's runs (F slots, F rows)
//   K_worows       the strings and the one-base counts onto those rows
// None of it runs in plans without negative starts (mpc_input.neg_reads).
// Several shards: K_wopack turns each shard's list into records that are
// gathered (mpc.h MPC_BUF_WRAP_ALL); K_woprep then runs on the gathered list on
// every shard -- the same positions, runs, M and R everywhere -- while
// K_wocover and K_worows count only the shard's own reads and strings (the
// rows are summed), and "the run has a one-base write", which K_layout<true>
// needs of ALL reads, is a flag reduced over the shards (MPC_BUF_WRAP_COVER)
// that K_wofold enters into the run's longest LEFT string.
#pragma once

#include "mpc_k_common.h"

namespace {

__device__ __forceinline__ uint64_t wo_sort_key(const WoEv& e) {
  return ((uint64_t)(uint32_t)e.g << 32) | ((uint64_t)(uint32_t)e.read << 2) | (uint64_t)(uint32_t)e.type;
}
__device__ __forceinline__ int64_t wo_key_read(uint64_t k) { return (int64_t)((k >> 2) & 0x3fffffffu); }

// exclusive scan of x[0, n) in place by K_woprep's one workgroup; returns the total
__device__ int64_t block_scan_excl(int32_t* x, int64_t n, int32_t (&s_w)[16]) {
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < n; b0 += blockDim.x) {
    const int64_t k = b0 + threadIdx.x;
    const int v = k < n ? x[k] : 0;
    int tot;
    const int inc = block_scan(v, tot, s_w);
    if (k < n) x[k] = (int32_t)(carry + inc - v);
    carry += tot;
    __syncthreads();  // s_w: the next pass
  }
  return carry;
}

// first listed position with g >= x among [0, np)
__device__ __forceinline__ int wo_lower(const WoPos* pos, int np, int64_t x) {
  int lo = 0, hi = np;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pos[mid].g < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int32_t wo_len(const Dev& d, const WoEv& e) {
  if (e.type == kWoIns) return e.len;
  const int64_t* off = e.type == kWoUp ? d.up_off : d.down_off;
  const int64_t L = off[e.read + 1] - off[e.read];
  return L > 0x7fffffff ? 0x7fffffff : (int32_t)L;
}

// strings in the list the replay runs over: this shard's own (one shard), or
// every shard's, gathered behind the header record (the same on every shard)
__device__ __forceinline__ int64_t wo_listed(const Dev& d) {
  const int64_t n = d.wo_x ? (int64_t)wo_all(d)[0].g : (int64_t)d.status[MPC_ST_WRAP_EVENTS];
  return n < d.wo_cap ? n : d.wo_cap;
}
__device__ __forceinline__ uint64_t wo_rec_key(const WoRec& e) {
  return ((uint64_t)(uint32_t)e.g << 32) | ((uint64_t)(uint32_t)e.gread << 2) | (uint64_t)(uint32_t)e.type;
}

// n_shards > 1, after K_parse: this shard's strings as exchange records
__global__ __launch_bounds__(256) void K_wopack(Dev d) {
  const int64_t n = min<int64_t>((int64_t)d.status[MPC_ST_WRAP_EVENTS], d.wo_cap);
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const WoEv ev = d.wo[k];
    WoRec r;
    r.g = ev.g; r.gread = (int32_t)(d.read_offset + ev.read); r.len = wo_len(d, ev); r.type = ev.type;
    r.shard = d.shard; r.ev = (int32_t)k;
    wo_rec(d)[k] = r;
  }
}

__global__ __launch_bounds__(1024) void K_woprep(Dev d) {
  __shared__ int32_t s_w[16];
  const bool sh = d.wo_x != nullptr;  // the gathered list: keys by global read, lengths from the records
  const WoRec* all = wo_all(d);
  int32_t* cov = wo_cov(d);
  const int64_t n = wo_listed(d);
  if (sh) {
    // more strings than the list bound holds (kWoCapMax): as on one shard
    if (threadIdx.x == 0 && (int64_t)all[0].g > d.wo_cap) atomicOr(&d.status[MPC_ST_FLAGS], DE_UNSUP);
    for (int64_t k = threadIdx.x; k < 2 * n + 1; k += blockDim.x) cov[k] = 0;  // (runs <= 2 n)
  }
  if (n == 0) {
    if (threadIdx.x == 0) d.status[MPC_ST_WRAP_POS] = 0u;
    return;
  }
  int64_t P2 = 1;
  while (P2 < n) P2 <<= 1;
  uint64_t* key = d.wo_key;
  uint32_t* idx = d.wo_idx;
  for (int64_t k = threadIdx.x; k < P2; k += blockDim.x) {
    key[k] = k >= n ? ~0ull : sh ? wo_rec_key(all[1 + k]) : wo_sort_key(d.wo[k]);
    idx[k] = (uint32_t)k;
  }
  __syncthreads();
  // bitonic sort of (key, idx): keys are distinct but for a read's '+' strings
  // at one position, which are LEFT strings of one run (any order)
  for (int64_t size = 2; size <= P2; size <<= 1)
    for (int64_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (int64_t t = threadIdx.x; t < P2 / 2; t += blockDim.x) {
        const int64_t lo = 2 * stride * (t / stride) + (t % stride), hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const uint64_t a = key[lo], b = key[hi];
        if ((a > b) == asc && a != b) {
          key[lo] = b; key[hi] = a;
          const uint32_t x = idx[lo]; idx[lo] = idx[hi]; idx[hi] = x;
        }
      }
      __syncthreads();
    }
  // positions: segments of equal g
  int32_t* tmp = d.wo_erun + d.wo_cap;
  auto starts = [&](int64_t k) { return k == 0 || (key[k] >> 32) != (key[k - 1] >> 32); };
  for (int64_t k = threadIdx.x; k < n; k += blockDim.x) tmp[k] = starts(k) ? 1 : 0;
  __syncthreads();
  const int64_t npos = block_scan_excl(tmp, n, s_w);  // tmp[k] = positions starting before k
  for (int64_t k = threadIdx.x; k < n; k += blockDim.x) {
    const bool st = starts(k);
    const int32_t p = st ? tmp[k] : tmp[k] - 1;
    if (st) { d.wo_pos[p].g = (int32_t)(key[k] >> 32); d.wo_pos[p].beg = (int32_t)k; }
    if (k == n - 1 || starts(k + 1)) d.wo_pos[p].end = (int32_t)(k + 1);
  }
  __syncthreads();
  // runs per position: one more than its RIGHT strings
  for (int64_t p = threadIdx.x; p < npos; p += blockDim.x) {
    int32_t m = 0;
    for (int32_t e = d.wo_pos[p].beg; e < d.wo_pos[p].end; ++e) m += (int32_t)(key[e] & 3u) == kWoDown;
    d.wo_pos[p].nrun = m + 1;
    tmp[p] = m + 1;
  }
  __syncthreads();
  block_scan_excl(tmp, npos, s_w);
  for (int64_t p = threadIdx.x; p < npos; p += blockDim.x) {
    WoPos& P = d.wo_pos[p];
    const int32_t run0 = tmp[p];
    P.run0 = run0;
    for (int32_t j = 0; j < P.nrun; ++j) {
      WoRun z;
      z.M = 0; z.R = 0; z.hiR = 0; z.loR = 0; z.C[0] = z.C[1] = z.C[2] = z.C[3] = 0u;
      d.wo_run[run0 + j] = z;
    }
    int32_t j = 0;
    for (int32_t e = P.beg; e < P.end; ++e) {
      d.wo_erun[e] = j;  // RIGHT strings before it: its run (a RIGHT string closes run j)
      int32_t L, type;
      if (sh) { const WoRec rc = all[1 + idx[e]]; L = rc.len; type = rc.type; }
      else { const WoEv ev = d.wo[idx[e]]; L = wo_len(d, ev); type = ev.type; }
      WoRun& R = d.wo_run[run0 + j];
      if (type == kWoDown) { R.R = L; ++j; }
      else if (L > R.M) R.M = L;
    }
  }
  if (threadIdx.x == 0) d.status[MPC_ST_WRAP_POS] = (uint32_t)npos;
}

// one thread per read: the read's one-base writes (:79 matches, :96
// substitutions) at the listed positions, counted per run
__device__ void wo_cover_read(const Dev& d, int np, int64_t r);
__global__ __launch_bounds__(256) void K_wocover(Dev d) {
  const int np = (int)d.status[MPC_ST_WRAP_POS];
  if (np == 0) return;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < d.N; r += (int64_t)gridDim.x * blockDim.x)
    wo_cover_read(d, np, r);
}
__device__ void wo_cover_read(const Dev& d, int np, int64_t r) {
  const int s = d.sample[r];
  const int64_t n = d.n_of[s], gb = d.gbase[s];
  const int pa = wo_lower(d.wo_pos, np, gb), pb = wo_lower(d.wo_pos, np, gb + n);
  if (pa == pb) return;
  const uint8_t* ref = d.ref + d.ref_off[s];
  auto hit = [&](int p, int code) {
    const WoPos P = d.wo_pos[p];
    int lo = P.beg, hi = P.end;  // the position's first string from a read >= r (keys: global reads)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (wo_key_read(d.wo_key[mid]) < d.read_offset + r) lo = mid + 1; else hi = mid;
    }
    const int32_t j = lo < P.end ? d.wo_erun[lo] : P.nrun - 1;
    atomicAdd(&d.wo_run[P.run0 + j].C[code], 1u);
    if (d.wo_x) wo_cov(d)[P.run0 + j] = 1;  // (exchange: MAX; C itself stays this shard's)
  };
  // the tokenizer of :306-320: an operator applies to the operand gathered
  // after it when the next operator comes with a non-empty operand, the last
  // one unconditionally.  Data errors were flagged by K_parse: stop there.
  const int64_t b = d.cs_off[r], e = d.cs_off[r + 1];
  int64_t i = d.tstart[r], o0 = b, olen = 0;
  uint32_t op = 0;
  for (int64_t x = b;; ++x) {
    const bool end = x >= e;
    const uint32_t c = end ? 0u : d.cs[x];
    const bool sp = !end && (c == ':' || c == 'Z' || c == '+' || c == '-' || c == '*');
    if (!end && !sp) { ++olen; continue; }
    if (end || olen > 0) {
      if (op == ':') {
        // int(operand) exactly as K_parse takes it (analyze_long): every form
        // py_int accepts advances here too, or the read's later one-base
        // writes at listed positions would be lost without any flag
        int64_t m = 0;
        if (!py_int(d.cs + o0, olen, &m)) return;  // ValueError: K_parse flagged DE_VALUE
        if (m < 0) m = 0;
        if (m > (1ll << 40)) m = 1ll << 40;
        const int64_t k0 = i < 0 ? 0 : i, k1 = i + m < n ? i + m : n;
        for (int p = k0 < k1 ? wo_lower(d.wo_pos, np, gb + k0) : pb; p < pb && d.wo_pos[p].g < gb + k1; ++p) {
          const int code = base_code_exact(ref[d.wo_pos[p].g - gb]);
          if (code >= 0) hit(p, code);  // (else KeyError: K_layout flags it)
        }
        i += m;
      } else if (op == '*') {
        if (olen == 0) return;
        if (i >= 0 && i < n) {
          const int p = wo_lower(d.wo_pos, np, gb + i);
          if (p < pb && d.wo_pos[p].g == gb + i) {
            const int code = code_upper(d.cs[o0 + olen - 1]);
            if (code >= 0) hit(p, code);
          }
        }
        i += 1;
      } else if (op == '-') {
        i += olen;
      } else if (op != '+' && op != 'Z') {
        return;  // unknown operator (:100-102)
      }
      if (i >= n) return;  // any later one-base write is past the end
    }
    if (end) break;
    op = c;
    o0 = x + 1;
    olen = 0;
  }
}

// n_shards > 1, before K_layout<true>: the cover flags reduced over the shards
// (MAX) enter the replay as what they stand for, a LEFT string of length 1 in
// the run.  K_layout<true> takes m = max(M, c1) with c1 from this shard's C;
// with M >= 1 wherever ANY shard has a one-base write, m is the same on every
// shard, and K_layout itself stays the kernel of the one-shard plan.  (M is
// rebuilt by K_woprep every step; nothing after the layout reads it.)
__global__ __launch_bounds__(256) void K_wofold(Dev d) {
  const int np = (int)d.status[MPC_ST_WRAP_POS];
  const int32_t* cov = wo_cov(d);
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < np; p += (int64_t)gridDim.x * blockDim.x) {
    const WoPos P = d.wo_pos[p];
    for (int32_t j = 0; j < P.nrun; ++j)
      if (cov[P.run0 + j] != 0 && d.wo_run[P.run0 + j].M < 1) d.wo_run[P.run0 + j].M = 1;
  }
}

}  // namespace

// the wrapped odd positions of a plan with negative starts: their runs, the
// one-base writes of this shard's reads
static void launch_wrap(const mpc_plan* p, const Dev& d, hipStream_t st) {
  hipLaunchKernelGGL(K_woprep, dim3(1), dim3(1024), 0, st, d);
  if (p->N > 0) hipLaunchKernelGGL(K_wocover, dim3(nblk(p->N, 256)), dim3(256), 0, st, d);
}
