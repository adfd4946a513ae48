// mpc_link.hip -- linkage_qc on gfx950 (include/mpc_linkage.h; DESIGN.md
// "linkage_qc"): K_lnkparse walks every record's cs tag with the tokenizer of
// K_covparse (mpc_cswalk.h) and writes the record's allele code at every site,
// K_lnkplanes turns the allele matrix into bit-planes (one u64 word per 64
// records, site and code), K_lnkpair counts the co-occurrences of every site
// pair as popcount(plane & plane) -- exact integers, no matrix unit.
//
// Scratch: u64 status key (the first 64 bytes), then the planes u64[W][K][8],
// W = ceil(N / 64), word-major so that K_lnkplanes stores and K_lnkpair loads
// consecutive addresses.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "mpc.h"
#include "mpc_coverage.h"
#include "mpc_cstables.h"
#include "mpc_cswalk.h"
#include "mpc_device.h"
#include "mpc_launch.h"
#include "mpc_linkage.h"

namespace {
using namespace mpc;

typedef long long i64;
typedef unsigned long long u64;

constexpr int kLnkWaves = 16;  // the grid and the record batching of K_covparse
constexpr int kLnkThreads = 64 * kLnkWaves;
constexpr int kLnkMaxWgs = 256;
constexpr int kMaxK = MPC_LNK_MAX_SITES;
constexpr int kPlaneHead = 64;  // bytes of scratch before the planes
constexpr int kPlaneWaves = 4;
constexpr int kPairWaves = 4;
constexpr int kPairWordsPerSplit = 128;  // words one workgroup of K_lnkpair sums
constexpr int kPairMaxSplits = 32;

__device__ __forceinline__ void wave_lds_sync() {
  // LDS written by some lanes of this wave, read by others
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// first index in [lo, hi) with keys[index] >= x
__device__ __forceinline__ int key_lower_bound(const uint32_t* keys, int lo, int hi, uint32_t x) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t sub_code(uint32_t y) {
  y |= 32u;
  return y == 'a' ? 2u : y == 'c' ? 3u : y == 'g' ? 4u : y == 't' ? 5u : 6u;
}

// what a token does to the record's allele row (the effects policy of cs_chunk)
struct LnkFx {
  static constexpr bool kBase = true;
  const uint32_t* keys;  // LDS: every site key
  uint8_t* row;          // LDS: this wave's allele row
  int k0, cur, k1;       // wave-uniform: the sample's keys, and those not yet behind the walk
  uint32_t kreg0, kreg1; // per lane: two of the sample's keys
  uint32_t lastb;
  __device__ __forceinline__ void carried_match(uint32_t) const {}
  __device__ __forceinline__ void carried_sub() const {}
  __device__ __forceinline__ void point(uint32_t key, uint32_t code) const {
    const int i = key_lower_bound(keys, cur, k1, key);
    if (i < k1 && keys[i] == key) row[i] = (uint8_t)code;
  }
  __device__ __forceinline__ void carried_sub_at(uint32_t p) const { point(2u * p + 1u, sub_code(lastb)); }
  __device__ __forceinline__ void count(bool, uint32_t, bool, bool, bool, int, bool) const {}
  // no key in [2 p0, 2 p1 + 1]: nothing in this chunk can land on a site.  Two ballots over the
  // sample's keys in registers (lane ln: keys k0 + ln and k0 + 64 + ln, 0xffffffff past the sample's
  // last: above every real key) also move cur past the keys behind the walk.
  __device__ __forceinline__ bool look(i64 p0, i64 p1) {
    const i64 lo = 2 * p0, hi = 2 * p1 + 1;
    const i64 a = (i64)kreg0, b = (i64)kreg1;
    const int behind = __popcll(ballot(a < lo)) + __popcll(ballot(b < lo));
    cur = k0 + behind < k1 ? k0 + behind : k1;
    return (ballot(a >= lo && a <= hi && kreg0 != 0xffffffffu) | ballot(b >= lo && b <= hi && kreg1 != 0xffffffffu)) != 0;
  }
  __device__ __forceinline__ void emit(bool hit, bool del_piece, uint32_t pos, uint32_t reach, uint32_t y) const {
    if (!del_piece) {
      point(hit ? 2u * pos + 1u : 2u * pos, hit ? sub_code(y) : 7u);
      return;
    }
    for (int i = key_lower_bound(keys, cur, k1, 2u * pos + 1u); i < k1 && keys[i] < 2u * reach; ++i)
      if (keys[i] & 1u) row[i] = 7;
  }
};

// grid: workgroups over contiguous cuts of per_wg records; wave w of a workgroup takes every 16th
// (K_covparse's batching: a wave reads the tables of its next 64 records lane-parallel, then walks them).
__global__ __launch_bounds__(kLnkThreads) void K_lnkparse(
    const uint8_t* __restrict__ cs, const int64_t* __restrict__ cs_off, const int64_t* __restrict__ tstart,
    const int32_t* __restrict__ rec_sample, const i64 n_records, const i64 per_wg,
    const int64_t* __restrict__ pos_off, const int32_t n_samples, const int64_t* __restrict__ site_off,
    const int64_t* __restrict__ site_key, const int K, uint8_t* __restrict__ alleles, u64* __restrict__ err_key) {
  __shared__ uint32_t keys[kMaxK];
  __shared__ uint8_t rows[kLnkWaves][kMaxK];
  const int tid = (int)threadIdx.x, ln = lane(), wave = tid >> 6;
  const uint64_t lemask = (2ull << ln) - 1ull;  // lanes at or below this one
  if (tid < kMaxK) keys[tid] = tid < K ? (uint32_t)site_key[tid] : 0xffffffffu;
  uint8_t* row = rows[wave];
  row[ln] = 0;
  row[ln + 64] = 0;
  __syncthreads();

  const i64 r0 = (i64)blockIdx.x * per_wg;
  const i64 r1 = r0 + per_wg < n_records ? r0 + per_wg : n_records;
  for (i64 rb = r0 + wave; rb < r1; rb += (i64)kLnkWaves * 64) {
    const i64 rj = rb + (i64)kLnkWaves * ln;
    int32_t m_s = -1, m_len = -1, m_k0 = 0, m_k1 = 0;
    i64 m_a = 0, m_ts = 0, m_L = 0;
    if (rj < r1) {
      m_s = rec_sample[rj];
      m_a = cs_off[rj];
      const i64 len = cs_off[rj + 1] - m_a;
      m_ts = tstart[rj];
      if (m_s >= 0 && m_s < n_samples) {
        m_L = pos_off[m_s + 1] - pos_off[m_s] - 1;
        m_k0 = (int32_t)site_off[m_s];
        m_k1 = (int32_t)site_off[m_s + 1];
      } else m_s = -1;
      if (len >= 0 && len <= INT32_MAX) {
        m_len = (int32_t)len;
        if (len >= 2 && cs[m_a] == 'Z' && cs[m_a + 1] == ':') { m_a += 2; m_len -= 2; }
      }
    }
    const i64 left = (r1 - rb + kLnkWaves - 1) / kLnkWaves;
    const int count = left < 64 ? (int)left : 64;
    uint32_t nb[kCsK];
    const uint8_t* q = cs + rl64(m_a, 0);
    int len = (int32_t)rl((uint32_t)m_len, 0);
    cs_load_tile(nb, q, len, 0);
    for (int j = 0; j < count; ++j) {
      const i64 r = rb + (i64)kLnkWaves * j;
      const int32_t s = (int32_t)rl((uint32_t)m_s, j);
      const i64 ts = rl64(m_ts, j);
      const uint32_t L = (uint32_t)rl64(m_L, j);
      const int k0 = (int)rl((uint32_t)m_k0, j), k1 = (int)rl((uint32_t)m_k1, j);
      const uint8_t* const cq = q;
      const int clen = len;
      uint32_t bt[kCsK];
#pragma unroll
      for (int k = 0; k < kCsK; ++k) bt[k] = nb[k];
      if (j + 1 < count) {
        q = cs + rl64(m_a, j + 1);
        len = (int32_t)rl((uint32_t)m_len, j + 1);
        cs_load_tile(nb, q, len, 0);
      }
      uint8_t* arow = alleles + r * K;
      if (s < 0) {
        if (ln == 0) cs_report(err_key, r, MPC_COV_RANGE);
        for (int i = ln; i < K; i += 64) arow[i] = 0;
        continue;
      }
      Walk w = {ts, 0u, 0, 0, clen < 0, ts < 0 || ts > (i64)L};
      LnkFx fx = {keys, row, k0, k0, k1, k0 + ln < k1 ? keys[k0 + ln] : 0xffffffffu,
                  k0 + 64 + ln < k1 ? keys[k0 + 64 + ln] : 0xffffffffu, 0u};
      for (int t0 = 0; t0 < clen && !w.bad; t0 += kCsTile) {
        if (t0 > 0) cs_load_tile(bt, cq, clen, t0);
#pragma unroll
        for (int k = 0; k < kCsK; ++k) {
          const int cb = t0 + k * 64;
          if (cb < clen && !w.bad) cs_chunk(bt[k], clen - cb < 64 ? clen - cb : 64, cb + 64 >= clen, L, lemask, fx, w);
        }
      }
      if ((w.bad || w.oor) && ln == 0) cs_report(err_key, r, w.bad ? MPC_COV_MALFORMED : MPC_COV_RANGE);
      // the row: covered ? max(code, 1) : 0, consecutive lanes on consecutive bytes; cleared for the next record
      wave_lds_sync();
      const i64 e = w.p;
      for (int i = ln; i < K; i += 64) {
        uint32_t code = 0;
        if (i >= k0 && i < k1) {
          const uint32_t key = keys[i];
          const i64 p = (i64)(key >> 1);
          const bool covered = p >= ts && ((key & 1u) ? p < e : p <= e);
          const uint32_t v = row[i];
          code = covered ? (v > 1u ? v : 1u) : 0u;
        }
        arow[i] = (uint8_t)code;
        row[i] = 0;
      }
      wave_lds_sync();
    }
  }
}

// grid: kPlaneWaves words per workgroup, one wave per word of 64 records (lane = record).  The
// wave's 64 x K bytes are one contiguous run of the record-major matrix: staged in LDS with
// consecutive lanes on consecutive dwords, then read back one site at a time.  8 ballots per
// site; lane 8 j + a keeps the word of (site kb + j, code a), so a store covers 8 sites.
// Workgroup 0 also decodes the status key of K_lnkparse (status may be null).
__global__ __launch_bounds__(64 * kPlaneWaves) void K_lnkplanes(
    const uint8_t* __restrict__ alleles, const i64 N, const int K, u64* __restrict__ planes,
    u64* __restrict__ err_key, int32_t* __restrict__ status) {
  __shared__ uint32_t stage[kPlaneWaves][64 * kMaxK / 4];
  const int tid = (int)threadIdx.x, ln = lane(), wave = tid >> 6;
  if (blockIdx.x == 0 && tid == 0 && status) {
    const u64 key = *err_key;
    if (key) cs_status(key, status);
  }
  const i64 W = (N + 63) / 64;
  const i64 wd = (i64)blockIdx.x * kPlaneWaves + wave;
  if (wd >= W) return;
  const i64 rec0 = wd * 64;
  const int nrec = N - rec0 < 64 ? (int)(N - rec0) : 64;
  const int nbytes = nrec * K;
  const uint8_t* src = alleles + rec0 * K;  // (4-byte aligned: the matrix is, and rec0 * K is a multiple of 64)
  uint32_t* st = stage[wave];
  const int n4 = nbytes >> 2;
  for (int i = ln; i < n4; i += 64) st[i] = reinterpret_cast<const uint32_t*>(src)[i];
  if (ln == 0 && (nbytes & 3)) {
    uint32_t v = 0;
    for (int b = 0; b < (nbytes & 3); ++b) v |= (uint32_t)src[n4 * 4 + b] << (8 * b);
    st[n4] = v;
  }
  wave_lds_sync();
  const uint8_t* sb = reinterpret_cast<const uint8_t*>(st);
  const bool have = ln < nrec;
  u64* out = planes + wd * K * 8;
  for (int kb = 0; kb < K; kb += 8) {
    u64 mine = 0;
#pragma unroll 1  // (unrolled, the 64 ballots of a step are all kept in SGPRs and spill)
    for (int j = 0; j < 8; ++j) {
      const int k = kb + j;
      const uint32_t code = (have && k < K) ? (uint32_t)(sb[ln * K + k] & 7u) : 8u;
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        const u64 m = ballot(code == (uint32_t)a);
        if (ln == j * 8 + a) mine = m;
      }
    }
    if (kb * 8 + ln < K * 8) out[kb * 8 + ln] = mine;
  }
}

// grid: (ceil(pairs / kPairWaves), splits).  One wave per site pair i <= j, lane = (a, b); a
// workgroup sums its split of the words, then every lane with a non-zero sum adds it to
// pair[i][j][a][b] and, off the diagonal, to the mirror pair[j][i][b][a].  pair is zero before.
__global__ __launch_bounds__(64 * kPairWaves) void K_lnkpair(const u64* __restrict__ planes, const i64 W, const int K,
                                                             const i64 words_per_split, uint32_t* __restrict__ pair) {
  const int ln = lane(), wave = (int)threadIdx.x >> 6;
  const i64 n_pairs = (i64)K * (K + 1) / 2;
  const i64 t = (i64)blockIdx.x * kPairWaves + wave;
  if (t >= n_pairs) return;
  // row i of the upper triangle holds K - i pairs: the largest i with i (2K - i + 1) / 2 <= t
  int i = 0;
  i64 before = 0;
  while (before + (K - i) <= t) { before += K - i; ++i; }
  const int j = i + (int)(t - before);
  const int a = ln >> 3, b = ln & 7;
  const i64 w0 = (i64)blockIdx.y * words_per_split;
  const i64 w1 = w0 + words_per_split < W ? w0 + words_per_split : W;
  const u64* pa = planes + (i64)i * 8 + a;
  const u64* pb = planes + (i64)j * 8 + b;
  const i64 stride = (i64)K * 8;
  uint32_t sum = 0;
  for (i64 w = w0; w < w1; ++w) sum += (uint32_t)__popcll(pa[w * stride] & pb[w * stride]);
  if (!sum) return;
  __hip_atomic_fetch_add(&pair[(((i64)i * K + j) * 8 + a) * 8 + b], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (i != j)
    __hip_atomic_fetch_add(&pair[(((i64)j * K + i) * 8 + b) * 8 + a], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int lnk_fail(const char* fn, const std::string& what) {
  return mpc_fail_(MPC_E_ARG, (std::string(fn) + ": " + what).c_str());
}
using mpc_launch::hip_fail;

// K_lnkplanes + K_lnkpair (pair is cleared here); status / err_key as K_lnkplanes takes them
int launch_pairs(const char* fn, const uint8_t* d_alleles, int64_t N, int32_t K, uint32_t* d_pair, void* d_scratch,
                 int32_t* d_status, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d_pair, 0, (size_t)K * K * 64 * sizeof(uint32_t), st);
  if (e != hipSuccess) return hip_fail(fn, "clearing pair", e);
  u64* err_key = (u64*)d_scratch;
  u64* planes = (u64*)((char*)d_scratch + kPlaneHead);
  const int64_t W = (N + 63) / 64;
  if (W > 0) {  // (no record: no status to decode either)
    hipLaunchKernelGGL(K_lnkplanes, dim3((unsigned)((W + kPlaneWaves - 1) / kPlaneWaves)), dim3(64 * kPlaneWaves), 0, st,
                       d_alleles, (i64)N, (int)K, planes, err_key, d_status);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(fn, "K_lnkplanes", e);
    int64_t splits = (W + kPairWordsPerSplit - 1) / kPairWordsPerSplit;
    if (splits > kPairMaxSplits) splits = kPairMaxSplits;
    const int64_t per = (W + splits - 1) / splits;
    splits = (W + per - 1) / per;
    const int64_t n_pairs = (int64_t)K * (K + 1) / 2;
    hipLaunchKernelGGL(K_lnkpair, dim3((unsigned)((n_pairs + kPairWaves - 1) / kPairWaves), (unsigned)splits),
                       dim3(64 * kPairWaves), 0, st, planes, (i64)W, (int)K, (i64)per, d_pair);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(fn, "K_lnkpair", e);
  }
  return MPC_OK;
}

}  // namespace

extern "C" int mpc_linkage_tile_bytes(void) { return kCsTile; }

extern "C" int64_t mpc_linkage_scratch_bytes(int64_t n_records, int32_t n_sites) {
  if (n_records < 0 || n_records > INT32_MAX || n_sites < 1 || n_sites > kMaxK) return 0;
  return kPlaneHead + ((n_records + 63) / 64) * (int64_t)n_sites * 8 * (int64_t)sizeof(uint64_t);
}

extern "C" int mpc_linkage_pairs(const uint8_t* d_alleles, int64_t n_records, int32_t n_sites, uint32_t* d_pair,
                                 void* d_scratch, void* stream) {
  const char* fn = "mpc_linkage_pairs";
  if (n_records < 0 || n_records > INT32_MAX) return lnk_fail(fn, "n_records outside [0, 2^31)");
  if (n_sites < 1 || n_sites > kMaxK) return lnk_fail(fn, "n_sites outside [1, " + std::to_string(kMaxK) + "]");
  if (!d_pair || !d_scratch || (n_records > 0 && !d_alleles)) return lnk_fail(fn, "null pointer");
  if (((uintptr_t)d_alleles & 3) != 0) return lnk_fail(fn, "d_alleles is not 4-byte aligned");
  if (((uintptr_t)d_scratch & 7) != 0) return lnk_fail(fn, "d_scratch is not 8-byte aligned");
  return launch_pairs(fn, d_alleles, n_records, n_sites, d_pair, d_scratch, nullptr, (hipStream_t)stream);
}

extern "C" int mpc_linkage_run(const uint8_t* d_cs, const int64_t* d_cs_off, const int64_t* d_tstart,
                               const int32_t* d_rec_sample, int64_t n_records, const int64_t* d_pos_off,
                               int32_t n_samples, const int64_t* d_site_off, const int64_t* d_site_key,
                               int32_t n_sites, uint8_t* d_alleles, uint32_t* d_pair, void* d_scratch,
                               int32_t* d_status, void* stream) {
  const char* fn = "mpc_linkage_run";
  if (n_records < 0 || n_records > INT32_MAX) return lnk_fail(fn, "n_records outside [0, 2^31)");
  if (n_samples < 1) return lnk_fail(fn, "n_samples < 1");
  if (n_sites < 1 || n_sites > kMaxK) return lnk_fail(fn, "n_sites outside [1, " + std::to_string(kMaxK) + "]");
  if (!d_pos_off || !d_site_off || !d_site_key || !d_pair || !d_scratch || !d_status || !d_cs_off ||
      (n_records > 0 && (!d_cs || !d_tstart || !d_rec_sample || !d_alleles)))
    return lnk_fail(fn, "null pointer");
  if (((uintptr_t)d_alleles & 3) != 0) return lnk_fail(fn, "d_alleles is not 4-byte aligned");
  if (((uintptr_t)d_scratch & 7) != 0) return lnk_fail(fn, "d_scratch is not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t S = (size_t)n_samples, K = (size_t)n_sites;
  std::vector<int64_t> h;
  if (const int rc = mpc_launch::read_back<int64_t>(st, {{d_pos_off, S + 1}, {d_site_off, S + 1}, {d_site_key, K}}, h, fn,
                                                    "sample and site tables"))
    return rc;
  const std::string bad = mpc_host::check_sites(h.data(), h.data() + S + 1, h.data() + 2 * (S + 1), S, (int64_t)K);
  if (!bad.empty()) return lnk_fail(fn, bad);
  hipError_t e = hipMemsetAsync(d_scratch, 0, kPlaneHead, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_status, 0, 2 * sizeof(int32_t), st);
  if (e != hipSuccess) return hip_fail(fn, "clearing the status", e);
  if (n_records > 0) {
    const mpc_launch::RecordGrid g = mpc_launch::record_grid(n_records, kLnkWaves, kLnkMaxWgs);
    hipLaunchKernelGGL(K_lnkparse, dim3((unsigned)g.wgs), dim3(kLnkThreads), 0, st, d_cs, d_cs_off, d_tstart, d_rec_sample,
                       (i64)n_records, (i64)g.per_wg, d_pos_off, n_samples, d_site_off, d_site_key, (int)n_sites, d_alleles,
                       (u64*)d_scratch);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(fn, "K_lnkparse", e);
  }
  return launch_pairs(fn, d_alleles, n_records, n_sites, d_pair, d_scratch, d_status, st);
}
