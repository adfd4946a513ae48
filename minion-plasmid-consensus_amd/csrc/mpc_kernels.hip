// libmpc: MI355X (gfx950) pileup + consensus for the consensus rule of the
// MinION plasmid pipeline.  Hot path = Steps 4-6 of
// /root/reference/src/mapped_paf_read_parser.py (include/mpc.h maps every
// reference function to its replacement; DESIGN.md has layouts and rooflines).
//
// Pipeline (one stream, no host synchronization):
//   parse     K_clear        zero the per-launch state
//             K_parse        per workgroup: contiguous reads of one sample.  cs
//                            ':'+op units -> substitution / deletion / span
//                            tallies (LDS), insertion events (64-event pages
//                            per 64-gap bucket, written once), i_end, LEFT-event
//                            gap bitmap, error flags
//             K_subs/K_subsum tally mode 3: substitution events -> tallies
//   index     K_rsplit_units RIGHT events: mixed gaps -> sort keys, RIGHT-only
//                            gaps -> longest flank; insertion work units
//             K_rsort        stable (gap, read) order of the mixed RIGHT events
//             K_rstart       per-gap ranges in the sorted list, RIGHT run lengths
//   runs      K_runs, K_runR (several shards) global run index space
//   tally     K_left         longest LEFT string per run (insertions, upstream flanks)
//   layout    K_layout       per-gap replay of the slot-layout state of
//                            processBaseString_* (:37-72) -> row counts, then
//                            row offsets + depth (look-back scan), odd rows
//   rows      K_ins, K_flank insertion / flank bases onto their slot rows
//   consensus K_call         per-slot top/second/tie/N (:363-439), max depth
//             K_select       threshold test + ordered compaction of the calls
//                            (look-back scan)
//
// This file: the phases of the C-ABI and binding a plan to its workspace.  The
// kernels, each stage with its argument fillers and launchers, are the
// mpc_k_*.h headers included below in pipeline order -- ONE translation unit,
// so the device code is what the single file compiled to.  The host planner
// (mpc_plan_create and every entry point that touches no device) is
// mpc_plan.cpp / mpc_plan.h; the constants and sizing functions planner and
// kernels share are mpc_geometry.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "mpc.h"

// What this library was compiled with (mpc_build_flags): product builds set
// none of the measurement switches below on the command line.  Recorded before
// the #ifndef defaults further down give them their product values.
#if defined(MPC_STAMPS) || defined(MPC_STAMPS_LEFT)
#define MPC_BF_STAMPS_ 1
#else
#define MPC_BF_STAMPS_ 0
#endif
#if defined(MPC_TUNING_OVERRIDES)
#define MPC_BF_TUNING_ 2
#else
#define MPC_BF_TUNING_ 0
#endif
#if defined(MPC_LDS_BASE_MODES) || defined(MPC_LAYOUT_GAPS) || defined(MPC_FLANK_WAVES) || \
    defined(MPC_FLANK_BLOCKS_MAX) || defined(MPC_FLANK_SMALL_BELOW)
#define MPC_BF_VARIANT_ 4
#else
#define MPC_BF_VARIANT_ 0
#endif

// (after the record above: mpc_geometry.h and mpc_k_rows.h give those switches
// their defaults)
#include "mpc_k_common.h"
#include "mpc_k_parse.h"
#include "mpc_k_index.h"
#include "mpc_k_left.h"
#include "mpc_k_wrap.h"
#include "mpc_k_layout.h"
#include "mpc_k_rows.h"
#include "mpc_k_call.h"

// ===========================================================================
// Host side: binding a plan (mpc_plan.h; planned by mpc_plan.cpp), launches, phases
// ===========================================================================
// look-back launch epochs (K_layout, K_select): one process-wide sequence, so a
// status word another plan left in reused memory never carries a live tag; 0 is
// never used (zeroed words)
static uint32_t next_epoch() {
  static std::atomic<uint32_t> e{0};
  uint32_t v;
  do v = (e.fetch_add(1) + 1) & 0x3fffffffu; while (v == 0);
  return v;
}

#define HIPCHK(x)                                                                  \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) return fail(MPC_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

// One launch clears every accumulator of a run (status, bitmaps, tallies, rows).
struct ClearArgs {
  uint32_t* ptr[24];
  int64_t words[24];
  uint32_t value[24];
  int32_t n;
};
__global__ __launch_bounds__(256) void K_clear(ClearArgs c) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int k = 0; k < c.n; ++k) {
    uint32_t* p = c.ptr[k];
    const uint32_t v = c.value[k];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.words[k]; i += stride) p[i] = v;
  }
}

extern "C" {

int mpc_build_flags(void) { return MPC_BF_STAMPS_ | MPC_BF_TUNING_ | MPC_BF_VARIANT_; }

int mpc_plan_bind(mpc_plan* p, void* ws, size_t bytes) {
  if (!p || !ws) return fail(MPC_E_ARG, "null argument");
  if (bytes < p->ws_bytes) return fail(MPC_E_WORKSPACE, "workspace too small");
  if (((uintptr_t)ws & 255) != 0) return fail(MPC_E_ARG, "workspace must be 256-byte aligned");
  if (((uintptr_t)p->in.cs & 15) != 0) return fail(MPC_E_ARG, "cs buffer must be 16-byte aligned");
  if (((uintptr_t)p->in.up & 3) != 0 || ((uintptr_t)p->in.down & 3) != 0)
    return fail(MPC_E_ARG, "flank buffers must be 4-byte aligned");
  p->ws = (uint8_t*)ws;
  HIPCHK(hipMemcpy(at<int32_t>(p, mpc_plan::B_NOF), p->h_n.data(), 4 * p->S, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(at<int32_t>(p, mpc_plan::B_GBASE), p->h_gbase.data(), 4 * (p->S + 1), hipMemcpyHostToDevice));
  if (!p->work_parse.empty())
    HIPCHK(hipMemcpy(at<int32_t>(p, mpc_plan::B_WPARSE), p->work_parse.data(), 4 * p->work_parse.size(), hipMemcpyHostToDevice));
  if (!p->work_bc.empty())
    HIPCHK(hipMemcpy(at<int32_t>(p, mpc_plan::B_WBC), p->work_bc.data(), 4 * p->work_bc.size(), hipMemcpyHostToDevice));
  if (!p->work_wave.empty())
    HIPCHK(hipMemcpy(at<int32_t>(p, mpc_plan::B_WWAVE), p->work_wave.data(), 4 * p->work_wave.size(),
                     hipMemcpyHostToDevice));
  if (!p->work_sub.empty())
    HIPCHK(hipMemcpy(at<int32_t>(p, mpc_plan::B_WSUB), p->work_sub.data(), 4 * p->work_sub.size(), hipMemcpyHostToDevice));
  if (!p->work_subsum.empty())
    HIPCHK(hipMemcpy(at<int32_t>(p, mpc_plan::B_WSUBSUM), p->work_subsum.data(), 4 * p->work_subsum.size(),
                     hipMemcpyHostToDevice));
  HIPCHK(hipFuncSetAttribute(parse_kernel(p), hipFuncAttributeMaxDynamicSharedMemorySize,
                             p->parse_lds));
  p->bound = true;
  p->runt_dirty = true;
  return MPC_OK;
}


#define NEED_BOUND(p) do { if (!(p) || !(p)->bound) return fail(MPC_E_STATE, "plan not bound"); } while (0)

int mpc_parse(mpc_plan* p, void* stream) {
  NEED_BOUND(p);
  hipStream_t st = (hipStream_t)stream;
  Dev d = plan_dev(p);
  {
    ClearArgs c{};
    bool over = false;
    auto add = [&](void* ptr, int64_t words, uint32_t v) {
      if (c.n == 24) { over = true; return; }  // ClearArgs holds 24 ranges
      c.ptr[c.n] = reinterpret_cast<uint32_t*>(ptr); c.words[c.n] = words; c.value[c.n] = v; ++c.n;
    };
    add(d.status, MPC_ST_FIRST_READ, 0u);                // (disjoint ranges: no ordering between threads)
    add(d.status + MPC_ST_FIRST_READ, 1, 0xffffffffu);
    add(d.status + MPC_ST_FIRST_READ + 1, MPC_ST_WORDS - MPC_ST_FIRST_READ - 1, 0u);
    add(d.hasleft, (int64_t)(p->sz[mpc_plan::B_HASLEFT] / 4), 0u);
    add(d.ovf_cnt, 1, 0u);
    add(d.diff, p->G, 0u);
    add(d.sub, 4 * p->G, 0u);
    add(d.maxR, p->G, 0u);
    if (p->rsort_multi) add(d.gcnt, p->G + 1, 0u);
    if (p->tally_mode == 4) {  // the bucket page words and page counts of the HBM-state parse
      add(at<int32_t>(p, mpc_plan::B_BKCUR), (int64_t)p->n_parse_wg * p->nbmax, kPgInit);
      add(at<int32_t>(p, mpc_plan::B_BKCNT), (int64_t)p->n_parse_wg * p->nbmax, 0u);
    }
    add(d.maxdepth, p->S, 0u);
    add(d.ksum, 2 * p->cnt[mpc_plan::B_KSUM], 0u);  // look-back status words (epoch-tagged as well)
    add(d.bsum, 2 * p->cnt[mpc_plan::B_BSUM], 0u);
    add(d.M, p->runs_cap, 0u);
    add(d.runR, p->runs_cap, 0u);
    if (p->runt_dirty) add(d.runt, 16 * p->runs_cap, 0u);
    add(d.rows, 4 * p->row_cap, 0u);
    add(d.meta, (int64_t)(p->sz[mpc_plan::B_META] / 4), 0u);
    if (over) return fail(MPC_E_STATE, "K_clear range table overflow");
    const int64_t most = std::max<int64_t>(4 * p->row_cap, std::max<int64_t>(4 * p->G, (p->runt_dirty ? 16 : 1) * p->runs_cap));
    hipLaunchKernelGGL(K_clear, dim3(std::min<unsigned>(nblk(most, 256), 1024)), dim3(256), 0, st, c);
    HIPCHK(hipGetLastError());
    p->runt_dirty = false;  // only once the clear is enqueued
  }
  if (p->n_parse_wg > 0) {
    launch_parse(p, d, st);
    launch_subs(p, d, st);
  }
  if (d.wo_x)  // several shards, negative starts: the strings as exchange records
    hipLaunchKernelGGL(K_wopack, dim3(std::min<unsigned>(nblk(p->wo_cap, 256), 64)), dim3(256), 0, st, d);
  HIPCHK(hipGetLastError());
  return MPC_OK;
}

int mpc_index(mpc_plan* p, void* stream) {
  NEED_BOUND(p);
  hipStream_t st = (hipStream_t)stream;
  Dev d = plan_dev(p);
  const int32_t nrb = (int32_t)((p->N + kRS - 1) / kRS);
  // the insertion work units need only the parse: cut in the RIGHT-split launch
  // (one stream: a second one's event fork/join cost more than the overlap, measured)
  const int32_t nub = (int32_t)((p->n_bc + kUnitEntriesPerBlock - 1) / kUnitEntriesPerBlock);  // unit-cutting blocks
  if (nrb + nub > 0) hipLaunchKernelGGL(K_rsplit_units, dim3(nrb + nub), dim3(kRS), 0, st, d, unit_args(p, d), nrb);
  launch_rsort(p, d, st);
  hipLaunchKernelGGL(K_rstart, dim3(nblk(std::max<int64_t>(p->G + 1, p->N))), dim3(256), 0, st, d);  // (M <= N)
  HIPCHK(hipGetLastError());
  return MPC_OK;
}

int mpc_runs(mpc_plan* p, void* stream) {
  NEED_BOUND(p);
  hipStream_t st = (hipStream_t)stream;
  Dev d = plan_dev(p);
  if (p->n_shards > 1) {
    hipLaunchKernelGGL(K_runs, dim3(nblk(p->G + 1, kRunsGB)), dim3(kRunsGB), 0, st, d, next_epoch());
    if (p->N > 0) hipLaunchKernelGGL(K_runR, dim3(std::min<unsigned>(nblk(p->N), 1024)), dim3(256), 0, st, d);
  }
  HIPCHK(hipGetLastError());
  return MPC_OK;
}

int mpc_tally(mpc_plan* p, void* stream) {
  NEED_BOUND(p);
  hipStream_t st = (hipStream_t)stream;
  Dev d = plan_dev(p);
  launch_left(p, d, st);  // (units: mpc_index)
  p->runt_dirty = true;  // until K_ins has mapped (and cleared) the run tallies
  HIPCHK(hipGetLastError());
  return MPC_OK;
}


int mpc_wrap(mpc_plan* p, void* stream) {
  NEED_BOUND(p);
  hipStream_t st = (hipStream_t)stream;
  Dev d = plan_dev(p);
  if (p->n_shards > 1 && p->wo_cap > 0) launch_wrap(p, d, st);  // (one shard: mpc_layout launches them)
  HIPCHK(hipGetLastError());
  return MPC_OK;
}

int mpc_layout(mpc_plan* p, void* stream) {
  NEED_BOUND(p);
  hipStream_t st = (hipStream_t)stream;
  Dev d = plan_dev(p);
  if (p->wo_cap > 0) {  // negative starts: the wrapped odd positions first
    if (p->n_shards == 1) launch_wrap(p, d, st);
    else hipLaunchKernelGGL(K_wofold, dim3(std::min<unsigned>(nblk(p->wo_cap, 256), 64)), dim3(256), 0, st, d);
    hipLaunchKernelGGL(K_layout<true>, dim3(nblk(p->G, kGB)), dim3(kGB), 0, st, d, next_epoch());
  } else {
    hipLaunchKernelGGL(K_layout<false>, dim3(nblk(p->G, kGB)), dim3(kGB), 0, st, d, next_epoch());
  }
  HIPCHK(hipGetLastError());
  return MPC_OK;
}

int mpc_rows(mpc_plan* p, void* stream) {
  NEED_BOUND(p);
  hipStream_t st = (hipStream_t)stream;
  Dev d = plan_dev(p);
  hipLaunchKernelGGL(K_ins, dim3(ins_grid(p)), dim3(kUB), 0, st, ins_args(p, d));
  HIPCHK(hipGetLastError());
  p->runt_dirty = false;  // K_ins (enqueued) zeroes every run tally it maps (all runs of all gaps)
  if (p->N > 0) launch_flank(p, d, st);
  if (p->wo_cap > 0) hipLaunchKernelGGL(K_worows, dim3(64), dim3(256), 0, st, d);
  HIPCHK(hipGetLastError());
  return MPC_OK;
}

int mpc_consensus(mpc_plan* p, double mdf, double gtf, void* stream) {
  NEED_BOUND(p);
  hipStream_t st = (hipStream_t)stream;
  Dev d = plan_dev(p);
  d.mdf = mdf;
  d.gtf = gtf;
  const int64_t R = p->row_cap;
  if (nblk(R, 256) > kCallBlocksMax) hipLaunchKernelGGL(K_call<kCRBig>, dim3(nblk(R, 256 * kCRBig)), dim3(256), 0, st, d, R);
  else hipLaunchKernelGGL(K_call<1>, dim3(nblk(R, 256)), dim3(256), 0, st, d, R);
  hipLaunchKernelGGL(K_select, dim3(nblk(R, kKB)), dim3(256), 0, st, d, R, next_epoch());
  HIPCHK(hipGetLastError());
  return MPC_OK;
}

int mpc_profile_kernel(mpc_plan* p, int which, void* stream) {
  NEED_BOUND(p);
  hipStream_t st = (hipStream_t)stream;
  Dev d = plan_dev(p);
  if (p->N == 0) return MPC_OK;
  switch (which) {
    case MPC_K_PARSE:  // re-adds the odd tallies: status/tallies are stale until the next mpc_run
      launch_parse(p, d, st);
      break;
    case MPC_K_LEFT:
      launch_left(p, d, st);
      p->runt_dirty = true;
      break;
    case MPC_K_INS:
      hipLaunchKernelGGL(K_ins, dim3(ins_grid(p)), dim3(kUB), 0, st, ins_args(p, d));
      break;
    case MPC_K_FLANK:
      launch_flank(p, d, st);
      break;
    case MPC_K_RSORT:
      launch_rsort(p, d, st);
      break;
    default:
      return fail(MPC_E_ARG, "unknown kernel");
  }
  HIPCHK(hipGetLastError());
  return MPC_OK;
}

#if defined(MPC_STAMPS) || defined(MPC_STAMPS_LEFT)
// diagnostic build only: per-wave K_parse (K_left) segment cycle sums (kStampSeg per wave)
int mpc_debug_stamps(uint64_t* out, int64_t n_words) {
  const int64_t nw = std::min<int64_t>(n_words, (int64_t)kStampWaves * kStampSeg);
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), (size_t)nw * 8, 0, hipMemcpyDeviceToHost));
  return MPC_OK;
}
int mpc_debug_stamps_clear(void) {
  static std::vector<uint64_t> z((size_t)kStampWaves * kStampSeg, 0);
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z.data(), z.size() * 8, 0, hipMemcpyHostToDevice));
  return MPC_OK;
}
#endif

int mpc_run(mpc_plan* p, double mdf, double gtf, void* stream) {
  int rc;
  if ((rc = mpc_parse(p, stream))) return rc;
  if ((rc = mpc_index(p, stream))) return rc;
  if ((rc = mpc_runs(p, stream))) return rc;
  if ((rc = mpc_tally(p, stream))) return rc;
  if ((rc = mpc_layout(p, stream))) return rc;
  if ((rc = mpc_rows(p, stream))) return rc;
  return mpc_consensus(p, mdf, gtf, stream);
}

}  // extern "C"
