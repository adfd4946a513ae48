// The plan behind the C-ABI's mpc_plan handle (include/mpc.h): what the host
// planner (mpc_plan.cpp, no HIP) decides and the phases (mpc_kernels.hip, with
// the argument fillers and launchers of the mpc_k_*.h stage headers) launch from.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "mpc.h"
#include "mpc_geometry.h"

// sets the message mpc_last_error() returns; every translation unit of the
// library reports through it (mpc_plan.cpp)
__attribute__((visibility("hidden"))) int mpc_fail_(int code, const char* msg);
static inline int fail(int code, const std::string& msg) { return mpc_fail_(code, msg.c_str()); }

struct mpc_plan {
  mpc_input in;
  std::vector<int64_t> ref_len, read_begin;
  std::vector<int32_t> h_n, h_gbase;
  int64_t N = 0, Ng = 0, G = 0, row_cap = 0, runs_cap = 0, ins_cap = 0, ovf_cap = 0, pages_cap = 0;
  int64_t wo_cap = 0, wo_p2 = 1;  // strings into wrapped odd positions (negative starts): list bound, sort size
  int32_t S = 0;
  int32_t overrides = 0;  // MPC_OVR_* (experiment builds only)
  uint32_t sentinel = 0;
  int end_bit = 0;
  bool rsort_multi = false;  // mixed RIGHT events sorted by K_rscan / K_rscatter / K_rsegsort (many reads)
  size_t ws_bytes = 0;
  uint8_t* ws = nullptr;
  std::vector<int32_t> work_parse, work_bc, work_sub;  // int4 records
  std::vector<int32_t> work_subsum;                   // int4 {sample, window, first K_subs block, end}
  int subsum_rows = 0;                                // most K_subs blocks of one (sample, window)
  std::vector<int32_t> work_wave;                     // per parse workgroup: kMaxCh + 1 chunk boundaries
  int32_t sub_wins = 0;                               // tally mode 3: substitution-event windows
  int64_t subev_cap = 0;
  int n_parse_wg = 0, parse_lds = 0, nbmax = 1, parse_win = 1024, parse_nw = 8;
  int defer_off = 0;                                  // K_parse deferred placement: its queues' LDS offset (0: off)
  int64_t n_bc = 0, units_cap = 0, max_wg_reads = 0;
  int32_t left_ub = 1024;  // K_left threads per block
  int32_t shard = 0, n_shards = 1;
  int tally_mode = 0;  // K_parse TM
  // The workspace buffers, in layout order (count and element size of each:
  // size_buffers in mpc_plan.cpp, one entry per name, in this order).
  enum {
    B_STATUS, B_NOF, B_GBASE, B_IEND, B_PGOWN, B_INSSORT, B_BKCNT, B_BKOFF, B_RBASE, B_OVF, B_OVFCNT,
    B_HASLEFT, B_KIN, B_VIN, B_KOUT, B_VOUT, B_KTMP, B_VTMP, B_BCNT, B_BPRE, B_RLEN, B_RPOS, B_RSTART, B_RSLOC, B_ROFF, B_RCNT, B_RCNTALL,
    // MAXR, M, RUNR adjacent and in this order: one MAX exchange over their span (mpc.h)
    B_DIFF, B_SUB, B_MAXR, B_M, B_RUNR, B_HIR, B_LOR, B_LOF, B_ROWCNT, B_ROWBASE, B_BSUM, B_ROWS,
    B_META, B_RES, B_KEEP, B_KSUM, B_CALLS, B_NCALLS, B_MAXD, B_SROW, B_WPARSE, B_WBC, B_UNITS, B_RUNT,
    B_SUBEV, B_SUBCNT, B_WSUB, B_BKCUR, B_WWAVE, B_SUBSLAB, B_WSUBSUM, B_GCNT, B_KSLOT, B_RSFLAG, B_PGLIST,
    B_WOEV, B_WOKEY, B_WOIDX, B_WOERUN, B_WOPOS, B_WORUN, B_WOREC, B_WOALL, B_WOCOV, B_COUNT
  };
  size_t off[B_COUNT];
  size_t sz[B_COUNT];
  int64_t cnt[B_COUNT];
  bool bound = false;
  bool runt_dirty = true;  // runt may hold tallies: K_clear zeroes it (K_ins zeroes what it maps)
};
