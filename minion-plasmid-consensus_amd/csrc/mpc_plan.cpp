// libmpc's host planner: every C-ABI entry point (include/mpc.h) that touches
// no device.  mpc_plan_create turns the shape of an input into the parse
// geometry, the work tables and the workspace layout the phases of
// mpc_kernels.hip launch from (the kernels and their launchers: mpc_k_*.h).
// Plain C++ (no HIP): what it shares with the kernels is mpc_geometry.h.
#include "mpc_plan.h"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <memory>

using namespace mpc_geom;

static thread_local std::string g_err;
int mpc_fail_(int code, const char* msg) { g_err = msg; return code; }

namespace {

constexpr int kLdsCap = 160 * 1024;
constexpr int kMaxWavesCu = 16;  // VGPR budget of K_parse (<= 128 VGPRs -> 4 waves per SIMD)

// what one planning step leaves for the next ones and the plan does not keep
struct Scratch {
  int64_t n_max = 0;          // longest reference
  bool sub_events = false;    // tally mode 3 would keep its substitutions as window events (K_subs)
  int per_cu = 1;             // resident parse workgroups per CU
  std::vector<int> pw_begin;  // [S + 1] first parse workgroup of every sample
};

int parse_lds_of(const mpc_plan& p, const Scratch& sc, int win, int tm, int nw) {
  return win == 512    ? parse_lds_bytes<512>((int)sc.n_max, tm, p.nbmax, nw)
         : win == 2048 ? parse_lds_bytes<2048>((int)sc.n_max, tm, p.nbmax, nw)
                       : parse_lds_bytes<1024>((int)sc.n_max, tm, p.nbmax, nw);
}

// the shard, the coordinate spaces (gaps, runs, rows) and the event list bounds
int size_spaces(mpc_plan& p, const mpc_input& in, int64_t row_cap) {
  p.in = in;
  p.S = in.n_samples;
  p.N = in.n_reads;
  p.Ng = in.n_reads_global > 0 ? in.n_reads_global : in.n_reads;
  p.n_shards = in.n_shards > 0 ? in.n_shards : 1;
  p.shard = in.shard;
  if (p.shard < 0 || p.shard >= p.n_shards) return fail(MPC_E_ARG, "shard out of range");
  if (p.Ng < p.N || in.read_offset < 0 || in.read_offset + p.N > p.Ng)
    return fail(MPC_E_ARG, "read shard [read_offset, read_offset + n_reads) outside [0, n_reads_global)");
  p.ref_len.assign(in.h_ref_len, in.h_ref_len + p.S);
  p.read_begin.assign(in.h_read_begin, in.h_read_begin + p.S + 1);
  p.h_n.resize(p.S);
  p.h_gbase.resize(p.S + 1);
  int64_t g = 0;
  for (int s = 0; s < p.S; ++s) {
    if (p.ref_len[s] < 0 || p.ref_len[s] > kMaxRefLen) return fail(MPC_E_ARG, "reference length out of range (at most 2^22 - 2 bases)");
    p.h_n[s] = (int32_t)p.ref_len[s];
    p.h_gbase[s] = (int32_t)g;
    g += p.ref_len[s] + 1;
  }
  p.h_gbase[p.S] = (int32_t)g;
  p.G = g;
  if (p.G >= (1ll << 30)) return fail(MPC_E_ARG, "too many positions");
  if (p.Ng >= (1ll << 30)) return fail(MPC_E_ARG, "too many reads (event words hold 30-bit read indices)");
  p.row_cap = row_cap > 0 ? row_cap : 1;
  if (p.row_cap >= (1ll << 31)) return fail(MPC_E_ARG, "row capacity must be < 2^31");
  p.runs_cap = p.Ng + p.G;
  p.ins_cap = in.cs_bytes / 2 + 3 * p.N + 16;  // insertions (>= 2 cs bytes each) + slack per read
  p.ovf_cap = in.cs_bytes / 6 + 16;
  // strings Python's negative wrap writes into odd positions: <= 2 flanks per
  // read with a negative start plus its '+' insertions (>= 2 cs bytes each);
  // one shard only (the replay needs every string of a position)
  if (in.neg_reads < 0 || in.neg_cs_bytes < 0) return fail(MPC_E_ARG, "negative neg_reads / neg_cs_bytes");
  // (several shards: neg_reads / neg_cs_bytes are the totals over all of them, so every shard
  // sizes the same list and holds all shards' strings after the gather)
  p.wo_cap = in.neg_reads > 0 ? std::min<int64_t>(kWoCapMax, 2 * in.neg_reads + in.neg_cs_bytes / 2 + 16) : 0;
  while (p.wo_p2 < p.wo_cap) p.wo_p2 <<= 1;
  int eb = 1;
  while ((1ll << eb) <= p.G + 1) ++eb;
  p.end_bit = eb;
  p.sentinel = (uint32_t)((1ull << eb) - 1);
  return MPC_OK;
}

// parse geometry: tally mode, window and waves per workgroup that give the
// most resident waves per CU (ties: the earlier candidate -- LDS tallies,
// larger windows, the 12-byte tallies)
int choose_parse_geometry(mpc_plan& p, Scratch& sc) {
  for (int s = 0; s < p.S; ++s) {
    sc.n_max = std::max<int64_t>(sc.n_max, p.ref_len[s]);
    p.nbmax = std::max<int>(p.nbmax, (int)((p.ref_len[s] + 1 + kBW - 1) / kBW));
  }
  // score = resident waves x window efficiency (measured at C2: 512 B windows
  // cost ~25 % more per byte than 2 KiB ones, 1 KiB ~5 %).  Tally mode 3 keeps
  // only depth in LDS; its substitutions are window events (K_subs) while the
  // reference fits kMaxSubWins windows, and then it competes on score: at C3 /
  // C4 (10 kb) its 16 waves beat tm 2's 12 (parse 3060 -> 2947 us, 3396 ->
  // 3004 us), at C2 tm 1 with 16 waves wins the tie (167 vs 197 us).  Beyond
  // that its substitutions are global atomics: only when tm 1 / 2 do not fit.
  sc.sub_events = sc.n_max <= (int64_t)kSubWin * kMaxSubWins;
  static const int cand[10][2] = {{1, 2048}, {2, 2048}, {1, 1024}, {2, 1024}, {3, 2048}, {3, 1024},
                                  {1, 512}, {0, 2048}, {0, 1024}, {0, 512}};
  int best = -1;
  // tuning override for measurements: MPC_PARSE_GEOMETRY="tm,win,nw" takes that
  // candidate when it fits the LDS budget (else the planner's choice)
  int o_tm = -1, o_win = -1, o_nw = -1;
#ifdef MPC_TUNING_OVERRIDES  // experiment builds only (scripts/geom_ab.py); reported in mpc_plan_info.overrides
  if (const char* e = getenv("MPC_PARSE_GEOMETRY")) sscanf(e, "%d,%d,%d", &o_tm, &o_win, &o_nw);
#endif
  for (const auto& c : cand)
    for (int nw : {16, 12, 8}) {
      if (c[0] == 3 && !sc.sub_events && best > 0) break;  // global-atomic tm 3 only when nothing else fits
      if (c[0] == 0 && best > 0) break;                     // tm 0 only when no LDS mode fits
      const int lds = parse_lds_of(p, sc, c[1], c[0], nw);
      if (lds > kLdsCap) continue;
      const int wgs = std::max(1, std::min(kLdsCap / lds, kMaxWavesCu / nw));
      int score = wgs * nw * (c[1] == 512 ? 75 : c[1] == 1024 ? 95 : 100);
      const bool forced = c[0] == o_tm && c[1] == o_win && nw == o_nw;
      if (forced) score = 1 << 30;
      if (score > best) {
        best = score; p.tally_mode = c[0]; p.parse_win = c[1]; p.parse_nw = nw; sc.per_cu = wgs;
        p.overrides = forced ? (p.overrides | MPC_OVR_GEOMETRY) : (p.overrides & ~MPC_OVR_GEOMETRY);
      }
    }
  if (best < 0) {
    // references beyond every LDS mode (~312 kb): per-gap parse state in HBM
    for (int nw : {16, 12, 8}) {
      const int lds = parse_lds_bytes<1024>((int)sc.n_max, 4, p.nbmax, nw);
      if (lds > kLdsCap) continue;
      const int wgs = std::max(1, std::min(kLdsCap / lds, kMaxWavesCu / nw));
      if (wgs * nw > best) { best = wgs * nw; p.tally_mode = 4; p.parse_win = 1024; p.parse_nw = nw; sc.per_cu = wgs; }
    }
  }
  if (best < 0) return fail(MPC_E_ARG, "reference too long for the LDS budget");
  p.parse_lds = parse_lds_of(p, sc, p.parse_win, p.tally_mode, p.parse_nw);
  return MPC_OK;
}

// workgroups of a sample of ns reads at R reads per workgroup: >= 64 reads
// each, at most wcap (the 16-bit tallies)
int64_t sample_wgs(int64_t ns, int64_t R, int64_t wcap) {
  int64_t ch = (ns + R - 1) / R;
  ch = std::min<int64_t>(ch, (ns + 63) / 64);
  return std::max<int64_t>(ch, (ns + wcap - 1) / wcap);
}

// boundaries of [a, b) cut into k parts: equal cs BYTES when the host copy
// of cs_off is given (the parse time of a read range follows its bytes, not
// its read count: a count split left waves idle at the epilogue barrier 22 %
// of their time, profiles/r03_stamps), else equal read counts
void cut(const int64_t* hco, int64_t a, int64_t b, int64_t k, std::vector<int64_t>& out) {
  out.assign((size_t)k + 1, a);
  out[(size_t)k] = b;
  for (int64_t c = 1; c < k; ++c) {
    int64_t x = a + (b - a) * c / k;
    if (hco) {
      const int64_t tgt = hco[a] + (hco[b] - hco[a]) * c / k;
      x = std::lower_bound(hco + a, hco + b + 1, tgt) - hco;
    }
    out[(size_t)c] = std::min(std::max(x, out[(size_t)c - 1]), b);
  }
}

// workgroups per sample: the smallest largest-chunk R with sum_s ceil(ns / R)
// <= the resident slots (256 CUs x per_cu), so that the parse is one balanced
// wave of workgroups (C5: 24 samples x 10 instead of x 11 = 264 > 256 slots,
// whose 8 second-wave workgroups doubled K_parse); >= 64 reads per workgroup
void split_workgroups(mpc_plan& p, Scratch& sc) {
  const int cus = p.in.parse_cus > 0 && p.in.parse_cus < 256 ? p.in.parse_cus : 256;
  int64_t target = (int64_t)cus * sc.per_cu;
#ifdef MPC_TUNING_OVERRIDES
  if (const char* e = getenv("MPC_PARSE_WGS")) {  // measurement override
    target = std::max<int64_t>(1, atoll(e));
    p.overrides |= MPC_OVR_WGS;
  }
#endif
  const int64_t wcap = wg_reads_cap(p.tally_mode);
  int64_t R_lo = 1, R_hi = std::max<int64_t>(p.N, 1);
  while (R_lo < R_hi) {
    const int64_t mid = (R_lo + R_hi) / 2;
    int64_t tot = 0;
    for (int s = 0; s < p.S; ++s) tot += sample_wgs(p.read_begin[s + 1] - p.read_begin[s], mid, wcap);
    if (tot <= target) R_hi = mid; else R_lo = mid + 1;
  }
  std::vector<int64_t> bnd;
  sc.pw_begin.assign(p.S + 1, 0);
  for (int s = 0; s < p.S; ++s) {
    sc.pw_begin[s] = (int)(p.work_parse.size() / 4);
    const int64_t a = p.read_begin[s], b = p.read_begin[s + 1], ns = b - a;
    if (ns <= 0) continue;
    const int64_t ch = sample_wgs(ns, R_lo, wcap);
    cut(p.in.h_cs_off, a, b, ch, bnd);
    bool capped = true;  // the byte split must keep the 16-bit tallies' reads-per-workgroup cap
    for (int64_t c = 0; c < ch; ++c) capped &= bnd[(size_t)c + 1] - bnd[(size_t)c] <= wcap;
    for (int64_t c = 0; c < ch; ++c) {
      const int64_t x = capped ? bnd[(size_t)c] : a + ns * c / ch;
      const int64_t y = capped ? bnd[(size_t)c + 1] : a + ns * (c + 1) / ch;
      if (y > x) p.work_parse.insert(p.work_parse.end(), {s, (int32_t)x, (int32_t)y, 0});
      p.max_wg_reads = std::max<int64_t>(p.max_wg_reads, y - x);
    }
  }
  sc.pw_begin[p.S] = (int)(p.work_parse.size() / 4);
  p.n_parse_wg = sc.pw_begin[p.S];
}

// the chunks of every workgroup (its waves take them in turn): nw chunks
// with 5/8 of the bytes, then nw with a quarter and nw with the last
// eighth, so the last chunks taken are the small ones (measured against 4
// groups of 1/2..1/8, 2 groups, equal quarters and one chunk per wave:
// DESIGN.md "Parse work split")
void build_chunk_table(mpc_plan& p) {
  constexpr int kGroups = 3;
  const int64_t* hco = p.in.h_cs_off;
  const int nw = p.parse_nw, nch = std::min(kMaxCh, kGroups * nw);
  std::vector<int64_t> part;
  for (size_t k = 0; k < p.work_parse.size(); k += 4) {
    const int64_t a = p.work_parse[k + 1], b = p.work_parse[k + 2];
    std::vector<int64_t> cb{a};
    static constexpr double grp[kGroups] = {0.625, 0.25, 0.125};
    // groups only while the smallest chunks still hold about half a window
    // (else one chunk per wave: C1's 3 KiB per wave ran 11 % slower cut in three)
    const int64_t wg_bytes = hco ? hco[b] - hco[a] : (b - a) * (p.in.cs_bytes / std::max<int64_t>(1, p.N));
    const int ng = wg_bytes >= 4 * (int64_t)nw * p.parse_win ? kGroups : 1;
    int64_t lo = a;
    double acc = 0;
    for (int g = 0; g < ng && (int)cb.size() - 1 < nch; ++g) {
      acc += grp[g];
      int64_t hi = b;
      if (g < ng - 1) {  // group end: the read where the cumulative byte fraction is reached
        if (hco) hi = std::lower_bound(hco + a, hco + b + 1, hco[a] + (int64_t)((hco[b] - hco[a]) * acc)) - hco;
        else hi = a + (int64_t)((b - a) * acc);
        hi = std::min(std::max(hi, lo), b);
      }
      cut(hco, lo, hi, nw, part);
      for (int c = 1; c <= nw; ++c) cb.push_back(part[(size_t)c]);
      lo = hi;
    }
    p.work_parse[k + 3] = (int32_t)(cb.size() - 1);
    for (int c = 0; c <= kMaxCh; ++c) p.work_wave.push_back((int32_t)cb[(size_t)std::min<int>(c, (int)cb.size() - 1)]);
  }
}

// tally mode 3: substitutions as events per kSubWin-position window (K_subs);
// then whether K_parse defers its insertion placement
void build_subs_tables(mpc_plan& p, const Scratch& sc) {
  const std::vector<int>& pw_begin = sc.pw_begin;
  p.sub_wins = 0;
  if (p.tally_mode == 3 && sc.sub_events) {
    p.sub_wins = (int32_t)((sc.n_max + kSubWin - 1) / kSubWin);
    // parse workgroups per K_subs block: about one block per CU (each block's
    // LDS tally is 128 KiB; more blocks = more flush atomics, fewer = fewer CUs)
    int64_t pairs = 0;
    for (int s = 0; s < p.S; ++s)
      pairs += ((p.ref_len[s] + kSubWin - 1) / kSubWin) * (int64_t)(pw_begin[s + 1] - pw_begin[s]);
    const int kc = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)kSubsWG, (pairs + 255) / 256,
                                                                 65535 / std::max<int64_t>(1, p.max_wg_reads)}));
    for (int s = 0; s < p.S; ++s)
      for (int w = 0; w * (int64_t)kSubWin < p.ref_len[s]; ++w) {
        const int b0 = (int)(p.work_sub.size() / 4);
        for (int c = pw_begin[s]; c < pw_begin[s + 1]; c += kc)
          p.work_sub.insert(p.work_sub.end(), {s, w, c, std::min(c + kc, pw_begin[s + 1])});
        const int b1 = (int)(p.work_sub.size() / 4);
        if (b1 > b0) p.work_subsum.insert(p.work_subsum.end(), {s, w, b0, b1});
        p.subsum_rows = std::max(p.subsum_rows, b1 - b0);
      }
  }
  // deferred placement: the per-wave queues after the parse LDS, when they fit
  p.defer_off = 0;
  if (p.parse_win == 2048 && p.in.neg_reads == 0 &&
      (p.tally_mode == 1 || (p.tally_mode == 3 && p.sub_wins == 1))) {
    const int off = (p.parse_lds + 15) & ~15;
    const int end = off + defer_bytes(p.parse_nw);
    if (end <= kLdsCap && std::max(1, std::min(kLdsCap / end, kMaxWavesCu / p.parse_nw)) == sc.per_cu) {
      p.defer_off = off;
      p.parse_lds = end;
    }
  }
}

// the insertion buckets' work entries (K_rsplit_units cuts them into units) and K_left's block size
void build_bucket_work(mpc_plan& p, const Scratch& sc) {
  const std::vector<int>& pw_begin = sc.pw_begin;
  for (int s = 0; s < p.S; ++s) {
    const int nb = (int)((p.ref_len[s] + 1 + kBW - 1) / kBW);
    if (pw_begin[s + 1] == pw_begin[s]) continue;  // no reads: nothing to tally
    for (int b = 0; b < nb; ++b)  // insertion buckets
      for (int c = pw_begin[s]; c < pw_begin[s + 1]; c += 256)
        p.work_bc.insert(p.work_bc.end(), {s, b, c, std::min(c + 256, pw_begin[s + 1])});
  }
  p.n_bc = (int64_t)(p.work_bc.size() / 4);
  // K_left blocks of 512 threads (units of 8 k events) when there are many
  // small insertion buckets: C5's 24 x 469 buckets of ~3 k events each are
  // ~22 units per block in turn, whose fixed per-unit cost dominated at 1024
  // threads (K_left 352 -> 287 us).  Few or large buckets (C1-C4) keep 1024
  // (measured 4-45 % slower at 512: one unit per block, latency-bound).  The
  // bucket size is estimated from the cs bytes per (sample, bucket)
  int64_t nb_all = 0;
  for (int s = 0; s < p.S; ++s) nb_all += (p.ref_len[s] + 1 + kBW - 1) / kBW;
  p.left_ub = nb_all > 4 * 512 && p.in.cs_bytes / nb_all < (256 << 10) ? 512 : kUB;
  // insertion events in 64-event pages per (parse workgroup, bucket)
  // (parse_page_base: the last workgroup's region ends at this bound)
  p.pages_cap = parse_page_base(p.in.cs_bytes, p.N, p.n_parse_wg, p.nbmax) + 1;
  // work units of left_ub * kEPT / 64 pages
  p.units_cap = p.pages_cap / (p.left_ub * kEPT / kPgEv) + p.n_bc + 1;
}

// The workspace, stated once: every buffer of mpc_plan's enum with its element
// count and element size, in layout order.
struct BufSize { int b; int64_t count; size_t elem; };
int size_buffers(mpc_plan& p) {
  using P = mpc_plan;
  const int64_t N = p.N, Ng = p.Ng, G = p.G, R = p.row_cap, RU = p.runs_cap, S = p.S;
  const int64_t nbg = (G + kGB - 1) / kGB, nbk = (R + kKB - 1) / kKB, nrb = (N + kRS - 1) / kRS;
  const int64_t wg_buckets = (int64_t)p.n_parse_wg * p.nbmax;
  // K_rsort's one workgroup gathers and sorts in time that grows with the read
  // blocks (C3, 977 blocks: 88 us): many reads take the multi-workgroup path
  p.rsort_multi = nrb > kRsortMultiBlocks;
  const bool multi = p.rsort_multi;
  p.subev_cap = p.sub_wins ? p.in.cs_bytes / kSubEvBytes + 2 * N + 16 : 0;
  const int64_t wo = p.wo_cap, wo_sort = wo ? p.wo_p2 : 0;
  const int64_t wo_x = p.n_shards > 1 ? p.wo_cap : 0;  // the exchange buffers (counts in int32 words but WOCOV)
  const BufSize list[] = {
      {P::B_STATUS, MPC_ST_WORDS, 4}, {P::B_NOF, S, 4}, {P::B_GBASE, S + 1, 4}, {P::B_IEND, N, 4},
      {P::B_PGOWN, p.pages_cap, 4}, {P::B_INSSORT, p.pages_cap * kPgEv, 4},
      {P::B_BKCNT, wg_buckets, 4}, {P::B_BKOFF, wg_buckets, 4}, {P::B_RBASE, p.n_parse_wg, 8},
      {P::B_OVF, p.ovf_cap, sizeof(Ovf)}, {P::B_OVFCNT, 1, 4}, {P::B_HASLEFT, (G + 31) / 32 + 1, 4},
      {P::B_KIN, N, 4}, {P::B_VIN, N, 4}, {P::B_KOUT, N, 4}, {P::B_VOUT, N, 4}, {P::B_KTMP, N, 4}, {P::B_VTMP, N, 4},
      {P::B_BCNT, nrb + 1, 4}, {P::B_BPRE, nrb + 1, 4}, {P::B_RLEN, Ng, 4}, {P::B_RPOS, N > 0 ? N : 1, 4},
      {P::B_RSTART, G + 1, 4}, {P::B_RSLOC, G + 1, 4}, {P::B_ROFF, G + 1, 4},
      {P::B_RCNT, G, 4}, {P::B_RCNTALL, G * p.n_shards, 4},
      {P::B_DIFF, G, 4}, {P::B_SUB, G * 4, 4}, {P::B_MAXR, G, 4},
      {P::B_M, RU, 4}, {P::B_RUNR, RU, 4}, {P::B_HIR, RU, 4}, {P::B_LOR, RU, 4},
      {P::B_LOF, G, 4}, {P::B_ROWCNT, G, 4}, {P::B_ROWBASE, G, 4},
      {P::B_BSUM, 2 * nbg, 8},  // K_layout's look-back status words (rows, diff) per block
      {P::B_ROWS, R * 4, 4}, {P::B_META, (R + 3) / 4 * 4, 1}, {P::B_RES, R * 4, 4}, {P::B_KEEP, nbk * 256, 4},
      {P::B_KSUM, nbk, 8},  // K_select's per-block look-back status words
      {P::B_CALLS, R * 4, 4}, {P::B_NCALLS, S + 1, 4}, {P::B_MAXD, S, 4}, {P::B_SROW, S, 4},
      {P::B_WPARSE, (int64_t)p.work_parse.size(), 4}, {P::B_WBC, (int64_t)p.work_bc.size(), 4},
      {P::B_UNITS, p.units_cap * 8, 4},  // 2 int4 per unit
      {P::B_RUNT, RU * 16, 4},           // per run: inline LEFT bases [bi from the 3' end][code]
      {P::B_SUBEV, p.subev_cap * p.sub_wins, 2},
      {P::B_SUBCNT, p.sub_wins ? (int64_t)p.n_parse_wg * kMaxCh * kMaxSubWins : 0, 4},
      {P::B_WSUB, (int64_t)p.work_sub.size(), 4}, {P::B_BKCUR, p.tally_mode == 4 ? wg_buckets : 0, 4},
      {P::B_WWAVE, (int64_t)p.work_wave.size(), 4},
      {P::B_SUBSLAB, (int64_t)(p.work_sub.size() / 4) * kSubWin * 2, 4},
      {P::B_WSUBSUM, (int64_t)p.work_subsum.size(), 4},
      {P::B_GCNT, multi ? G + 1 : 0, 4}, {P::B_KSLOT, multi ? nrb * (int64_t)kRS : 0, 4},
      {P::B_RSFLAG, multi ? 4 + 2 * ((G + 1 + kScanBlk - 1) / kScanBlk) : 0, 4},
      {P::B_PGLIST, p.pages_cap, 4},
      {P::B_WOEV, wo, sizeof(WoEv)}, {P::B_WOKEY, wo_sort, 8}, {P::B_WOIDX, wo_sort, 4},
      {P::B_WOERUN, 2 * wo, 4},  // run of every sorted string, then K_woprep's scratch
      {P::B_WOPOS, wo, sizeof(WoPos)}, {P::B_WORUN, wo ? 2 * wo + 1 : 0, sizeof(WoRun)},
      {P::B_WOREC, wo_x * 6, 4}, {P::B_WOALL, wo_x ? (wo_x + 1) * 6 : 0, 4}, {P::B_WOCOV, wo_x ? 2 * wo_x + 1 : 0, 4},
  };
  static_assert(sizeof(list) / sizeof(list[0]) == P::B_COUNT, "one entry per workspace buffer");
  for (int b = 0; b < P::B_COUNT; ++b) {
    if (list[b].b != b) return fail(MPC_E_STATE, "workspace buffer list is not in layout order");
    p.cnt[b] = list[b].count;
    p.sz[b] = (size_t)std::max<int64_t>(list[b].count, 1) * list[b].elem;
  }
  return MPC_OK;
}

// the public names of the buffers a caller may look up (mpc_plan_buffer)
constexpr int kPublicBuffer[][2] = {
    {MPC_BUF_STATUS, mpc_plan::B_STATUS}, {MPC_BUF_CALLS, mpc_plan::B_CALLS}, {MPC_BUF_NCALLS, mpc_plan::B_NCALLS},
    {MPC_BUF_MAXDEPTH, mpc_plan::B_MAXD}, {MPC_BUF_ROWS, mpc_plan::B_ROWS}, {MPC_BUF_ROWMETA, mpc_plan::B_META},
    {MPC_BUF_RIGHT_CNT, mpc_plan::B_RCNT}, {MPC_BUF_RIGHT_CNT_ALL, mpc_plan::B_RCNTALL},
    {MPC_BUF_HASLEFT, mpc_plan::B_HASLEFT}, {MPC_BUF_MAXR, mpc_plan::B_MAXR}, {MPC_BUF_RUN_M, mpc_plan::B_M},
    {MPC_BUF_RUN_R, mpc_plan::B_RUNR}, {MPC_BUF_DIFF, mpc_plan::B_DIFF}, {MPC_BUF_SUB, mpc_plan::B_SUB},
    {MPC_BUF_WRAP_REC, mpc_plan::B_WOREC}, {MPC_BUF_WRAP_ALL, mpc_plan::B_WOALL}, {MPC_BUF_WRAP_COVER, mpc_plan::B_WOCOV},
};
static_assert(sizeof(kPublicBuffer) / sizeof(kPublicBuffer[0]) == MPC_BUF_COUNT, "one entry per public MPC_BUF_*");

int layout_workspace(mpc_plan& p) {
  if (int rc = size_buffers(p)) return rc;
  size_t o = 0;
  for (int b = 0; b < mpc_plan::B_COUNT; ++b) {
    o = (o + 255) & ~(size_t)255;
    p.off[b] = o;
    o += p.sz[b];
  }
  // the device side finds the three exchange buffers of the wrapped odd positions from one pointer
  if (p.off[mpc_plan::B_WOALL] != p.off[mpc_plan::B_WOREC] + (size_t)wo_a256((int64_t)p.sz[mpc_plan::B_WOREC]) ||
      p.off[mpc_plan::B_WOCOV] != p.off[mpc_plan::B_WOALL] + (size_t)wo_a256((int64_t)p.sz[mpc_plan::B_WOALL]))
    return fail(MPC_E_STATE, "exchange buffers of the wrapped odd positions are not adjacent");
  p.ws_bytes = (o + 255) & ~(size_t)255;
  return MPC_OK;
}

}  // namespace

extern "C" {

int mpc_version(void) { return MPC_ABI_VERSION; }

size_t mpc_input_layout(size_t* off, int cap) {
#define MPC_F(f) offsetof(mpc_input, f)
  static const size_t o[] = {MPC_F(ref), MPC_F(ref_off), MPC_F(cs), MPC_F(cs_off), MPC_F(tstart), MPC_F(up),
                             MPC_F(up_off), MPC_F(down), MPC_F(down_off), MPC_F(sample), MPC_F(n_samples),
                             MPC_F(h_ref_len), MPC_F(h_read_begin), MPC_F(n_reads), MPC_F(cs_bytes), MPC_F(cs_base),
                             MPC_F(read_offset), MPC_F(n_reads_global), MPC_F(shard), MPC_F(n_shards),
                             MPC_F(h_cs_off), MPC_F(parse_cus), MPC_F(neg_reads), MPC_F(neg_cs_bytes)};
#undef MPC_F
  static_assert(sizeof(o) / sizeof(o[0]) == MPC_INPUT_FIELDS, "mpc_input field table");
  for (int k = 0; off && k < cap && k < MPC_INPUT_FIELDS; ++k) off[k] = o[k];
  return sizeof(mpc_input);
}
const char* mpc_last_error(void) { return g_err.c_str(); }

int mpc_plan_create(const mpc_input* in, int64_t row_cap, mpc_plan** out) {
  if (!in || !out) return fail(MPC_E_ARG, "null argument");
  if (in->n_samples <= 0) return fail(MPC_E_ARG, "n_samples must be > 0");
  std::unique_ptr<mpc_plan> p(new mpc_plan());
  Scratch sc;
  if (int rc = size_spaces(*p, *in, row_cap)) return rc;
  if (int rc = choose_parse_geometry(*p, sc)) return rc;
  split_workgroups(*p, sc);
  build_chunk_table(*p);
  build_subs_tables(*p, sc);
  build_bucket_work(*p, sc);
  if (int rc = layout_workspace(*p)) return rc;
  p->in.h_cs_off = nullptr;  // host array only read while planning
  *out = p.release();
  return MPC_OK;
}

int mpc_plan_destroy(mpc_plan* p) {
  std::unique_ptr<mpc_plan> owned(p);  // freed here
  return MPC_OK;
}

int mpc_plan_get_info(const mpc_plan* p, mpc_plan_info* info) {
  if (!p || !info) return fail(MPC_E_ARG, "null argument");
  info->tally_mode = p->tally_mode;
  info->parse_window = p->parse_win;
  info->parse_waves = p->parse_nw;
  info->parse_lds_bytes = p->parse_lds;
  info->deferred_placement = p->defer_off > 0 ? 1 : 0;
  info->reserved = 0;
  info->parse_workgroups = p->n_parse_wg;
  info->max_reads_per_workgroup = p->max_wg_reads;
  info->reads_per_workgroup_cap = wg_reads_cap(p->tally_mode);
  info->workspace_bytes = (int64_t)p->ws_bytes;
  info->overrides = p->overrides;
  return MPC_OK;
}

// host copies of the parse work tables (tests / tools): n_wg * 4 int32 records
// {sample, first read, end read, chunks} and n_wg * (MPC_PARSE_CHUNKS + 1)
// chunk boundaries; either pointer may be NULL; returns the workgroup count
int mpc_plan_parse_tables(const mpc_plan* p, int32_t* work, int32_t* chunks) {
  if (!p) return fail(MPC_E_ARG, "null argument");
  if (work) std::copy(p->work_parse.begin(), p->work_parse.end(), work);
  if (chunks) std::copy(p->work_wave.begin(), p->work_wave.end(), chunks);
  return p->n_parse_wg;
}

int mpc_plan_workspace_bytes(const mpc_plan* p, size_t* bytes) {
  if (!p || !bytes) return fail(MPC_E_ARG, "null argument");
  *bytes = p->ws_bytes;
  return MPC_OK;
}

int mpc_plan_set_input(mpc_plan* p, const mpc_input* in) {
  if (!p || !in) return fail(MPC_E_ARG, "null argument");
  if (in->n_reads != p->N || in->n_samples != p->S || in->cs_bytes > p->in.cs_bytes ||
      (in->neg_reads > 0) != (p->in.neg_reads > 0))  // (the K_parse the plan bound; the list capacity stays)
    return fail(MPC_E_ARG, "input shape differs from the plan");
  p->in = *in;
  p->in.h_cs_off = nullptr;  // the work split stays the one planned
  return MPC_OK;
}

int mpc_plan_buffer(const mpc_plan* p, int which, size_t* off, int64_t* count) {
  if (!p || !off || !count) return fail(MPC_E_ARG, "null argument");
  for (const auto& m : kPublicBuffer)
    if (m[0] == which) {
      *off = p->off[m[1]];
      *count = p->cnt[m[1]];
      return MPC_OK;
    }
  return fail(MPC_E_ARG, "unknown buffer");
}

}  // extern "C"
