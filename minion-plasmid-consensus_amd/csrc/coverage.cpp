// coverage.cpp -- host half of coverage_qc (include/mpc_coverage.h):
//   mpc_coverage_host    plain scalar walk over the definition, one base at a
//                        time: the CPU checker of K_covparse / K_covfinish, the
//                        timing baseline, --device cpu
//   mpc_coverage_ingest  memory-mapped, multi-threaded PAF read: target, span,
//                        mapq, read length, strand and the cs bytes per kept line
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "host_file.h"
#include "host_threads.h"
#include "mpc_coverage.h"
#include "mpc_cstables.h"
#include "mpc_cswalk_host.h"

namespace {

using sv = std::string_view;

constexpr int kOk = 0;  // MPC_OK of mpc.h

thread_local mpc_host::LastError g_cerr;

using mpc_host::parallel;

// ---------------------------------------------------------------- the walk

// what a token does to the pileup (the effects policy of cs_walk, mpc_cswalk_host.h):
// row is the sample's first row (u32[L + 1][4]), the counts are the record's
struct RowFx {
  uint32_t* row;
  uint64_t n_match = 0, mism = 0, insev = 0, insb = 0, delev = 0, delb = 0;
  void match(int64_t p, int64_t n) {
    for (int64_t i = 0; i < n; ++i) ++row[(p + i) * 4 + 0];
    n_match += (uint64_t)n;
  }
  void mismatch(int64_t p, uint8_t) { ++row[p * 4 + 0]; ++row[p * 4 + 2]; ++mism; }
  void deletion(int64_t p, int64_t n) {
    for (int64_t i = 0; i < n; ++i) ++row[(p + i) * 4 + 1];
    ++delev;
    delb += (uint64_t)n;
  }
  void insertion(int64_t p, int64_t n) { ++row[p * 4 + 3]; ++insev; insb += (uint64_t)n; }
};

// ---------------------------------------------------------------- PAF ingest

// Policy: digits only (1-18 of them); anything else refuses the line.
bool plain_int(sv s, int64_t* out) {
  int64_t v;
  if (s.empty() || s.size() > 18 || mpc_host::leading_digits(s, &v) != s.size()) return false;
  *out = v;
  return true;
}

struct Line {
  sv name, target, cs;
  int64_t qlen, tlen, tstart, tend, mapq;
  char strand;
};

// nullptr, or what is wrong with the line
const char* parse_line(sv line, Line* r) {
  sv col[12];
  size_t a = 0;
  int n = 0;
  sv tags;
  while (n < 12) {
    const size_t e = line.find('\t', a);
    col[n++] = line.substr(a, e == sv::npos ? sv::npos : e - a);
    if (e == sv::npos) { a = line.size(); break; }
    a = e + 1;
  }
  if (n < 12) return "fewer than 12 columns";
  tags = a <= line.size() ? line.substr(a) : sv();
  int64_t unused;
  for (int k : {2, 3, 9, 10})
    if (!plain_int(col[k], &unused)) return "an integer column is not plain digits";
  if (!plain_int(col[1], &r->qlen) || !plain_int(col[6], &r->tlen) || !plain_int(col[7], &r->tstart) ||
      !plain_int(col[8], &r->tend) || !plain_int(col[11], &r->mapq))
    return "an integer column is not plain digits";
  if (col[4].size() != 1 || (col[4][0] != '+' && col[4][0] != '-')) return "the strand is neither + nor -";
  r->name = col[0];
  r->strand = col[4][0];
  r->target = col[5];
  bool found = false;
  for (size_t t = 0; t < tags.size();) {
    size_t e = tags.find('\t', t);
    if (e == sv::npos) e = tags.size();
    const sv tag = tags.substr(t, e - t);
    if (tag.size() >= 3 && tag.compare(0, 3, "cs:") == 0) {
      r->cs = tag.substr(3);
      found = true;
      break;
    }
    t = e + 1;
  }
  return found ? nullptr : "no cs: field";
}

struct Holder {
  std::vector<int32_t> target, mapq;
  std::vector<int64_t> tstart, tend, qlen, cs_off, name_off, target_len;
  std::vector<uint8_t> strand, cs;
  std::string names;
};

int ingest_fail(mpc_coverage_paf* out, const std::string& msg) {
  out->status = 1;
  snprintf(out->message, sizeof(out->message), "%s", msg.c_str());
  return 1;
}

}  // namespace

extern "C" {

const char* mpc_coverage_last_error(void) { return g_cerr.msg.c_str(); }

int mpc_coverage_host(const uint8_t* cs, const int64_t* cs_off, const int64_t* tstart, const int32_t* rec_sample,
                      int64_t n_records, const int64_t* pos_off, const int64_t* region, int32_t n_samples,
                      uint32_t min_depth, uint32_t* rows, uint64_t* stats, int32_t* status, int threads,
                      int64_t* rec_out) {
  if (n_records < 0 || n_records > INT32_MAX) return g_cerr.fail("mpc_coverage_host: n_records outside [0, 2^31)");
  if (n_samples < 1) return g_cerr.fail("mpc_coverage_host: n_samples < 1");
  if (!pos_off || !region || !rows || !stats || !status || !cs_off || (n_records > 0 && (!cs || !tstart || !rec_sample)))
    return g_cerr.fail("mpc_coverage_host: null pointer");
  const size_t S = (size_t)n_samples;
  const std::string bad = mpc_host::check_samples(pos_off, region, S);
  if (!bad.empty()) return g_cerr.fail("mpc_coverage_host: " + bad);
  const size_t n_words = (size_t)pos_off[S] * 4;
  std::fill(rows, rows + n_words, 0u);
  std::fill(stats, stats + S * MPC_COV_STATS, (uint64_t)0);
  status[0] = status[1] = 0;

  // every thread walks its cut of the records into rows of its own (thread 0:
  // the output itself); as many threads as fit 1 GiB of such copies
  const int T = mpc_host::clamp_threads(threads, std::min<int64_t>(n_records, (int64_t)((1ull << 30) / (n_words * 4 + 1)) + 1));
  std::vector<std::vector<uint32_t>> priv((size_t)T);
  std::vector<std::vector<uint64_t>> pstat((size_t)T);
  mpc_host::walk_records(n_records, T, status, [&](int k) {
    uint32_t* my = rows;
    if (k > 0) {
      priv[(size_t)k].assign(n_words, 0u);
      my = priv[(size_t)k].data();
    }
    pstat[(size_t)k].assign(S * 7, 0);
    uint64_t* ps = pstat[(size_t)k].data();
    return [=](int64_t r) {
      const int32_t s = rec_sample[r];
      if (s < 0 || s >= n_samples) return (int)MPC_COV_RANGE;
      RowFx fx = {my + pos_off[s] * 4};
      int64_t end = 0;
      const int code = mpc_host::cs_walk(cs + cs_off[r], cs_off[r + 1] - cs_off[r], tstart[r],
                                         pos_off[s + 1] - pos_off[s] - 1, fx, &end);
      if (code != MPC_COV_OK) return code;
      uint64_t* st = ps + (size_t)s * 7;
      st[0] += 1; st[1] += fx.n_match; st[2] += fx.mism; st[3] += fx.insev; st[4] += fx.insb; st[5] += fx.delev; st[6] += fx.delb;
      if (rec_out) {
        rec_out[2 * r] = end;
        rec_out[2 * r + 1] = (int64_t)(fx.n_match + fx.mism + fx.insb);
      }
      return (int)MPC_COV_OK;
    };
  });
  for (int k = 0; k < T; ++k)
    for (size_t s = 0; s < S; ++s)
      for (int j = 0; j < 7; ++j) stats[s * MPC_COV_STATS + j] += pstat[(size_t)k][s * 7 + j];
  if (T > 1)
    parallel(T, [&](int k) {
      const size_t a = n_words * (size_t)k / T, b = n_words * (size_t)(k + 1) / T;
      for (int j = 1; j < T; ++j) {
        const uint32_t* src = priv[(size_t)j].data();
        for (size_t i = a; i < b; ++i) rows[i] += src[i];
      }
    });
  for (size_t s = 0; s < S; ++s) {
    const uint32_t* row = rows + pos_off[s] * 4;
    uint64_t* st = stats + s * MPC_COV_STATS;
    const int64_t lo = region[2 * s], hi = region[2 * s + 1];
    uint64_t mn = UINT64_MAX, mx = 0;
    for (int64_t i = lo; i < hi; ++i) {
      const uint64_t d = row[i * 4];
      st[7] += d;
      st[8] += d * d;
      mn = std::min(mn, d);
      mx = std::max(mx, d);
      st[11] += d < min_depth;
      st[12] += row[i * 4 + 1];
    }
    st[9] = hi > lo ? mn : 0;
    st[10] = mx;
  }
  return kOk;
}

void mpc_coverage_ingest_free(mpc_coverage_paf* o) {
  if (!o) return;
  delete static_cast<Holder*>(o->owner);
  const int32_t status = o->status;
  char msg[sizeof(o->message)];
  memcpy(msg, o->message, sizeof(msg));
  memset(o, 0, sizeof(*o));
  o->status = status;
  memcpy(o->message, msg, sizeof(msg));
}

int mpc_coverage_ingest(const char* paf_path, int mode, int n_threads, mpc_coverage_paf* out) {
  if (!out) return 1;
  memset(out, 0, sizeof(*out));
  if (!paf_path) return ingest_fail(out, "no PAF path");
  if (mode != 0 && mode != 1) return ingest_fail(out, "mode is neither 0 (first alignment per read) nor 1 (all)");
  mpc_host::Mapped f;
  if (!f.open(paf_path, true)) return ingest_fail(out, std::string(paf_path) + ": cannot be read");
  const int T = mpc_host::clamp_threads(n_threads, (long long)(f.n / (1 << 16) + 1));

  // cuts at line starts (ascending: n k / T and line_start_at_or_after are both monotone)
  std::vector<size_t> cut((size_t)T + 1, f.n);
  for (int k = 0; k < T; ++k) cut[(size_t)k] = mpc_host::line_start_at_or_after(f.p, f.n, f.n * (size_t)k / T);
  std::vector<std::vector<Line>> part((size_t)T);
  std::vector<int64_t> bad_line((size_t)T, -1);  // local index of the first bad line
  std::vector<const char*> bad_why((size_t)T, nullptr);
  std::vector<int64_t> n_lines((size_t)T, 0);
  parallel(T, [&](int k) {
    size_t a = cut[(size_t)k];
    const size_t b = cut[(size_t)k + 1];
    auto& v = part[(size_t)k];
    int64_t n = 0;
    while (a < b) {
      const void* nl = memchr(f.p + a, '\n', b - a);
      const size_t e = nl ? (size_t)(static_cast<const char*>(nl) - f.p) : b;
      sv line(f.p + a, e - a);
      if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
      Line r;
      const char* why = parse_line(line, &r);
      if (why) {
        if (bad_line[(size_t)k] < 0) { bad_line[(size_t)k] = n; bad_why[(size_t)k] = why; }
      } else v.push_back(r);
      ++n;
      a = e + 1;
    }
    n_lines[(size_t)k] = n;
  });
  int64_t before = 0;
  for (int k = 0; k < T; ++k) {
    if (bad_line[(size_t)k] >= 0)
      return ingest_fail(out, std::string(paf_path) + ": line " + std::to_string(before + bad_line[(size_t)k] + 1) + ": " +
                                  bad_why[(size_t)k]);
    before += n_lines[(size_t)k];
  }
  out->n_lines = before;

  // first alignment per read name, targets in first-appearance order (in file order)
  Holder* h = new Holder;
  out->owner = h;
  std::unordered_set<sv> seen;
  std::unordered_map<sv, int32_t> tidx;
  std::vector<const Line*> kept;
  int64_t line_no = 0;
  size_t cs_bytes = 0;
  for (int k = 0; k < T; ++k)
    for (const Line& r : part[(size_t)k]) {
      ++line_no;
      auto it = tidx.find(r.target);
      if (it == tidx.end()) {
        it = tidx.emplace(r.target, (int32_t)h->target_len.size()).first;
        h->name_off.push_back((int64_t)h->names.size());
        h->names.append(r.target);
        h->target_len.push_back(r.tlen);
      } else if (h->target_len[(size_t)it->second] != r.tlen) {
        const std::string msg = std::string(paf_path) + ": line " + std::to_string(line_no) + ": target " +
                                std::string(r.target) + " has lengths " + std::to_string(h->target_len[(size_t)it->second]) +
                                " and " + std::to_string(r.tlen);
        mpc_coverage_ingest_free(out);
        return ingest_fail(out, msg);
      }
      if (mode == 0 && !seen.insert(r.name).second) continue;
      kept.push_back(&r);
      h->target.push_back(it->second);
      cs_bytes += r.cs.size();
    }
  h->name_off.push_back((int64_t)h->names.size());
  const size_t n = kept.size();
  h->tstart.resize(n); h->tend.resize(n); h->qlen.resize(n); h->mapq.resize(n); h->strand.resize(n);
  h->cs_off.resize(n + 1);
  h->cs.resize(cs_bytes + 8);
  size_t off = 0;
  for (size_t i = 0; i < n; ++i) {
    h->cs_off[i] = (int64_t)off;
    off += kept[i]->cs.size();
  }
  h->cs_off[n] = (int64_t)off;
  parallel(T, [&](int k) {
    const size_t a = n * (size_t)k / T, b = n * (size_t)(k + 1) / T;
    for (size_t i = a; i < b; ++i) {
      const Line& r = *kept[i];
      h->tstart[i] = r.tstart; h->tend[i] = r.tend; h->qlen[i] = r.qlen;
      h->mapq[i] = (int32_t)std::min<int64_t>(r.mapq, INT32_MAX);
      h->strand[i] = (uint8_t)r.strand;
      if (!r.cs.empty()) memcpy(h->cs.data() + h->cs_off[i], r.cs.data(), r.cs.size());
    }
  });
  out->n_records = (int64_t)n;
  out->n_targets = (int64_t)h->target_len.size();
  out->target = h->target.data(); out->tstart = h->tstart.data(); out->tend = h->tend.data();
  out->qlen = h->qlen.data(); out->mapq = h->mapq.data(); out->strand = h->strand.data();
  out->cs = h->cs.data(); out->cs_off = h->cs_off.data();
  out->target_names = h->names.data(); out->target_name_off = h->name_off.data(); out->target_len = h->target_len.data();
  return 0;
}

}  // extern "C"
