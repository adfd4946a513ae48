// align.cpp -- host half of align_reads (include/mpc_align.h):
//   mpc_align_revcomp_host  the minus-strand queries (--device cpu)
//   mpc_align_plan          strand, mapped or not, band sizes, launch cuts
//   mpc_align_trace_host    the band trace of mpc_bandtrace.h over a job table:
//                           the CPU checker of K_atrace, the timing baseline,
//                           --device cpu
//   mpc_align_render        end rule + PAF lines of a batch
//   mpc_align_cs_sizes_host, mpc_align_cs_write_host
//                           the pileup's inputs of a traced launch (the handoff):
//                           the CPU checker of K_acslen and K_acswrite
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "host_file.h"
#include "host_threads.h"
#include "mpc_align.h"
#include "mpc_bandtrace.h"

namespace {
using namespace mpc_band;
using mpc_host::clamp_threads;

constexpr int kOk = 0;  // MPC_OK of mpc.h

thread_local mpc_host::LastError g_aerr;

void put_int(std::string& s, int64_t v) { s += std::to_string(v); }

// One read's PAF line (empty: no '=' op).
void render_one(const uint8_t* q, const uint8_t* t, const int64_t* job, bool minus, const int32_t* o, const int32_t* runs,
                const char* name, size_t name_len, const char* tname, std::string& line) {
  const int64_t m = job[1], n = job[3], end = job[5];
  // runs are end -> start: the kept span between the outermost '=' runs (end_rule, mpc_bandtrace.h)
  EndRule e;
  if (!end_rule(runs, o[6], e)) return;
  const int64_t a_q = e.a_q, b_q = e.b_q, ts = o[1] + e.a_t, te = end - e.b_t, n_eq = e.n_eq, n_ops = e.n_ops;
  line.append(name, name_len);
  line += '\t'; put_int(line, m);
  line += '\t'; put_int(line, minus ? b_q : a_q);
  line += '\t'; put_int(line, minus ? m - a_q : m - b_q);
  line += '\t'; line += minus ? '-' : '+';
  line += '\t'; line += tname;
  line += '\t'; put_int(line, n);
  line += '\t'; put_int(line, ts);
  line += '\t'; put_int(line, te);
  line += '\t'; put_int(line, n_eq);
  line += '\t'; put_int(line, n_ops);
  line += "\t255\tNM:i:"; put_int(line, n_ops - n_eq);
  line += "\tcs:Z:";
  size_t at = line.size();
  line.resize(at + (size_t)e.cs_bytes);
  int64_t i = a_q, j = ts;
  for (int32_t k = e.last; k >= e.first; --k) {
    put_run_cs((uint8_t*)&line[at], runs[k], q, i, t, j);
    at += (size_t)run_cs_bytes(runs[k]);
    i += run_read_bases(runs[k]);
    j += run_target_bases(runs[k]);
  }
  line += '\n';
}

}  // namespace

extern "C" const char* mpc_align_last_error(void) { return g_aerr.msg.c_str(); }

extern "C" int mpc_align_revcomp_host(uint8_t* seq, int64_t seq_bytes, const int64_t* tab, int32_t n_reads, int threads) {
  if (n_reads < 0) return g_aerr.fail("mpc_align_revcomp_host: n_reads < 0");
  if (n_reads == 0) return kOk;
  if (!seq || !tab) return g_aerr.fail("mpc_align_revcomp_host: null pointer");
  for (int32_t r = 0; r < n_reads; ++r)
    if (const int bad = check_revcomp(tab + 3 * (int64_t)r, seq_bytes))
      return g_aerr.fail("mpc_align_revcomp_host: read " + std::to_string(r) + ": " + fault_text(bad));
  const int nt = clamp_threads(threads, n_reads);
  std::atomic<int32_t> next{0};
  mpc_host::parallel(nt, [&](int) {
    for (int32_t r; (r = next.fetch_add(64)) < n_reads;)
      for (int32_t k = r; k < std::min(n_reads, r + 64); ++k) {
        const int64_t src = tab[3 * (int64_t)k], len = tab[3 * (int64_t)k + 1], dst = tab[3 * (int64_t)k + 2];
        for (int64_t x = 0; x < len; ++x) seq[dst + x] = (uint8_t)complement(seq[src + len - 1 - x]);
      }
  });
  return kOk;
}

extern "C" int mpc_align_plan(const int32_t* scan, const int32_t* lens, int32_t n_reads, double max_error,
                              int64_t workspace_bytes, int64_t* plan, int32_t* cuts, int32_t* n_launches) {
  if (n_reads < 0) return g_aerr.fail("mpc_align_plan: n_reads < 0");
  if (!n_launches || !cuts || (n_reads > 0 && (!scan || !lens || !plan))) return g_aerr.fail("mpc_align_plan: null pointer");
  if (!(max_error >= 0.0) || workspace_bytes < 0) return g_aerr.fail("mpc_align_plan: max_error or workspace_bytes < 0");
  int32_t nl = 0;
  int64_t flag_off = 0, run_off = 0;
  bool open = false;  // the current launch holds a mapped read
  cuts[0] = 0;
  for (int32_t r = 0; r < n_reads; ++r) {
    const int32_t* s = scan + 4 * (int64_t)r;
    int64_t* p = plan + 8 * (int64_t)r;
    const int64_t m = lens[r];
    if (m < 1 || m > MPC_VERIFY_MAX_QUERY) return g_aerr.fail("mpc_align_plan: read " + std::to_string(r) + ": length outside [1, 65536]");
    if (s[0] < 0 || s[2] < 0 || s[1] < 0 || s[3] < 0) return g_aerr.fail("mpc_align_plan: read " + std::to_string(r) + ": negative scan result");
    const bool minus = s[2] < s[0];  // a tie is '+'
    const int64_t d = minus ? s[2] : s[0], end = minus ? s[3] : s[1];
    const double lim = std::floor(max_error * (double)m);
    const bool mapped = (double)d <= lim && d <= MPC_ALIGN_MAX_EDITS;
    p[0] = minus; p[1] = mapped; p[2] = d; p[3] = end; p[4] = 2 * d + 1;
    p[5] = p[6] = p[7] = 0;
    if (!mapped) continue;
    const int64_t need = m * row_pitch(d);
    if (need > workspace_bytes)
      return g_aerr.fail("mpc_align_plan: read " + std::to_string(r) + " needs " + std::to_string(need) +
                   " flag bytes, the workspace budget is " + std::to_string(workspace_bytes));
    if (open && flag_off + need > workspace_bytes) {  // close the launch before this read
      cuts[++nl] = r;
      flag_off = run_off = 0;
      open = false;
    }
    p[5] = need; p[6] = flag_off; p[7] = run_off;
    flag_off += need;
    run_off += 2 * d + 1;
    open = true;
  }
  cuts[++nl] = n_reads;
  if (n_reads == 0) nl = 0;
  *n_launches = nl;
  return kOk;
}

extern "C" int mpc_align_trace_host(const uint8_t* seq, int64_t seq_bytes, const int64_t* jobs, int32_t n_jobs,
                                    int32_t* out, int32_t* runs, int64_t runs_cap, int threads) {
  if (n_jobs < 0) return g_aerr.fail("mpc_align_trace_host: n_jobs < 0");
  if (n_jobs == 0) return kOk;
  if (!seq || !jobs || !out || !runs) return g_aerr.fail("mpc_align_trace_host: null pointer");
  for (int32_t r = 0; r < n_jobs; ++r)
    if (const int bad = check_job(jobs + 8 * (int64_t)r, seq_bytes, runs_cap))
      return g_aerr.fail("mpc_align_trace_host: read " + std::to_string(r) + ": " + fault_text(bad));
  const int nt = clamp_threads(threads, n_jobs);
  std::atomic<int32_t> next{0};
  std::atomic<int> oom{0};
  mpc_host::parallel(nt, [&](int) {
    Band s;
    for (int32_t r; (r = next.fetch_add(1)) < n_jobs;) {
      const int64_t* j = jobs + 8 * (int64_t)r;
      try {
        band_trace(seq + j[0], j[1], seq + j[2], j[3], j[4], j[5], out + 8 * (int64_t)r, runs + j[7], s);
      } catch (const std::bad_alloc&) {
        oom = 1;
        return;
      }
    }
  });
  if (oom) return g_aerr.fail("mpc_align_trace_host: out of memory for a band");
  for (int32_t r = 0; r < n_jobs; ++r)
    if (out[8 * (int64_t)r] != MPC_ALIGN_OK)
      return g_aerr.fail("mpc_align_trace_host: read " + std::to_string(r) + ": the band does not give the scan's distance at (m, end)",
                   MPC_ALIGN_E_SCAN);
  return kOk;
}

extern "C" int mpc_align_render(const uint8_t* seq, int64_t seq_bytes, const int64_t* jobs, int32_t n_jobs,
                                const uint8_t* strand, const int32_t* out, const int32_t* runs, int64_t runs_cap,
                                const char* names, const int64_t* name_off, const char* tname, char* buf, int64_t buf_cap,
                                int64_t* line_len, int64_t* written, int threads) {
  if (n_jobs < 0) return g_aerr.fail("mpc_align_render: n_jobs < 0");
  if (!written) return g_aerr.fail("mpc_align_render: null pointer");
  *written = 0;
  if (n_jobs == 0) return kOk;
  if (!seq || !jobs || !strand || !out || !runs || !names || !name_off || !tname || !line_len || (!buf && buf_cap > 0))
    return g_aerr.fail("mpc_align_render: null pointer");
  for (int32_t r = 0; r < n_jobs; ++r) {
    const int64_t* j = jobs + 8 * (int64_t)r;
    const int32_t* o = out + 8 * (int64_t)r;
    const char* bad = fault_text(check_job(j, seq_bytes, runs_cap));
    if (!bad && o[0] != MPC_ALIGN_OK) bad = "status is not MPC_ALIGN_OK";
    if (!bad && check_traced(j, o)) bad = "trace output outside its bounds";
    if (!bad && name_off[r + 1] < name_off[r]) bad = "name offsets descend";
    // the runs must walk exactly the read and the target span (they index both sequences)
    if (!bad) bad = fault_text(check_walk(j, o, runs + j[7]));
    if (bad) return g_aerr.fail("mpc_align_render: read " + std::to_string(r) + ": " + bad);
  }
  // contiguous shares of reads per thread, joined in order
  const int nt = clamp_threads(threads, n_jobs);
  std::vector<std::string> part((size_t)nt);
  mpc_host::parallel(nt, [&](int k) {
    const int32_t r0 = (int32_t)((int64_t)n_jobs * k / nt), r1 = (int32_t)((int64_t)n_jobs * (k + 1) / nt);
    std::string& s = part[(size_t)k];
    for (int32_t r = r0; r < r1; ++r) {
      const int64_t* j = jobs + 8 * (int64_t)r;
      const size_t before = s.size();
      render_one(seq + j[0], seq + j[2], j, strand[r] != 0, out + 8 * (int64_t)r, runs + j[7], names + name_off[r],
                 (size_t)(name_off[r + 1] - name_off[r]), tname, s);
      line_len[r] = (int64_t)(s.size() - before);
    }
  });
  int64_t total = 0;
  for (const std::string& s : part) total += (int64_t)s.size();
  *written = total;
  if (total > buf_cap) return g_aerr.fail("mpc_align_render: the buffer holds " + std::to_string(buf_cap) + " bytes, the lines need " + std::to_string(total));
  int64_t at = 0;
  for (const std::string& s : part) {
    std::memcpy(buf + at, s.data(), s.size());
    at += (int64_t)s.size();
  }
  return kOk;
}

// ---- the handoff to the pileup: the host twins of K_acslen and K_acswrite ------
namespace {

// the size row of one traced read (checked by check_traced and check_walk)
void size_row(const int64_t* j, const int32_t* o, const int32_t* runs, int64_t* z) {
  EndRule e;
  for (int k = 0; k < 8; ++k) z[k] = 0;
  if (!end_rule(runs, o[6], e)) return;
  z[0] = 1; z[1] = 2 + e.cs_bytes; z[2] = e.a_q; z[3] = e.b_q;
  z[4] = o[1] + e.a_t; z[5] = j[5] - e.b_t; z[6] = e.n_eq; z[7] = e.n_ops;
}

// 0, or why read r's job, trace row or runs are refused
int check_read(const int64_t* j, const int32_t* o, const int32_t* runs, int64_t seq_bytes, int64_t runs_cap) {
  if (const int bad = check_job(j, seq_bytes, runs_cap)) return bad;
  if (const int bad = check_traced(j, o)) return bad;
  return check_walk(j, o, runs + j[7]);
}

}  // namespace

extern "C" int mpc_align_cs_sizes_host(const int64_t* jobs, int32_t n_jobs, int64_t seq_bytes, const int32_t* out,
                                       const int32_t* runs, int64_t runs_cap, int64_t* sizes, int threads) {
  if (n_jobs < 0) return g_aerr.fail("mpc_align_cs_sizes_host: n_jobs < 0");
  if (n_jobs == 0) return kOk;
  if (!jobs || !out || !runs || !sizes) return g_aerr.fail("mpc_align_cs_sizes_host: null pointer");
  for (int32_t r = 0; r < n_jobs; ++r)
    if (const int bad = check_read(jobs + 8 * (int64_t)r, out + 8 * (int64_t)r, runs, seq_bytes, runs_cap))
      return g_aerr.fail("mpc_align_cs_sizes_host: read " + std::to_string(r) + ": " + fault_text(bad));
  const int nt = clamp_threads(threads, n_jobs);
  std::atomic<int32_t> next{0};
  mpc_host::parallel(nt, [&](int) {
    for (int32_t r; (r = next.fetch_add(64)) < n_jobs;)
      for (int32_t k = r; k < std::min(n_jobs, r + 64); ++k) {
        const int64_t* j = jobs + 8 * (int64_t)k;
        size_row(j, out + 8 * (int64_t)k, runs + j[7], sizes + 8 * (int64_t)k);
      }
  });
  return kOk;
}

extern "C" int mpc_align_cs_write_host(const uint8_t* seq, int64_t seq_bytes, const int64_t* jobs, int32_t n_jobs,
                                       const int32_t* out, const int32_t* runs, int64_t runs_cap, const int64_t* sizes,
                                       const int64_t* place, uint8_t* cs, int64_t cs_bytes, uint8_t* up, int64_t up_bytes,
                                       uint8_t* down, int64_t down_bytes, int threads) {
  const char* fn = "mpc_align_cs_write_host";
  if (n_jobs < 0) return g_aerr.fail(std::string(fn) + ": n_jobs < 0");
  if (n_jobs == 0) return kOk;
  if (!seq || !jobs || !out || !runs || !sizes || !place || cs_bytes < 0 || up_bytes < 0 || down_bytes < 0 ||
      (!cs && cs_bytes > 0) || (!up && up_bytes > 0) || (!down && down_bytes > 0))
    return g_aerr.fail(std::string(fn) + ": null pointer or negative size");
  const int64_t cap[3] = {cs_bytes, up_bytes, down_bytes};
  int64_t at[3] = {0, 0, 0};
  for (int32_t r = 0; r < n_jobs; ++r) {
    const int64_t* j = jobs + 8 * (int64_t)r;
    const int64_t* z = sizes + 8 * (int64_t)r;
    int bad = check_read(j, out + 8 * (int64_t)r, runs, seq_bytes, runs_cap);
    if (!bad) {
      int64_t own[8];
      size_row(j, out + 8 * (int64_t)r, runs + j[7], own);
      if (std::memcmp(own, z, sizeof(own)) != 0) bad = kSizes;
    }
    if (!bad) bad = check_place(j, z, place + 3 * (int64_t)r, cap, at);
    if (bad) return g_aerr.fail(std::string(fn) + ": read " + std::to_string(r) + ": " + fault_text(bad));
  }
  const int nt = clamp_threads(threads, n_jobs);
  std::atomic<int32_t> next{0};
  mpc_host::parallel(nt, [&](int) {
    for (int32_t r; (r = next.fetch_add(16)) < n_jobs;)
      for (int32_t k = r; k < std::min(n_jobs, r + 16); ++k) {
        const int64_t* j = jobs + 8 * (int64_t)k;
        const int64_t* z = sizes + 8 * (int64_t)k;
        const int64_t* p = place + 3 * (int64_t)k;
        if (!z[0]) continue;
        const uint8_t* q = seq + j[0];
        const uint8_t* t = seq + j[2];
        const int32_t* rn = runs + j[7];
        EndRule e;
        end_rule(rn, out[8 * (int64_t)k + 6], e);
        uint8_t* dst = cs + p[0];
        dst[0] = 'Z'; dst[1] = ':';
        int64_t b = 2, qi = z[2], tj = z[4];
        for (int32_t x = e.last; x >= e.first; --x) {
          put_run_cs(dst + b, rn[x], q, qi, t, tj);
          b += run_cs_bytes(rn[x]);
          qi += run_read_bases(rn[x]);
          tj += run_target_bases(rn[x]);
        }
        for (int64_t x = 0; x < z[2]; ++x) up[p[1] + x] = upper_ascii(q[x]);
        for (int64_t x = 0; x < z[3]; ++x) down[p[2] + x] = upper_ascii(q[j[1] - z[3] + x]);
      }
  });
  return kOk;
}
