// Stand-alone driver of csrc/align.cpp (with csrc/verify.cpp for the host scan)
// for the sanitizer build (tests/test_align_sanitized.py): align_driver CASES
// CASES holds batches, one token per field:
//   T <target name> <target>
//   B <max_error> <budget>      (budget 0: the largest single read's need, so
//                                that the plan cuts the batch into many launches)
//   R <name> <read>             (any number)
//   E
// Per batch the driver runs what align.py runs -- reverse complements, host
// scan, plan, the launches' traces, render -- and prints
//   batch <k> launches <n>
//   read <r> scan <4> plan <5> [out <8> runs <n_runs values>]
//   paf <bytes of the lines>
//   <the lines>
// A refused plan prints "batch <k> error <message>".  Every array has its exact
// size: a read or write past an end is a report.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "mpc_align.h"

struct Batch {
  std::string tname, target;
  double max_error = 0.2;
  int64_t budget = 0;
  std::vector<std::string> names, reads;
};

static int run(const Batch& b, int k) {
  const int32_t R = (int32_t)b.reads.size();
  const int64_t n = (int64_t)b.target.size();
  std::vector<int64_t> plus((size_t)R), minus((size_t)R);
  std::vector<int32_t> lens((size_t)R);
  int64_t total = 0;
  for (int32_t r = 0; r < R; ++r) {
    lens[(size_t)r] = (int32_t)b.reads[(size_t)r].size();
    plus[(size_t)r] = n + total;
    total += lens[(size_t)r];
  }
  for (int32_t r = 0; r < R; ++r) minus[(size_t)r] = plus[(size_t)r] + total;
  std::vector<uint8_t> seq((size_t)(n + 2 * total));  // exact: no slack after the last reverse complement
  std::memcpy(seq.data(), b.target.data(), (size_t)n);
  std::vector<int64_t> rc((size_t)R * 3), pairs((size_t)R * 8);
  for (int32_t r = 0; r < R; ++r) {
    std::memcpy(seq.data() + plus[(size_t)r], b.reads[(size_t)r].data(), (size_t)lens[(size_t)r]);
    const int64_t row[3] = {plus[(size_t)r], lens[(size_t)r], minus[(size_t)r]};
    std::memcpy(&rc[(size_t)r * 3], row, sizeof(row));
    const int64_t pr[8] = {plus[(size_t)r], lens[(size_t)r], 0, n, minus[(size_t)r], lens[(size_t)r], 0, n};
    std::memcpy(&pairs[(size_t)r * 8], pr, sizeof(pr));
  }
  if (mpc_align_revcomp_host(seq.data(), (int64_t)seq.size(), rc.data(), R, 3) != 0) return 70;
  std::vector<int32_t> scan((size_t)R * 4);
  if (mpc_verify_scan_host(seq.data(), pairs.data(), 2 * R, scan.data(), 3) != 0) return 71;
  std::vector<int64_t> plan((size_t)R * 8);
  std::vector<int32_t> cuts((size_t)R + 1);
  int32_t nl = 0;
  int64_t budget = b.budget;
  if (budget == 0) {
    if (mpc_align_plan(scan.data(), lens.data(), R, b.max_error, (int64_t)1 << 40, plan.data(), cuts.data(), &nl) != 0) return 72;
    for (int32_t r = 0; r < R; ++r) budget = plan[(size_t)r * 8 + 5] > budget ? plan[(size_t)r * 8 + 5] : budget;
  }
  if (mpc_align_plan(scan.data(), lens.data(), R, b.max_error, budget, plan.data(), cuts.data(), &nl) != 0) {
    std::printf("batch %d error %s\n", k, mpc_align_last_error());
    return 0;
  }
  std::printf("batch %d launches %d\n", k, nl);
  std::vector<std::string> per((size_t)R);
  std::string paf;
  for (int32_t l = 0; l < nl; ++l) {
    std::vector<int32_t> idx;
    for (int32_t r = cuts[(size_t)l]; r < cuts[(size_t)l + 1]; ++r)
      if (plan[(size_t)r * 8 + 1]) idx.push_back(r);
    const int32_t J = (int32_t)idx.size();
    std::vector<int64_t> jobs((size_t)J * 8), name_off((size_t)J + 1, 0);
    std::vector<uint8_t> strand((size_t)J);
    std::string names;
    int64_t runs_cap = 0, cap = 0;
    for (int32_t j = 0; j < J; ++j) {
      const int64_t* p = &plan[(size_t)idx[(size_t)j] * 8];
      const int32_t r = idx[(size_t)j];
      const int64_t job[8] = {p[0] ? minus[(size_t)r] : plus[(size_t)r], lens[(size_t)r], 0, n, p[2], p[3], p[6], p[7]};
      std::memcpy(&jobs[(size_t)j * 8], job, sizeof(job));
      strand[(size_t)j] = (uint8_t)p[0];
      names += b.names[(size_t)r];
      name_off[(size_t)j + 1] = (int64_t)names.size();
      runs_cap = p[7] + p[4];  // exact: the last read's runs end the buffer
    }
    std::vector<int32_t> out((size_t)J * 8), runs((size_t)runs_cap);
    const int trc = mpc_align_trace_host(seq.data(), (int64_t)seq.size(), jobs.data(), J, out.data(), runs.data(), runs_cap, 3);
    if (trc != 0) {
      std::printf("batch %d trace error %d %s\n", k, trc, mpc_align_last_error());
      return 0;
    }
    for (int32_t j = 0; j < J; ++j) {
      const int32_t* o = &out[(size_t)j * 8];
      cap += (int64_t)b.names[(size_t)idx[(size_t)j]].size() + (int64_t)b.tname.size() + 140 + 3 * ((int64_t)o[3] + o[4] + o[5]) + 7 * (int64_t)o[6];
      std::string& s = per[(size_t)idx[(size_t)j]];
      s = " out";
      for (int c = 0; c < 8; ++c) s += " " + std::to_string(o[c]);
      s += " runs";
      for (int32_t x = 0; x < o[6]; ++x) s += " " + std::to_string(runs[(size_t)(jobs[(size_t)j * 8 + 7] + x)]);
    }
    std::vector<char> buf((size_t)cap);
    std::vector<int64_t> line_len((size_t)J);
    int64_t written = -1;
    if (mpc_align_render(seq.data(), (int64_t)seq.size(), jobs.data(), J, strand.data(), out.data(), runs.data(), runs_cap,
                         names.data(), name_off.data(), b.tname.c_str(), buf.data(), cap, line_len.data(), &written, 3) != 0) {
      std::printf("batch %d render error %s\n", k, mpc_align_last_error());
      return 0;
    }
    // a buffer one byte short is refused, with the size needed, and nothing is written past it
    if (written > 0) {
      std::vector<char> tight((size_t)written - 1);
      int64_t need = -1;
      if (mpc_align_render(seq.data(), (int64_t)seq.size(), jobs.data(), J, strand.data(), out.data(), runs.data(), runs_cap,
                           names.data(), name_off.data(), b.tname.c_str(), tight.data(), written - 1, line_len.data(),
                           &need, 2) == 0 || need != written)
        return 73;
    }
    paf.append(buf.data(), (size_t)written);
  }
  for (int32_t r = 0; r < R; ++r) {
    std::printf("read %d scan", r);
    for (int c = 0; c < 4; ++c) std::printf(" %d", scan[(size_t)r * 4 + c]);
    std::printf(" plan");
    for (int c = 0; c < 5; ++c) std::printf(" %" PRId64, plan[(size_t)r * 8 + c]);
    std::printf("%s\n", per[(size_t)r].c_str());
  }
  std::printf("paf %zu\n", paf.size());
  std::fwrite(paf.data(), 1, paf.size(), stdout);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 64;
  std::ifstream in(argv[1]);
  if (!in) return 65;
  std::string tok;
  Batch b;
  int k = 0;
  while (in >> tok) {
    if (tok == "T") {
      b = Batch();
      if (!(in >> b.tname >> b.target)) return 66;
    } else if (tok == "B") {
      if (!(in >> b.max_error >> b.budget)) return 66;
    } else if (tok == "R") {
      std::string name, read;
      if (!(in >> name >> read)) return 66;
      b.names.push_back(name);
      b.reads.push_back(read);
    } else if (tok == "E") {
      if (const int rc = run(b, k++)) return rc;
    } else {
      return 67;
    }
  }
  return 0;
}
