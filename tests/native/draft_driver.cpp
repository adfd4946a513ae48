// Stand-alone driver of csrc/draft.cpp (with csrc/align.cpp and csrc/verify.cpp
// for scan, plan and trace) for the sanitizer build
// (tests/test_draft_sanitized.py): draft_driver CASES
// CASES holds, one token per field:
//   T <target>  R <read> (any number)  E <budget>
//       one round on the host as draft.py runs it -- reverse complements, scan,
//       plan (max_error 0.3; budget 0: the largest single read's need, so that
//       the votes come in many launches), traces, votes, call -- printed as
//         round launches <n> voted <n>
//         w <row> <word> <value>          every non-zero tally word, in order
//         call <rc> info <8 values> draft <bytes or ->
//   C <draft> <k> then k times <row> <word> <value>
//       the call on injected tallies, printed as the "call" line above
// Every array has its exact size: a read or write past an end is a report.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "mpc_draft.h"

static void print_call(const std::vector<uint32_t>& tally, const std::string& draft) {
  const int64_t n = (int64_t)draft.size();
  int32_t info[8];
  // first with no room at all: the length needed comes back and nothing is written
  int rc = mpc_draft_call_host(tally.data(), (const uint8_t*)draft.data(), n, nullptr, 0, info);
  std::vector<uint8_t> fresh((size_t)(info[0] == MPC_DRAFT_CALLED ? info[1] : 0));
  if (info[0] == MPC_DRAFT_CALLED && info[1] > 0)
    rc = mpc_draft_call_host(tally.data(), (const uint8_t*)draft.data(), n, fresh.data(), (int64_t)fresh.size(), info);
  std::printf("call %d info", rc);
  for (int k = 0; k < 8; ++k) std::printf(" %d", info[k]);
  std::printf(" draft %s\n", fresh.empty() ? "-" : std::string(fresh.begin(), fresh.end()).c_str());
}

static int run_round(const std::string& target, const std::vector<std::string>& reads, int64_t budget) {
  const int32_t R = (int32_t)reads.size();
  const int64_t n = (int64_t)target.size();
  std::vector<int64_t> plus((size_t)R), minus((size_t)R);
  std::vector<int32_t> lens((size_t)R);
  int64_t total = 0;
  for (int32_t r = 0; r < R; ++r) {
    lens[(size_t)r] = (int32_t)reads[(size_t)r].size();
    plus[(size_t)r] = n + total;
    total += lens[(size_t)r];
  }
  for (int32_t r = 0; r < R; ++r) minus[(size_t)r] = plus[(size_t)r] + total;
  std::vector<uint8_t> seq((size_t)(n + 2 * total));  // exact: no slack after the last reverse complement
  std::memcpy(seq.data(), target.data(), (size_t)n);
  std::vector<int64_t> rc((size_t)R * 3), pairs((size_t)R * 8);
  for (int32_t r = 0; r < R; ++r) {
    std::memcpy(seq.data() + plus[(size_t)r], reads[(size_t)r].data(), (size_t)lens[(size_t)r]);
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
  if (budget == 0) {
    if (mpc_align_plan(scan.data(), lens.data(), R, 0.3, (int64_t)1 << 40, plan.data(), cuts.data(), &nl) != 0) return 72;
    for (int32_t r = 0; r < R; ++r) budget = plan[(size_t)r * 8 + 5] > budget ? plan[(size_t)r * 8 + 5] : budget;
  }
  if (mpc_align_plan(scan.data(), lens.data(), R, 0.3, budget, plan.data(), cuts.data(), &nl) != 0) return 72;
  std::vector<uint32_t> tally((size_t)(n + 1) * MPC_DRAFT_ROW, 0);  // exact: row n is the last
  int voted = 0;
  for (int32_t l = 0; l < nl; ++l) {
    std::vector<int64_t> jobs;
    int64_t runs_cap = 0;
    for (int32_t r = cuts[(size_t)l]; r < cuts[(size_t)l + 1]; ++r) {
      const int64_t* p = &plan[(size_t)r * 8];
      if (!p[1]) continue;
      const int64_t job[8] = {p[0] ? minus[(size_t)r] : plus[(size_t)r], lens[(size_t)r], 0, n, p[2], p[3], p[6], p[7]};
      jobs.insert(jobs.end(), job, job + 8);
      runs_cap = p[7] + p[4];  // exact: the last read's runs end the buffer
    }
    const int32_t J = (int32_t)(jobs.size() / 8);
    std::vector<int32_t> out((size_t)J * 8), runs((size_t)runs_cap), status((size_t)J, -1);
    if (mpc_align_trace_host(seq.data(), (int64_t)seq.size(), jobs.data(), J, out.data(), runs.data(), runs_cap, 3) != 0) return 73;
    // two threads' shares and the sum of their tallies, then one thread
    const int threads = l % 2 ? 1 : 2;
    const int vrc = mpc_draft_vote_host(seq.data(), (int64_t)seq.size(), jobs.data(), J, out.data(), runs.data(), runs_cap,
                                        tally.data(), n, status.data(), threads);
    if (vrc != 0) {
      std::printf("vote error %d %s\n", vrc, mpc_draft_last_error());
      return 0;
    }
    for (int32_t j = 0; j < J; ++j) voted += status[(size_t)j] == MPC_DRAFT_VOTED;
    if (l == 0 && J > 0) {
      // runs that end one column late are refused for that read alone, and a table with too many runs outright
      std::vector<uint32_t> spare(tally.size(), 0);
      std::vector<int32_t> wrong(out);
      wrong[1] += 1;
      if (wrong[1] <= jobs[5] &&
          (mpc_draft_vote_host(seq.data(), (int64_t)seq.size(), jobs.data(), J, wrong.data(), runs.data(), runs_cap, spare.data(),
                               n, status.data(), 2) != MPC_DRAFT_E_RUNS || status[0] != MPC_DRAFT_BAD_RUNS))
        return 74;
      wrong[6] = (int32_t)(2 * jobs[4] + 2);
      if (mpc_draft_vote_host(seq.data(), (int64_t)seq.size(), jobs.data(), J, wrong.data(), runs.data(), runs_cap, spare.data(), n,
                              status.data(), 2) != -1)
        return 75;
    }
  }
  std::printf("round launches %d voted %d\n", nl, voted);
  for (size_t w = 0; w < tally.size(); ++w)
    if (tally[w]) std::printf("w %zu %zu %u\n", w / MPC_DRAFT_ROW, w % MPC_DRAFT_ROW, tally[w]);
  print_call(tally, target);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 64;
  std::ifstream in(argv[1]);
  if (!in) return 65;
  std::string tok, target;
  std::vector<std::string> reads;
  while (in >> tok) {
    if (tok == "T") {
      reads.clear();
      if (!(in >> target)) return 66;
    } else if (tok == "R") {
      std::string read;
      if (!(in >> read)) return 66;
      reads.push_back(read);
    } else if (tok == "E") {
      int64_t budget;
      if (!(in >> budget)) return 66;
      if (const int rc = run_round(target, reads, budget)) return rc;
    } else if (tok == "C") {
      std::string draft;
      size_t k;
      if (!(in >> draft >> k)) return 66;
      std::vector<uint32_t> tally((draft.size() + 1) * MPC_DRAFT_ROW, 0);
      for (size_t x = 0; x < k; ++x) {
        size_t row, word;
        uint32_t v;
        if (!(in >> row >> word >> v) || row > draft.size() || word >= MPC_DRAFT_ROW) return 66;
        tally[row * MPC_DRAFT_ROW + word] = v;
      }
      print_call(tally, draft);
    } else {
      return 67;
    }
  }
  return 0;
}
