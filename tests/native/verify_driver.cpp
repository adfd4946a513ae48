// Stand-alone driver of csrc/verify.cpp for the sanitizer build
// (tests/test_verify_cpu.py): verify_driver PAIRS THREADS
// PAIRS holds one "query<TAB>text" line per pair.  Prints, per pair,
// "distance end start n= nX nI nD cigar" from mpc_verify_scan_host (all pairs
// in one call) and mpc_verify_script.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "mpc_verify.h"

int main(int argc, char** argv) {
  if (argc != 3) return 64;
  std::ifstream in(argv[1]);
  if (!in) return 65;
  std::vector<uint8_t> seq;
  std::vector<int64_t> pairs;
  std::string line;
  while (std::getline(in, line)) {
    const size_t tab = line.find('\t');
    if (tab == std::string::npos) return 66;
    pairs.push_back((int64_t)seq.size());
    pairs.push_back((int64_t)tab);
    seq.insert(seq.end(), line.begin(), line.begin() + (long)tab);
    pairs.push_back((int64_t)seq.size());
    pairs.push_back((int64_t)(line.size() - tab - 1));
    seq.insert(seq.end(), line.begin() + (long)tab + 1, line.end());
  }
  const int32_t n = (int32_t)(pairs.size() / 4);
  std::vector<int32_t> out((size_t)n * 2, -7);
  seq.shrink_to_fit();  // (exact size: a read past the last sequence is a report)
  if (mpc_verify_scan_host(seq.data(), pairs.data(), n, out.data(), atoi(argv[2])) != 0) {
    fprintf(stderr, "%s\n", mpc_verify_last_error());
    return 1;
  }
  for (int32_t p = 0; p < n; ++p) {
    const int64_t* r = &pairs[(size_t)p * 4];
    int32_t start = 0, cnt[4];
    std::vector<char> cigar(1 << 16);
    if (mpc_verify_script(seq.data() + r[0], r[1], seq.data() + r[2], r[3], out[2 * p], out[2 * p + 1], &start, cnt,
                          cigar.data(), cigar.size()) != 0) {
      fprintf(stderr, "%s\n", mpc_verify_last_error());
      return 1;
    }
    printf("%d %d %d %d %d %d %d %s\n", out[2 * p], out[2 * p + 1], start, cnt[0], cnt[1], cnt[2], cnt[3], cigar.data());
  }
  return 0;
}
