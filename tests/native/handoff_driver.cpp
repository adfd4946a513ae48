// Stand-alone driver of the handoff's host twins in csrc/align.cpp
// (mpc_align_cs_sizes_host, mpc_align_cs_write_host) for the sanitizer build
// (tests/test_handoff_sanitized.py): handoff_driver CASES
// CASES holds launches, one token per field:
//   L <seq bytes> <jobs> <runs>
//   <the blob in hex> <8 x jobs job values> <8 x jobs out values> <runs values>
// Per launch the driver sizes the reads, places them back to back, writes them
// into buffers of EXACTLY the bytes needed, and prints
//   launch <k> sizes <8 x jobs values>
//   cs <hex>  up <hex>  down <hex>          (one line each)
// Then it asks for the same launch with each buffer one byte short, which must
// be refused with nothing written.  Every array has its exact size: a read or
// write past an end is a report.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "mpc_align.h"

static void print_hex(const char* what, const std::vector<uint8_t>& b) {
  std::printf("%s ", what);
  for (uint8_t c : b) std::printf("%02x", c);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return 64;
  std::ifstream in(argv[1]);
  if (!in) return 65;
  std::string tok;
  for (int k = 0; in >> tok; ++k) {
    int64_t seq_bytes = 0, n_runs = 0;
    int32_t J = 0;
    std::string hex;
    if (tok != "L" || !(in >> seq_bytes >> J >> n_runs >> hex) || (int64_t)hex.size() != 2 * seq_bytes) return 66;
    std::vector<uint8_t> seq((size_t)seq_bytes);
    for (int64_t x = 0; x < seq_bytes; ++x) seq[(size_t)x] = (uint8_t)std::stoi(hex.substr((size_t)(2 * x), 2), nullptr, 16);
    std::vector<int64_t> jobs((size_t)J * 8), sizes((size_t)J * 8), place((size_t)J * 3);
    std::vector<int32_t> out((size_t)J * 8), runs((size_t)n_runs);
    for (auto& v : jobs) if (!(in >> v)) return 66;
    for (auto& v : out) if (!(in >> v)) return 66;
    for (auto& v : runs) if (!(in >> v)) return 66;
    if (mpc_align_cs_sizes_host(jobs.data(), J, seq_bytes, out.data(), runs.data(), n_runs, sizes.data(), 3) != 0) {
      std::printf("launch %d error %s\n", k, mpc_align_last_error());
      continue;
    }
    std::printf("launch %d sizes", k);
    for (int64_t v : sizes) std::printf(" %" PRId64, v);
    std::printf("\n");
    int64_t end[3] = {0, 0, 0};
    for (int32_t r = 0; r < J; ++r)
      for (int c = 0; c < 3; ++c) {
        place[(size_t)r * 3 + c] = end[c];
        end[c] += sizes[(size_t)r * 8 + 1 + c];
      }
    std::vector<uint8_t> cs((size_t)end[0], 0xA5), up((size_t)end[1], 0xA5), down((size_t)end[2], 0xA5);
    // one byte short, buffer by buffer: refused, and the (exact, shorter) buffers stay as they were
    for (int c = 0; c < 3; ++c) {
      if (end[c] == 0) continue;
      int64_t cap[3] = {end[0], end[1], end[2]};
      --cap[c];
      std::vector<uint8_t> a((size_t)cap[0], 0xA5), b((size_t)cap[1], 0xA5), d((size_t)cap[2], 0xA5);
      if (mpc_align_cs_write_host(seq.data(), seq_bytes, jobs.data(), J, out.data(), runs.data(), n_runs, sizes.data(),
                                  place.data(), a.data(), cap[0], b.data(), cap[1], d.data(), cap[2], 2) == 0)
        return 70;
      for (const auto* v : {&a, &b, &d})
        for (uint8_t x : *v)
          if (x != 0xA5) return 71;
    }
    if (mpc_align_cs_write_host(seq.data(), seq_bytes, jobs.data(), J, out.data(), runs.data(), n_runs, sizes.data(),
                                place.data(), cs.data(), end[0], up.data(), end[1], down.data(), end[2], 3) != 0) {
      std::printf("launch %d write error %s\n", k, mpc_align_last_error());
      continue;
    }
    print_hex("cs", cs);
    print_hex("up", up);
    print_hex("down", down);
  }
  return 0;
}
