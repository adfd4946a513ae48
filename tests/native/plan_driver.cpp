// Stand-alone driver of csrc/mpc_plan.cpp for the sanitizer build
// (tests/test_plan_sanitized.py): plan_driver CASES
// CASES is what tests/plan_shapes.py write_case_file writes: per case a header
// line, the reference lengths, the read boundaries and, if given, the cs
// offsets.  Plans every case, prints what parse_driver_output reads back --
// "name rc" and either the message or the plan info, the workspace bytes, the
// parse tables as CRC-32 and (offset, count) of every MPC_BUF_* -- and
// destroys the plan.  Every array has its exact size: a read or write past an
// end is a report.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "mpc.h"

static uint32_t crc32(const void* data, size_t n) {  // zlib's polynomial, bitwise
  const uint8_t* b = static_cast<const uint8_t*>(data);
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    c ^= b[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

static bool read_array(std::ifstream& in, std::vector<int64_t>& v, size_t n) {
  v.assign(n, 0);
  v.shrink_to_fit();
  for (size_t k = 0; k < n; ++k)
    if (!(in >> v[k])) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 64;
  std::ifstream in(argv[1]);
  if (!in) return 65;
  if (mpc_version() != MPC_ABI_VERSION) return 66;
  std::vector<size_t> layout(MPC_INPUT_FIELDS);
  if (mpc_input_layout(layout.data(), MPC_INPUT_FIELDS) != sizeof(mpc_input)) return 67;
  std::string name;
  while (in >> name) {
    int null_mode = 0, has_off = 0, n_arr = 0;
    int64_t row_cap = 0, n_samples = 0, shard = 0, n_shards = 0, parse_cus = 0;
    mpc_input inp;
    memset(&inp, 0, sizeof(inp));
    if (!(in >> null_mode >> row_cap >> n_samples >> n_arr >> inp.n_reads >> inp.cs_bytes >> inp.read_offset >>
          inp.n_reads_global >> shard >> n_shards >> parse_cus >> inp.neg_reads >> inp.neg_cs_bytes >> has_off))
      return 68;
    std::vector<int64_t> ref_len, read_begin, cs_off;
    if (!read_array(in, ref_len, (size_t)n_arr) || !read_array(in, read_begin, (size_t)n_arr + 1)) return 69;
    if (has_off && !read_array(in, cs_off, (size_t)inp.n_reads + 1)) return 70;
    inp.n_samples = (int32_t)n_samples;
    inp.shard = (int32_t)shard;
    inp.n_shards = (int32_t)n_shards;
    inp.parse_cus = (int32_t)parse_cus;
    inp.h_ref_len = ref_len.data();
    inp.h_read_begin = read_begin.data();
    inp.h_cs_off = has_off ? cs_off.data() : nullptr;
    mpc_plan* plan = nullptr;
    const int rc = mpc_plan_create(null_mode == 1 ? nullptr : &inp, row_cap, null_mode == 2 ? nullptr : &plan);
    if (rc != MPC_OK) {
      printf("%s %d %s\n", name.c_str(), rc, mpc_last_error());
      continue;
    }
    mpc_plan_info info;
    size_t ws = 0;
    if (mpc_plan_get_info(plan, &info) != MPC_OK || mpc_plan_workspace_bytes(plan, &ws) != MPC_OK) return 71;
    const int n_wg = mpc_plan_parse_tables(plan, nullptr, nullptr);
    if (n_wg < 0) return 72;
    std::vector<int32_t> work((size_t)n_wg * 4), chunks((size_t)n_wg * (MPC_PARSE_CHUNKS + 1));
    work.shrink_to_fit();
    chunks.shrink_to_fit();
    if (mpc_plan_parse_tables(plan, work.data(), chunks.data()) != n_wg) return 73;
    printf("%s 0 %d %d %d %d %d %d %" PRId64 " %" PRId64 " %" PRId64 " %d %d %zu %d %u %u", name.c_str(), info.tally_mode,
           info.parse_window, info.parse_waves, info.parse_lds_bytes, info.parse_workgroups, info.overrides,
           info.max_reads_per_workgroup, info.reads_per_workgroup_cap, info.workspace_bytes, info.deferred_placement,
           info.reserved, ws, n_wg, crc32(work.data(), work.size() * 4), crc32(chunks.data(), chunks.size() * 4));
    for (int b = 0; b < MPC_BUF_COUNT; ++b) {
      size_t off = 0;
      int64_t count = 0;
      if (mpc_plan_buffer(plan, b, &off, &count) != MPC_OK) return 74;
      printf(" %zu %" PRId64, off, count);
    }
    printf("\n");
    size_t off = 0;
    int64_t count = 0;
    if (mpc_plan_buffer(plan, -1, &off, &count) != MPC_E_ARG || mpc_plan_buffer(plan, MPC_BUF_COUNT, &off, &count) != MPC_E_ARG)
      return 75;
    // the same shape again (a new batch), then a shape the plan does not hold
    inp.h_cs_off = nullptr;
    if (mpc_plan_set_input(plan, &inp) != MPC_OK) return 76;
    inp.n_reads += 1;
    if (mpc_plan_set_input(plan, &inp) != MPC_E_ARG) return 77;
    if (mpc_plan_destroy(plan) != MPC_OK) return 78;
  }
  return 0;
}
