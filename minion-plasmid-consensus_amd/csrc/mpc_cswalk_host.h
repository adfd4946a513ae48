// mpc_cswalk_host.h -- the one host walk of the short-form cs grammar of
// include/mpc_coverage.h, shared by coverage.cpp and linkage.cpp: the scalar
// counterpart of mpc_cswalk.h, one token at a time, straight from the
// definition.  Plain C++17, no HIP.
//
// What a token DOES is the effects policy Fx; each call is made only while the
// walk is inside the target, with the token's position p:
//   match(p, n)      :N       n bases [p, p + n) aligned and equal
//   mismatch(p, y)   *xy      base p aligned, read base y
//   deletion(p, n)   -letters n bases [p, p + n) deleted
//   insertion(p, n)  +letters n read bases inserted before base p
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_threads.h"
#include "mpc_coverage.h"

namespace mpc_host {

inline bool is_letter(uint8_t c) { return (uint8_t)((c | 32) - 'a') < 26; }
inline bool is_digit(uint8_t c) { return (uint8_t)(c - '0') < 10; }

// One record on a target of L bases.  Returns MPC_COV_* and, unless malformed,
// the end position; malformed wins over out of range, so the grammar is
// followed to the end of the cs even once p has left the target.
template <class Fx>
int cs_walk(const uint8_t* q, int64_t len, int64_t ts, int64_t L, Fx& fx, int64_t* end) {
  if (len < 0) return MPC_COV_MALFORMED;
  if (len >= 2 && q[0] == 'Z' && q[1] == ':') { q += 2; len -= 2; }
  bool oor = ts < 0 || ts > L;
  int64_t p = ts, k = 0;
  while (k < len) {
    const uint8_t op = q[k++];
    const int64_t a = k;
    if (op == ':') {
      int64_t n = 0;
      while (k < len && is_digit(q[k])) {
        if (k - a == 9) return MPC_COV_MALFORMED;  // a tenth digit
        n = n * 10 + (q[k++] - '0');
      }
      if (k == a) return MPC_COV_MALFORMED;
      if (!oor && p + n <= L) { fx.match(p, n); p += n; }
      else oor = true;
    } else if (op == '*') {
      if (len - k < 2 || !is_letter(q[k]) || !is_letter(q[k + 1])) return MPC_COV_MALFORMED;
      k += 2;
      if (k < len && is_letter(q[k])) return MPC_COV_MALFORMED;
      if (!oor && p < L) { fx.mismatch(p, q[k - 1]); ++p; }
      else oor = true;
    } else if (op == '-' || op == '+') {
      while (k < len && is_letter(q[k])) ++k;
      const int64_t n = k - a;
      if (n == 0) return MPC_COV_MALFORMED;
      if (op == '-') {
        if (!oor && p + n <= L) { fx.deletion(p, n); p += n; }
        else oor = true;
      } else {
        if (!oor && p <= L) fx.insertion(p, n);
        else oor = true;
      }
    } else {
      return MPC_COV_MALFORMED;
    }
  }
  *end = p;
  return oor ? MPC_COV_RANGE : MPC_COV_OK;
}

// Records [0, n_records) cut over T threads in record order.  make(k) sets up
// thread k and returns its record function r -> MPC_COV_*; status[0..1] takes
// the code and the index of the smallest record that is not MPC_COV_OK (the
// caller has cleared it).
template <class Make>
void walk_records(int64_t n_records, int T, int32_t* status, Make make) {
  std::vector<int64_t> first_bad((size_t)T, INT64_MAX);
  std::vector<int> first_code((size_t)T, 0);
  parallel(T, [&](int k) {
    auto record = make(k);
    const int64_t a = n_records * k / T, b = n_records * (k + 1) / T;
    for (int64_t r = a; r < b; ++r) {
      const int code = record(r);
      if (code != MPC_COV_OK && first_bad[(size_t)k] == INT64_MAX) {
        first_bad[(size_t)k] = r;
        first_code[(size_t)k] = code;
      }
    }
  });
  for (int k = 0; k < T; ++k)
    if (first_bad[(size_t)k] != INT64_MAX && status[0] == 0) {  // (cuts are in record order)
      status[0] = first_code[(size_t)k];
      status[1] = (int32_t)first_bad[(size_t)k];
    }
}

}  // namespace mpc_host
