// mpc_launch.h -- what the launchers of the five tool .hip files (mpc_verify,
// mpc_cov, mpc_link, mpc_align, mpc_draft) share on the host side of a launch: the error
// message of libmpc.so, the read-back of device tables the host checks before
// it launches, and the record grid of the two cs walks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "mpc.h"

// mpc_plan.cpp: sets the message mpc_last_error() returns
__attribute__((visibility("hidden"))) int mpc_fail_(int code, const char* msg);

namespace mpc_launch {

// "<fn>: <what>: <the HIP error>" as MPC_E_HIP
inline int hip_fail(const char* fn, const char* what, hipError_t e) {
  return mpc_fail_(MPC_E_HIP, (std::string(fn) + ": " + what + ": " + hipGetErrorString(e)).c_str());
}

template <class T>
struct DeviceTable {
  const T* d;
  size_t count;
};

// The device tables `parts`, one behind the other, into h: async copies on the
// stream, then ONE wait for it.  MPC_OK, or hip_fail(fn, what, .).
template <class T>
int read_back(hipStream_t st, std::initializer_list<DeviceTable<T>> parts, std::vector<T>& h, const char* fn,
              const char* what) {
  size_t total = 0;
  for (const auto& p : parts) total += p.count;
  h.resize(total);
  hipError_t e = hipSuccess;
  size_t at = 0;
  for (const auto& p : parts) {
    if (e == hipSuccess) e = hipMemcpyAsync(h.data() + at, p.d, p.count * sizeof(T), hipMemcpyDeviceToHost, st);
    at += p.count;
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e == hipSuccess ? MPC_OK : hip_fail(fn, what, e);
}

// Workgroups over contiguous cuts of per_wg records, `waves` records side by
// side in a workgroup, at most max_wgs workgroups, none empty (n_records >= 1).
struct RecordGrid {
  int64_t wgs, per_wg;
};
inline RecordGrid record_grid(int64_t n_records, int waves, int max_wgs) {
  int64_t wgs = (n_records + waves - 1) / waves;
  if (wgs > max_wgs) wgs = max_wgs;
  const int64_t per_wg = (n_records + wgs - 1) / wgs;
  return {(n_records + per_wg - 1) / per_wg, per_wg};
}

}  // namespace mpc_launch
