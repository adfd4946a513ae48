// host_threads.h -- default worker-thread count of the host-side libraries,
// and the fork-join they all use.
#pragma once
#include <sched.h>

#include <cstddef>
#include <cstdlib>
#include <thread>
#include <vector>

namespace mpc_host {
// OMP_NUM_THREADS when set (the GPU pool sets it to the job's CPU share), else
// the CPUs this process may run on.  Not hardware_concurrency() alone: that
// counts the whole machine, and a shared box gives a job a fraction of it.
inline int host_threads() {
  if (const char* e = getenv("OMP_NUM_THREADS")) {
    const int v = atoi(e);
    if (v > 0) return v;
  }
  cpu_set_t cs;
  if (sched_getaffinity(0, sizeof(cs), &cs) == 0 && CPU_COUNT(&cs) > 0) return CPU_COUNT(&cs);
  const unsigned hw = std::thread::hardware_concurrency();
  return hw ? (int)hw : 4;
}

// the threads asked for (<= 0: host_threads()), at most one per unit of work, at least 1
inline int clamp_threads(int threads, long long work) {
  const long long nt = threads > 0 ? threads : host_threads();
  return (int)(nt < work ? nt : work < 1 ? 1 : work);
}

// f(0) ... f(T - 1), one thread each (T <= 1: f(0) on the caller's), joined on return
template <class F>
void parallel(int T, F f) {
  if (T <= 1) { f(0); return; }
  std::vector<std::thread> th;
  th.reserve((size_t)T);
  for (int k = 0; k < T; ++k) th.emplace_back(f, k);
  for (auto& t : th) t.join();
}
}  // namespace mpc_host
