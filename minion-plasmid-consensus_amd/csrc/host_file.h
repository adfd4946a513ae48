// host_file.h -- what the host parsers of libmpc_ingest.so share around their
// own grammars: the read-only file mapping, the cut of a text at line starts,
// the decimal digit loop, and the per-tool last-error message.  Host only.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <string_view>

namespace mpc_host {

// A file mapped read-only; an empty file maps nothing and reads as "".
struct Mapped {
  enum Step { kNone, kOpen, kStat, kNotRegular, kMmap };
  const char* p = "";
  size_t n = 0;
  void* m = nullptr;
  int fd = -1;
  Step failed = kNone;  // the step open() gave up at
  Mapped() = default;
  Mapped(const Mapped&) = delete;
  Mapped(Mapped&& o) noexcept : p(o.p), n(o.n), m(o.m), fd(o.fd), failed(o.failed) {
    o.p = ""; o.n = 0; o.m = nullptr; o.fd = -1;
  }
  ~Mapped() {
    if (m && m != MAP_FAILED) munmap(m, n);
    if (fd >= 0) close(fd);
  }
  bool fail(Step s) { failed = s; return false; }
  bool open(const char* path, bool regular_only = false) {
    fd = ::open(path, O_RDONLY);
    if (fd < 0) return fail(kOpen);
    struct stat st;
    if (fstat(fd, &st) != 0) return fail(kStat);
    if (regular_only && !S_ISREG(st.st_mode)) return fail(kNotRegular);
    n = (size_t)st.st_size;
    if (n == 0) return true;
    m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) return fail(kMmap);
    madvise(m, n, MADV_SEQUENTIAL);
    p = static_cast<const char*>(m);
    return true;
  }
};

// The first line start at or after byte x of the n bytes at p (a line = up to
// and including '\n'; 0 and n count as line starts).  Monotone in x.
inline size_t line_start_at_or_after(const char* p, size_t n, size_t x) {
  if (x == 0) return 0;
  if (x >= n) return n;
  const void* nl = memchr(p + x - 1, '\n', n - (x - 1));
  return nl ? (size_t)(static_cast<const char*>(nl) - p) + 1 : n;
}

// The decimal digits s starts with, at most 18 (they fit an int64_t): their
// value in *v, their count returned.  The plain_int of each parser states what
// it accepts around them.
inline size_t leading_digits(std::string_view s, int64_t* v) {
  size_t k = 0;
  int64_t x = 0;
  for (; k < s.size() && k < 18 && s[k] >= '0' && s[k] <= '9'; ++k) x = x * 10 + (s[k] - '0');
  *v = x;
  return k;
}

// The message a tool's mpc_*_last_error() returns: one thread_local instance per tool.
struct LastError {
  std::string msg;
  int fail(const std::string& m, int code = -1) {  // (-1: MPC_E_ARG of mpc.h)
    msg = m;
    return code;
  }
};

}  // namespace mpc_host
