// ingest.cpp -- native host ingest: Steps 1-3 of
// /root/reference/src/mapped_paf_read_parser.py behind include/mpc_ingest.h.
//
// The result is byte-identical to minion-plasmid-consensus_amd/ingest.py (the
// Python restatement the CLI falls back to):
//   Step 1 (:161-184)  every non-'>' line of the reference, rstrip()ed and
//                      upper-cased, concatenated
//   Step 2 (:192-245)  per PAF line: rstrip().split('\t'); int() of columns 1, 2,
//                      3, 7; minus strand flips (qs, qe) to (qlen-qe, qlen-qs);
//                      cs = first field starting with "cs:", without "cs:";
//                      the FIRST line of a read name wins
//   Step 3 (:253-277)  per reads-FASTA record named in the PAF: sequence lines
//                      rstrip()ed, upper-cased, joined; minus strand reverse-
//                      complemented (KeyError outside ACGTN); upstream = seq[:qs],
//                      downstream = seq[qe:] with Python slicing; a duplicate
//                      name is processed again and the last record wins
// Host-side only (g++ -pthread); the files are memory-mapped and parsed by
// all cores: PAF lines and FASTA records are independent, only the PAF dedup
// (file order) is sequential.
#include "mpc_ingest.h"
#include "host_file.h"
#include "host_threads.h"

#include <sys/mman.h>
#include <emmintrin.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <string_view>
#include <thread>
#include <memory>
#include <vector>

namespace {

using sv = std::string_view;

using mpc_host::line_start_at_or_after;
using mpc_host::Mapped;

// str.isspace() restricted to ASCII (what rstrip() removes)
inline bool py_space(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f); }
inline sv rstrip(sv s) {
  size_t e = s.size();
  while (e > 0 && py_space((unsigned char)s[e - 1])) --e;
  return s.substr(0, e);
}
inline char upper(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }

using mpc_host::host_threads;
using mpc_host::parallel;

// MPC_INGEST_TIMING=1: wall time of each ingest phase on stderr (a measurement
// aid; called from the launching thread only).  phase(nullptr) starts the clock.
void phase(const char* what) {
  static const bool on = getenv("MPC_INGEST_TIMING") != nullptr;
  static std::chrono::steady_clock::time_point prev;
  if (!on) return;
  const auto t = std::chrono::steady_clock::now();
  if (what) fprintf(stderr, "ingest %-16s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t - prev).count());
  prev = t;
}

// bytes Python decodes or translates in text mode: anything >= 0x80, '\r'
bool needs_python(const Mapped& f, int T) {
  std::atomic<bool> bad{false};
  parallel(T, [&](int k) {
    const size_t a = f.n * k / T, b = f.n * (k + 1) / T;
    for (size_t i = a; i < b && !bad.load(std::memory_order_relaxed);) {
      const size_t e = std::min(b, i + (size_t)(1 << 16));
      unsigned x = 0;
      for (; i < e; ++i) {
        const unsigned char c = (unsigned char)f.p[i];
        x |= (unsigned)(c >= 0x80) | (unsigned)(c == '\r');
      }
      if (x) bad = true;
    }
  });
  return bad.load();
}

// Byte classes of 64 bytes at p (n <= 64 valid), SSE2 (x86-64 baseline): bit i
// of nl = p[i] is '\n'; of odd = p[i] is outside "ACGTNacgtn\n"; of py = p[i]
// is a byte Python's text mode decodes or translates (>= 0x80, '\r')
struct ByteClasses {
  uint64_t nl, odd, py;
};
inline ByteClasses classify64(const char* p, size_t n) {
  alignas(16) char tail[64];
  if (n < 64) {
    memset(tail, '\n', sizeof(tail));  // padding: newlines, masked off below
    memcpy(tail, p, n);
    p = tail;
  }
  const __m128i df = _mm_set1_epi8((char)0xDF), nlv = _mm_set1_epi8('\n'), crv = _mm_set1_epi8('\r');
  const __m128i A = _mm_set1_epi8('A'), C = _mm_set1_epi8('C'), G = _mm_set1_epi8('G'), T = _mm_set1_epi8('T'),
                N = _mm_set1_epi8('N');
  ByteClasses m{0, 0, 0};
  for (int q = 0; q < 4; ++q) {
    const __m128i v = _mm_loadu_si128(reinterpret_cast<const __m128i*>(p + 16 * q));
    const __m128i u = _mm_and_si128(v, df);  // upper() on ASCII letters; maps no other byte onto A C G T N
    const __m128i nl = _mm_cmpeq_epi8(v, nlv);
    const __m128i base = _mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(u, A), _mm_cmpeq_epi8(u, C)),
                                      _mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(u, G), _mm_cmpeq_epi8(u, T)),
                                                   _mm_cmpeq_epi8(u, N)));
    m.nl |= (uint64_t)(uint32_t)_mm_movemask_epi8(nl) << (16 * q);
    m.odd |= (uint64_t)(~(uint32_t)_mm_movemask_epi8(_mm_or_si128(base, nl)) & 0xFFFFu) << (16 * q);
    m.py |= (uint64_t)(uint32_t)(_mm_movemask_epi8(v) | _mm_movemask_epi8(_mm_cmpeq_epi8(v, crv))) << (16 * q);
  }
  if (n < 64) {
    const uint64_t keep = ((uint64_t)1 << n) - 1;
    m.nl &= keep; m.odd &= keep; m.py &= keep;
  }
  return m;
}

// PAF byte classes of 64 bytes at p (n <= 64 valid): bit i of nl / tab = p[i]
// is '\n' / '\t'; of py as in classify64
struct PafClasses {
  uint64_t nl, tab, py;
};
inline PafClasses classify_paf64(const char* p, size_t n) {
  alignas(16) char tail[64];
  if (n < 64) {
    memset(tail, ' ', sizeof(tail));
    memcpy(tail, p, n);
    p = tail;
  }
  const __m128i nlv = _mm_set1_epi8('\n'), tbv = _mm_set1_epi8('\t'), crv = _mm_set1_epi8('\r');
  PafClasses m{0, 0, 0};
  for (int q = 0; q < 4; ++q) {
    const __m128i v = _mm_loadu_si128(reinterpret_cast<const __m128i*>(p + 16 * q));
    m.nl |= (uint64_t)(uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(v, nlv)) << (16 * q);
    m.tab |= (uint64_t)(uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(v, tbv)) << (16 * q);
    m.py |= (uint64_t)(uint32_t)(_mm_movemask_epi8(v) | _mm_movemask_epi8(_mm_cmpeq_epi8(v, crv))) << (16 * q);
  }
  return m;
}

// Policy: Python int() of a plain decimal field, [-]digits.  0 = ok, 1 = not an
// int for Python either (empty, stray chars), 2 = let Python decide (sign '+',
// spaces, '_', very long)
int plain_int(sv s, int64_t* out) {
  if (s.empty()) return 1;
  const bool neg = s[0] == '-';
  const sv d = s.substr(neg ? 1 : 0);
  if (d.empty()) return 1;
  if (d.size() > 18) return 2;
  int64_t v;
  const size_t k = mpc_host::leading_digits(d, &v);
  if (k < d.size()) return (d[k] == '+' || d[k] == '_' || py_space((unsigned char)d[k])) ? 2 : 1;
  *out = neg ? -v : v;
  return 0;
}

struct Fail {
  int code = MPC_INGEST_OK;  // OK / ERROR / FALLBACK
  size_t pos = SIZE_MAX;     // file position of the first failing line (errors are reported in file order)
  std::string msg;
  void set(int c, size_t p, std::string m) {
    if (c == MPC_INGEST_FALLBACK) {
      if (code != MPC_INGEST_FALLBACK) { code = c; pos = p; msg = std::move(m); }
    } else if (code == MPC_INGEST_OK || (code == MPC_INGEST_ERROR && p < pos)) {
      code = c; pos = p; msg = std::move(m);
    }
  }
  void merge(const Fail& o) {
    if (o.code != MPC_INGEST_OK) set(o.code, o.pos, o.msg);
  }
};

struct PafRec {
  sv name, cs;
  int64_t qs, qe, ts;
  bool minus;
};

// one PAF line (:197-234)
int parse_paf_line(sv line, PafRec* r, std::string* err) {
  const sv s = rstrip(line);
  sv f[8];
  int nf = 0;
  sv cs;
  bool have_cs = false;
  size_t b = 0;
  for (;;) {  // split('\t'): every field, the cs tag may be anywhere
    const size_t e = s.find('\t', b);
    const sv fld = s.substr(b, e == sv::npos ? sv::npos : e - b);
    if (nf < 8) f[nf] = fld;
    ++nf;
    if (!have_cs && fld.size() >= 3 && fld.compare(0, 3, "cs:") == 0) { cs = fld.substr(3); have_cs = true; }
    if (e == sv::npos) break;
    b = e + 1;
  }
  int64_t qlen = 0, qs = 0, qe = 0, ts = 0;
  const int idx[4] = {1, 2, 3, 7};
  int64_t* dst[4] = {&qlen, &qs, &qe, &ts};
  for (int k = 0; k < 4; ++k) {  // int(line[1]), int(line[2]), int(line[3]), int(line[7])
    if (idx[k] >= nf) { *err = "IndexError: list index out of range"; return MPC_INGEST_ERROR; }
    const int rc = plain_int(f[idx[k]], dst[k]);
    if (rc == 2) return MPC_INGEST_FALLBACK;
    if (rc == 1) { *err = "ValueError: invalid literal for int(): '" + std::string(f[idx[k]].substr(0, 40)) + "'"; return MPC_INGEST_ERROR; }
  }
  r->name = f[0];
  r->minus = f[4] == "-";
  if (r->minus) { const int64_t a = qlen - qe, c = qlen - qs; qs = a; qe = c; }  // :226-228
  if (!have_cs) { *err = "IndexError: no cs: tag"; return MPC_INGEST_ERROR; }
  r->cs = cs;
  r->qs = qs; r->qe = qe; r->ts = ts;
  return MPC_INGEST_OK;
}

// Python s[:k] / s[k:] bounds for a string of length L
inline int64_t py_cut(int64_t L, int64_t k) {
  if (k < 0) k += L;
  return k < 0 ? 0 : (k > L ? L : k);
}

// Read name -> record: open addressing, linear probing, built by all threads at
// once.  A slot holds (hash high 32 bits << 32 | record index); empty = ~0.
// Records of one name share the high bits, so keeping the MINIMUM slot value
// (a CAS loop) keeps the name's first record in file order (:237-243) whatever
// order the threads insert in.
struct NameTable {
  std::unique_ptr<std::atomic<uint64_t>[]> slot;
  uint64_t mask = 0;
  static uint64_t hash(sv name) { return (uint64_t)std::hash<sv>()(name); }
  void init(int64_t n, int T) {
    uint64_t cap = 1024;
    while (cap < (uint64_t)n * 2) cap <<= 1;
    slot.reset(new std::atomic<uint64_t>[cap]);
    mask = cap - 1;
    parallel(T, [&](int k) {
      for (uint64_t i = cap * (uint64_t)k / (uint64_t)T; i < cap * (uint64_t)(k + 1) / (uint64_t)T; ++i)
        slot[i].store(~(uint64_t)0, std::memory_order_relaxed);
    });
  }
  // name_of(index) -> the name of a record already inserted.  A slot value is
  // published with release and read with acquire, so the record it names
  // (written by the publishing thread before the insert) is visible to a
  // thread that compares names through it.
  template <class NameOf>
  void insert(uint32_t idx, sv name, uint64_t h, NameOf name_of) {
    const uint64_t v = (h >> 32) << 32 | idx;
    for (uint64_t p = h & mask;; p = (p + 1) & mask) {
      uint64_t cur = slot[p].load(std::memory_order_acquire);
      for (;;) {
        if (cur == ~(uint64_t)0) {
          if (slot[p].compare_exchange_weak(cur, v, std::memory_order_acq_rel, std::memory_order_acquire)) return;
          continue;  // cur reloaded
        }
        if ((cur >> 32) != (v >> 32) || name_of((uint32_t)cur) != name) break;  // another name: probe on
        while (v < cur && !slot[p].compare_exchange_weak(cur, v, std::memory_order_acq_rel, std::memory_order_acquire)) {}
        return;
      }
    }
  }
  // slot value of a name, ~0: absent
  template <class NameOf>
  uint64_t find(sv name, NameOf name_of) const {
    const uint64_t h = hash(name);
    for (uint64_t p = h & mask;; p = (p + 1) & mask) {
      const uint64_t cur = slot[p].load(std::memory_order_acquire);
      if (cur == ~(uint64_t)0) return cur;
      if ((cur >> 32) == (h >> 32) && name_of((uint32_t)cur) == name) return cur;
    }
  }
};

struct Flank {
  size_t pos = SIZE_MAX;  // file position of the record (duplicates: the last wins)
  std::string up, down;
};


// One (assembly, PAF) job of a launch.  Several jobs may share ONE reads FASTA
// (the sense and antisense consensus jobs of a sample, Snakefile:401-423): it
// is then scanned once for all of them (mpc_ingest_multi).
struct Job {
  Mapped fr, fp;
  std::string ref;
  std::vector<PafRec> keep;  // first line per read name, file order
  NameTable names;           // name -> index in keep
  std::vector<Flank> flanks;
  int64_t n_lines = 0;
  Fail fail;
  bool live = true;  // Steps 1-2 passed: take part in Step 3
  int64_t lookup(sv name) const {  // record of a read name, -1: not in this PAF
    const uint64_t v = names.find(name, [&](uint32_t i) { return keep[i].name; });
    return v == ~(uint64_t)0 ? -1 : (int64_t)(uint32_t)v;
  }
};

// Steps 1-2 of one job (the files are open and ASCII-checked)
void job_ref_paf(Job& J, int T) {
  // ---- Step 1: reference (:161-184) ----
  J.ref.reserve(J.fr.n);
  for (size_t a = 0; a < J.fr.n;) {
    const char* nl = static_cast<const char*>(memchr(J.fr.p + a, '\n', J.fr.n - a));
    const size_t e = nl ? (size_t)(nl - J.fr.p) : J.fr.n;
    const sv line(J.fr.p + a, e - a);
    if (line.empty() || line[0] != '>')
      for (char c : rstrip(line)) J.ref.push_back(upper(c));
    a = e + 1;
  }
  // ---- Step 2: PAF (:192-245), chunks of lines in parallel, dedup in file order ----
  const Mapped& fp = J.fp;
  std::vector<std::vector<PafRec>> recs(T);
  std::vector<Fail> fails(T);
  std::vector<int64_t> nlines(T, 0);
  // One classified pass (classify_paf64): line ends, the first 8 tab positions
  // and the first field starting "cs:" of every line, and the Python text-mode
  // bytes (the job falls back).  A line of >= 8 fields with a cs tag and plain
  // integers is read from those positions; any other line goes through
  // parse_paf_line for the reference's exact error.
  std::atomic<bool> py{false};
  parallel(T, [&](int k) {
    // [a, b) moved forward to line starts (a last line without '\n' counts)
    const size_t a = line_start_at_or_after(fp.p, fp.n, fp.n * k / T), b = line_start_at_or_after(fp.p, fp.n, fp.n * (k + 1) / T);
    size_t tabs[8];
    int ntab = 0;
    size_t cs0 = SIZE_MAX, cs1 = SIZE_MAX;  // the cs field's value [cs0, cs1) (cs1: the next tab)
    auto slow = [&](size_t x, size_t e) {
      PafRec r;
      std::string err;
      const int rc = parse_paf_line(sv(fp.p + x, e - x), &r, &err);
      if (rc == MPC_INGEST_OK) recs[k].push_back(r);
      else fails[k].set(rc, x, rc == MPC_INGEST_ERROR ? "PAF line: " + err : std::string("PAF integer field for Python"));
    };
    auto line_at = [&](size_t x, size_t e) {  // [x, e): the line without '\n'
      ++nlines[k];
      size_t re = e;  // rstrip()
      while (re > x && py_space((unsigned char)fp.p[re - 1])) --re;
      int nt = ntab < 8 ? ntab : 8;  // (fields 0-7 need the first 8 tabs only)
      while (nt > 0 && tabs[nt - 1] >= re) --nt;  // tabs in the stripped tail split nothing
      if (nt < 7 || cs0 == SIZE_MAX || cs0 > re) { slow(x, e); return; }  // < 8 fields or no cs: exact error
      auto fld = [&](int i) {
        const size_t f0 = i == 0 ? x : tabs[i - 1] + 1;
        const size_t f1 = i < nt ? tabs[i] : re;
        return sv(fp.p + f0, f1 - f0);
      };
      PafRec r;
      int64_t qlen = 0, qs = 0, qe = 0, ts = 0;
      if (plain_int(fld(1), &qlen) | plain_int(fld(2), &qs) | plain_int(fld(3), &qe) | plain_int(fld(7), &ts)) {
        slow(x, e);
        return;
      }
      r.name = fld(0);
      r.minus = fld(4) == "-";
      if (r.minus) { const int64_t u = qlen - qe, v = qlen - qs; qs = u; qe = v; }  // :226-228
      const size_t ce = cs1 < re ? cs1 : re;
      r.cs = sv(fp.p + cs0, ce - cs0);
      r.qs = qs; r.qe = qe; r.ts = ts;
      recs[k].push_back(r);
    };
    auto field_start = [&](size_t f) {  // a field starts at f: the first "cs:" one is the tag
      if (cs0 == SIZE_MAX && f + 3 <= fp.n && fp.p[f] == 'c' && fp.p[f + 1] == 's' && fp.p[f + 2] == ':') cs0 = f + 3;
    };
    size_t ls = a;
    if (a < b) field_start(a);
    for (size_t blk = a, nb = 0; blk < b; blk += 64, ++nb) {
      const PafClasses m = classify_paf64(fp.p + blk, std::min<size_t>(64, b - blk));
      if (m.py || ((nb & 1023) == 0 && py.load(std::memory_order_relaxed))) { py = true; return; }
      uint64_t ev = m.nl | m.tab;
      while (ev) {
        const int i = __builtin_ctzll(ev);
        ev &= ev - 1;
        const size_t pos = blk + (size_t)i;
        if ((m.tab >> i) & 1u) {
          if (ntab < 8) tabs[ntab] = pos;
          ++ntab;
          if (cs0 != SIZE_MAX && cs1 == SIZE_MAX && pos >= cs0) cs1 = pos;
          if (pos + 1 < b) field_start(pos + 1);
        } else {
          line_at(ls, pos);
          ls = pos + 1;
          ntab = 0;
          cs0 = cs1 = SIZE_MAX;
          if (ls < b) field_start(ls);
        }
      }
    }
    if (ls < b) line_at(ls, b);  // a last line without '\n'
  });
  if (py.load()) {
    J.fail.set(MPC_INGEST_FALLBACK, 0, "non-ASCII byte or carriage return: Python text-mode semantics");
    J.live = false;
    return;
  }
  for (auto& f : fails) J.fail.merge(f);
  if (J.fail.code != MPC_INGEST_OK) { J.live = false; return; }
  phase("  paf lines");
  size_t total = 0;
  for (int k = 0; k < T; ++k) { J.n_lines += nlines[k]; total += recs[k].size(); }
  if (total >= ((size_t)1 << 32) - 1) {
    J.fail.set(MPC_INGEST_ERROR, 0, "more than 2^32 - 2 PAF lines (unsupported)");
    J.live = false;
    return;
  }
  // first line per name wins (:237-243): every thread inserts its own lines into
  // one table (NameTable keeps the lowest line index per name), the winners are
  // marked from the table and compacted in file order, and the table is then
  // rewritten to hold indices into keep.
  std::vector<PafRec> all;
  all.resize(total);
  std::vector<size_t> base((size_t)T + 1, 0);
  for (int k = 0; k < T; ++k) base[(size_t)k + 1] = base[(size_t)k] + recs[(size_t)k].size();
  const int64_t NA = (int64_t)total;
  J.names.init(NA, T);
  auto name_all = [&](uint32_t i) { return all[i].name; };
  parallel(T, [&](int k) {
    std::copy(recs[(size_t)k].begin(), recs[(size_t)k].end(), all.begin() + (ptrdiff_t)base[(size_t)k]);
    std::vector<PafRec>().swap(recs[(size_t)k]);
    for (size_t i = base[(size_t)k]; i < base[(size_t)k + 1]; ++i)
      J.names.insert((uint32_t)i, all[i].name, NameTable::hash(all[i].name), name_all);
  });
  phase("  paf name table");
  const uint64_t cap = J.names.mask + 1;
  std::vector<uint8_t> first((size_t)NA, 0);
  parallel(T, [&](int k) {
    for (uint64_t p = cap * (uint64_t)k / (uint64_t)T; p < cap * (uint64_t)(k + 1) / (uint64_t)T; ++p) {
      const uint64_t v = J.names.slot[p].load(std::memory_order_relaxed);
      if (v != ~(uint64_t)0) first[(uint32_t)v] = 1;
    }
  });
  phase("  paf first");
  std::vector<uint32_t> kidx((size_t)NA);
  uint32_t nk = 0;
  for (int64_t i = 0; i < NA; ++i) { kidx[(size_t)i] = nk; nk += first[(size_t)i]; }
  J.keep.resize(nk);
  parallel(T, [&](int k) {
    for (int64_t i = NA * k / T; i < NA * (k + 1) / T; ++i)
      if (first[(size_t)i]) J.keep[kidx[(size_t)i]] = all[(size_t)i];
    for (uint64_t p = cap * (uint64_t)k / (uint64_t)T; p < cap * (uint64_t)(k + 1) / (uint64_t)T; ++p) {
      const uint64_t v = J.names.slot[p].load(std::memory_order_relaxed);
      if (v != ~(uint64_t)0) J.names.slot[p].store((v >> 32) << 32 | kidx[(uint32_t)v], std::memory_order_relaxed);
    }
  });
  phase("  paf keep");
  J.flanks.resize(J.keep.size());
}

// Step 3 (:253-277) for every live job, ONE pass over the reads FASTA: chunks of
// records in parallel.  A record's sequence is never materialized: its lines
// stay in the mapping as (start, rstripped length) spans and only the flank
// bytes are copied out (a 10 kb read has ~80 flank bytes).
// seq = "".join(line.rstrip().upper()) (:270), so seq[i] is upper() of the span
// byte at position i.  Each byte is classified once (classify64): the line
// ends, whether a line holds anything but bases (then, and only then, it is
// rstripped and checked byte by byte) and the bytes that need Python's text
// mode.  Returns true when the file holds such a byte (the caller falls back).
bool jobs_fasta(std::vector<Job>& jobs, const Mapped& fa, int T) {
  const int nj = (int)jobs.size();
  std::mutex locks[64];
  std::vector<std::vector<Fail>> ffails((size_t)nj, std::vector<Fail>((size_t)T));
  std::atomic<bool> py{false};
  auto rec_start = [&](size_t x) {  // first header line ('>' at a line start) at or after x
    size_t y = line_start_at_or_after(fa.p, fa.n, x);
    while (y < fa.n && fa.p[y] != '>') {
      const char* nl = static_cast<const char*>(memchr(fa.p + y, '\n', fa.n - y));
      y = nl ? (size_t)(nl - fa.p) + 1 : fa.n;
    }
    return y;
  };
  parallel(T, [&](int k) {
    const size_t a = k == 0 ? 0 : rec_start(fa.n * k / T), b = k == T - 1 ? fa.n : rec_start(fa.n * (k + 1) / T);
    std::vector<sv> spans;
    std::vector<int64_t> span_end;             // cumulative rstripped length after each span
    std::vector<int64_t> cur((size_t)nj, -1);  // record of the current name per job, -1: not in its PAF
    bool any = false;
    size_t cur_pos = 0;
    int valid = -1;  // every byte of the record in ACGTN after upper(): -1 not checked yet
    bool rec_odd = false;  // a sequence byte of the record (after rstrip) is outside ACGTN after upper()
    char bad_c = '?';
    // copy seq[i0, i1) (upper-cased) to dst, forward
    auto copy_fwd = [&](int64_t i0, int64_t i1, char* dst) {
      size_t j = std::upper_bound(span_end.begin(), span_end.end(), i0) - span_end.begin();
      for (int64_t i = i0; i < i1; ++j) {
        const int64_t s0 = span_end[j] - (int64_t)spans[j].size();
        const int64_t e = std::min(i1, span_end[j]);
        for (; i < e; ++i) *dst++ = upper(spans[j][(size_t)(i - s0)]);
      }
    };
    // "".join([BASE_COMPLIMENT[x.upper()] for x in seq[::-1]]) (:263) raises a
    // KeyError for any byte of the WHOLE sequence outside ACGTN (after upper();
    // for ASCII, (c & 0xDF) is upper() on letters and maps no other byte onto
    // A, C, G, T, N); the first offending byte in seq[::-1] order is reported
    auto is_base = [](char ch) {
      const unsigned u = (unsigned char)ch & 0xDFu;
      return u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'N';
    };
    auto check_rc = [&]() {
      if (valid >= 0) return;
      const bool bad = rec_odd;
      valid = bad ? 0 : 1;
      if (bad)
        for (auto it = spans.rbegin(); it != spans.rend() && bad_c == '?'; ++it)
          for (size_t i = it->size(); i-- > 0;)
            if (!is_base((*it)[i])) { bad_c = upper((*it)[i]); break; }
    };
    auto done = [&]() {  // :259-265 for the record just read, in every job whose PAF names it
      if (!any) return;
      const int64_t L = span_end.empty() ? 0 : span_end.back();
      for (int j = 0; j < nj; ++j) {
        const int64_t c = cur[(size_t)j];
        if (c < 0) continue;
        Job& J = jobs[(size_t)j];
        const PafRec& r = J.keep[(size_t)c];
        if (r.minus) {
          check_rc();
          if (!valid) {
            ffails[(size_t)j][(size_t)k].set(MPC_INGEST_ERROR, cur_pos,
                                             "KeyError: '" + std::string(1, bad_c) + "' (reverse complement of read " +
                                                 std::string(r.name.substr(0, 80)) + ")");
            continue;
          }
        }
        const int64_t u = py_cut(L, r.qs), d = py_cut(L, r.qe);
        std::string up((size_t)u, '\0'), down((size_t)(L - d), '\0');
        if (!r.minus) {
          copy_fwd(0, u, &up[0]);
          copy_fwd(d, L, &down[0]);
        } else {  // rc[i] = comp(seq[L-1-i]): rc[:u] from seq[L-u, L), rc[d:] from seq[0, L-d), both reversed
          auto comp_rev = [](std::string& s) {
            std::reverse(s.begin(), s.end());
            for (char& ch : s) ch = ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'G' ? 'C' : ch == 'C' ? 'G' : 'N';
          };
          copy_fwd(L - u, L, &up[0]);
          comp_rev(up);
          copy_fwd(0, L - d, &down[0]);
          comp_rev(down);
        }
        std::lock_guard<std::mutex> g(locks[(c + 17 * j) & 63]);
        Flank& fl = J.flanks[(size_t)c];
        if (fl.pos == SIZE_MAX || cur_pos > fl.pos) {  // a duplicate name: the last record wins
          fl.pos = cur_pos;
          fl.up = std::move(up);
          fl.down = std::move(down);
        }
      }
    };
    // one line [x, e) without its '\n'; odd: it holds a byte outside "ACGTNacgtn"
    auto line_at = [&](size_t x, size_t e, bool odd) {
      const sv line(fa.p + x, e - x);
      if (!line.empty() && line[0] == '>') {
        done();
        const sv name = rstrip(line).substr(1);  // whole header line (:267); "" is never processed (:260)
        any = false;
        for (int j = 0; j < nj; ++j) {
          cur[(size_t)j] = (name.empty() || !jobs[(size_t)j].live) ? -1 : jobs[(size_t)j].lookup(name);
          any |= cur[(size_t)j] >= 0;
        }
        cur_pos = x;
        valid = -1;
        rec_odd = false;
        bad_c = '?';
        spans.clear();
        span_end.clear();
      } else if (any) {
        const sv s = odd ? rstrip(line) : line;  // :270 (a line of bases only has nothing to strip)
        if (!s.empty()) {
          spans.push_back(s);
          span_end.push_back((span_end.empty() ? 0 : span_end.back()) + (int64_t)s.size());
          if (odd && !rec_odd)
            for (char ch : s)
              if (!is_base(ch)) { rec_odd = true; break; }
        }
      }
    };
    size_t ls = a;      // start of the current line
    bool lodd = false;  // the current line holds a non-base byte so far
    for (size_t blk = a, nb = 0; blk < b; blk += 64, ++nb) {
      const ByteClasses m = classify64(fa.p + blk, std::min<size_t>(64, b - blk));
      if (m.py || ((nb & 1023) == 0 && py.load(std::memory_order_relaxed))) { py = true; return; }
      uint64_t nl = m.nl, odd = m.odd;
      while (nl) {
        const int i = __builtin_ctzll(nl);
        line_at(ls, blk + (size_t)i, lodd || (odd & (((uint64_t)1 << i) - 1)) != 0);
        ls = blk + (size_t)i + 1;
        lodd = false;
        nl &= nl - 1;
        odd &= ~(((uint64_t)2 << i) - 1);  // bits <= i belong to finished lines
      }
      lodd |= odd != 0;
    }
    if (ls < b) line_at(ls, b, lodd);  // a last line without '\n'
    done();
  });
  if (py.load()) return true;
  for (int j = 0; j < nj; ++j)
    for (auto& f : ffails[(size_t)j]) jobs[(size_t)j].fail.merge(f);
  return false;
}

// Output buffers.  Large ones (a GB of cs at C3) are anonymous mappings on
// transparent huge pages: written once right after allocation, 4 KiB pages
// cost a fault each (the fresh-page writes took ~2x the copy) and a slow
// unmap.  A 64-byte header before the data records how to release it.
constexpr size_t kHuge = (size_t)2 << 20;
struct OutHeader {
  uint64_t magic;
  void* base;
  size_t len;
};
constexpr uint64_t kMagicMalloc = 0x6d70636d616c6c63ull, kMagicMap = 0x6d70636d6d617070ull;
void* out_alloc(size_t n) {
  if (n >= 2 * kHuge) {
    const size_t len = n + 64 + kHuge;
    void* m = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m != MAP_FAILED) {
      uint8_t* a = reinterpret_cast<uint8_t*>(((uintptr_t)m + kHuge - 1) & ~(uintptr_t)(kHuge - 1));
      madvise(a, len - (size_t)(a - (uint8_t*)m), MADV_HUGEPAGE);
      *reinterpret_cast<OutHeader*>(a) = OutHeader{kMagicMap, m, len};
      return a + 64;
    }
  }
  uint8_t* a = static_cast<uint8_t*>(malloc(n + 64));
  if (!a) return nullptr;
  *reinterpret_cast<OutHeader*>(a) = OutHeader{kMagicMalloc, a, n + 64};
  return a + 64;
}
// frees p; a mapping is appended to *maps instead (unmapped off the caller's clock)
void out_free(void* p, std::vector<std::pair<void*, size_t>>* maps) {
  if (!p) return;
  const OutHeader h = *reinterpret_cast<const OutHeader*>(static_cast<uint8_t*>(p) - 64);
  if (h.magic == kMagicMap) maps->emplace_back(h.base, h.len);
  else free(h.base);
}

// one job's result packed in PAF first-occurrence order (:292)
void job_pack(Job& J, int T, mpc_ingest_out* out) {
  const int64_t N = (int64_t)J.keep.size();
  size_t ncs = 0, nup = 0, ndn = 0;
  for (int64_t i = 0; i < N; ++i) {
    const PafRec& r = J.keep[(size_t)i];
    const Flank& f = J.flanks[(size_t)i];
    if (f.pos == SIZE_MAX) {  // paf[read_name]["upstream_seq"] -> KeyError (:303)
      J.fail.set(MPC_INGEST_ERROR, 0, "KeyError: 'upstream_seq' (read " + std::string(r.name.substr(0, 80)) +
                                          " not in the reads file)");
      return;
    }
    if (r.ts < MPC_TSTART_MIN || r.ts >= ((int64_t)1 << 31)) {  // negative: wrapped on the device (mpc.h)
      J.fail.set(MPC_INGEST_ERROR, 0, "target start out of range (unsupported)");
      return;
    }
    ncs += r.cs.size(); nup += f.up.size(); ndn += f.down.size();
  }
  auto alloc = [](size_t n) { return out_alloc(n); };
  out->ref = (uint8_t*)alloc(J.ref.size());
  memcpy(out->ref, J.ref.data(), J.ref.size());
  out->ref_len = (int64_t)J.ref.size();
  out->cs = (uint8_t*)alloc(ncs); out->up = (uint8_t*)alloc(nup); out->down = (uint8_t*)alloc(ndn);
  out->cs_off = (int64_t*)alloc(8 * (N + 1)); out->up_off = (int64_t*)alloc(8 * (N + 1));
  out->down_off = (int64_t*)alloc(8 * (N + 1));
  out->tstart = (int64_t*)alloc(8 * N); out->aligned = (int64_t*)alloc(8 * N);
  size_t oc = 0, ou = 0, od = 0;
  for (int64_t i = 0; i < N; ++i) {  // offsets (serial prefix), then the copies by read ranges on all threads
    const PafRec& r = J.keep[(size_t)i];
    out->cs_off[i] = (int64_t)oc; out->up_off[i] = (int64_t)ou; out->down_off[i] = (int64_t)od;
    oc += r.cs.size(); ou += J.flanks[(size_t)i].up.size(); od += J.flanks[(size_t)i].down.size();
    out->tstart[i] = r.ts;
    out->aligned[i] = r.qe - r.qs;
  }
  out->cs_off[N] = (int64_t)oc; out->up_off[N] = (int64_t)ou; out->down_off[N] = (int64_t)od;
  parallel(T, [&](int k) {
    // read range of thread k: equal shares of the cs bytes (the bulk of the copy)
    auto at = [&](size_t x) { return (int64_t)(std::lower_bound(out->cs_off, out->cs_off + N, (int64_t)x) - out->cs_off); };
    const int64_t i0 = at(oc * k / T), i1 = k == T - 1 ? N : at(oc * (k + 1) / T);
    for (int64_t i = i0; i < i1; ++i) {
      memcpy(out->cs + out->cs_off[i], J.keep[(size_t)i].cs.data(), J.keep[(size_t)i].cs.size());
      memcpy(out->up + out->up_off[i], J.flanks[(size_t)i].up.data(), J.flanks[(size_t)i].up.size());
      memcpy(out->down + out->down_off[i], J.flanks[(size_t)i].down.data(), J.flanks[(size_t)i].down.size());
    }
  });
  out->n_reads = N;
  out->n_alignments = J.n_lines;
}

// The mappings (GBs of page-cache pages: unmapping 10 GB costs ~0.2 s) and the
// name tables are released by a detached thread, off the caller's clock: the
// results are copies, nothing points into them any more.
void release_async(std::vector<Job>&& jobs, Mapped&& fa) {
  struct Held {
    std::vector<Job> jobs;
    Mapped fa;
  };
  Held* h = new Held{std::move(jobs), std::move(fa)};
  try {
    std::thread([h] { delete h; }).detach();
  } catch (...) {  // no thread: release here
    delete h;
  }
}

}  // namespace

extern "C" {

int mpc_ingest_version(void) { return 3; }  // 3: + mpc_ingest_multi; 2: + mpc_write_calls, mpc_py_float_repr, pseudopair

void mpc_ingest_free(mpc_ingest_out* o) {
  if (!o) return;
  std::vector<std::pair<void*, size_t>> maps;
  for (void* b : {(void*)o->ref, (void*)o->cs, (void*)o->cs_off, (void*)o->tstart, (void*)o->up, (void*)o->up_off,
                  (void*)o->down, (void*)o->down_off, (void*)o->aligned})
    out_free(b, &maps);
  if (!maps.empty()) {  // a GB of output pages: unmapped by a detached thread
    try {
      std::thread([maps] { for (const auto& m : maps) munmap(m.first, m.second); }).detach();
    } catch (...) {
      for (const auto& m : maps) munmap(m.first, m.second);
    }
  }
  o->ref = o->cs = o->up = o->down = nullptr;
  o->cs_off = o->tstart = o->up_off = o->down_off = o->aligned = nullptr;
}

int mpc_ingest_multi(int n_jobs, const char* const* ref_paths, const char* const* paf_paths, const char* reads_path,
                     int n_threads, mpc_ingest_out* outs) {
  if (n_jobs <= 0) return MPC_INGEST_OK;
  phase(nullptr);
  for (int j = 0; j < n_jobs; ++j) memset(&outs[j], 0, sizeof(outs[j]));
  auto finish = [&](mpc_ingest_out* out, int code, const std::string& msg) {
    out->status = code;
    snprintf(out->message, sizeof(out->message), "%s", msg.c_str());
    if (code != MPC_INGEST_OK) mpc_ingest_free(out);
  };
  auto finish_all = [&](int code, const std::string& msg) {
    for (int j = 0; j < n_jobs; ++j) finish(&outs[j], code, msg);
    return code;
  };
  const int T = std::max(1, std::min(n_threads > 0 ? n_threads : host_threads(), 64));
  std::vector<Job> jobs((size_t)n_jobs);
  // a job's own errors in the reference's order: its reference, then its PAF,
  // then the reads file (:161, :192, :253)
  for (int j = 0; j < n_jobs; ++j) {
    Job& J = jobs[(size_t)j];
    if (!J.fr.open(ref_paths[j])) J.fail.set(MPC_INGEST_ERROR, 0, std::string("cannot open ") + ref_paths[j]);
    else if (!J.fp.open(paf_paths[j])) J.fail.set(MPC_INGEST_ERROR, 0, std::string("cannot open ") + paf_paths[j]);
    if (J.fail.code != MPC_INGEST_OK) J.live = false;
  }
  Mapped fa;
  const bool fa_ok = fa.open(reads_path);
  phase("open");
  for (auto& J : jobs) {
    if (!J.live) continue;
    const bool py = needs_python(J.fr, T);  // (the PAF is checked in its parse pass)
    phase("  ascii ref");
    if (py) {
      J.fail.set(MPC_INGEST_FALLBACK, 0, "non-ASCII byte or carriage return: Python text-mode semantics");
      J.live = false;
      continue;
    }
    job_ref_paf(J, T);
    phase("ref+paf");
    if (J.live && !fa_ok) {
      J.fail.set(MPC_INGEST_ERROR, 0, std::string("cannot open ") + reads_path);
      J.live = false;
    }
  }
  // the reads file is checked for Python text-mode bytes in the same pass; such
  // a byte sends every job to Python, whatever else failed
  if (fa_ok && jobs_fasta(jobs, fa, T))
    return finish_all(MPC_INGEST_FALLBACK, "non-ASCII byte or carriage return: Python text-mode semantics");
  phase("reads fasta");
  for (int j = 0; j < n_jobs; ++j) {
    Job& J = jobs[(size_t)j];
    if (J.fail.code == MPC_INGEST_OK) job_pack(J, T, &outs[j]);
    finish(&outs[j], J.fail.code, J.fail.msg);
  }
  phase("pack");
  release_async(std::move(jobs), std::move(fa));
  phase("release");
  return outs[0].status;
}

int mpc_ingest(const char* ref_path, const char* paf_path, const char* reads_path, int n_threads,
               mpc_ingest_out* out) {
  return mpc_ingest_multi(1, &ref_path, &paf_path, reads_path, n_threads, out);
}

}  // extern "C"
