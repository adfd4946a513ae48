/*
 * mpc_align.h -- C-ABI of align_reads: exact alignment of full-length plasmid
 * reads to a one-record assembly, written as a cs-tagged PAF (the step the
 * reference Snakefile's rule final_alignment_paf runs minimap2 for).
 *
 * Definition (everything is integer, every output is exact; DESIGN.md
 * "align_reads")
 *   target     the assembly FASTA holds exactly one record; t has length n,
 *              1 <= n < 2^31; its name is the header up to the first whitespace
 *   reads      every FASTA record in file order; the name is the header up to
 *              the first whitespace; 1 <= m <= MPC_VERIFY_MAX_QUERY, reads
 *              outside that range are skipped and counted
 *   bytes      sequences hold ASCII letters only (anything else is refused:
 *              it would break the cs grammar)
 *   symbols    compared exactly as in mpc_verify.h: upper-cased, A C G T are
 *              codes 0-3, every other read byte is code 4, every other target
 *              byte is code 5 (a non-ACGT symbol matches nothing)
 *   strands    q+ = the read, q- = its reverse complement (A C G T complemented
 *              case-insensitively, the case kept; every other letter kept and
 *              only reversed).  For each, (d, end) is mpc_verify_scan's result
 *              with q as the query and t as the text.  The smaller d wins, a
 *              tie is '+'.
 *   mapped     iff d <= min(floor(max_error * m), MPC_ALIGN_MAX_EDITS); an
 *              unmapped read gets no PAF line
 *   script     the canonical traceback of mpc_verify.h from (m, end): diagonal
 *              first, then up, then left
 *   ops        verify's '=' is a match, 'X' a substitution '*', 'D' (a read
 *              base missing from the target) an INSERTION '+', 'I' (an extra
 *              target base) a DELETION '-'
 *   ends       every op before the first '=' and after the last '=' is
 *              dropped; a read with no '=' is unmapped.  a / b = dropped
 *              leading / trailing ops that consume read bases (X, D): the
 *              oriented query span is [a, m - b).  The target span [ts, te)
 *              runs from the traceback's start to its end, moved inward by the
 *              dropped ops that consume target bases (X, I).
 *   PAF line   tab separated, '\n' terminated: read name, m, qs, qe, strand,
 *              target name, n, ts, te, number of '=', number of ops in the
 *              kept span, 255, NM:i:<non-'=' ops in the kept span>, cs:Z:<cs>.
 *              '+': (qs, qe) = (a, m - b); '-': coordinates on the original
 *              read, (qs, qe) = (b, m - a).
 *   cs         short form: ":<run>" per '=' run, "*<target base><read base>"
 *              per substitution, "+<read bases>" per insertion run,
 *              "-<target bases>" per deletion run; bases lower-case, read
 *              bases from the oriented read.
 * The read is aligned globally: junk at a read end that lies over target
 * interior is aligned, not clipped.
 *
 * Tables
 *   job   int64[8] per read  {q_off, m, t_off, n, d, end, flag_off, run_off}:
 *         byte offsets of the ORIENTED query and of the target in the sequence
 *         blob, the scan's (d, end), the read's byte offset in the flag
 *         workspace (m rows of roundup(2 d + 1, 64) bytes) and the int32 index
 *         of its first run (capacity 2 d + 1 runs)
 *   out   int32[8] per read  {status, start, n_eq, n_x, n_i, n_d, n_runs, 0}
 *         (counts in verify's op letters = X I D)
 *   runs  int32, (length << 2 | op), op 0 '=' 1 'X' 2 'I' 3 'D', in traceback
 *         order (end -> start)
 *
 * The band: row i (1 <= i <= m) holds columns j = i + (end - m) - d + b,
 * 0 <= b < W = 2 d + 1; cells with j < 0 or j > n are infinite; the value at
 * (m, end) must be d, else the read's status is MPC_ALIGN_BAD_SCAN.
 *
 * mpc_align_revcomp, mpc_align_trace, mpc_align_cs_sizes and mpc_align_cs_write
 * live in libmpc.so (HIP, gfx950; errors
 * through mpc_last_error of mpc.h); everything else lives in libmpc_ingest.so
 * (host only; errors through mpc_align_last_error).  All return 0 or a
 * negative code (the MPC_E_* values of mpc.h).
 */
#ifndef MPC_ALIGN_H
#define MPC_ALIGN_H

#include <stddef.h>
#include <stdint.h>

#include "mpc_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_ALIGN_MAX_EDITS 4096 /* largest distance a read is mapped at */
#define MPC_ALIGN_DEFAULT_WORKSPACE ((int64_t)2 << 30)

#define MPC_ALIGN_OK 0
#define MPC_ALIGN_BAD_SCAN 1 /* the band's value at (m, end) is not d (or the traceback left the band) */
#define MPC_ALIGN_BAD_JOB 2  /* a job the host would have refused (the kernel touched nothing) */

#define MPC_ALIGN_E_SCAN (-5) /* mpc_align_trace[_host]: at least one read ended with MPC_ALIGN_BAD_SCAN */

/* ---- device (libmpc.so) ---------------------------------------------------- */

/* K_arevcomp: n_reads reverse complements in one launch on the caller's
 * stream.  d_tab[3 r ..] = {src_off, len, dst_off}, byte offsets into d_seq
 * (seq_bytes long); the table is read back and bounds-checked on the host
 * before the launch (one stream wait); a source may not overlap a destination. */
int mpc_align_revcomp(uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_tab, int32_t n_reads, void* stream);

/* K_atrace: band DP, traceback and run encoding of n_jobs reads in ONE launch
 * (one wave64 per read).  The job table is read back and validated on the host
 * before the launch: lengths, 0 <= d <= MPC_ALIGN_MAX_EDITS, 0 <= end <= n,
 * sequences inside d_seq, flag rows inside d_flags and in ascending, disjoint
 * order, runs inside d_runs.  After the launch the call waits for the stream,
 * reads the statuses and returns MPC_ALIGN_E_SCAN when any is not
 * MPC_ALIGN_OK; d_out and d_runs are valid either way. */
int mpc_align_trace(const uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_jobs, int32_t n_jobs, uint8_t* d_flags,
                    int64_t flags_bytes, int32_t* d_out, int32_t* d_runs, int64_t runs_cap, void* stream);

/* ---- the handoff to the pileup (reads_consensus; DESIGN.md "reads_consensus") --
 * What mpc_input (mpc.h) wants of a traced read, built from its job, out row
 * and runs without the PAF text in between.  With the end rule above (a / b
 * the dropped leading / trailing read bases, a_t / b_t the dropped leading /
 * trailing target bases):
 *   kept    0 for a read with no '=' run: no PAF line, no pileup read
 *   tstart  start + a_t;  tend = end - b_t
 *   cs      "Z:" followed by the cs string of the PAF line
 *   up      oriented read [0, a), upper-cased;  down  oriented read [m - b, m)
 * size row   int64[8] per read  {kept, cs_len, up_len, down_len, tstart, tend,
 *            n_eq, n_ops} (cs_len counts the "Z:"; all 0 when not kept)
 * place row  int64[3] per read  {cs_off, up_off, down_off}: where the read's
 *            bytes go in the three output buffers; ascending in job order,
 *            disjoint, inside the buffers (a read that is not kept owns none)
 * status     int32 per read: MPC_ALIGN_OK, or MPC_ALIGN_BAD_JOB for a read the
 *            kernel refused (nothing of it was written)
 */

/* K_acslen: the size rows of n_jobs traced reads (the device tensors of one
 * mpc_align_trace launch), one wave64 per read.  The job table and the out rows
 * are read back and checked on the host before the launch (the job rule, the
 * trace output inside its bounds); after it the call waits for the stream and
 * refuses, naming the read, a read whose runs do not walk exactly its m read
 * bases and its target span (its row: kept = -1). */
int mpc_align_cs_sizes(const int64_t* d_jobs, int32_t n_jobs, int64_t seq_bytes, const int32_t* d_out,
                       const int32_t* d_runs, int64_t runs_cap, int64_t* d_sizes, void* stream);

/* K_acswrite: cs, up and down of every kept read at its place, one wave64 per
 * read.  Jobs, out rows, size rows and places are read back and checked on the
 * host before the launch (places ascending, disjoint and inside cs_bytes /
 * up_bytes / down_bytes; run spans inside runs_cap).  The kernel measures the
 * read again and writes only when that gives the size row it was handed; after
 * the launch the call waits, reads d_status and refuses a read with a status.
 * No byte outside the reads' own slots is written. */
int mpc_align_cs_write(const uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_jobs, int32_t n_jobs,
                       const int32_t* d_out, const int32_t* d_runs, int64_t runs_cap, const int64_t* d_sizes,
                       const int64_t* d_place, uint8_t* d_cs, int64_t cs_bytes, uint8_t* d_up, int64_t up_bytes,
                       uint8_t* d_down, int64_t down_bytes, int32_t* d_status, void* stream);

/* ---- host (libmpc_ingest.so) ----------------------------------------------- */

/* The host twins of the two calls above, same tables, reads spread over
 * `threads` host threads: the checker of the kernels and the sanitizer target.
 * Both check every read first (job rule, trace output, the runs' walk; the
 * writer also that each size row is the one the runs give, and the places) and
 * write nothing when one is refused. */
int mpc_align_cs_sizes_host(const int64_t* jobs, int32_t n_jobs, int64_t seq_bytes, const int32_t* out,
                            const int32_t* runs, int64_t runs_cap, int64_t* sizes, int threads);
int mpc_align_cs_write_host(const uint8_t* seq, int64_t seq_bytes, const int64_t* jobs, int32_t n_jobs,
                            const int32_t* out, const int32_t* runs, int64_t runs_cap, const int64_t* sizes,
                            const int64_t* place, uint8_t* cs, int64_t cs_bytes, uint8_t* up, int64_t up_bytes,
                            uint8_t* down, int64_t down_bytes, int threads);

/* The reverse complements on the host (--device cpu), same table. */
int mpc_align_revcomp_host(uint8_t* seq, int64_t seq_bytes, const int64_t* tab, int32_t n_reads, int threads);

/* From the scan results of n_reads reads (scan[4 r ..] = {d+, end+, d-, end-},
 * lens[r] = m): plan[8 r ..] = {strand (0 '+', 1 '-'), mapped, d, end, W,
 * flag_bytes, flag_off, run_off} (the last three 0 for an unmapped read;
 * offsets restart at 0 in every launch), and the cut of the reads into
 * launches whose flag bytes fit workspace_bytes: launch k holds the mapped
 * reads among [cuts[k], cuts[k + 1]); cuts has room for n_reads + 1 entries.
 * A mapped read that alone needs more than workspace_bytes: MPC_E_ARG. */
int mpc_align_plan(const int32_t* scan, const int32_t* lens, int32_t n_reads, double max_error, int64_t workspace_bytes,
                   int64_t* plan, int32_t* cuts, int32_t* n_launches);

/* The outputs of mpc_align_trace from the scalar band DP, reads spread over
 * `threads` host threads (<= 0: the job's CPU share); flag_off is not used
 * (each thread keeps its own band). */
int mpc_align_trace_host(const uint8_t* seq, int64_t seq_bytes, const int64_t* jobs, int32_t n_jobs, int32_t* out,
                         int32_t* runs, int64_t runs_cap, int threads);

/* The PAF lines of n_jobs traced reads, in job order, into buf.  strand[r] is
 * 0 or 1; names holds the read names back to back, name_off[r], name_off[r + 1]
 * their ends; tname is NUL terminated.  line_len[r] = bytes written for read r
 * (0: no '=' op, no line).  *written = total bytes; a buf_cap too small is
 * MPC_E_ARG with *written = the bytes needed. */
int mpc_align_render(const uint8_t* seq, int64_t seq_bytes, const int64_t* jobs, int32_t n_jobs, const uint8_t* strand,
                     const int32_t* out, const int32_t* runs, int64_t runs_cap, const char* names,
                     const int64_t* name_off, const char* tname, char* buf, int64_t buf_cap, int64_t* line_len,
                     int64_t* written, int threads);

/* message of the last failed host call of this header on this thread */
const char* mpc_align_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPC_ALIGN_H */
