/*
 * mpc_coverage.h -- C-ABI of coverage_qc: per-position depth, deletion,
 * mismatch and insertion counts of every PAF target, straight from the target
 * span and the cs tag of each alignment (acceptance criterion 1 of the
 * reference README, "at least 100,000x mean coverage", without the SAM /
 * samtools / Qualimap arm of the reference pipeline).
 *
 * Definition (DESIGN.md "coverage_qc")
 *   record   (sample s, tstart, cs bytes); a sample is one PAF target of length
 *            L_s (PAF column 7)
 *   cs       short form: an optional leading "Z:", then tokens
 *              ':' 1-9 digits | '*' exactly 2 letters | '+' letters | '-' letters
 *            (letters [A-Za-z], '+' / '-' at least one).  Any other byte makes
 *            the record MALFORMED: '=' '~' whitespace '_' a sign, a tenth
 *            digit, an operator with an empty operand.
 *   walk     p = tstart, tokens in order:
 *              :N    p .. p+N-1 each one ALIGNED observation; p += N (N = 0 legal)
 *              *xy   p one ALIGNED and one MISMATCH observation; p += 1
 *              -seq  p .. p+len-1 each one DELETED observation, one deletion
 *                    event of len bases; p += len
 *              +seq  one INSERTION observation at p ("before reference base
 *                    p", 0 <= p <= L), one insertion event of len bases
 *            OUT OF RANGE: tstart < 0 or the final p > L_s.
 *   rows     u32[n_pos][4] = {depth (aligned), deleted, mismatch, insertion},
 *            n_pos = sum (L_s + 1), sample s from row pos_off[s]; row L_s of a
 *            sample can be non-zero only in `insertion`
 *   stats    u64[n_samples][16]; 0-6 over whole records, 7-12 over the sample's
 *            region [lo, hi) within [0, L_s):
 *              0 records   1 match bases   2 mismatch bases   3 insertion events
 *              4 inserted bases   5 deletion events   6 deleted bases
 *              7 sum depth   8 sum depth^2   9 min depth   10 max depth
 *              11 positions with depth < min_depth   12 sum deleted   13-15 0
 *            (9 and 10 are 0 for an empty region)
 *   status   i32[2] = {code, record}: 0 ok, 1 malformed, 2 out of range;
 *            record = the SMALLEST offending record index, code 1 wins when
 *            that record is both.  code != 0: rows and stats are unspecified.
 *
 * mpc_coverage_run / mpc_coverage_tile_bytes live in libmpc.so (HIP, gfx950;
 * errors through mpc_last_error of mpc.h); everything else lives in
 * libmpc_ingest.so (host only).  All return 0 or a negative code (the MPC_E_*
 * values of mpc.h) unless stated otherwise.
 */
#ifndef MPC_COVERAGE_H
#define MPC_COVERAGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_COV_STATS 16
#define MPC_COV_OK 0
#define MPC_COV_MALFORMED 1
#define MPC_COV_RANGE 2

/* K_covparse + K_covfinish on the caller's stream.  d_cs_off[n_records + 1]:
 * byte offsets into d_cs; d_rec_sample[r] in [0, n_samples); d_pos_off
 * [n_samples + 1] with pos_off[s + 1] - pos_off[s] = L_s + 1; d_region
 * [n_samples][2] = {lo, hi}, 0 <= lo <= hi <= L_s.  d_rows (n_pos x 4 u32, the
 * only scratch), d_stats (8-byte aligned) and d_status are cleared by the call.
 * pos_off and region are validated on the host before the launch: the call
 * reads those two tables back and waits for the stream once; the kernels are
 * only enqueued.  Limits: 0 <= n_records < 2^31, 1 <= n_samples, n_pos < 2^31. */
int mpc_coverage_run(const uint8_t* d_cs, const int64_t* d_cs_off, const int64_t* d_tstart,
                     const int32_t* d_rec_sample, int64_t n_records,
                     const int64_t* d_pos_off /*[S+1]*/, const int64_t* d_region /*[S][2]*/, int32_t n_samples,
                     uint32_t min_depth, uint32_t* d_rows, uint64_t* d_stats, int32_t* d_status, void* stream);

/* cs bytes K_covparse takes per tile (64 lanes x k bytes, one byte per lane
 * and 64-byte chunk): the boundaries its carried state crosses. */
int mpc_coverage_tile_bytes(void);

/* The same results from a plain scalar walk over the definition, one base at
 * a time, records spread over `threads` host threads (<= 0: the job's CPU
 * share): the CPU checker, the timing baseline and the path of --device cpu.
 * rec_out (may be NULL): [n_records][2] = {the walk's final p, match + mismatch
 * + inserted bases} of every record the walk finished. */
int mpc_coverage_host(const uint8_t* cs, const int64_t* cs_off, const int64_t* tstart, const int32_t* rec_sample,
                      int64_t n_records, const int64_t* pos_off, const int64_t* region, int32_t n_samples,
                      uint32_t min_depth, uint32_t* rows, uint64_t* stats, int32_t* status, int threads,
                      int64_t* rec_out);

/* One PAF file, memory-mapped, lines parsed on n_threads threads (<= 0: the
 * job's CPU share).  mode 0 keeps the first alignment per read name (what the
 * consensus is called from), mode 1 every line.  Targets are numbered in
 * first-appearance order.  Errors (status 1, message names the 1-based line):
 * fewer than 12 columns, no cs: field, an integer that is not plain digits, a
 * strand other than + or -, one target name with two lengths.  Outputs are
 * owned by the library: release them with mpc_coverage_ingest_free(). */
typedef struct {
  int64_t n_records;     /* kept lines */
  int64_t n_lines;       /* lines of the file */
  int64_t n_targets;
  int32_t* target;       /* [n_records] target index */
  int64_t* tstart;       /* [n_records] PAF column 8 */
  int64_t* tend;         /* [n_records] PAF column 9 */
  int64_t* qlen;         /* [n_records] PAF column 2 */
  int32_t* mapq;         /* [n_records] PAF column 12 */
  uint8_t* strand;       /* [n_records] '+' or '-' */
  uint8_t* cs;           /* the bytes after "cs:" of every kept line, concatenated */
  int64_t* cs_off;       /* [n_records + 1] */
  char* target_names;    /* concatenated, not NUL separated */
  int64_t* target_name_off; /* [n_targets + 1] */
  int64_t* target_len;   /* [n_targets] PAF column 7 */
  void* owner;
  int32_t status;        /* 0 ok, 1 error */
  char message[256];
} mpc_coverage_paf;
int mpc_coverage_ingest(const char* paf_path, int mode, int n_threads, mpc_coverage_paf* out);
void mpc_coverage_ingest_free(mpc_coverage_paf* out);

/* message of the last failed mpc_coverage_host on this thread */
const char* mpc_coverage_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPC_COVERAGE_H */
