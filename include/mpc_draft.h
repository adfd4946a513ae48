/*
 * mpc_draft.h -- C-ABI of draft_assembly: the sense / antisense assembly the
 * reads are then aligned to, from the first reads of merged.fasta (the step
 * the reference Snakefile's rules subsample_fasta, canu_denovo_assembly,
 * select_top_assembly and revcomp_assembly run canu for).  Every read is a
 * full-length copy of one linearised plasmid on either strand, so the assembly
 * is: pick the most central read, align the sample to it, take a per-column
 * majority vote, repeat.  Scan, plan and trace are mpc_align.h's; this header
 * adds the vote and the call.
 *
 * Definition (everything is integer, every output is exact and independent of
 * launch cuts and of the order of the atomic adds; DESIGN.md "draft_assembly")
 *   sample     the first S records (default 500; 0: all) of the reads FASTA
 *              with 1 <= length <= MPC_VERIFY_MAX_QUERY, upper-cased; records
 *              outside that range are skipped and counted; FASTA rules and
 *              refusals as in mpc_align.h
 *   seed       a <= b the two middle values of the sorted sample lengths (a = b
 *              for an odd count); candidates: the C reads (default 8) with the
 *              smallest |2 len - (a + b)|, ties by file order.  Each candidate
 *              is scanned as the target of the whole sample (both strands,
 *              mpc_verify_scan); a read counts as mapped iff
 *              min(d+, d-) <= min(floor(max_error m), MPC_ALIGN_MAX_EDITS).
 *              The seed is the candidate with the smallest
 *              (-mapped, sum of d over the mapped reads, file index).
 *   round      the sample is aligned to the draft as align_reads does it (scan,
 *              mpc_align_plan, trace, launches under the workspace budget); the
 *              runs of every mapped read with status MPC_ALIGN_OK are voted,
 *              then the new draft is called.  At most `rounds` (default 3); a
 *              round that returns its draft unchanged ends the loop.
 *   vote       a read's runs are walked from the alignment's start to its end;
 *              the end rule is mpc_align.h's (ops before the first '=' and
 *              after the last '=' are dropped, a read with no '=' votes
 *              nothing).  Kept target span [ts, te); i = position in the
 *              ORIENTED read, j = target column.  Tallies are uint32, rows
 *              0 .. n of MPC_DRAFT_ROW words:
 *                [0] starts  [1] ends  [2] eq_on  [3] eq_off  [4] del_on
 *                [5] del_off  [8 + c] sub  [16 + 4 s + c] ins (s < 8); rest 0
 *              per read          starts[ts] += 1, ends[te] += 1
 *              '=' over [j, j+L) eq_on[j] += 1, eq_off[j + L] += 1 (difference
 *                                arrays: two adds whatever the length)
 *              'X' run           sub[j + x][code(q[i + x])] += 1 for codes 0-3
 *              'I' (an extra target base: a DELETION)
 *                                del_on[j] += 1, del_off[j + L] += 1
 *              'D' (a read base missing from the target: an INSERTION in front
 *              of column j)      ins[j][s][code(q[i + s])] += 1 for
 *                                s < min(L, MPC_DRAFT_SLOTS), codes 0-3
 *              codes as in mpc_verify.h (A C G T = 0-3 after upper-casing).
 *   call       cov, eq, del = prefix sums of (on - off) over rows 0 .. j;
 *              base[j][c] = sub[j][c] + (eq[j] if c is the code of the draft's
 *              byte at j, else 0); gcov[j] = cov[j] - starts[j];
 *              maxcov = max of cov over columns 0 .. n - 1; maxcov = 0 is an
 *              error ("no read mapped").  lo = first column with
 *              2 cov >= maxcov, hi = last such column + 1.  For j in [lo, hi):
 *                if j > lo, for s = 0 .. 7 in turn: emit the smallest code
 *                  holding max_c ins[j][s][c] while 2 sum_c ins[j][s][c] >
 *                  gcov[j]; stop at the first slot that fails
 *                the column: sum_c base[j][c] = 0: emit the draft's byte as it
 *                  is; else 2 del[j] > cov[j]: emit nothing; else M = max_c
 *                  base[j][c]: emit the draft's code if it holds M, otherwise
 *                  the smallest code that holds M
 *              Emitted codes are written as upper-case A C G T.  A new draft
 *              longer than MPC_DRAFT_MAX_LEN is an error.
 *   info       int32[8] {status, new length, lo, hi, maxcov, changed, dropped,
 *              inserted}: changed = voted columns kept with a code other than
 *              the draft's, dropped = voted columns that emit nothing,
 *              inserted = bases emitted from insertion slots.
 * The tallies must come from fewer than 2^30 voted reads (prefix sums are
 * 32-bit).
 *
 * Tables: job, out and runs are mpc_align.h's, as mpc_align_trace[_host] left
 * them; every job of a vote has the tallies' n as its target length.
 *   vote status  int32 per job: MPC_DRAFT_VOTED, MPC_DRAFT_BAD_RUNS (the runs do
 *                not walk exactly the read and [start, end): nothing of the read
 *                is added), MPC_DRAFT_NO_MATCH (no '=' run), MPC_DRAFT_NOT_TRACED
 *                (the out row's status is not MPC_ALIGN_OK)
 *
 * mpc_draft_vote and mpc_draft_call live in libmpc.so (HIP, gfx950; errors
 * through mpc_last_error of mpc.h), the _host twins in libmpc_ingest.so (errors
 * through mpc_draft_last_error).  All return 0 or a negative code.
 */
#ifndef MPC_DRAFT_H
#define MPC_DRAFT_H

#include <stddef.h>
#include <stdint.h>

#include "mpc_align.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_DRAFT_ROW 48        /* uint32 words of a tally row */
#define MPC_DRAFT_SLOTS 8       /* insertion slots in front of a column */
#define MPC_DRAFT_MAX_LEN 131072 /* longest draft voted on or called */

#define MPC_DRAFT_VOTED 0
#define MPC_DRAFT_BAD_RUNS 1
#define MPC_DRAFT_NO_MATCH 2
#define MPC_DRAFT_NOT_TRACED 3

#define MPC_DRAFT_CALLED 0
#define MPC_DRAFT_EMPTY 1 /* info status: maxcov = 0 */
#define MPC_DRAFT_LONG 2  /* info status: the new draft is longer than MPC_DRAFT_MAX_LEN */

#define MPC_DRAFT_E_RUNS (-6)  /* vote: at least one read ended with MPC_DRAFT_BAD_RUNS */
#define MPC_DRAFT_E_EMPTY (-7) /* call: no read mapped */
#define MPC_DRAFT_E_LONG (-8)  /* call: new draft longer than MPC_DRAFT_MAX_LEN */

/* ---- device (libmpc.so) ---------------------------------------------------- */

/* K_dvote: the votes of n_jobs traced reads in ONE launch (one wave64 per
 * read), added to d_tally ((n + 1) * MPC_DRAFT_ROW words, zeroed by the caller
 * before the first launch of a round).  d_jobs, d_out and d_runs are what
 * mpc_align_trace was given and left on the device.  The job and out tables are
 * read back and validated on the host before the launch: the job rule of
 * mpc_align_trace (without the flag rows), every target length = n,
 * 1 <= n <= MPC_DRAFT_MAX_LEN, and for a read with status MPC_ALIGN_OK
 * 0 <= n_runs <= 2 d + 1 and 0 <= start <= end.  After the launch the call
 * waits for the stream, reads d_status (n_jobs words) and returns
 * MPC_DRAFT_E_RUNS when any is MPC_DRAFT_BAD_RUNS. */
int mpc_draft_vote(const uint8_t* d_seq, int64_t seq_bytes, const int64_t* d_jobs, int32_t n_jobs, const int32_t* d_out,
                   const int32_t* d_runs, int64_t runs_cap, uint32_t* d_tally, int64_t n, int32_t* d_status, void* stream);

/* K_dcall: the new draft of d_draft (n bytes) from d_tally, into d_new (new_cap
 * bytes), and d_info (8 words); d_work: 3 (n + 1) words of scratch.  One
 * launch of one workgroup; the call waits for the stream, reads d_info and
 * returns MPC_DRAFT_E_EMPTY, MPC_DRAFT_E_LONG, or MPC_E_ARG when the new draft
 * does not fit new_cap (nothing is written past new_cap). */
int mpc_draft_call(const uint32_t* d_tally, const uint8_t* d_draft, int64_t n, uint8_t* d_new, int64_t new_cap,
                   int32_t* d_work, int32_t* d_info, void* stream);

/* ---- host (libmpc_ingest.so) ----------------------------------------------- */

/* The same votes on the host: reads spread over `threads` host threads (<= 0:
 * the job's CPU share), each with tallies of its own, summed at the end. */
int mpc_draft_vote_host(const uint8_t* seq, int64_t seq_bytes, const int64_t* jobs, int32_t n_jobs, const int32_t* out,
                        const int32_t* runs, int64_t runs_cap, uint32_t* tally, int64_t n, int32_t* status, int threads);

/* The same call on the host (info is filled whatever the result). */
int mpc_draft_call_host(const uint32_t* tally, const uint8_t* draft, int64_t n, uint8_t* new_draft, int64_t new_cap,
                        int32_t* info);

/* message of the last failed host call of this header on this thread */
const char* mpc_draft_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPC_DRAFT_H */
