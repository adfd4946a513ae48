/*
 * mpc_verify.h -- C-ABI of verify_consensus: exact, unbanded placement of an
 * expected sequence (the query q, length m) inside a consensus (the text t,
 * length n), the check the reference README asks for by hand ("Check the
 * results": align the consensus with the reference, every plasmid base must
 * match).
 *
 * Definition (Sellers, unit costs; DESIGN.md "verify_consensus")
 *   symbols   bytes are compared after ASCII upper-casing; A C G T are codes
 *             0-3, every other query byte is code 4, every other text byte is
 *             code 5: a non-ACGT symbol matches nothing, not even itself
 *   D[0][j] = 0, D[i][0] = i,
 *   D[i][j] = min(D[i-1][j-1] + (q[i] != t[j]), D[i-1][j] + 1, D[i][j-1] + 1)
 *   distance = min_j D[m][j];  end = the SMALLEST j attaining it
 *   script    traceback from (m, end): diagonal if j > 0 and D[i-1][j-1] + cost
 *             == D[i][j] ('=' on a match, 'X' otherwise), else up if D[i-1][j]
 *             + 1 == D[i][j] ('D': a query base missing from the text), else
 *             left ('I': an extra text base); it stops at i = 0, start = j
 *             there; the text span is [start, end), 0-based
 *
 * Limits: 1 <= m <= MPC_VERIFY_MAX_QUERY, 0 <= n < 2^31.
 *
 * mpc_verify_scan lives in libmpc.so (HIP, gfx950; errors through
 * mpc_last_error of mpc.h); mpc_verify_scan_host, mpc_verify_script and
 * mpc_verify_last_error live in libmpc_ingest.so (host only).  All return 0 or
 * a negative code (the MPC_E_* values of mpc.h).
 */
#ifndef MPC_VERIFY_H
#define MPC_VERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_VERIFY_MAX_QUERY 65536 /* longest query (64 lanes x 16 blocks x 64 rows) */
#define MPC_VERIFY_MAX_EDITS 1024  /* largest distance an edit script is produced for */

/* Score-only scan of n_pairs independent pairs in ONE launch on the caller's
 * stream (K_vscan: one wave64 per pair).  d_seq holds every query and text as
 * raw file bytes (upper-casing and the code mapping happen on the device);
 * d_pairs[4 p ..] = {q_off, q_len, t_off, t_len} of pair p, byte offsets into
 * d_seq; d_out[2 p ..] = {distance, end}.  The caller guarantees that every
 * [off, off + len) lies inside d_seq.  The lengths are validated on the host
 * before the launch: the call reads the pair table back (n_pairs x 32 bytes)
 * and waits for the stream once; the scan itself is only enqueued. */
int mpc_verify_scan(const uint8_t* d_seq, const int64_t* d_pairs, int32_t n_pairs, int32_t* d_out, void* stream);

/* The same results from a plain scalar DP over the definition, pairs spread
 * over `threads` host threads (<= 0: the job's CPU share): the CPU checker,
 * the timing baseline and the path of --device cpu. */
int mpc_verify_scan_host(const uint8_t* seq, const int64_t* pairs, int32_t n_pairs, int32_t* out, int threads);

/* The canonical edit script of one pair, given the scan's (distance, end):
 * a DP over the band of diagonals |(j - i) - (end - m)| <= distance, which
 * holds every optimal path (memory m x roundup(2 distance + 1, 64) bytes),
 * then the traceback above.  counts = number of '=', 'X', 'I', 'D' ops; cigar = their
 * run-length encoding from start to end (e.g. "1998=1X12=2D640="), NUL
 * terminated.  Fails (MPC_E_ARG) when the band's value at (m, end) is not
 * `distance` -- a cross-check of the scan -- or when cigar_cap is too small.
 * distance > MPC_VERIFY_MAX_EDITS: no script, cigar "*", *start and counts -1. */
int mpc_verify_script(const uint8_t* q, int64_t m, const uint8_t* t, int64_t n, int32_t distance, int32_t end,
                      int32_t* start, int32_t counts[4] /* = X I D */, char* cigar, size_t cigar_cap);

/* message of the last failed mpc_verify_scan_host / mpc_verify_script on this thread */
const char* mpc_verify_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPC_VERIFY_H */
