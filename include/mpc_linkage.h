/*
 * mpc_linkage.h -- C-ABI of linkage_qc: the allele every alignment carries at
 * a set of variable sites, and how the alleles co-occur across alignments.  A
 * pileup is a sum over reads; whether the 5 % second peaks at a few positions
 * are independent errors or ONE sub-population (a second clone in the prep)
 * needs the per-read alleles.
 *
 * Definition (DESIGN.md "linkage_qc")
 *   records, cs grammar, walk and status are exactly mpc_coverage.h's: a record
 *            is (sample s, tstart, cs bytes), the cs short form with an optional
 *            "Z:"; a record can be MALFORMED or OUT OF RANGE; status = {code,
 *            smallest offending record}, malformed wins; with code != 0 the
 *            outputs are unspecified.
 *   sites    site_off[S + 1] groups the K sites by sample (a sample may have
 *            none); site_key[K] = 2p + 1 for the BASE site at reference base p
 *            (0 <= p < L_s), 2p for the GAP site "before base p" (0 <= p <= L_s);
 *            strictly increasing within a sample; 1 <= K <= MPC_LNK_MAX_SITES.
 *   allele   code of record r (sample s, walking tstart .. end e) at site k:
 *              0        not covered: a site of another sample; BASE p with
 *                       p < tstart or p >= e; GAP p with p < tstart or p > e
 *              1        reference: BASE p inside a :N run; GAP p passed with no
 *                       '+' token at walk position p
 *              2 3 4 5  BASE p hit by *xy with lower(y) = a c g t
 *              6        BASE p hit by *xy with any other letter y
 *              7        BASE p inside a '-' run; GAP p with one or more '+'
 *                       tokens at walk position p
 *            (inserted / deleted base identities and lengths are out of scope)
 *   alleles  u8[N][K], record-major
 *   pair     u32[K][K][8][8]: pair[i][j][a][b] = #{r : alleles[r][i] = a and
 *            alleles[r][j] = b}; written whole, mirrored half included; the
 *            diagonal [i][i][a][a] holds the per-site allele counts
 *   status   i32[2] as mpc_coverage.h
 *
 * mpc_linkage_run / _pairs / _tile_bytes / _scratch_bytes live in libmpc.so
 * (HIP, gfx950; errors through mpc_last_error of mpc.h); mpc_linkage_host /
 * _pairs_host live in libmpc_ingest.so (errors through
 * mpc_linkage_last_error).  All return 0 or a negative MPC_E_* code of mpc.h
 * unless stated otherwise.
 */
#ifndef MPC_LINKAGE_H
#define MPC_LINKAGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_LNK_MAX_SITES 128
#define MPC_LNK_CODES 8

/* K_lnkparse + K_lnkplanes + K_lnkpair on the caller's stream.  The record
 * tables are mpc_coverage_run's.  d_site_off[n_samples + 1], d_site_key
 * [n_sites] (both int64).  d_alleles: n_records x n_sites bytes, 4-byte
 * aligned; d_pair: n_sites^2 x 64 u32; d_scratch: mpc_linkage_scratch_bytes()
 * bytes, 8-byte aligned; all three and d_status are written whole by the call.
 * pos_off, site_off and site_key are validated on the host before the launch
 * (one read-back, one wait for the stream); when they are refused nothing is
 * written.  Limits: 0 <= n_records < 2^31, 1 <= n_samples, n_pos < 2^31. */
int mpc_linkage_run(const uint8_t* d_cs, const int64_t* d_cs_off, const int64_t* d_tstart,
                    const int32_t* d_rec_sample, int64_t n_records, const int64_t* d_pos_off /*[S+1]*/,
                    int32_t n_samples, const int64_t* d_site_off /*[S+1]*/, const int64_t* d_site_key /*[K]*/,
                    int32_t n_sites, uint8_t* d_alleles, uint32_t* d_pair, void* d_scratch, int32_t* d_status,
                    void* stream);

/* K_lnkplanes + K_lnkpair on a given allele matrix (codes are taken & 7). */
int mpc_linkage_pairs(const uint8_t* d_alleles, int64_t n_records, int32_t n_sites, uint32_t* d_pair,
                      void* d_scratch, void* stream);

/* cs bytes K_lnkparse takes per tile: the boundaries its carried state crosses */
int mpc_linkage_tile_bytes(void);

/* bytes of the caller-owned scratch buffer (the status key and the bit-planes
 * u64[ceil(N / 64)][K][8]); 0 when the arguments are outside the limits */
int64_t mpc_linkage_scratch_bytes(int64_t n_records, int32_t n_sites);

/* The same results from a plain scalar walk, records spread over `threads`
 * host threads (<= 0: the job's CPU share): the CPU checker of the kernels, the
 * timing baseline and the path of --device cpu. */
int mpc_linkage_host(const uint8_t* cs, const int64_t* cs_off, const int64_t* tstart, const int32_t* rec_sample,
                     int64_t n_records, const int64_t* pos_off, int32_t n_samples, const int64_t* site_off,
                     const int64_t* site_key, int32_t n_sites, uint8_t* alleles, uint32_t* pair, int32_t* status,
                     int threads);
int mpc_linkage_pairs_host(const uint8_t* alleles, int64_t n_records, int32_t n_sites, uint32_t* pair, int threads);

/* message of the last failed mpc_linkage_host / _pairs_host on this thread */
const char* mpc_linkage_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPC_LINKAGE_H */
