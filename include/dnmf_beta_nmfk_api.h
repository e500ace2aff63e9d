/* dnmf_beta_nmfk_api.h -- the per-column statistic of a rank-estimation sweep under the beta-divergence (dnmf_beta_column_div*).  Part
 * of the C ABI of include/dnmf.h, which includes this file at its end: include dnmf.h, not this file (the error codes,
 * DNMF_TUNED_MAX_K and the workspace contract are there).  A header and a ctypes table (pydnmfk_amd/_lib.py: BETA_NMFK_SIGNATURES) of
 * their own: include/dnmf_beta_api.h and its table are pinned function by function by tests/test_beta_workspace_cpu.py; these entry
 * points are held to the same contract by tests/test_capi_beta_nmfk.py and tests/test_gpu_beta_nmfk.py. */
#ifndef DNMF_BETA_NMFK_API_H
#define DNMF_BETA_NMFK_API_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* div[c] = sum_i d_beta(a_ic | s_ic + eps) and pw[c] = sum_i a_ic^beta (float64, c < n; a^beta := 0 at a = 0, beta > 0) over this
 * rank's rows: dnmf_beta_divergence column by column, with the sum that makes it comparable across columns.  Both scale as lambda^beta
 * when a column is scaled by lambda, so div[c] / pw[c] -- formed by the caller after the sums have crossed the ranks -- is
 * scale-invariant for every beta.  At beta = 0 pw[c] is the row count and the ratio is dnmf_is_column_div's mean per entry; at beta = 2
 * it is half the square of the Frobenius per-column relative error (PyNMF.column_err, pyDNMF.py:221-239).  At beta = 1 the terms are
 * a log(a / s') - a + s' and a, at beta = 0 q - log q - 1 and 1.  No counterpart in the reference; it stands where column_err stands
 * in an NMFk sweep (pyDNMFk.py:248).  The structure of dnmf_is_column_div: S tiles in MFMA accumulators, fp32 over the 16 rows a lane
 * holds of a 32-row block, float64 from there on; every row chunk leaves a PAIR of float64 per column in `ws` (the slab of
 * dnmf_masked_column_err), an ending adds them in chunk order and STORES div and pw (nothing is accumulated into them, no atomics: two
 * calls are bit-identical).  -2 <= beta <= 4, 1 <= k <= DNMF_TUNED_MAX_K; any shape and leading dimensions.  A misaligned `ws` is
 * refused with DNMF_EWS as the first check, a beta outside the range (a NaN included) with DNMF_EINVAL next, then the rank, pointers
 * and shapes, then a short workspace (DNMF_EWS, the needed size in the text).  Nothing outside the slab, div[0..n) and pw[0..n) is
 * written.
 * `ws`: dnmf_beta_column_div_ws_bytes(m, n, k) bytes, 16-byte aligned (0: bad shape or rank). */
size_t dnmf_beta_column_div_ws_bytes(long m, long n, int k);
/* Its launch plan, host arithmetic only: out = {rowblks_per_chunk, nchunks, ncolblk} with the values of dnmf_is_column_div_plan; the
 * slab takes nchunks * 2 * ncolblk * 128 doubles (a pair per chunk and column). */
int dnmf_beta_column_div_plan(long m, long n, int k, long out[3]);
int dnmf_beta_column_div(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                         float beta, double* div, double* pw, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DNMF_BETA_NMFK_API_H */
