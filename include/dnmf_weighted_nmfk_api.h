/* dnmf_weighted_nmfk_api.h -- the per-column statistic of a rank-estimation sweep under per-entry weights (dnmf_weighted_column_div*).
 * Part of the C ABI of include/dnmf.h, which includes this file at its end: include dnmf.h, not this file (the error codes,
 * DNMF_TUNED_MAX_K and the workspace contract are there).  A header and a ctypes table (pydnmfk_amd/_lib.py: WEIGHTED_NMFK_SIGNATURES)
 * of their own, the arrangement of include/dnmf_beta_nmfk_api.h: include/dnmf_weighted_api.h and its table stay as they are; these
 * entry points are held to the same contract by tests/test_weighted_nmfk_cpu.py and tests/test_gpu_weighted_nmfk.py. */
#ifndef DNMF_WEIGHTED_NMFK_API_H
#define DNMF_WEIGHTED_NMFK_API_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Two float64 sums per column c < n over this rank's rows, both over the positions with v > 0 ONLY (V of A's shape, leading dimension
 * ldv; norm 0 fro, 1 kl, 2 is, 3 beta with -2 <= beta <= 4, `beta` read under norm 3 alone), s = (W H)_ic, s' = s + eps:
 *   norm 0       num[c] = sum_i v (a - s)^2             den[c] = sum_i v a^2       (eps is not read)
 *   norm 1, 2, 3 num[c] = sum_i v d_beta(a | s')        den[c] = sum_i v a^beta    (a under kl; 1 under is: the column's weight sum;
 *                                                                                   a^beta := 0 at a = 0, beta > 0)
 * Under norm 3, beta = 0 and beta = 1 take the is and kl forms.  The caller forms sqrt(num / den) under norm 0 and num / den otherwise,
 * after the sums have crossed the ranks (PyNMF.weighted_column_divergence): both sums scale alike with a column's scale and with its
 * weights' scale, so the statistic is invariant under either.  A column without a positive weight yields den = 0.
 * The test v > 0 SELECTS the terms and never multiplies them: what A holds under a non-positive weight (NaN, inf, 0, a negative
 * number) changes nothing, and under 0/1 weights norm 0 is dnmf_masked_column_err on A with NaN where v = 0, bit for bit.
 * No counterpart in the reference; it stands where column_err stands in an NMFk sweep (pyDNMFk.py:248).  The structure of
 * dnmf_beta_column_div with V loaded beside A: S tiles in MFMA accumulators, fp32 over the 16 rows a lane holds of a 32-row block,
 * float64 from there on; every row chunk leaves a PAIR of float64 per column in `ws` (the slab of dnmf_masked_column_err), an ending
 * adds them in chunk order and STORES num and den (nothing is accumulated into them, no atomics: two calls are bit-identical).
 * 1 <= k <= DNMF_TUNED_MAX_K; any shape and leading dimensions.  A misaligned `ws` is refused with DNMF_EWS as the first check, an
 * unknown norm or a beta outside the range (a NaN included) with DNMF_EINVAL next, then the rank, pointers and shapes, then a short
 * workspace (DNMF_EWS, both sizes in the text).  Nothing outside the slab, num[0..n) and den[0..n) is written.
 * `ws`: dnmf_weighted_column_div_ws_bytes(m, n, k) bytes, 16-byte aligned (0: bad shape or rank). */
size_t dnmf_weighted_column_div_ws_bytes(long m, long n, int k);
/* Its launch plan, host arithmetic only: out = {rowblks_per_chunk, nchunks, ncolblk} with the values of dnmf_beta_column_div_plan; the
 * slab takes nchunks * 2 * ncolblk * 128 doubles (a pair per chunk and column). */
int dnmf_weighted_column_div_plan(long m, long n, int k, long out[3]);
int dnmf_weighted_column_div(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, const float* H,
                             long ldh, int k, float eps, int norm, float beta, double* num, double* den, void* ws, size_t ws_bytes,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DNMF_WEIGHTED_NMFK_API_H */
