/* dnmf_weighted_api.h -- the MU pair rules under per-entry weights (dnmf_weighted_*).  Part of the C ABI of include/dnmf.h, which
 * includes this file at its end: include dnmf.h, not this file (the error codes, DNMF_TUNED_MAX_K and the workspace contract are there).
 * The family has a header and a ctypes table (pydnmfk_amd/_lib.py: WEIGHTED_SIGNATURES) of its own. */
#ifndef DNMF_WEIGHTED_API_H
#define DNMF_WEIGHTED_API_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-entry weights on dense float32 data (csrc/dnmf_weighted.h) ----
 * No counterpart in the reference.  The objective is sum_ij v_ij d(a_ij | (W H)_ij) with V >= 0 of A's shape (leading dimension ldv,
 * given after lda) and d the norm's: `int norm` = 0 Frobenius, 1 Kullback-Leibler, 2 Itakura-Saito, 3 the beta-divergence of `float
 * beta` (read under norm 3 alone; -2 <= beta <= 4).  With (u_n, u_d) the norm's own pair (dnmf_masked_*, dnmf_is_*, dnmf_beta_*) and
 * F = H^T (W side) or W (H side):
 *     num = (V . u_n) F,   den = (V . u_d) F,   X <- X . rule(num / (den + eps))
 * with the norm's own rule: the weighted majorisation-minimisation step, which never increases the weighted objective.  v = 0 means
 * NOT OBSERVED: the test is v > 0, and where it fails `a` is not looked at (it may be NaN, inf, 0 or negative).  Where v > 0 the data
 * must be what the norm takes (callers check).  The launch geometry is the norm's own (dnmf_weighted_plan returns the numbers of
 * dnmf_masked_plan / dnmf_is_plan / dnmf_beta_plan), the partial sums are added in the same fixed order, no float atomics: with 0/1
 * weights the results are those of the unweighted entry points bit for bit (fro, kl: of dnmf_masked_* on A with NaN where v = 0).
 * 1 <= k <= DNMF_TUNED_MAX_K; any shape and any leading dimensions.  Bad arguments return DNMF_EINVAL with a dnmf_last_error text (a
 * norm outside 0..3 and, under norm 3, a beta outside the range included); the *_bytes functions return 0.
 * `ws`: dnmf_weighted_ws_bytes(m, n, k) bytes, 16-byte aligned, serves every entry point below but the whole fit, under every norm.  A
 * misaligned `ws` is refused with DNMF_EWS as the first check; one that is too small with DNMF_EWS and both sizes in the message. */
size_t dnmf_weighted_ws_bytes(long m, long n, int k);
/* The launch plans of `norm`, host arithmetic only: the eight numbers of dnmf_is_plan. */
int dnmf_weighted_plan(long m, long n, int k, int norm, long out[8]);
/* the pair stored, [m x k] (W side) or [k x n] (H side) with the same leading dimension ldo */
int dnmf_weighted_aht_pair(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, const float* H,
                           long ldh, int k, float eps, int norm, float beta, float* num, float* den, long ldo, void* ws, size_t ws_bytes,
                           void* stream);
int dnmf_weighted_wta_pair(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, const float* H,
                           long ldh, int k, float eps, int norm, float beta, float* num, float* den, long ldo, void* ws, size_t ws_bytes,
                           void* stream);
/* the pair applied where nothing crosses ranks: W in place after the pass has read it, H alike with max(., eps) if clamp != 0 */
int dnmf_weighted_update_w(const float* A, long m, long n, long lda, const float* V, long ldv, float* W, long ldw, const float* H, long ldh,
                           int k, float eps, int norm, float beta, void* ws, size_t ws_bytes, void* stream);
int dnmf_weighted_update_h(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, float* H, long ldh,
                           int k, float eps, int norm, float beta, int clamp, void* ws, size_t ws_bytes, void* stream);
/* sq (two doubles, device) = {sum v (a - s)^2, sum v a^2} over v > 0, s = W H: the squares of the weighted relative error's two norms.
 * S tiles in MFMA accumulators, fp32 per 32 x 128 tile and lane, float64 from there on, every tile's sums in their own slots of `ws`
 * and the slots added in a fixed order: two calls are bit-identical. */
int dnmf_weighted_resid_sqnorm(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, const float* H,
                               long ldh, int k, double* sq, void* ws, size_t ws_bytes, void* stream);
/* *out (double, device) = sum v d(a | s + eps) over v > 0 with d of the norm (1: a log(a / s') - a + s'; 2: q - log q - 1; 3: d_beta);
 * under norm 0 half of sum v (a - s)^2.  The same walk. */
int dnmf_weighted_divergence(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, const float* H,
                             long ldh, int k, float eps, int norm, float beta, double* out, void* ws, size_t ws_bytes, void* stream);
/* A whole weighted MU fit on one rank as ONE call (pyDNMF.py:138-182): `itr` steps of dnmf_weighted_update_w (iff w_update) and
 * dnmf_weighted_update_h with the clamp of H and then of W at the steps i % 10 == 0, normalize_features and sq_out = the pair of
 * dnmf_weighted_resid_sqnorm (the caller takes the square roots).  Host sequencing of the launches above on `stream`: no host
 * synchronisation inside.  One problem per call.  `ws`: dnmf_weighted_ws_bytes_fit(m, n, k) bytes, 16-byte aligned. */
size_t dnmf_weighted_ws_bytes_fit(long m, long n, int k);
int dnmf_weighted_mu_fit(const float* A, long m, long n, long lda, const float* V, long ldv, float* W, long ldw, float* H, long ldh, int k,
                         float eps, int norm, float beta, int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DNMF_WEIGHTED_API_H */
