/* dnmf_beta_api.h -- the beta-divergence entry points of libdnmf_hip.so (dnmf_beta_*).  Part of the C ABI of include/dnmf.h, which
 * includes this file at its end: include dnmf.h, not this file (the error codes, DNMF_TUNED_MAX_K and the workspace contract are there).
 * The family has a header and a ctypes table (pydnmfk_amd/_lib.py: BETA_SIGNATURES) of its own; its entry points are held to the
 * workspace contract of dnmf.h by tests/test_beta_workspace_cpu.py and tests/test_gpu_beta_workspace.py. */
#ifndef DNMF_BETA_API_H
#define DNMF_BETA_API_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the beta-divergence for any beta in [-2, 4] on dense float32 data (csrc/dnmf_beta.h) ----
 * No counterpart in the reference.  d_beta(a | s) = (a^beta + (beta - 1) s^beta - beta a s^(beta - 1)) / (beta (beta - 1)); beta = 2, 1, 0 are
 * the Frobenius (halved), Kullback-Leibler and Itakura-Saito objectives.  The rule is the majorisation-minimisation MU of Fevotte &
 * Idier (2011), scikit-learn's for beta_loss=<float>.  With S' = W H + eps, P = S'^(beta - 2) element-wise and F = H^T (W side) or W (H side):
 *     num = (A . P) F,   den = (S' . P) F,   X <- X . (num / (den + eps))^gamma
 *     gamma = 1 / (2 - beta) for beta < 1,   1 for 1 <= beta <= 2,   1 / (beta - 1) for beta > 2
 * which never increases D_beta(A | S').  The pairs are the kernels of the masked and Itakura-Saito pairs in a fourth mode, with
 * dnmf_is_plan's launch geometry; the element-wise step is p = exp2((beta - 2) log2 s') by v_log_f32 and v_exp_f32 and two multiplies.
 * Every entry point takes `float beta` after `eps` and returns DNMF_EINVAL unless -2 <= beta <= 4: within that range the value of P at a
 * padded position, 2^(-23 (beta - 2)), is finite, so padding adds exactly nothing (csrc/dnmf_beta.h).  There is no mask: a NaN of A is not
 * skipped; callers check A > 0 for beta <= 0 and A >= 0 for beta > 0.  beta = 1 and beta = 2 run these kernels like any other value: the
 * same objectives as the KL and Frobenius entry points, not their rules' bits.  1 <= k <= DNMF_TUNED_MAX_K; any shape and any leading
 * dimensions.  Partial sums are added in a fixed order, no float atomics: bit-reproducible.  Bad arguments return DNMF_EINVAL with a
 * dnmf_last_error text; the *_bytes functions return 0.
 * `ws`: dnmf_beta_ws_bytes(m, n, k) bytes, 16-byte aligned, serves every entry point below but the whole fit; nothing outside the first
 * bytes an entry point needs (the side's slab, the divergence's slots) is written.  A misaligned `ws` is refused with DNMF_EWS as the
 * first check, a beta outside the range next. */
size_t dnmf_beta_ws_bytes(long m, long n, int k);
/* The launch plans, host arithmetic only (nothing is launched): the eight numbers of dnmf_is_plan, with its values. */
int dnmf_beta_plan(long m, long n, int k, long out[8]);
/* the pair stored: num = (A . P) F, den = (S' . P) F, [m x k] (W side) or [k x n] (H side) with the same leading dimension ldo -- the two
 * halves of one contiguous buffer where the sums cross ranks (one allreduce, then dnmf_beta_ratio_update) */
int dnmf_beta_aht_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                       float beta, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream);
int dnmf_beta_wta_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                       float beta, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream);
/* the pair applied where nothing crosses ranks: W <- W * (num / (den + eps))^gamma in place after the pass has read it, H alike with
 * max(., eps) if clamp != 0 (pyDNMF.py:170-172) */
int dnmf_beta_update_w(const float* A, long m, long n, long lda, float* W, long ldw, const float* H, long ldh, int k, float eps,
                       float beta, void* ws, size_t ws_bytes, void* stream);
int dnmf_beta_update_h(const float* A, long m, long n, long lda, const float* W, long ldw, float* H, long ldh, int k, float eps,
                       float beta, int clamp, void* ws, size_t ws_bytes, void* stream);
/* X[r][c] <- X[r][c] * (num[r][c] / (den[r][c] + eps))^gamma(beta), max(., eps) if clamp != 0: the rule on a stored pair (ldo: the leading
 * dimension of num and den) -- the same function as the endings above; gamma = 1 takes the plain quotient, a quotient of 0 gives 0 */
int dnmf_beta_ratio_update(float* X, long rows, long cols, long ldx, const float* num, const float* den, long ldo, float eps, float beta,
                           int clamp, void* stream);
/* *out (double, device) = D_beta(A | W H + eps) = sum d_beta(a | s + eps) over the block; at beta = 1 the sum of a log(a / s') - a + s'
 * (s' where a = 0), at beta = 0 of q - log q - 1, q = a / s'; a^beta is 0 at a = 0.  The structure of dnmf_is_divergence: S tiles in MFMA
 * accumulators, fp32 per 32 x 128 tile and lane, float64 from there on, every tile's sum in its own slot of `ws` and the slots added
 * in a fixed order: two calls are bit-identical. */
int dnmf_beta_divergence(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                         float beta, double* out, void* ws, size_t ws_bytes, void* stream);
/* A whole beta-divergence MU fit on one rank as ONE call (pyDNMF.py:138-182): `itr` steps of dnmf_beta_update_w (iff w_update) and
 * dnmf_beta_update_h with the clamp of H and then of W at the steps i % 10 == 0, normalize_features and sq_out = {||A - W H||^2,
 * ||A||^2} (the Frobenius pair, as after dnmf_is_mu_fit; the caller takes the square roots).  Host sequencing of the launches above on
 * `stream`: no host synchronisation inside.  One problem per call.
 * `ws`: dnmf_beta_ws_bytes_fit(m, n, k) bytes, 16-byte aligned (0: bad shape or rank). */
size_t dnmf_beta_ws_bytes_fit(long m, long n, int k);
int dnmf_beta_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, float beta,
                     int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DNMF_BETA_API_H */
