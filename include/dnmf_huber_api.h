/* dnmf_huber_api.h -- the Huber-loss entry points of libdnmf_hip.so (dnmf_huber_*).  Part of the C ABI of include/dnmf.h, which
 * includes this file at its end: include dnmf.h, not this file (the error codes, DNMF_TUNED_MAX_K and the workspace contract are there).
 * The family has a header and a ctypes table (pydnmfk_amd/_lib.py: HUBER_SIGNATURES) of its own; its entry points are held to the
 * workspace contract of dnmf.h by tests/test_capi_huber.py and tests/test_gpu_huber.py. */
#ifndef DNMF_HUBER_API_H
#define DNMF_HUBER_API_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- robust NMF under the Huber loss for any threshold delta > 0 on dense float32 data (csrc/dnmf_huber.h) ----
 * No counterpart in the reference.  rho_delta(r) = r^2 / 2 for |r| <= delta, delta |r| - delta^2 / 2 otherwise; the objective is
 * sum rho_delta(a - s'), s' = W H + eps.  The rule is MU on the quadratic that majorises rho_delta at the current residual (iteratively
 * reweighted least squares).  With P = min(1, delta / |A - S'|) element-wise and F = H^T (W side) or W (H side):
 *     num = (A . P) F,   den = (S' . P) F,   X <- X . num / (den + eps)
 * which never increases the objective.  The pairs are the kernels of the masked, Itakura-Saito and beta pairs in a fifth mode, with
 * dnmf_beta_plan's launch geometry; the element-wise step is p = min(1, delta * rcp(|a - s'|)) by v_rcp_f32 and two multiplies.
 * Every entry point takes `float delta` after `eps` and returns DNMF_EINVAL unless delta > 0 (a NaN is refused; inf is accepted and is
 * the Frobenius objective: P = 1 exactly, the beta = 2 step of dnmf_beta_* bit for bit).  The value of P at a padded position is in
 * (0, 1] for every such delta, so padding adds exactly nothing (csrc/dnmf_huber.h).  There is no mask: a NaN of A is not skipped; callers
 * check that A is finite and >= 0.  1 <= k <= DNMF_TUNED_MAX_K; any shape and any leading dimensions.  Partial sums are added in a fixed
 * order, no float atomics: bit-reproducible.  Bad arguments return DNMF_EINVAL with a dnmf_last_error text that names the entry point;
 * dnmf_huber_ws_bytes returns 0.
 * `ws`: dnmf_huber_ws_bytes(m, n, k) bytes, 16-byte aligned, serves EVERY entry point below, the whole fit included; an entry point
 * needs, and writes, only the first bytes of it (the side's slab, the objective's slots, the fit's layout) and accepts any size from
 * that need on.  Nothing is retained between calls.  A misaligned `ws` is refused with DNMF_EWS as the first check, a delta that is
 * not accepted next. */
size_t dnmf_huber_ws_bytes(long m, long n, int k);
/* the pair stored: num = (A . P) F, den = (S' . P) F, [m x k] (W side, F = H^T) or [k x n] (H side, F = W) with the same leading dimension
 * ldo -- the two halves of one contiguous buffer where the sums cross ranks (one allreduce, then dnmf_csr_ratio_update: the plain ratio) */
int dnmf_huber_uht_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                        float delta, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream);
int dnmf_huber_wtu_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                        float delta, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream);
/* the pair applied where nothing crosses ranks: W <- W * num / (den + eps) in place after the pass has read it, H alike with
 * max(., eps) if clamp != 0 (pyDNMF.py:170-172) */
int dnmf_huber_update_w(const float* A, long m, long n, long lda, float* W, long ldw, const float* H, long ldh, int k, float eps,
                        float delta, void* ws, size_t ws_bytes, void* stream);
int dnmf_huber_update_h(const float* A, long m, long n, long lda, const float* W, long ldw, float* H, long ldh, int k, float eps,
                        float delta, int clamp, void* ws, size_t ws_bytes, void* stream);
/* *out (double, device) = sum rho_delta(a - (s + eps)) over the block.  The structure of dnmf_beta_divergence: S tiles in MFMA
 * accumulators, fp32 per 32 x 128 tile and lane, float64 from there on, every tile's sum in its own slot of `ws` and the slots added in
 * a fixed order: two calls are bit-identical. */
int dnmf_huber_loss(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                    float delta, double* out, void* ws, size_t ws_bytes, void* stream);
/* A whole Huber MU fit on one rank as ONE call (pyDNMF.py:138-182): `itr` steps of dnmf_huber_update_w (iff w_update) and
 * dnmf_huber_update_h with the clamp of H and then of W at the steps i % 10 == 0, normalize_features and sq_out = {||A - W H||^2,
 * ||A||^2} (the Frobenius pair, as after dnmf_beta_mu_fit; the caller takes the square roots).  Host sequencing of the launches above on
 * `stream`: no host synchronisation inside; the factors are bit-identical to those of the step calls made one by one.  One problem per
 * call. */
int dnmf_huber_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, float delta,
                      int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DNMF_HUBER_API_H */
