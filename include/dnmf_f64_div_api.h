/* dnmf_f64_div_api.h -- Itakura-Saito and the beta-divergence on float64 data (dnmf_is_f64_*, dnmf_beta_f64_*).  Part of the C ABI of
 * include/dnmf.h, which includes this file at its end: include dnmf.h, not this file (the error codes and the workspace contract are
 * there). */
#ifndef DNMF_F64_DIV_API_H
#define DNMF_F64_DIV_API_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rules of dnmf_is_* and dnmf_beta_* in float64 on the fp64 matrix cores (csrc/dnmf_f64_div.h) ----
 * The reference computes in the dtype of the data (pyDNMF.py:68), and scikit-learn runs these rules in float64.  With eps the float64
 * machine epsilon, S' = W H + eps and F = H^T (W side) or W (H side):
 *     IS:    R = 1 / S',          num = (A . R . R) F,  den = R F,         X <- X . sqrt(num / (den + eps))
 *     beta:  P = S'^(beta - 2),   num = (A . P) F,      den = (S' . P) F,  X <- X . (num / (den + eps))^gamma
 *     gamma = 1 / (2 - beta) for beta < 1,   1 for 1 <= beta <= 2,   1 / (beta - 1) for beta > 2
 * (Fevotte & Idier 2011).  A wave forms 16 x 16 tiles of W H with v_mfma_f64_16x16x4_f64, turns them into the pair in registers and
 * feeds both halves into second products that share their F operands; no m x n image is written.  P takes multiplies, a refined
 * reciprocal and a refined reciprocal square root whenever 2 (beta - 2) is an integer, the double-precision pow otherwise; beta = 0
 * takes the Itakura-Saito pair.  The beta entry points take `double beta` after `eps` and return DNMF_EINVAL unless -2 <= beta <= 4:
 * within that range the value of P at a padded position, 2^(-52 (beta - 2)), is finite in float64, so padding adds exactly nothing.
 * There is no mask: callers check A > 0 for IS and beta <= 0, A >= 0 for beta > 0.
 * 1 <= k <= 64 (DNMF_EINVAL beyond; the *_ws_bytes functions return 0); any shape and any leading dimensions, 16-byte accesses where
 * rows allow.  The partial sums of the column splits (W side) and row chunks (H side) are added in a fixed order, no float atomics:
 * bit-reproducible.
 * `ws`: dnmf_is_f64_ws_bytes(m, n, k) = dnmf_beta_f64_ws_bytes(m, n, k) bytes, 16-byte aligned, serves every entry point below; nothing
 * outside the first bytes an entry point needs (the side's slabs, the divergence's slots) is written.  A misaligned `ws` is refused
 * with DNMF_EWS as the first check, a beta outside the range next, a workspace that is too small with DNMF_EWS. */
size_t dnmf_is_f64_ws_bytes(long m, long n, int k);
size_t dnmf_beta_f64_ws_bytes(long m, long n, int k);
/* the pair stored: [m x k] (W side, aht) or [k x n] (H side, wta), num and den with the same leading dimension ldo -- the two halves of
 * one contiguous buffer where the sums cross ranks */
int dnmf_is_f64_aht_pair(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps,
                         double* num, double* den, long ldo, void* ws, size_t ws_bytes, void* stream);
int dnmf_is_f64_wta_pair(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps,
                         double* num, double* den, long ldo, void* ws, size_t ws_bytes, void* stream);
int dnmf_beta_f64_aht_pair(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps,
                           double beta, double* num, double* den, long ldo, void* ws, size_t ws_bytes, void* stream);
int dnmf_beta_f64_wta_pair(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps,
                           double beta, double* num, double* den, long ldo, void* ws, size_t ws_bytes, void* stream);
/* the pair applied where nothing crosses ranks: the factor is updated in place after the pass has read it; H with max(., eps) if
 * clamp != 0 (pyDNMF.py:170-172) */
int dnmf_is_f64_update_w(const double* A, long m, long n, long lda, double* W, long ldw, const double* H, long ldh, int k, double eps, void* ws,
                         size_t ws_bytes, void* stream);
int dnmf_is_f64_update_h(const double* A, long m, long n, long lda, const double* W, long ldw, double* H, long ldh, int k, double eps, int clamp,
                         void* ws, size_t ws_bytes, void* stream);
int dnmf_beta_f64_update_w(const double* A, long m, long n, long lda, double* W, long ldw, const double* H, long ldh, int k, double eps,
                           double beta, void* ws, size_t ws_bytes, void* stream);
int dnmf_beta_f64_update_h(const double* A, long m, long n, long lda, const double* W, long ldw, double* H, long ldh, int k, double eps,
                           double beta, int clamp, void* ws, size_t ws_bytes, void* stream);
/* the rule on a stored pair (ldo: the leading dimension of num and den), max(., eps) if clamp != 0 -- the same function as the endings
 * above, so the same bits; gamma = 1 takes the plain quotient, a quotient of 0 gives 0 */
int dnmf_is_f64_ratio_update(double* X, long rows, long cols, long ldx, const double* num, const double* den, long ldo, double eps, int clamp,
                             void* stream);
int dnmf_beta_f64_ratio_update(double* X, long rows, long cols, long ldx, const double* num, const double* den, long ldo, double eps, double beta,
                               int clamp, void* stream);
/* *out (double, device) = D_IS / D_beta(A | W H + eps) over the block, in float64 arithmetic: at beta = 1 the sum of a log(a / s') - a + s'
 * (s' where a = 0), at beta = 0 of q - log q - 1, q = a / s'; a^beta is 0 at a = 0.  Every workgroup's sum has its own slot of `ws` and
 * the slots are added in a fixed order: two calls are bit-identical. */
int dnmf_is_f64_divergence(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps,
                           double* out, void* ws, size_t ws_bytes, void* stream);
int dnmf_beta_f64_divergence(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps,
                             double beta, double* out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DNMF_F64_DIV_API_H */
