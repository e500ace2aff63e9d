/* dnmf_slab_api.h -- the slab pair-rule fits of libdnmf_hip.so (dnmf_pair_slab_*).  Part of the C ABI of include/dnmf.h, which includes
 * this file at its end: include dnmf.h, not this file (the error codes are there).  The family has a header and a ctypes table
 * (pydnmfk_amd/_lib.py: SLAB_SIGNATURES) of its own. */
#ifndef DNMF_SLAB_API_H
#define DNMF_SLAB_API_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- whole Itakura-Saito / beta-divergence / weighted MU fits of a BATCH of same-shape dense float32 problems, two launches per step
 * for all of them (csrc/dnmf_slab.h) ----
 * What dnmf_is_mu_fit / dnmf_beta_mu_fit / dnmf_weighted_mu_fit compute -- `itr` steps of the W side (iff w_update) and the H side with
 * the clamp of H and then of W at the steps i % 10 == 0, normalize_features, and the pair of squared norms -- for every problem of the
 * batch together: a workgroup of the W phase owns 64 rows of one problem, one of the H phase 64 columns, and the factor it does not
 * own passes through its LDS in panels.  Nothing waits for another workgroup, nothing needs co-residency, there is no workspace, no
 * atomic and no time-out.  Every sum has one association that depends on (m, n, k) alone, so problem b of a batch has the bits of the
 * same problem fitted alone; against the launch-chain fits and the resident fits the agreement is to float32 rounding, not bit for
 * bit.  1 <= k <= 64, m and n up to 2^30, batch up to 65535. */
#define DNMF_SLAB_IS 0
#define DNMF_SLAB_BETA 1
/* The plan of a shape, host arithmetic only (nothing is launched): out = {eligible 0/1, bytes of LDS of a workgroup (the larger of the
 * two phases), KP (16 for k <= 16, 32 for k <= 32, 64 for k <= 64, 0 for any other rank), waves per workgroup, 64-row slabs (workgroups
 * of a W phase per problem), 64-column slabs (workgroups of an H phase per problem), panels of H a workgroup of the W phase walks,
 * panels of W a workgroup of the H phase walks}.  Eligible: 1 <= k <= 64 and m, n <= 2^30. */
int dnmf_pair_slab_plan(long m, long n, int k, long out[8]);
/* `batch` >= 1 problems of one shape: problem b reads A + b a_stride (leading dimension lda) and updates W + b w_stride (ldw) and
 * H + b h_stride (ldh) in place (strides in elements; not read when batch == 1); sq_out[b] = {||A - W H||^2, ||A||^2} (device doubles,
 * stored).  mode DNMF_SLAB_IS ignores `beta`; DNMF_SLAB_BETA takes -2 <= beta <= 4 and runs beta = 0 as Itakura-Saito.  Nothing outside
 * the m x k and k x n blocks is written, A is never written.  2 itr + 1 launches (itr + 1 without w_update) on `stream`.  Returns
 * DNMF_OK, DNMF_EINVAL (bad arguments, a rank outside 1..64: refused before any HIP call) or DNMF_EHIP. */
int dnmf_pair_slab_fit_batch(int mode, float beta, const float* A, long a_stride, long lda, float* W, long w_stride, long ldw, float* H,
                             long h_stride, long ldh, long m, long n, int k, float eps, int w_update, int itr, int batch, double* sq_out,
                             void* stream);
/* The same under per-entry weights V >= 0 of A's shape (what dnmf_weighted_mu_fit computes, csrc/dnmf_weighted.h), for the four norms
 * of dnmf_weighted_*: norm 0 fro, 1 kl, 2 is, 3 beta (`beta` is read under norm 3 alone, -2 <= beta <= 4; beta = 0 runs as is).  Problem
 * b reads its weights at V + b v_stride (leading dimension ldv); v_stride = 0 is legal: every problem of the batch reads the same V (an
 * NMFk sweep perturbs the data and keeps the weights).  Where v > 0 fails the entry of A is not looked at (NaN, inf, 0, negative:
 * anything).  sq_out[b] = {sum v (A - W H)^2, sum v A^2} over v > 0, the pair of dnmf_weighted_resid_sqnorm.  Return codes as above. */
int dnmf_pair_slab_weighted_fit_batch(int norm, float beta, const float* A, long a_stride, long lda, const float* V, long v_stride, long ldv,
                                      float* W, long w_stride, long ldw, float* H, long h_stride, long ldh, long m, long n, int k, float eps,
                                      int w_update, int itr, int batch, double* sq_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DNMF_SLAB_API_H */
