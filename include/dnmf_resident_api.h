/* dnmf_resident_api.h -- the resident pair-rule fits of libdnmf_hip.so (dnmf_pair_resident_*).  Part of the C ABI of include/dnmf.h, which
 * includes this file at its end: include dnmf.h, not this file (the error codes are there).  The family has a header and a ctypes table
 * (pydnmfk_amd/_lib.py: RESIDENT_SIGNATURES) of its own. */
#ifndef DNMF_RESIDENT_API_H
#define DNMF_RESIDENT_API_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- whole Itakura-Saito / beta-divergence MU fits of SMALL dense float32 problems, one workgroup per problem (csrc/dnmf_resident.h) ----
 * What dnmf_is_mu_fit / dnmf_beta_mu_fit compute -- `itr` steps of the W side (iff w_update) and the H side with the clamp of H and then
 * of W at the steps i % 10 == 0, normalize_features, and {||A - W H||^2, ||A||^2} -- inside ONE kernel: W and H stay in the workgroup's
 * LDS from the first step to the last, A is read from global memory every step and never written.  Problems of a batch are independent
 * workgroups: nothing waits for another workgroup, nothing needs co-residency, there is no time-out and no workspace.  Every sum has one
 * association that depends on (m, n, k) alone, so problem b of a batch has the bits of the same problem fitted alone; against the
 * launch-chain fits the agreement is to float32 rounding, not bit for bit.  1 <= k <= 32; the shape must fit the LDS of one workgroup. */
#define DNMF_RESIDENT_IS 0
#define DNMF_RESIDENT_BETA 1
#define DNMF_RESIDENT_NOT_TAKEN 1   /* returned (nothing launched, no error text) where the shape does not fit one workgroup on this device */
/* The plan of a shape, host arithmetic only (nothing is launched): out = {eligible 0/1, bytes of LDS, KP (16 for k <= 16, 32 for
 * k <= 32, 0 for any other rank), waves per workgroup, 16-row tiles the busiest wave owns in a W phase, 16-column tiles the busiest wave
 * owns in an H phase, 16-row tiles, 16-column tiles}.  Eligible: 1 <= k <= 32 and the bytes are at most 160 KiB. */
int dnmf_pair_resident_plan(long m, long n, int k, long out[8]);
/* `batch` >= 1 problems of one shape: problem b reads A + b a_stride (leading dimension lda) and updates W + b w_stride (ldw) and
 * H + b h_stride (ldh) in place (strides in elements; not read when batch == 1); sq_out[b] = {||A - W H||^2, ||A||^2} (device doubles,
 * stored).  mode DNMF_RESIDENT_IS ignores `beta`; DNMF_RESIDENT_BETA takes -2 <= beta <= 4 and runs beta = 0 as Itakura-Saito.  Nothing
 * outside the m x k and k x n blocks is written.  Returns DNMF_OK, DNMF_RESIDENT_NOT_TAKEN (not eligible, or beyond the LDS a workgroup
 * of the current device may hold), DNMF_EINVAL (bad arguments, a rank outside 1..32) or DNMF_EHIP. */
int dnmf_pair_resident_fit_batch(int mode, float beta, const float* A, long a_stride, long lda, float* W, long w_stride, long ldw, float* H,
                                 long h_stride, long ldh, long m, long n, int k, float eps, int w_update, int itr, int batch,
                                 double* sq_out, void* stream);
/* The same whole fit under per-entry weights V >= 0 of A's shape (what dnmf_weighted_mu_fit computes, csrc/dnmf_weighted.h), for the four
 * norms of dnmf_weighted_*: norm 0 fro, 1 kl, 2 is, 3 beta (`beta` is read under norm 3 alone, -2 <= beta <= 4; beta = 0 runs as is).
 * Problem b reads its weights at V + b v_stride (leading dimension ldv); v_stride = 0 is legal: every problem of the batch reads the same
 * V (an NMFk sweep perturbs the data and keeps the weights).  V is read from global memory every step beside A and takes no LDS: the
 * plan is dnmf_pair_resident_plan's.  Where v > 0 fails the entry of A is not looked at (NaN, inf, 0, negative: anything).
 * sq_out[b] = {sum v (A - W H)^2, sum v A^2} over v > 0, the pair of dnmf_weighted_resid_sqnorm.  With weights that are all 1 the
 * factors and the pair under is / beta are those of dnmf_pair_resident_fit_batch bit for bit.  Return codes as above. */
int dnmf_pair_resident_weighted_fit_batch(int norm, float beta, const float* A, long a_stride, long lda, const float* V, long v_stride,
                                          long ldv, float* W, long w_stride, long ldw, float* H, long h_stride, long ldh, long m, long n,
                                          int k, float eps, int w_update, int itr, int batch, double* sq_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DNMF_RESIDENT_API_H */
