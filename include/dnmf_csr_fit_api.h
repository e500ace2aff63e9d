/* dnmf_csr_fit_api.h -- whole MU fits of sparse (CSR) data blocks in libdnmf_hip.so, one problem or a batch of problems that share one
 * pattern (dnmf_csr_fit_*, dnmf_csr_mu_fit_batch).  Part of the C ABI of include/dnmf.h, which includes this file at its end: include
 * dnmf.h, not this file (the error codes are there).  The family has a header and a ctypes table (pydnmfk_amd/_lib.py:
 * CSR_FIT_SIGNATURES) of its own. */
#ifndef DNMF_CSR_FIT_API_H
#define DNMF_CSR_FIT_API_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- whole MU fits over a CSR block and the CSR of its transpose (csrc/dnmf_csr_batch.h, csrc/dnmf_csr_fit.hip) ----
 * `batch` >= 1 problems share ONE pattern -- row pointers and column indices of the block and of its transpose, both long-row lists (the
 * arrays of dnmf_csr_mm) -- and differ in their values and factors: the perturbed copies of an NMFk sweep.  The index stream is read once
 * per tile of BT problems, from problem-interleaved packed images of W and H^T in the workspace.  Problem b of a batch has the bits of
 * the same problem stepped through the single entry points (dnmf_csr_pack, dnmf_csr_mm / dnmf_csr_kl_mm / dnmf_csr_masked_update,
 * dnmf_gram_*, the update, clamp and normalisation launches, dnmf_csr_resid_sqnorm / dnmf_csr_masked_resid_sqnorm, dnmf_sqnorm). */

/* The plan of a shape, host arithmetic only: out = {KPAD (16 / 32 / 64 / 128 / 256), G = KPAD / 4 lanes per stored entry, BT problems
 * per tile (batch >= 2: 8 at KPAD 16, 4 at 32 and 64, 2 at 128 and 256; batch == 1: 1, the plain packed images), tiles = ceil(batch / BT), bytes of the interleaved image of W
 * (tiles x m x BT x KPAD floats), bytes of the image of H^T (tiles x n x BT x KPAD floats)}.  DNMF_EINVAL for a null `out`, m or n
 * outside 1 .. 2^31 - 1, k outside 1 .. DNMF_MAX_K, batch < 1. */
int dnmf_csr_fit_plan(long m, long n, int k, int batch, long out[6]);
/* bytes of workspace of dnmf_csr_mu_fit_batch; nseg_max = the larger of the two segment counts of the long-row lists.  0 for a bad shape */
size_t dnmf_csr_fit_ws_bytes(long m, long n, int k, int batch, int nseg_max);
/* What PyNMF runs for method 'mu' on one rank: `itr` steps in the step loop's launch order -- the W side iff w_update, the H side, the
 * clamp of H and then of W at the steps i % 10 == 0 --, normalize_features, and sq_out[b] = {||A - W H||^2, ||A||^2} (device doubles,
 * stored).  norm: 0 Frobenius, 1 KL.  missing: 0 -- an unstored entry is a zero; 1 -- it is not observed: rules and both sums run over the
 * stored positions (the passes end in the update itself).  crow [m + 1], col [nnz]: the block; t_crow [n + 1], t_col [nnz]: its
 * transpose; the long-row lists as for dnmf_csr_mm (NULL when n_long == 0).  val, t_val: [batch][nnz] float32, problem b at
 * + b val_stride elements (a multiple of 4, >= nnz; not read when batch == 1); nnz >= 1.  W + b w_stride (m x k, ldw) and H + b h_stride
 * (k x n, ldh) are updated in place; strides multiples of 4 elements that span one problem.  Nothing outside the m x k and k x n blocks
 * is written.  ws: 16-byte aligned, dnmf_csr_fit_ws_bytes.  No host synchronisation.  A null pointer, a bad shape or rank, batch < 1,
 * itr < 0 and a workspace that is too small return DNMF_EINVAL before any HIP call (dnmf_last_error says which). */
int dnmf_csr_mu_fit_batch(long m, long n, int k, int batch, long nnz, const int* crow, const int* col, const int* long_rows,
                          const int* long_segptr, int n_long, int nseg, const int* t_crow, const int* t_col, const int* t_long_rows,
                          const int* t_long_segptr, int t_n_long, int t_nseg, const float* val, const float* t_val, long val_stride, float* W,
                          long ldw, long w_stride, float* H, long ldh, long h_stride, int norm, int missing, float eps, int w_update, int itr,
                          void* ws, size_t ws_bytes, double* sq_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DNMF_CSR_FIT_API_H */
