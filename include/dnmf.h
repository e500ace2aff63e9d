/*
 * dnmf.h -- C ABI of libdnmf_hip.so: the MI355X (gfx950) multiplicative-update engine
 * that replaces the numpy hot path of lanl/pyDNMFk.
 *
 * The reference has no FFI layer: its hot path is reached by plain Python calls
 * (pyDNMFk/dist_nmf.py, pyDNMFk/pyDNMF.py).  Each entry point below names the reference
 * lines it replaces.  Calling convention:
 *   - every matrix is dense row-major fp32 in DEVICE memory, given as pointer + leading
 *     dimension (elements); the caller owns every buffer, nothing is retained;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is
 *     stream-ordered, no entry point synchronises the device or allocates memory; the library
 *     reads no environment variables;
 *   - every leading dimension must be >= the logical row length (lda >= n, ...);
 *   - `ws` is caller-provided device scratch of at least dnmf_ws_bytes(m, n, k) bytes -- or of the size query its section names
 *     (dnmf_ws_bytes_hblocks, _bf16x6, _fit, _1d / _2d, dnmf_f64_ws_bytes, dnmf_bcd_ws_bytes_w, dnmf_csr_ws_bytes, ...).  EVERY `ws`
 *     starts on a 16-byte boundary: the partial slabs are read and written as 16-byte vectors, and the padded factor images, the
 *     slots of the waiting kernels and the float64 sums sit at multiples of 256 bytes from it.  No kernel needs more than that; a
 *     workspace at any other address is refused with DNMF_EWS before anything else is looked at (float32, bf16x6, float64, whole fits,
 *     BCD, HALS and the grid steps: first of all checks; CSR, masked dense and Itakura-Saito: together with the size).  The
 *     workspace holds no state: what it contains before a call never shows in a result, and a result does not depend on ws_bytes
 *     once that reaches the query (tests/test_gpu_workspace.py holds every entry point to both);
 *   - return value: 0 on success, negative DNMF_E* on error (dnmf_last_error() has text);
 *   - k <= DNMF_MAX_K.  Internally k is padded to KP = 32/64/128/256; "gram" buffers G are
 *     always KP x KP, ld = KP, zero padded (dnmf_kp(k) returns KP).
 * Collectives: the kernels above the "Grid exchanges" section never communicate -- a host may issue the p_r x p_c grid
 * exchanges itself between these calls, exactly where the reference calls mpi4py (dist_nmf.py:681,707,114,163,169,195,
 * 202; pydnmfk_amd/dist_nmf.py does so over torch.distributed).  The last section binds RCCL at run time and offers
 * communicators plus whole 1D steps that enqueue kernels -> allreduce -> kernels on one stream.
 */
#ifndef DNMF_H
#define DNMF_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DNMF_MAX_K 256        /* the primitives, the local whole steps and the whole fits */
#define DNMF_TUNED_MAX_K 128  /* the tuned kernels' own limit: beyond it the contractions run as two passes over A and the k x k products
                               * on plain MFMA kernels (csrc/dnmf_wide.hip).  Also the limit of the float64 path, the bf16x6 arithmetic,
                               * bf16 storage of A in the error evaluation, the fused dnmf_aht_update_w, the block-column (hblocks)
                               * products and the library-sequenced grid steps (dnmf_*_step_1d / _2d: the host keeps its choreography) */
#define DNMF_OK 0
#define DNMF_EINVAL (-1)   /* bad shape / null pointer / k too large */
#define DNMF_EWS (-2)      /* workspace too small */
#define DNMF_EHIP (-3)     /* HIP launch error */
#define DNMF_ECOMM (-4)    /* RCCL missing or an RCCL call failed */

const char* dnmf_last_error(void);
int dnmf_version(void);
/* padded rank used for internal k x k buffers (32, 64, 128 or 256); <0 if k unsupported */
int dnmf_kp(int k);
/* scratch bytes sufficient for ANY entry point below on an m x n block with rank k */
size_t dnmf_ws_bytes(long m, long n, int k);

/* ---- Gram matrices (dist_nmf.py:679 `np.matmul(A.T, A)` in global_gram; :113 in 2D) ---- */
/* G[KP x KP] = H H^T for H [k x n] (called as global_gram(H.T), dist_nmf.py:729,241) */
int dnmf_gram_hht(const float* H, int k, long n, long ldh, float* G, void* ws, size_t ws_bytes, void* stream);
/* G[KP x KP] = W^T W for W [m x k] (global_gram(W), dist_nmf.py:748,222) */
int dnmf_gram_wtw(const float* W, long m, int k, long ldw, float* G, void* ws, size_t ws_bytes, void* stream);

/* ---- The two big contractions (dist_nmf.py:705 `np.matmul(A, B)` in global_mm; :166,:198 in 2D) ---- */
/* AH[m x k] = A[m x n] H[k x n]^T        (global_mm(A_ij, H_j.T), dist_nmf.py:730; AH_glob :198) */
int dnmf_aht(const float* A, long m, long n, long lda, const float* H, int k, long ldh,
             float* AH, long ldah, void* stream);
/* The same product with H given as n / nh COLUMN BLOCKS stacked [q][k][nh] -- the receive buffer of the allgather of the
 * ranks' k x nh slices (AH_glob, dist_nmf.py:195-197; np.hstack there), so that the 2D step needs no re-assembly copy.
 * n % nh == 0 and nh % 32 == 0 (DNMF_EINVAL otherwise: assemble H and call dnmf_aht). */
int dnmf_aht_hblocks(const float* A, long m, long n, long lda, const float* Hs, long nh, int k,
                     float* AH, long ldah, void* stream);
/* AtW[k x n] = W[m x k]^T A[m x n]       (global_mm(W_i.T, A_ij), dist_nmf.py:749; ATW_glob :166) */
int dnmf_wta(const float* A, long m, long n, long lda, const float* W, int k, long ldw,
             float* AtW, long ldatw, void* ws, size_t ws_bytes, void* stream);
/* W^T A AND the Gram matrix of the same W in one call: AtW as dnmf_wta, G as dnmf_gram_wtw (KP x KP, zero padded) -- the two
 * reductions the H phase sends through ONE allreduce (dist_nmf.py:705 twice, :681 / :707, :747-748).  For k <= 16 the Gram
 * rides in the same two launches: the wave of column block 0 of every row chunk sums W^T W over its rows (the W value a lane
 * holds is the A and the B operand of that product: one more MFMA per step, no more loads), the reduction launch sums the
 * partial tiles.  For k > 16 it is dnmf_gram_wtw followed by dnmf_wta (a riding Gram in the 32-wide kernel was measured:
 * no gain over the two launches it saves).  `ws` >= dnmf_ws_bytes(m, n, k). */
int dnmf_wta_gram(const float* A, long m, long n, long lda, const float* W, int k, long ldw, float* AtW, long ldatw,
                  float* G, void* ws, size_t ws_bytes, void* stream);

/* ---- Multiplicative updates (element-wise multiply/divide with the small k x k product) ----
 * G must be symmetric (the Gram matrices are).  These two kernels address a tile through 32-bit offsets: leading
 * dimensions up to 2^23 (W side) / 2^24 (H side) elements, DNMF_EINVAL beyond. */
/* W *= AH / (W G + eps), G = H H^T       (dist_nmf.py:731-732, :244-245) */
int dnmf_mu_update_w(float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G,
                     float eps, void* stream);
/* H *= AtW / (H^T G + eps)^T, G = W^T W  (dist_nmf.py:750-751, :224-225); clamp!=0 also applies
 * H = max(H, eps) afterwards (pyDNMF.py:156,171) */
int dnmf_mu_update_h(float* H, int k, long n, long ldh, const float* AtW, long ldatw, const float* G,
                     float eps, int clamp, void* stream);
/* Fused W phase for p_c == 1 (no exchange between the GEMM and the update):
 * W *= (A H^T) / (W G + eps) in one pass over A  (dist_nmf.py:716-732) */
int dnmf_aht_update_w(const float* A, long m, long n, long lda, const float* H, int k, long ldh,
                      const float* G, float* W, long ldw, float eps, void* stream);

/* ---- The W phase from a transposed image of A (csrc/dnmf_timg.hip; fp32 A, 32 < k <= 64) ----
 * A is constant for a whole fit.  With At[c][i] = A[i][c] (n x m, leading dimension ldat = m rounded up to 4) in device memory,
 * A H^T becomes a product whose contraction index runs down the rows of both operands: it streams At from global memory
 * straight into the matrix cores (no LDS round trip, a higher held clock) and then applies the same fused update.  Every output
 * element runs the SAME chain of MFMA steps as in the kernel behind dnmf_aht_update_w, so results are BIT-EQUAL with and
 * without the image: which path ran never shows in the numbers.
 *   dnmf_wimage_bytes(m, n)   bytes of the image buffer of an m x n block (the image + room for H^T, rebuilt every W phase)
 *   dnmf_wimage_build         writes the image (one read and one write of A; m, n, lda, ldat multiples of 4, 16-byte aligned)
 *   dnmf_wimage_bind/unbind   names the image of (A, m, n, lda) to the CALLING THREAD.  While bound, dnmf_aht_update_w,
 *                             dnmf_mu_fro_step and dnmf_mu_fro_fit on exactly that (A, m, n, lda) -- one problem, no batch --
 *                             take the image where the plan below takes it and the kernel of dnmf_aht_update_w otherwise,
 *                             silently.  THE CALLER KEEPS THE IMAGE CURRENT: after any write to A, rebuild or unbind -- a stale
 *                             image gives silently wrong factors.  Unbind before freeing either buffer.
 *   dnmf_set_wimage(mode)     process-wide: 0 off, 1 auto (default: where a sweep measured a gain -- m a multiple of 131072, i.e. the
 *                             128-row blocks fill whole half-rounds of 1024 waves, and m * n >= 2^27), 2 forced (any size the
 *                             conditions admit; up to 2 x slower than the other kernel on small or ragged row counts).  Returns the previous setting; other values only query.
 *   dnmf_wimage_plan          out = {taken, reason, R, grid, KT, launches} for a bound image under the current mode, answered
 *                             by the function the launch decides with; launches = W phases the calling thread has run from an
 *                             image so far (the only way to tell: the results do not show it).  a_aligned: A, the image and H are 16-byte aligned and ldh % 4 == 0;
 *                             w_aligned: W and G are 16-byte aligned, ldw % 4 == 0, 128 rows of W lie within 2 GiB.  Conditions:
 *                             n % 32 == 0, m % 4 == 0, lda % 4 == 0, 32 < k <= 64, k % 4 == 0, rows of the image short enough for
 *                             descriptor windows of R >= 8 rows ((R + 8) * ldat * 4 < 2^31; R a power of two).  reason: 0 taken,
 *                             1 mode off, 2 shape, 3 alignment of A / image / H, 4 alignment of W / k % 4, 5 rank, 6 auto mode and
 *                             a shape where it does not pay, 7 descriptor windows. */
size_t dnmf_wimage_bytes(long m, long n);
int dnmf_wimage_build(const float* A, long m, long n, long lda, float* At, long ldat, void* stream);
int dnmf_wimage_bind(const float* A, long m, long n, long lda, float* At, long ldat);
void dnmf_wimage_unbind(void);
int dnmf_set_wimage(int mode);
int dnmf_wimage_plan(long m, long n, int k, long lda, int a_aligned, int w_aligned, int out[6]);

/* ---- One whole local MU/Frobenius step on one rank (dist_nmf.py:755-771 with p_r = p_c = 1),
 * W first then H with the new W; clamp!=0 applies pyDNMF.py:155-157 after the step. ---- */
/* k <= 32 on fp32 A with n a multiple of 4 up to 4096 (8192 at k <= 16; by default from 2048), m >= 4096, 16-byte aligned rows (and w_update != 0): the step reads A
 * ONCE (csrc/dnmf_team.h): teams of ceil(n / 512) workgroups share 16-row slabs by columns, exchange their 16 x k partials of A H^T inside the
 * kernel, update the slab's W rows and add W_new^T A from the LDS copy of the slab -- dist_nmf.py:729-732 feeding :748-751 without a
 * second pass.  Same update rule; the sums over n run in another association than the two-pass kernels' (results agree to fp32
 * rounding, not bit for bit; runs of the same shape are bit-identical).  All its workgroups (one per CU) must be resident together: the
 * launch starts with a census and writes nothing unless every workgroup has been seen (a shared GPU: dnmf_hals_sweep_status reports the
 * time-out, W is untouched by that launch).  dnmf_mu_fro_onepass(m, n, k) != 0: steps of this shape take it on this device;
 * dnmf_set_onepass(0) switches it off process-wide (returns the previous setting). */
/* Process-wide switch of every kernel whose workgroups wait for each other (the whole fits of small problems, the persistent HALS W sweep
 * -- local and across ranks --, the one-pass MU/FRO step): on (default) / off = their launch-chain forms everywhere (same update rules, no
 * co-residency needed: for a GPU shared with another process or stream).  Returns the previous setting.  PyNMF switches it off for the
 * rest of the process, and fits again from the initial factors, when dnmf_hals_sweep_status reports a time-out. */
int dnmf_set_persistent(int on);
int dnmf_mu_fro_onepass(long m, long n, int k);
int dnmf_set_onepass(int on);
int dnmf_mu_fro_step(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh,
                     int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, void* stream);

/* ---- HALS / Frobenius sweeps (dist_nmf.py:873-934; 2D :411-470).  They reuse dnmf_gram_*, dnmf_aht, dnmf_wta. ---- */
/* One column of the W sweep (dist_nmf.py:886-887): first applies the pending normalisation of column kk-1
 * (W[:,kk-1] /= sqrt(*prev_ss2), skipped if prev_ss2 is NULL or 0), then
 * W[:,kk] = max(W[:,kk]*G[kk][kk] + AH[:,kk] - W G[:,kk], eps) and *ss2_out = sum_i W[i][kk]^2 (device double).
 * With p_r > 1 the caller allreduces *ss2_out between calls (utils.py:390 inside `norm`, dist_nmf.py:889). */
int dnmf_hals_w_col(float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G, int kk,
                    const double* prev_ss2, float eps, double* ss2_out, void* stream);
/* W[:,col] /= sqrt(*ss2) if > 0 (dist_nmf.py:890-891, the normalisation of the last column) */
int dnmf_hals_w_scale(float* W, long m, long ldw, int col, const double* ss2, void* stream);
/* the whole W sweep on one rank (no allreduce of the norms): k column launches + the final scale; ss2 = k doubles */
int dnmf_hals_update_w(float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G, float eps,
                       double* ss2, void* stream);
/* The same W sweep in ONE launch when the rank's rows fit on the device at once (one lane per row for the whole sweep:
 * W and AH are read once, W written once; grid-wide column norms through per-workgroup fp64 slots reduced in a fixed
 * order -- bitwise reproducible); otherwise it runs dnmf_hals_update_w.  `ws` >= dnmf_ws_bytes(m, k, k). dist_nmf.py:884-891
 * The persistent kernel's workgroups wait for each other: do not run two of these sweeps concurrently on one device
 * (two streams, or two processes sharing a GPU with factors of tens of thousands of rows) -- each could hold the
 * resources the other's remaining workgroups need.  One process per GPU and one stream, the product's model, is safe. */
int dnmf_hals_sweep_w(float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G, float eps,
                      void* ws, size_t ws_bytes, void* stream);
/* What dnmf_hals_sweep_w would run for an m x k factor with these pitches on the current device (nothing is launched; the decision is
 * the one the sweep itself takes).  w_aligned16 / ah_aligned16 != 0: W / AH start on a 16-byte boundary.  out = {route, KP, grid,
 * transform, vec, cap}: route 1 = the persistent sweep, 0 = k column launches (always for a wide rank, k > 128); KP = dnmf_kp(k); grid =
 * workgroups of the sweep kernel (512 rows each) or of one column launch (256 rows each, at most 2048: beyond that they stride);
 * transform = the variant of the sweep's first pass (0: 16-byte row access and whole tiles, 1: 16-byte row access with guards, 2: scalar
 * row access; -1 on route 0); vec = 1: the sweep kernel loads and stores its rows 16 bytes at a time; cap = workgroups of that
 * instantiation the device holds resident (0 for a wide rank).  It assumes a workspace of dnmf_ws_bytes(m, k, k), a single problem
 * (no batch) and reads the process-wide dnmf_set_persistent switch.  Refused: a null `out`, k outside 1..256, m < 1, a pitch below k. */
int dnmf_hals_sweep_plan(long m, int k, long ldw, long ldah, int w_aligned16, int ah_aligned16, int out[6]);
/* Did a persistent W sweep on the current device give up waiting for its other workgroups since the last call?  (Its
 * workgroups were not co-resident -- see above; the sweep then ends after about a second with NaN column norms instead of
 * hanging the GPU, and sets a sticky per-device word.)  *timed_out = 0 / 1; the word is cleared.  This call SYNCHRONISES
 * `stream` (the one entry point that does): call it where the host waits anyway, e.g. before the factors leave the GPU. */
int dnmf_hals_sweep_status(int* timed_out, void* stream);
/* H sweep: for kk: H[kk,:] = max(H[kk,:] + AtW[kk,:] - G[kk,:] H, eps), rows updated in sequence (dist_nmf.py:905-909) */
int dnmf_hals_update_h(float* H, int k, long n, long ldh, const float* AtW, long ldatw, const float* G, float eps,
                       void* stream);

/* ---- KL pieces (dist_nmf.py:776-869; 2D :294-343).  U = A / (W H + eps) is never materialised. ---- */
/* UHT[m x k] = (A / (W H + eps)) H^T     (glob_UX(axis=0), dist_nmf.py:806,810; UHT_glob :337-338) */
int dnmf_kl_uht(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                int k, float eps, float* UHT, long ldo, void* ws, size_t ws_bytes, void* stream);
/* The same product with H given as n / nh COLUMN BLOCKS stacked [q][k][nh] -- the receive buffer of the allgather of the
 * ranks' k x nh slices (gather_W_H, dist_nmf.py:283-287; np.hstack there) -- so that the 2D step needs no re-assembly copy.
 * n % nh == 0 and nh % 32 == 0 (DNMF_EINVAL otherwise: assemble H and call dnmf_kl_uht). */
int dnmf_kl_uht_hblocks(const float* A, long m, long n, long lda, const float* W, long ldw, const float* Hs, long nh,
                        int k, float eps, float* UHT, long ldo, void* ws, size_t ws_bytes, void* stream);
/* scratch bytes for dnmf_kl_uht_hblocks (one partial slab per column split, and a split never straddles a block: narrow
 * blocks need more slabs than dnmf_ws_bytes reserves); >= dnmf_ws_bytes(m, n, k) */
size_t dnmf_ws_bytes_hblocks(long m, long n, int k, long nh);
/* WTU[k x n] = W^T (A / (W H + eps))     (glob_UX(axis=1), dist_nmf.py:806,808; WTU_glob :311-312) */
int dnmf_kl_wtu(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                int k, float eps, float* WTU, long ldo, void* ws, size_t ws_bytes, void* stream);
/* x[k] = row sums of H [k x n]           (sum_along_axis(H, axis=1), dist_nmf.py:793-795) */
int dnmf_rowsum(const float* H, int k, long n, long ldh, float* x, void* stream);
/* x[k] = column sums of W [m x k]        (sum_along_axis(W, axis=0), dist_nmf.py:793; pyDNMF.py:187) */
int dnmf_colsum(const float* W, long m, int k, long ldw, float* x, void* ws, size_t ws_bytes, void* stream);
/* W[i][j] *= S[i][j] / (x[j] + eps)      (dist_nmf.py:828-830) */
int dnmf_kl_update_w(float* W, long m, int k, long ldw, const float* S, long lds_, const float* x, float eps,
                     void* stream);
/* H[j][c] *= S[j][c] / (x[j] + eps); clamp as above (dist_nmf.py:847-849) */
int dnmf_kl_update_h(float* H, int k, long n, long ldh, const float* S, long lds_, const float* x, float eps,
                     int clamp, void* stream);
/* One whole local MU/KL step on one rank (dist_nmf.py:851-869 with p_r = p_c = 1) */
int dnmf_mu_kl_step(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh,
                    int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, void* stream);

/* ---- PyNMF.fit helpers (pyDNMF.py:155-157, 185-194, 205-218) ---- */
/* X = max(X, eps) over a rows x cols matrix */
int dnmf_clamp_min(float* X, long rows, long cols, long ldx, float eps, void* stream);
/* W[i][j] /= (s[j] + eps) (pyDNMF.py:192) */
int dnmf_scale_cols_div(float* W, long m, int k, long ldw, const float* s, float eps, void* stream);
/* H[j][c] *= s[j] (pyDNMF.py:193) */
int dnmf_scale_rows_mul(float* H, int k, long n, long ldh, const float* s, void* stream);
/* *out (double, device) = sum A^2  (np.linalg.norm(A)**2, pyDNMF.py:208,215) */
int dnmf_sqnorm(const float* A, long m, long n, long lda, double* out, void* stream);
/* *out (double, device) = sum (A - W H)^2 without materialising the residual (pyDNMF.py:207,215) */
int dnmf_resid_sqnorm(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                      int k, double* out, void* stream);
/* the same with a workspace (dnmf_ws_bytes(m, n, k) is enough; NULL = dnmf_resid_sqnorm): ranks that are not a whole number of
 * 32-wide tiles (every k an NMFk sweep visits) are evaluated on zero-padded factor images in it by the LDS-staged kernel */
int dnmf_resid_sqnorm_ws(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                         int k, double* out, void* ws, size_t ws_bytes, void* stream);
/* per-column pieces of PyNMF.column_err (pyDNMF.py:221-239) over this rank's rows: num[c] += sum_i (A - W H)[i][c]^2,
 * den[c] += sum_i A[i][c]^2 (device doubles, n each, ACCUMULATED: the caller zeroes them; A - W H is never materialised) */
int dnmf_column_err(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                    int k, double* num, double* den, void* stream);

/* NMFk perturbation (pyDNMFk.py:42-44, sample.randM): X_per = X * (1 + noise_var + 2 noise_var U), U ~ U[0,1) per element from a
 * counter-based generator keyed by `seed` and the element's position (stateless: the same (seed, position) gives the same value).
 * One pass; bf16 != 0: X and X_per are bfloat16 (scaled in fp32, rounded once).  Any shape and alignment (16-byte aligned rows of
 * whole 8-element vectors take a vector kernel, everything else one element per thread -- the values are the same either way). */
int dnmf_perturb_uniform(const void* X, void* X_per, long rows, long cols, long ldx, long ldo, float noise_var,
                         unsigned long long seed, int bf16, void* stream);

/* ---- bf16 STORAGE of the data matrix (BASELINE config 5, "mixed precision"; no reference counterpart: numpy has no
 * bf16).  A is bfloat16 in device memory (pointer to 16-bit words, lda in elements, rows 8-byte aligned for the vector
 * path), widened exactly to fp32 in registers; W, H, every product and every accumulation stay fp32, so each call equals
 * its fp32 twin applied to float(A).  Same arguments otherwise. ---- */
int dnmf_aht_bf16a(const void* A, long m, long n, long lda, const float* H, int k, long ldh,
                   float* AH, long ldah, void* stream);
int dnmf_wta_bf16a(const void* A, long m, long n, long lda, const float* W, int k, long ldw,
                   float* AtW, long ldatw, void* ws, size_t ws_bytes, void* stream);
int dnmf_wta_gram_bf16a(const void* A, long m, long n, long lda, const float* W, int k, long ldw, float* AtW, long ldatw,
                        float* G, void* ws, size_t ws_bytes, void* stream);
int dnmf_aht_update_w_bf16a(const void* A, long m, long n, long lda, const float* H, int k, long ldh,
                            const float* G, float* W, long ldw, float eps, void* stream);
int dnmf_mu_fro_step_bf16a(const void* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh,
                           int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, void* stream);
int dnmf_sqnorm_bf16a(const void* A, long m, long n, long lda, double* out, void* stream);
int dnmf_resid_sqnorm_bf16a(const void* A, long m, long n, long lda, const float* W, long ldw, const float* H,
                            long ldh, int k, double* out, void* stream);
int dnmf_resid_sqnorm_ws_bf16a(const void* A, long m, long n, long lda, const float* W, long ldw, const float* H,
                               long ldh, int k, double* out, void* ws, size_t ws_bytes, void* stream);
int dnmf_column_err_bf16a(const void* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                          int k, double* num, double* den, void* stream);

/* ---- bf16x6: the two big contractions on the bf16 matrix cores with fp32-grade products (no reference counterpart; an
 * alternative arithmetic for global_mm, dist_nmf.py:705).  Every fp32 operand is cut into three bf16 pieces (x = x1 + x2 + x3
 * to 2^-24 |x|) and a product is the sum of the six largest piece products, each exact in the fp32 accumulator; the dropped
 * terms are below one fp32 rounding of the product (csrc/dnmf_split.h has the bound, tests/test_gpu_split.py the measurement
 * against float64).  Opt-in: the fp32-MFMA entry points above stay the default and the reference for parity.
 * Kernels exist for 32 < k <= 128, 16-byte aligned rows of A and n % 128 == 0; any other shape is forwarded to the fp32
 * entry point of the same name.  Same arguments as the fp32 twins plus a workspace of dnmf_ws_bytes_bf16x6(m, n, k) bytes
 * (the bf16 images of H and W^T, partial sums). ---- */
size_t dnmf_ws_bytes_bf16x6(long m, long n, int k);
int dnmf_aht_bf16x6(const float* A, long m, long n, long lda, const float* H, int k, long ldh,
                    float* AH, long ldah, void* ws, size_t ws_bytes, void* stream);
int dnmf_wta_bf16x6(const float* A, long m, long n, long lda, const float* W, int k, long ldw,
                    float* AtW, long ldatw, void* ws, size_t ws_bytes, void* stream);
int dnmf_aht_update_w_bf16x6(const float* A, long m, long n, long lda, const float* H, int k, long ldh,
                             const float* G, float* W, long ldw, float eps, void* ws, size_t ws_bytes, void* stream);
int dnmf_mu_fro_step_bf16x6(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh,
                            int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, void* stream);
/* The same four with A STORED as bfloat16 (dnmf_*_bf16a above): A is then its own single piece, a product is the sum of three
 * bf16 piece products (A times the three pieces of the fp32 factor), each exact in the fp32 accumulator -- the result equals
 * the fp32-MFMA twin on float(A) to fp32 rounding, at half the HBM bytes and a quarter of the matrix work of the fp32 A case.
 * Kernels for 16 < k <= 128 (k <= 16: the 16-wide fp32 kernels of the bf16a entry points are as fast). */
int dnmf_aht_bf16a_bf16x6(const void* A, long m, long n, long lda, const float* H, int k, long ldh,
                          float* AH, long ldah, void* ws, size_t ws_bytes, void* stream);
int dnmf_wta_bf16a_bf16x6(const void* A, long m, long n, long lda, const float* W, int k, long ldw,
                          float* AtW, long ldatw, void* ws, size_t ws_bytes, void* stream);
int dnmf_aht_update_w_bf16a_bf16x6(const void* A, long m, long n, long lda, const float* H, int k, long ldh,
                                   const float* G, float* W, long ldw, float eps, void* ws, size_t ws_bytes, void* stream);
int dnmf_mu_fro_step_bf16a_bf16x6(const void* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh,
                                  int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, void* stream);
/* The two KL products (dist_nmf.py:806-810) in the same arithmetic: S = W H, U H^T and W^T U as bf16 piece products, U = A / (S
 * + eps) in fp32 between them.  Kernels for every k <= 128 with n % 128 == 0 and 16-byte aligned rows of A; other shapes are forwarded to
 * dnmf_kl_uht / dnmf_kl_wtu / dnmf_mu_kl_step.  Workspace: dnmf_ws_bytes_bf16x6(m, n, k). */
int dnmf_kl_uht_bf16x6(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                       int k, float eps, float* UHT, long ldo, void* ws, size_t ws_bytes, void* stream);
int dnmf_kl_wtu_bf16x6(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                       int k, float eps, float* WTU, long ldo, void* ws, size_t ws_bytes, void* stream);
int dnmf_mu_kl_step_bf16x6(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh,
                           int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, void* stream);
/* Which kernels and loop trip counts the bf16x6 entry points choose for a shape: host only, launches nothing, answered by the
 * functions the entry points decide with.  lda in elements of A; a_bf16: A stored as bfloat16; a_aligned16: A starts on a 16-byte
 * boundary.  out = {0 the Frobenius entry points take the split kernels (else they forward to the fp32 twins),
 *   1 the KL entry points do (fp32 A only), 2 KT (32-wide tiles of the padded rank),
 *   3 tiles in flight in the interior A H^T main loop, 4 W^T A row chunks, 5 rows per chunk,
 *   6 KL W^T U row chunks, 7 32-row blocks per chunk, 8 KL U H^T column splits, 9 columns per split,
 *   10 / 11 the A H^T / W^T A kernels stream A past the caches (A of 256 MiB and more)}.
 * Fields 3-5, 10, 11 are 0 unless out[0], fields 6-9 unless out[1]; all are 0 when neither holds. */
int dnmf_bf16x6_plan(long m, long n, int k, long lda, int a_bf16, int a_aligned16, long out[12]);

/* ---- Whole fits on one rank (PyNMF.fit, pyDNMF.py:138-182 with p_r = p_c = 1): `itr` update steps with the clamp to eps
 * after the steps i % 10 == 0 (:155-157, :170-172), then normalize_features (:185-194) and the two squared norms of
 * relative_err (:205-218) -- everything enqueued on `stream` by ONE call: no host code between the launches, nothing
 * synchronises.  sq_out (device doubles) receives {sum (A - W H)^2, sum A^2} per problem; recon_err = sqrt of their ratio.
 * `batch` > 1: that many INDEPENDENT problems of one shape in every launch (blockIdx.z = problem) -- the perturbation fits of an
 * NMFk sweep (pyDNMFk.py:226-231), which the reference runs one after another.  Problem b's operands live at A + b a_stride,
 * W + b w_stride, H + b h_stride (strides in ELEMENTS, multiples of 16 bytes, each spanning at least one problem: e.g. stacked
 * [batch][m][lda] arrays) and its scratch at ws + b (ws_bytes_fit / batch); sq_out is [batch][2].  Problem b of a batched fit
 * runs the same kernels on the same operands as a fit of its own: results are bit-identical to `batch` single fits (strides
 * are ignored for batch == 1).  `ws` >= dnmf_ws_bytes_fit(m, n, k, batch).  The persistent HALS W sweep runs on as many problems
 * at a time as the device holds resident (a problem that does not fit on its own takes the column launches); `column_sweep` != 0 forces those.
 * After a HALS fit dnmf_hals_sweep_status tells whether a persistent sweep timed out.
 * SMALL MU problems (MU/KL on fp32 A; MU/FRO on fp32 or bf16-stored A; k <= 32, a 128-row slab of A -- in LDS or streamed from the L2 -- or a 64-row slab, all of H
 * and the slab's rows of W in the 160 KiB of LDS of a CU -- n up to ~2400 at k <= 16, ~1200 beyond -- and at most 64 slabs (m <= 8192): the reference's example sizes, swim 1024
 * x 256, wtsi 96 x 21) run the whole loop as ONE persistent kernel per batch (csrc/dnmf_small.h): a workgroup per slab keeps its data in
 * LDS across the steps, the problem's workgroups meet at ONE barrier per step and pass the new H as {value, step} granules (the waits of both are bounded the same way).  Same update rules, fp32 sums in another association
 * than the step kernels: results agree with dnmf_mu_{kl,fro}_step to fp32 rounding (not bit for bit); a batched fit still equals
 * `batch` single fits bit for bit.  All workgroups of a launch must be resident together (the library splits a batch into as many
 * launches as that takes; do not share the GPU with another stream meanwhile); a barrier that waits longer than 2 s gives up and
 * dnmf_hals_sweep_status reports it.  dnmf_mu_fit_persistent(m, n, k) != 0: fits of this shape take that kernel. */
size_t dnmf_ws_bytes_fit(long m, long n, int k, int batch);
int dnmf_mu_fit_persistent(long m, long n, int k);
/* != 0: dnmf_hals_fro_fit[_bf16a] with w_update != 0 and column_sweep == 0 runs fits of this shape on the persistent kernel too (A streamed
 * from the L2, fp32 or bf16-stored; the k column norms of a W sweep cross the problem's workgroups through value-as-flag slots) */
int dnmf_hals_fit_persistent(long m, long n, int k);
/* Which persistent kernel a whole fit of this shape takes and with what geometry, host arithmetic only (nothing is launched; the switch
 * dnmf_set_persistent is not consulted): the plan that a fit computes once and launches from (small_plan, csrc/dnmf_fit.hip).  method: 0 MU/FRO, 1 MU/KL, 2 HALS/FRO; bf16 != 0: A stored
 * as bfloat16 (the *_bf16a fits; refused for MU/KL); w_update as passed to the fit.
 * out = {route, KP, NW, ALDS, P, ns, cw, bf16_resident}.  route 0: none (the launch chain); 1: the barrier kernel of the method
 * (small_kl_fit_kernel / small_fro_fit_kernel, with W fixed the former at w_update = 0); 2: the W-fixed MU/KL kernel (small_kl_hfit_kernel:
 * all of W fits the LDS; no barrier); 3: the HALS kernel.  KP = 16 or 32 (k padded); NW = waves of a workgroup (slabs of 16 NW rows); ALDS != 0:
 * the slab of A lives in LDS, else it is streamed; P = workgroups per problem (slabs; route 2: 16-column tiles); ns = n rounded up to 16;
 * cw = columns of H a workgroup of the HALS kernel sweeps; bf16_resident != 0: the HALS kernel keeps the bf16 slab in LDS.  All zero behind
 * route 0.  Route 3 is what dnmf_hals_fro_fit[_bf16a] takes with column_sweep == 0; with column_sweep != 0 the fit takes the launch chain
 * whatever the query says.  Non-zero for an unknown method, bf16 with MU/KL, m or n < 1, k outside 1..32 or a null `out`. */
int dnmf_small_fit_plan(int method, int bf16, int w_update, long m, long n, int k, int out[8]);
/* Kernel launches of the persistent small fits since the library was loaded, counted on the host where a fit call has TAKEN the kernel
 * (a grid that the occupancy query finds not resident takes the launch chain instead and counts nothing): out = {small_kl_fit_kernel,
 * small_fro_fit_kernel (fp32 and bf16-stored A), small_kl_hfit_kernel, small_hals_fit_kernel}.  A batch that runs as several launches
 * counts each. */
int dnmf_small_fit_launches(unsigned long long out[4]);
/* seconds a barrier of the persistent small fit may wait before it gives up (default 2; process-wide, read at the next fit call) */
int dnmf_fit_set_timeout(double seconds);
int dnmf_mu_fro_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
                    int itr, int batch, long a_stride, long w_stride, long h_stride, double* sq_out, void* ws, size_t ws_bytes,
                    void* stream);
int dnmf_mu_kl_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
                   int itr, int batch, long a_stride, long w_stride, long h_stride, double* sq_out, void* ws, size_t ws_bytes,
                   void* stream);
int dnmf_hals_fro_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps,
                      int w_update, int itr, int column_sweep, int batch, long a_stride, long w_stride, long h_stride, double* sq_out,
                      void* ws, size_t ws_bytes, void* stream);
/* the Frobenius fits with A STORED as bfloat16 (dnmf_*_bf16a above; a_stride in bf16 elements) */
int dnmf_mu_fro_fit_bf16a(const void* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps,
                          int w_update, int itr, int batch, long a_stride, long w_stride, long h_stride, double* sq_out, void* ws,
                          size_t ws_bytes, void* stream);
int dnmf_hals_fro_fit_bf16a(const void* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps,
                            int w_update, int itr, int column_sweep, int batch, long a_stride, long w_stride, long h_stride,
                            double* sq_out, void* ws, size_t ws_bytes, void* stream);

/* ---- BCD: accelerated block coordinate descent for the Frobenius objective (method = 'bcd'; dist_nmf.py:940-1047 in 1D,
 * :474-579 in 2D, pyDNMF.py:151-152).  One update() runs `itr` iterations of: a projected-gradient W step with the Lipschitz
 * bound Lw = ||H H^T||_F, W divided by its column sums, the H step with Lh = ||W^T W||_F, the objective 1/2 ||A - W H||^2, then a
 * Nesterov extrapolation of W and H or, when the objective did not decrease, a restart from the last accepted pair.  float32
 * data and factors; rank 1 <= k <= DNMF_MAX_K.  Every scalar of the method (norms, Lipschitz bounds, t, the accept decision,
 * the extrapolation weights) lives in a device STATE BLOCK of 16 doubles `st` that these calls read and write: no call
 * returns a value to the host, so a host that sequences them (with its grid exchanges in between) never synchronises inside
 * an iteration.  The big products are the entry points above: dnmf_gram_hht / dnmf_aht (H H^T, A H^T), dnmf_wta_gram
 * (W^T A, W^T W), dnmf_resid_sqnorm_ws and dnmf_sqnorm.  The restart takes H H^T and A H^T of the last accepted H from a copy
 * kept by dnmf_bcd_extrapolate (the products are deterministic: the copy is what recomputing them would give). */
/* st from sq = {sum A^2, sum W0^2, sum H0^2} (device doubles, each summed over the ranks holding disjoint pieces):
 * obj_old = sum A^2 / 2, t_old = 1, Lw = Lh = 1 (initWandH, dist_nmf.py:947-965, :485-499) */
int dnmf_bcd_state_init(double* st, const double* sq, void* stream);
/* X_old = X_m = X0 / sqrt(sum X0^2) * sqrt(sqrt(sum A^2)) for W (which = 0) or H (which = 1) (dist_nmf.py:958-961) */
int dnmf_bcd_init_factor(const float* X0, long rows, long cols, long ld0, float* Xold, long ldo, float* Xm, long ldm, const double* st,
                         int which, void* stream);
/* L_old = L; L = ||G[:k, :k]||_F for the W bound (which = 0, G = H H^T, dist_nmf.py:998) or the H bound (which = 1, G = W^T W,
 * :1011); G is the KP x KP Gram buffer */
int dnmf_bcd_lipschitz(const float* G, int k, double* st, int which, void* stream);
/* scratch of dnmf_bcd_update_w on m rows (its column-sum partials) */
size_t dnmf_bcd_ws_bytes_w(long m, int k);
/* W = max(0, Wm - (Wm G - AHT) / Lw) for G = H H^T (KP x KP), and s[k] = the column sums of the new W over these m rows
 * (dist_nmf.py:999-1004; a host allreduces s when p_r != 1, :1006-1008).  W must not alias Wm.  ws >= dnmf_bcd_ws_bytes_w(m, k) */
int dnmf_bcd_update_w(const float* Wm, long ldwm, const float* AHT, long ldaht, const float* G, long m, int k, const double* st, float* W,
                      long ldw, float* s, void* ws, size_t ws_bytes, void* stream);
/* W[i][c] /= s[c], no eps (dist_nmf.py:1009) */
int dnmf_bcd_scale_cols(float* W, long m, int k, long ldw, const float* s, void* stream);
/* H = max(0, Hm - (G Hm - WTA) / Lh) for G = W^T W (KP x KP) (dist_nmf.py:1012-1015).  H must not alias Hm. */
int dnmf_bcd_update_h(const float* Hm, long ldhm, const float* WTA, long ldwta, const float* G, int k, long n, const double* st, float* H,
                      long ldh, void* stream);
/* the decision from sq[0] = sum (A - W H)^2 (global): obj = sq / 2, t = (1 + sqrt(1 + 4 t_old^2)) / 2; obj >= obj_old: restart,
 * else accept with ww = min((t_old - 1) / t, sqrt(Lw_old / Lw)), wh likewise, t_old = t, obj_old = obj (dist_nmf.py:1024-1047).  One lane. */
int dnmf_bcd_decide(double* st, const double* sq, void* stream);
/* the pass after the decision, one launch: accepted -> Wm = W + ww (W - W_old), W_old = W, the same for H, and AHTk / Gk keep
 * AHT / G (the products of the new H_old); restart -> Wm = W_old, Hm = H_old, AHT = AHTk, G = Gk (dist_nmf.py:1026-1047).
 * W, H are left as they are (the last iterate is what update() returns, accepted or not).  AHT / AHTk are m x k, G / Gk KP x KP. */
int dnmf_bcd_extrapolate(float* W, long ldw, float* Wold, long ldwo, float* Wm, long ldwm, long m, float* H, long ldh, float* Hold,
                         long ldho, float* Hm, long ldhm, long n, int k, float* AHT, long ldaht, float* AHTk, long ldahtk, float* G,
                         float* Gk, const double* st, void* stream);
/* workspace of dnmf_bcd_fro_fit for one problem (0 for an unsupported shape) */
size_t dnmf_bcd_ws_bytes(long m, long n, int k);
/* workspace of dnmf_bcd_fro_fit for `batch` problems: batch slices of dnmf_bcd_ws_bytes(m, n, k), slice z = problem z (0 for an
 * unsupported shape or batch < 1) */
size_t dnmf_bcd_ws_bytes_fit(long m, long n, int k, int batch);
/* A whole BCD fit on one rank (PyNMF.fit with method = 'bcd', pyDNMF.py:151-182): ONE update() of `itr` iterations, the clamp to
 * eps iff (itr - 1) % 10 == 0 (the fit's single trip has i = itr - 1), normalize_features and sq_out = {sum (A - W H)^2, sum A^2},
 * conventions of dnmf_mu_fro_fit.  w_update is ignored (the reference always updates W, dist_nmf.py:967).  batch >= 1 same-shape
 * problems, a_stride / w_stride / h_stride elements apart (ignored when batch == 1), sq_out[batch][2], ws >=
 * dnmf_bcd_ws_bytes_fit(m, n, k, batch): every launch covers all problems, each problem keeps its own state block, so the problems
 * of a batch accept or restart independently, and the results are bit-identical to fitting them one by one.  The same primitives in
 * the order a host choreography issues them: bit-identical to that sequence. */
int dnmf_bcd_fro_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
                     int itr, int batch, long a_stride, long w_stride, long h_stride, double* sq_out, void* ws, size_t ws_bytes,
                     void* stream);

/* ---- The update path in float64.  The reference computes in the dtype of A_ij (pyDNMF.py:68; its own tests feed float64,
 * tests/test_dist_nmf_1d.py:14-20): these are the float64 twins of the primitives above, on the fp64 matrix cores
 * (v_mfma_f64_16x16x4_f64), one tile shape each (0.61 / 0.72 of the fp64 MFMA peak per MU/FRO / MU/KL step at 65536 x 4096, k = 64).  Everything is `double`
 * in device memory, row-major, leading dimensions in elements; eps = 2.220446049250313e-16; k <= DNMF_TUNED_MAX_K; Gram matrices are
 * plain k x k blocks with their own leading dimension `ldg` (no padding contract).  `ws` >= dnmf_f64_ws_bytes(m, n, k) where an
 * entry point takes one.  The KL products (dnmf_f64_kl_uht / dnmf_f64_kl_wtu) keep the quotient U = A / (W H + eps) in registers up to
 * k = 64 and go through the materialised image beyond (dnmf_f64_kl_quot into an m x n buffer of the caller -- the reference materialises
 * it too, dist_nmf.py:806 -- followed by dnmf_f64_aht / dnmf_f64_wta on U); the error evaluation through the materialised squared residual (dnmf_f64_sqdiff) and the ordered sums.  Host sequencing of these
 * primitives (1D and 2D grids, exchanges over torch.distributed): pydnmfk_amd/dist_nmf.py with engine.HipOpsF64. ---- */
size_t dnmf_f64_ws_bytes(long m, long n, int k);
/* A whole float64 fit on one rank (PyNMF.fit, pyDNMF.py:138-182): `itr` steps of method 0 = MU/FRO (dist_nmf.py:716-751), 1 = MU/KL
 * (:806-849), 2 = HALS/FRO (:873-934) with the clamp after the steps i % 10 == 0, then normalize_features and the two squared norms
 * {sum (A - W H)^2, sum A^2} -> sq_out (device) -- the primitives below in the order pydnmfk_amd/dist_nmf.py issues them, enqueued by
 * ONE call (bit-identical to that step loop).  ws >= dnmf_f64_ws_bytes_fit(m, n, k): it holds the m x n quotient / residual image too. */
size_t dnmf_f64_ws_bytes_fit(long m, long n, int k);
/* != 0: a fit of this shape and method runs as ONE single-workgroup launch with A, W, H in LDS for all its steps (csrc/dnmf_f64_tiny.hip:
 * k <= 16 and everything within 160 KiB of LDS -- the reference's own test sizes, 24 x 12 with k = 2 over 2000 iterations,
 * tests/test_dist_nmf_1d.py:14-46): same update rules in plain float64 FMA chains (index-order sums: a few ulp from the primitives'
 * MFMA sums, so such a fit equals the step loop to ~1e-13, not bit for bit); no workgroup waits for another one (nothing to keep resident) */
int dnmf_f64_fit_tiny(long m, long n, int k, int method);
int dnmf_f64_fit(int method, const double* A, long m, long n, long lda, double* W, long ldw, double* H, long ldh, int k, double eps,
                 int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream);
/* C[m x kc] = X[m x n] Y[kc x n]^T   (A H^T: dist_nmf.py:730; H H^T = global_gram(H.T), :729, with X = Y = H) */
int dnmf_f64_aht(const double* X, long m, long n, long ldx, const double* Y, int kc, long ldy, double* C, long ldc, void* ws,
                 size_t ws_bytes, void* stream);
/* C[kc x n] = W[m x kc]^T A[m x n]   (W^T A: dist_nmf.py:749; W^T W = global_gram(W), :748, with A = W) */
int dnmf_f64_wta(const double* A, long m, long n, long lda, const double* W, int kc, long ldw, double* C, long ldc, void* ws,
                 size_t ws_bytes, void* stream);
/* W *= AH / (W G + eps)   (dist_nmf.py:731-732, :244-245) */
int dnmf_f64_mu_update_w(double* W, long m, int k, long ldw, const double* AH, long ldah, const double* G, long ldg, double eps,
                         void* stream);
/* H *= AtW / (G H + eps); clamp != 0: H = max(H, eps) afterwards   (dist_nmf.py:750-751, :224-225; pyDNMF.py:156) */
int dnmf_f64_mu_update_h(double* H, int k, long n, long ldh, const double* AtW, long ldatw, const double* G, long ldg, double eps,
                         int clamp, void* stream);
/* U[m x n] = A / (W H + eps)   (dist_nmf.py:806) */
int dnmf_f64_kl_quot(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps,
                     double* U, long ldu, void* stream);
/* The two KL products without the image: S[m x k] = (A / (W H + eps)) H^T (dist_nmf.py:806, :810) and S[k x n] = W^T (A / (W H + eps))
 * (:806, :808).  k <= 64: ONE pass over A each -- a wave forms a 16 x 16 tile of W H on the matrix cores, divides in registers and feeds
 * the quotient to the second product as an MFMA operand (csrc/dnmf_f64_kl.h); U may be NULL.  k > 64: dnmf_f64_kl_quot into U (m x n,
 * leading dimension n; DNMF_EINVAL if NULL) followed by dnmf_f64_aht / dnmf_f64_wta.  ws >= dnmf_f64_ws_bytes(m, n, k). */
int dnmf_f64_kl_uht(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps,
                    double* S, long lds_, double* U, void* ws, size_t ws_bytes, void* stream);
int dnmf_f64_kl_wtu(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps,
                    double* S, long lds_, double* U, void* ws, size_t ws_bytes, void* stream);
/* R[m x n] = (A - W H)^2 element-wise   (pyDNMF.py:207, :229) */
int dnmf_f64_sqdiff(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double* R,
                    long ldr, void* stream);
/* *out = sum X (sq == 0) or sum X^2 (sq != 0), fixed summation order   (np.linalg.norm(.)**2, pyDNMF.py:208,215) */
int dnmf_f64_sum(const double* X, long rows, long cols, long ldx, int sq, double* out, void* ws, size_t ws_bytes, void* stream);
/* x[c] = sum_r X[r][c] (or of squares)   (sum_along_axis(W, axis=0), dist_nmf.py:793; the column sums of column_err, pyDNMF.py:229) */
int dnmf_f64_colsum(const double* X, long m, long n, long ldx, int sq, double* x, void* ws, size_t ws_bytes, void* stream);
/* x[r] = sum_c H[r][c]   (sum_along_axis(H, axis=1), dist_nmf.py:793-795) */
int dnmf_f64_rowsum(const double* H, int k, long n, long ldh, double* x, void* stream);
/* element-wise passes.  op 0: X = max(X, eps) (pyDNMF.py:156); 1: X[r][c] /= x[c] + eps (:192); 2: X[r][c] *= x[r] (:193);
 * 3: X[r][c] *= S[r][c] / (x[r] + eps) (dist_nmf.py:847-849); 4: X[r][c] *= S[r][c] / (x[c] + eps) (:828-830); clamp != 0 (ops 3, 4):
 * max(., eps) afterwards */
int dnmf_f64_ew(int op, double* X, long rows, long cols, long ldx, const double* S, long lds_, const double* x, double eps, int clamp,
                void* stream);
/* HALS (dist_nmf.py:873-934): one column of the W sweep (as dnmf_hals_w_col; *ss2_out = this rank's sum of squares of the new
 * column, WRITTEN, not accumulated), the final scale, the H sweep */
int dnmf_f64_hals_w_col(double* W, long m, int k, long ldw, const double* AH, long ldah, const double* G, long ldg, int kk,
                        const double* prev_ss2, double eps, double* ss2_out, void* ws, size_t ws_bytes, void* stream);
int dnmf_f64_hals_w_scale(double* W, long m, long ldw, int col, const double* ss2, void* stream);
int dnmf_f64_hals_update_h(double* H, int k, long n, long ldh, const double* AtW, long ldatw, const double* G, long ldg, double eps,
                           void* stream);
/* Which kernel a float64 entry point launches for a shape, host arithmetic only (no GPU, nothing is launched): answered by the plan
 * functions the entry points themselves launch from (csrc/dnmf_f64.hip "launch plans"), so a test can assert the variant a shape reaches.
 * op (DNMF_F64_OP_*) and what m, n, k mean for it:
 *   AHT          X m x n, Y k x n (a Gram H H^T: m = k)       ld = {ldx, ldy}
 *   WTA          A m x n, W m x k (a Gram W^T W: n = k)       ld = {lda, ldw}
 *   KL_UHT, KL_WTU   A m x n at rank k                        ld = {lda, ldw, ldh}
 *   KL_QUOT, SQDIFF  the m x n image at rank k                ld = {lda, ldw, ldh, ldo}
 *   MU_UPDATE_W  W m x k (n ignored)     MU_UPDATE_H  H k x n (m ignored)
 *   SUM, COLSUM, EW  a matrix of m rows and n columns (k ignored)
 *   FIT          dnmf_f64_fit at m x n, rank k, `method` (itr >= 1)
 * `ld`: the row pitches that enter the 2 GiB descriptor-window checks, in elements; NULL or an entry <= 0: the packed pitch.  The
 * workspace is taken to be 16-byte aligned (the reduce width depends on it).  out (DNMF_F64_PLAN_*):
 *   FAMILY  DNMF_F64_FAM_*: NT = f64_nt_kernel, TN = f64_tn_kernel, KL_UHT / KL_WTU = the fused kernels of csrc/dnmf_f64_kl.h, NN_COLS =
 *           f64_nn_cols_kernel, NN_ROWS = f64_nn_rows_kernel (the W update), UPD_H = f64_upd_h_kernel, SUM / COLSUM / EW = the streaming
 *           kernels, FIT_TINY = the one-workgroup fit, FIT_CHAIN = the chain of primitives, IMAGE = a KL product that goes through the
 *           m x n image (k > 64: query KL_QUOT and AHT / WTA for its two launches), NONE = the entry point refuses the pitches
 *   NT      the template's NT (16-wide tiles of k), or KS (contraction steps of 4) for NN_COLS / NN_ROWS / UPD_H
 *   RT      row tiles per wave (NT, KL_UHT); the template's CT, column tiles per wave, for TN, KL_WTU, NN_COLS
 *   VEC, FULL  the template's flags (FULL: KL_UHT only)      D  register sets of operand loads in flight
 *   COUNT   column splits (NT, KL_UHT), row chunks (TN, KL_WTU, NN_COLS, COLSUM) or block partials (SUM)
 *   PER     columns per split / rows per chunk (the last one holds the rest)
 *   V       columns per thread of the ordered reduction that follows (2 or 1); 0: no reduction is launched
 *   GRID_X, GRID_Y  the grid of the main launch, in workgroups of 256 threads (SUM, EW: the grid-stride loop takes more than one
 *           trip when m n > 256 GRID_X); FIT: 1 x 1 for the tiny kernel, 0 for the chain
 *   WAVES   waves with work (TN, KL_WTU, NN_COLS: below 4 GRID_X the last workgroup has idle waves), else 4 GRID_X
 * Returns DNMF_EINVAL for a bad op, shape, rank, method or a null `out`. */
enum { DNMF_F64_OP_AHT = 0, DNMF_F64_OP_WTA, DNMF_F64_OP_KL_UHT, DNMF_F64_OP_KL_WTU, DNMF_F64_OP_KL_QUOT, DNMF_F64_OP_SQDIFF,
       DNMF_F64_OP_MU_UPDATE_W, DNMF_F64_OP_MU_UPDATE_H, DNMF_F64_OP_SUM, DNMF_F64_OP_COLSUM, DNMF_F64_OP_EW, DNMF_F64_OP_FIT };
enum { DNMF_F64_FAM_NONE = 0, DNMF_F64_FAM_NT, DNMF_F64_FAM_TN, DNMF_F64_FAM_KL_UHT, DNMF_F64_FAM_KL_WTU, DNMF_F64_FAM_NN_COLS,
       DNMF_F64_FAM_NN_ROWS, DNMF_F64_FAM_UPD_H, DNMF_F64_FAM_SUM, DNMF_F64_FAM_COLSUM, DNMF_F64_FAM_EW, DNMF_F64_FAM_FIT_TINY,
       DNMF_F64_FAM_FIT_CHAIN, DNMF_F64_FAM_IMAGE };
enum { DNMF_F64_PLAN_FAMILY = 0, DNMF_F64_PLAN_NT, DNMF_F64_PLAN_RT, DNMF_F64_PLAN_VEC, DNMF_F64_PLAN_FULL, DNMF_F64_PLAN_D,
       DNMF_F64_PLAN_COUNT, DNMF_F64_PLAN_PER, DNMF_F64_PLAN_V, DNMF_F64_PLAN_GRID_X, DNMF_F64_PLAN_GRID_Y, DNMF_F64_PLAN_WAVES,
       DNMF_F64_PLAN_LEN };
int dnmf_f64_plan(int op, long m, long n, int k, const long* ld, int method, long out[DNMF_F64_PLAN_LEN]);

/* Which kernel a float32 entry point of the MU/Frobenius path launches for a shape, host arithmetic only (no GPU, nothing is launched):
 * answered by the selectors the entry points themselves launch from (csrc/dnmf.hip "selectors", select_reduce of csrc/dnmf_host.h), so a
 * test can assert the variant and the loop trips a shape reaches.  bf16a != 0: the _bf16a form of the entry point (A stored as bfloat16).
 * op (DNMF_DENSE_OP_*), what m, n, k mean for it, and the operands whose pitch (`ld`, in elements; NULL or an entry <= 0: packed) and
 * address modulo 16 (`align`, in bytes; NULL: all 0) enter the choice, four entries each, in this order:
 *   AHT, AHT_HBLOCKS  A m x n, H k x n                 {A, H}       (AHT_HBLOCKS: ld[1] is the block width nh)
 *   AHT_UPDATE_W      A m x n, H k x n, W m x k        {A, H, W}    (without a bound transposed image: dnmf_wimage_plan answers for that)
 *   WTA, WTA_GRAM     A m x n, W m x k, AtW k x n      {A, W, AtW}  ws_bytes: the caller's workspace
 *   GRAM_HHT          H k x n (m ignored)              {H}
 *   GRAM_WTW          W m x k (n ignored)              {W}          ws_bytes as above
 *   MU_UPDATE_W       W, AH m x k (n ignored)          {W, AH}
 *   MU_UPDATE_H       H, AtW k x n (m ignored)         {H, AtW}
 *   EW                X m rows x n columns (k ignored) {X, S, x}    ew_op: 0 clamp_min, 1 scale_cols_div, 2 scale_rows_mul,
 *                                                                   3 kl_update_h, 4 kl_update_w
 *   KL_UHT, KL_UHT_HBLOCKS, KL_WTU   A m x n at rank k (float32)   {A, W, H, out}   ws_bytes as above (KL_UHT_HBLOCKS: ld[2] is the
 *                     block width nh)
 *   RESID_SQNORM, COLUMN_ERR   A m x n, W, H at rank k   {A, W, H}   ws_bytes (RESID_SQNORM): the workspace of the _ws form, 0 without
 *   SQNORM            A m x n (k ignored)              {A}
 * The workspace and the Gram buffers are taken to be 16-byte aligned.  out (DNMF_DENSE_PLAN_*):
 *   (KL and residual families) KL_UHT_PIPE = kl_uht_pipe_kernel on GRID_X whole 128-row tiles, EDGE = 1: kl_uht_kernel follows on the AUX
 *           ragged ones; KL_UHT = kl_uht_kernel alone; KL_WTU = kl_wtu_kernel (B0 / BL: 32-row blocks and rows left of the first / last
 *           chunk); RESID_LDS / RESID, COLERR (COUNT row chunks of PER rows per 128-column block), SQNORM (AUX: grid-stride trips);
 *           MODE = 1: the factors are first copied into zero-padded images in the workspace (pad_factors);
 *           KL16_UHT = kl_uht16_kernel (k <= 16; EDGE = 1: one split stored directly, no slabs; AUX: rows of the ragged last row tile),
 *           KL16_WTU = kl_wtu16_kernel (B0 / BL: 16-row blocks, two per trip, and rows left of the first / last chunk)
 *   FAMILY  DNMF_DENSE_FAM_*: NT16 = nt16_kernel, NT = nt_kernel, TN16 / TN16_GRAM = tn16_kernel without / with the riding Gram, TN =
 *           tn_kernel, UPDATE_W16 / UPDATE_W_SEQ / UPDATE_H_SEQ = the kernels of csrc/dnmf_update.h, EW = ew_kernel, WIDE = 128 < k <= 256: the
 *           entry point runs COUNT panel calls of PER columns of the factor (query them at k = 128 and k - 128, with the second panel's
 *           pitches and addresses: H + PER ldh, W + PER); for the ops that launch a plain kernel of csrc/dnmf_wide.hip, GRID_X, GRID_Y and
 *           BLOCK are that launch -- MU_UPDATE_W, KL_UHT, KL_WTU (the quotient U), RESID_SQNORM, COLUMN_ERR: wide_nn_rows_kernel, a wave per
 *           16-row strip, GRID_Y column ranges, AUX = 16-column tiles of a full range (the last range may have fewer, its last tile may be
 *           ragged; MU_UPDATE_W: one range over the k columns); MU_UPDATE_H: wide_upd_h_kernel, a wave per 16 columns, AUX = 16-row tiles
 *           of k; NONE = it refuses
 *           (workspace too small, a pitch beyond the 32-bit tile offsets, a shape that is neither a long-row nor a patch one)
 *   KT, FAST, MODE, PF, NT, V, EDGE, OCC   the template arguments of that name (MODE: 0 NT_STORE, 1 NT_FUSED_W; EW: 1 = the long-row form,
 *           V = 4 or 1; TN16: V = columns per lane; UPDATE_W16: the template's NWV is BLOCK / 64)
 *   NTEMP   the nontemporal flag: NTY of tn_kernel, the <.., 2, 2> form of update_h_seq_kernel, the streaming form of ew_kernel
 *   WFAST   NT_FUSED_W: W allows the vector path of the kernel's second product
 *   GRID_X, GRID_Y, BLOCK   the launch
 *   COUNT, PER   column splits and columns per split (NT), row chunks and rows per chunk (TN, TN16), tiles and rows / columns per tile
 *           (the updates)
 *   REDUCE  the reduction that follows: 0 none, 1 single stage, 2 the wide single stage, 3 two stages of SLICES slices, then one
 *   NK      NT, NT16: contraction tiles (32 columns; bf16 A: 64) of the first split; AUX: of the last split
 *   INTERIOR  NT: (row tile, split) workgroups whose tiles are all in bounds, i.e. that take an interior loop;  ELIGIBLE: those of them
 *           that take the descriptor loop of PF 10 / 13 (interior and inside the 2 GiB windows)
 *   B0_FULL, B0_TAIL, BL_FULL, BL_TAIL   TN, TN16: full register batches (8 rows; TN16: 16) of the pipelined loop and rows left to the
 *           predicated tail loop, for the first and for the last row chunk (a tn_kernel that is not FAST has no batches)
 *   AUX     the updates: trips of the grid-stride tile loop of the busiest wave; EW patch form: log2 of the threads along a row
 * Returns DNMF_EINVAL for a bad op, shape, rank, H layout or a null `out`. */
enum { DNMF_DENSE_OP_AHT = 0, DNMF_DENSE_OP_AHT_HBLOCKS, DNMF_DENSE_OP_AHT_UPDATE_W, DNMF_DENSE_OP_WTA, DNMF_DENSE_OP_WTA_GRAM,
       DNMF_DENSE_OP_GRAM_HHT, DNMF_DENSE_OP_GRAM_WTW, DNMF_DENSE_OP_MU_UPDATE_W, DNMF_DENSE_OP_MU_UPDATE_H, DNMF_DENSE_OP_EW,
       DNMF_DENSE_OP_KL_UHT, DNMF_DENSE_OP_KL_UHT_HBLOCKS, DNMF_DENSE_OP_KL_WTU, DNMF_DENSE_OP_RESID_SQNORM, DNMF_DENSE_OP_COLUMN_ERR,
       DNMF_DENSE_OP_SQNORM };
enum { DNMF_DENSE_FAM_NONE = 0, DNMF_DENSE_FAM_NT16, DNMF_DENSE_FAM_NT, DNMF_DENSE_FAM_TN16, DNMF_DENSE_FAM_TN16_GRAM, DNMF_DENSE_FAM_TN,
       DNMF_DENSE_FAM_UPDATE_W16, DNMF_DENSE_FAM_UPDATE_W_SEQ, DNMF_DENSE_FAM_UPDATE_H_SEQ, DNMF_DENSE_FAM_EW, DNMF_DENSE_FAM_WIDE,
       DNMF_DENSE_FAM_KL_UHT_PIPE, DNMF_DENSE_FAM_KL_UHT, DNMF_DENSE_FAM_KL_WTU, DNMF_DENSE_FAM_RESID_LDS, DNMF_DENSE_FAM_RESID,
       DNMF_DENSE_FAM_COLERR, DNMF_DENSE_FAM_SQNORM, DNMF_DENSE_FAM_KL16_UHT, DNMF_DENSE_FAM_KL16_WTU };
enum { DNMF_DENSE_PLAN_FAMILY = 0, DNMF_DENSE_PLAN_KT, DNMF_DENSE_PLAN_FAST, DNMF_DENSE_PLAN_MODE, DNMF_DENSE_PLAN_PF, DNMF_DENSE_PLAN_NT,
       DNMF_DENSE_PLAN_V, DNMF_DENSE_PLAN_EDGE, DNMF_DENSE_PLAN_OCC, DNMF_DENSE_PLAN_NTEMP, DNMF_DENSE_PLAN_WFAST, DNMF_DENSE_PLAN_GRID_X,
       DNMF_DENSE_PLAN_GRID_Y, DNMF_DENSE_PLAN_BLOCK, DNMF_DENSE_PLAN_COUNT, DNMF_DENSE_PLAN_PER, DNMF_DENSE_PLAN_REDUCE,
       DNMF_DENSE_PLAN_SLICES, DNMF_DENSE_PLAN_NK, DNMF_DENSE_PLAN_INTERIOR, DNMF_DENSE_PLAN_ELIGIBLE, DNMF_DENSE_PLAN_B0_FULL,
       DNMF_DENSE_PLAN_B0_TAIL, DNMF_DENSE_PLAN_BL_FULL, DNMF_DENSE_PLAN_BL_TAIL, DNMF_DENSE_PLAN_AUX, DNMF_DENSE_PLAN_LEN };
int dnmf_dense_plan(int op, int bf16a, long m, long n, int k, const long* ld, const int* align, size_t ws_bytes, int ew_op,
                    long out[DNMF_DENSE_PLAN_LEN]);
/* Every variant those selectors can return, from the selectors themselves (each is called over its whole discrete input domain): rows of
 * DNMF_DENSE_VARIANT_LEN values {FAMILY, KT, FAST, MODE, PF, NT, V, EDGE, NTEMP, bf16a} as dnmf_dense_plan reports them; rows repeat.
 * Returns the number of rows; at most `cap` of them are written to `rows` (NULL: count only). */
enum { DNMF_DENSE_VARIANT_LEN = 10 };
int dnmf_dense_plan_variants(long* rows, int cap);

/* ---- Grid exchanges inside the library (RCCL over xGMI; replaces MPI_comm, dist_comm.py:16-56, and the mpi4py calls of
 * global_gram / global_mm, dist_nmf.py:681,707).  RCCL is bound at run time (dlopen; an RCCL already in the process -- the
 * PyTorch host's -- is preferred), so the library loads without it; these entry points then return DNMF_ECOMM.
 * One communicator handle per rank (= per process = per GPU; the current HIP device at dnmf_comm_create is the rank's GPU).
 * Rank r sits at grid coordinates (i, j) = (r / p_c, r % p_c), the reference's Create_cart(reorder=False). ---- */
#define DNMF_UNIQUE_ID_BYTES 128
typedef struct dnmf_comm dnmf_comm_t;
/* rank 0: fill 128 bytes that every rank must pass to dnmf_comm_create (the host broadcasts them: mpi4py bcast,
 * torch.distributed broadcast_object_list, a file ...) */
int dnmf_comm_unique_id(void* id_out);
/* collective over all nranks processes; p_r * p_c == nranks; 2D grids also get the two sub-communicators
 * (cart_1d_row = the p_r ranks of one grid column, cart_1d_column = the p_c ranks of one grid row, dist_comm.py:25-51) */
int dnmf_comm_create(const void* unique_id, int nranks, int rank, int p_r, int p_c, dnmf_comm_t** out);
/* A communicator whose collectives the HOST performs (no RCCL in the process, or a transport of the host's own -- a GPU-aware
 * MPI under the reference's mpi4py driver; the multi-rank tests of this repository drive it with gloo):
 * every exchange of the step entry points calls fn(user, op, group, send, recv, count, stream) on the calling thread.
 *   op    DNMF_ALLREDUCE       recv == send: in-place SUM of `count` floats over the group (dist_nmf.py:114, :681, :707);
 *         DNMF_ALLREDUCE_F64 the same on doubles (the HALS steps only)
 *         DNMF_ALLGATHER       recv[q * count ...] = member q's `count` floats, members in group order (:163-165, :195-197)
 *         DNMF_REDUCE_SCATTER  send = members x count floats; recv = this member's block of the SUM (:169-171, :202)
 *   group 0 = all ranks, 1 = cart_1d_row (the p_r ranks of a grid column, ordered by grid row), 2 = cart_1d_column (the p_c
 *         ranks of a grid row, ordered by grid column) -- dist_comm.py:16-56; groups of one member are never passed
 *   send / recv are DEVICE pointers; everything enqueued on `stream` before the call produces `send`, everything enqueued
 *   after it consumes `recv`: the function either enqueues its transfer on `stream` or synchronises it, moves the data and
 *   returns when `recv` is complete.  Return 0, or non-zero to fail the step (DNMF_ECOMM). */
#define DNMF_ALLREDUCE 0
#define DNMF_ALLGATHER 1
#define DNMF_REDUCE_SCATTER 2
#define DNMF_ALLREDUCE_F64 3   /* as DNMF_ALLREDUCE on `count` DOUBLES (send / recv point to doubles): the HALS column norms */
/* send / recv are untyped: the element type is the op's (float32 for ops 0-2, float64 for DNMF_ALLREDUCE_F64) */
typedef int (*dnmf_collective_fn)(void* user, int op, int group, const void* send, void* recv, size_t count, void* stream);
int dnmf_comm_create_hosted(int nranks, int rank, int p_r, int p_c, dnmf_collective_fn fn, void* user, dnmf_comm_t** comm);
/* MEASUREMENT aid (bench.py --emulate-ranks, a one-GPU box): member `rank` of a p_r x p_c grid whose collectives are all issued
 * for real on a ONE-rank RCCL communicator -- launch and stream-ordering costs without a wire, buffers of the real grid's sizes.
 * The step entry points run as on the grid; the numbers they produce are not a factorisation of anything. */
int dnmf_comm_create_emulated(int p_r, int p_c, int rank, dnmf_comm_t** comm);
/* the RCCL this library bound at run time: *version = ncclGetVersion's code (e.g. 22604; 0 if the symbol is absent), `origin` =
 * how it was found ("already in the process" = the host framework's copy, or the library name that was loaded).  For run records. */
int dnmf_comm_rccl_version(int* version, char* origin, size_t origin_bytes);
/* ---- direct (two-shot) allreduce over IPC peer buffers -- an alternative to RCCL's ring for the small packed message of a 1D
 * step (2 MiB at BASELINE config 3; SURVEY section 5 "measure both").  Every rank exports a region of device memory, the host
 * moves the 64-byte handles (allgather over whatever it has), every rank maps its peers' regions.  One node, at most
 * DNMF_DIRECT_MAX_RANKS ranks, messages of an even number of floats.  Rank-ordered sums with one owner per element: every rank
 * ends with identical bits.  Works on RCCL and on hosted communicators alike (it needs neither). ---- */
#define DNMF_DIRECT_MAX_RANKS 16
#define DNMF_DIRECT_HANDLE_BYTES 80
/* allocate this rank's region (uncached device memory; DNMF_EHIP when the device has none to give -- there is no cached
 * fall-back) for messages of up to max_floats floats; handle_out receives DNMF_DIRECT_HANDLE_BYTES bytes (the IPC handle and the
 * region's capacity).  EVERY rank must pass the same max_floats: peers address each other's regions with one capacity. */
int dnmf_comm_direct_init(dnmf_comm_t* comm, size_t max_floats, void* handle_out);
/* handles = nranks x DNMF_DIRECT_HANDLE_BYTES bytes in rank order; DNMF_EINVAL when any rank's capacity differs from this rank's
 * (every rank sees every entry, so a mismatch fails the call on all of them) */
int dnmf_comm_direct_connect(dnmf_comm_t* comm, const void* handles);
/* undo init / connect (a set-up that failed on some rank): device synchronise, unmap the peers, free the own region.  The host
 * makes sure no peer is still reading this rank's region (a barrier); dnmf_comm_destroy does the same unmapping */
int dnmf_comm_direct_teardown(dnmf_comm_t* comm);
/* how long a wait of a direct allreduce may see no progress before it gives up (default 30 s; rank skew of seconds is ordinary:
 * result I/O on rank 0, first-call module loads) */
int dnmf_comm_set_direct_timeout(dnmf_comm_t* comm, double seconds);
/* Call on EVERY rank before the first step of a fit on new data (PyNMF.fit does): the next HALS W sweep over the ranks then agrees anew
 * on whether the one-launch cross-rank sweep applies (a host-synchronous 16-float allreduce).  The ranks re-open that agreement only at
 * events all of them see -- this call, another k, dnmf_set_persistent -- because a rank's local row count may change on some ranks only;
 * a step whose local row count differs from the agreed one without this call returns DNMF_EINVAL. */
int dnmf_comm_fit_begin(dnmf_comm_t* comm);
/* on != 0: allreduces over ALL ranks that fit the regions (the packed exchange of the 1D steps, dnmf_comm_allreduce with
 * group 0) take the direct path; everything else stays on RCCL / the hosted function */
int dnmf_comm_set_direct(dnmf_comm_t* comm, int on);
/* With the direct path on, the W sweep of the HALS steps on grids whose W rows are spread over ranks (p_r > 1; every 2D grid) is ONE
 * persistent launch instead of k column launches + k allreduces: every workgroup publishes its column partial into its slot of every
 * rank's slab (two 1 MiB slabs by sweep parity live in the exported regions), polls its own rank's slab and sums all ranks' slots in
 * slot order -- identical bits on every rank (csrc/dnmf_hals.h, HalsPeers).  Taken when EVERY rank can keep its rows resident (the
 * ranks agree once per shape through a 16-float allreduce; otherwise all of them keep the column launches).  A peer that stalls
 * longer than the direct time-out sets the sticky word dnmf_hals_sweep_status reports.  *count = such sweeps issued so far. */
int dnmf_comm_hals_xsweeps(dnmf_comm_t* comm, unsigned long long* count);
/* in-place SUM allreduce of `count` floats over all ranks through the peer regions, on `stream` */
int dnmf_comm_allreduce_direct(dnmf_comm_t* comm, float* buf, size_t count, void* stream);
/* the ONE-launch form for 1..8 doubles (the column norms of the HALS W sweep: k dependent 8-byte allreduces per iteration on
 * p_r > 1, pure latency): every rank pushes its values into its peers' regions, sums in rank order.  With dnmf_comm_set_direct
 * the HALS step entry points use it for their norm exchanges. */
int dnmf_comm_allreduce_direct_f64(dnmf_comm_t* comm, double* buf, size_t count, void* stream);
/* *timed_out != 0: a wait of a direct allreduce saw no progress for the time-out and gave up (a peer is gone): every result since
 * is INVALID.  Sticky.  Callers check it where they synchronise anyway -- PyNMF.fit at the end of a fit, all ranks agreeing on the
 * outcome before they raise -- and treat it as fatal. */
int dnmf_comm_direct_status(dnmf_comm_t* comm, int* timed_out);
int dnmf_comm_destroy(dnmf_comm_t* comm);
int dnmf_comm_info(const dnmf_comm_t* comm, int* nranks, int* rank, int* p_r, int* p_c);
/* column chunks of the overlapped H phase of dnmf_mu_fro_step_1d on a row grid (1 = one packed allreduce; <= 8) */
int dnmf_comm_set_overlap_chunks(dnmf_comm_t* comm, int chunks);
/* testing aid: with on != 0 a ONE-rank communicator still issues its RCCL calls (a 1 x 1 grid then behaves as a row grid),
 * so that the exchange path can be exercised on a single GPU */
int dnmf_comm_set_always_exchange(dnmf_comm_t* comm, int on);
/* measurement aid: with on != 0 the step entry points skip their RCCL calls (everything else -- kernels, events, the internal
 * stream -- as usual), so a rank's compute can be timed without the exchange; results are WRONG on more than one rank */
int dnmf_comm_set_null_exchange(dnmf_comm_t* comm, int on);
/* in-place SUM allreduce of `count` floats on `stream`; group 0 = all ranks, 1 = cart_1d_row, 2 = cart_1d_column
 * (comm.allreduce of dist_nmf.py:114,681,707 and the host's scalar reductions) */
int dnmf_comm_allreduce(dnmf_comm_t* comm, float* buf, size_t count, int group, void* stream);
/* workspace of the two 1D steps below for a rank holding an m_l x n_l block (kernel scratch + the packed exchange buffers) */
size_t dnmf_ws_bytes_1d(long m_l, long n_l, int k);
/* One whole MU / Frobenius step of one rank of a 1D grid, exchanges included (nmf_algorithms_1D.update, dist_nmf.py:755-771
 * with global_gram / global_mm :663-708): p_c == 1 (A, W row blocks; H replicated): fused W phase, then ONE allreduce of the
 * packed [W^T A | W^T W] message (or overlapped column chunks, see dnmf_comm_set_overlap_chunks); p_r == 1: the mirror
 * image with [A H^T | H H^T].  Everything is enqueued on `stream` (the chunked exchange on an internal stream, ordered by
 * events); the call returns without synchronising.  Same arithmetic as the per-kernel entry points called in that order. */
int dnmf_mu_fro_step_1d(const float* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k,
                        float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* comm, void* stream);
/* The same for MU / KL (dist_nmf.py:851-869 with sum_along_axis / glob_UX :776-811): [U H^T | rowsum H] is reduced when
 * p_r == 1, [W^T U | colsum W] when p_c == 1. */
int dnmf_mu_kl_step_1d(const float* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k,
                       float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* comm, void* stream);

/* The 2D grid (p_r > 1 and p_c > 1; nmf_algorithms_2D.update, dist_nmf.py:66-91).  The rank at grid position (i, j) = rank / p_c,
 * rank % p_c holds A_ij (m_l x n_l), the slice W_ij (m_w x k, contiguous: ldw == k) of its grid row's W_i and the slice H_ij
 * (k x n_h, contiguous: ldh == n_h) of its grid column's H_j; the slice sizes follow the reference's partition rule (utils.py:36-41:
 * of p members the first total % p hold one item more), m_w of m_l over the p_c ranks of the grid row, n_h of n_l over the p_r
 * ranks of the grid column -- anything else returns DNMF_EINVAL (pruned factors: the host keeps its choreography).  Exchanges:
 * allreduce of the Gram matrix / the factor sums over all ranks (:114, :346-349), allgather of H_ij over the p_r ranks of a grid
 * column and of W_ij over the p_c ranks of a grid row (:163-165, :195-197, :268-291), reduce-scatter of the products back to the
 * slices (:169-171, :202, :314-316, :340) -- all enqueued on `stream`, no host synchronisation.  Equal slices of whole
 * 32-column tiles: the kernels read the gathered H as column blocks and the H-phase product is formed slice by slice into the
 * reduce-scatter's send buffer (nothing is re-assembled); ragged slices (a dimension that does not divide: real data) are
 * exchanged at the pitch of the largest one, as MPI's Allgatherv / Reduce_scatter counts do, and H_j / W_i are assembled by
 * device copies. */
size_t dnmf_ws_bytes_2d(long m_l, long n_l, int k, int p_r, int p_c);
/* Fro_MU_update on the 2D grid (dist_nmf.py:207-263 with global_gram :107-117, AH_glob :186-205, ATW_glob :154-172) */
int dnmf_mu_fro_step_2d(const float* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh,
                        int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* comm, void* stream);
/* KL_MU_update on the 2D grid (dist_nmf.py:351-407 with sum_axis :346-349, gather_W_H :268-291, UHT_glob :330-343, WTU_glob :294-318) */
int dnmf_mu_kl_step_2d(const float* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh,
                       int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* comm, void* stream);

/* HALS / Frobenius steps with the exchanges inside (FRO_HALS_update, dist_nmf.py:873-934 on 1D grids, :411-470 on the 2D grid):
 * products and Gram matrices exchanged as in the MU steps above; the W sweep column by column -- where W's rows are spread over
 * ranks (p_r > 1, and every 2D grid) the 8-byte sum of squares of each column is allreduced between the column kernels
 * (utils.norm, utils.py:388-391); with local norms (1D, p_r == 1) it is dnmf_hals_sweep_w, or k column launches when
 * `column_sweep` != 0 -- then the H sweep; `clamp` != 0: H = max(H, eps), W = max(W, eps) afterwards (pyDNMF.py:170-172).
 * Workspaces: dnmf_ws_bytes_1d / dnmf_ws_bytes_2d. */
int dnmf_hals_fro_step_1d(const float* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k,
                          float eps, int w_update, int clamp, int column_sweep, void* ws, size_t ws_bytes, dnmf_comm_t* comm,
                          void* stream);
int dnmf_hals_fro_step_2d(const float* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh,
                          int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* comm, void* stream);

/* The Frobenius steps above with A STORED as bfloat16 (dnmf_*_bf16a: `A` points to 16-bit words, lda in elements; BASELINE config
 * 5's "mixed precision"): same arguments, same exchanges; on the 2D grid H_j is always assembled (the column-block form of A H^T
 * exists for fp32 A only). */
int dnmf_mu_fro_step_1d_bf16a(const void* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k,
                              float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* comm, void* stream);
int dnmf_mu_fro_step_2d_bf16a(const void* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh,
                              int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* comm, void* stream);
int dnmf_hals_fro_step_1d_bf16a(const void* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k,
                                float eps, int w_update, int clamp, int column_sweep, void* ws, size_t ws_bytes, dnmf_comm_t* comm,
                                void* stream);
int dnmf_hals_fro_step_2d_bf16a(const void* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh,
                                int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* comm, void* stream);

/* ---- Sparse data: the block as CSR (no counterpart in the reference, whose data block is a dense numpy array) ----
 * The one exception to "every matrix is dense" above.  A block of m x n with nnz stored entries is handed over as TWO CSR
 * images in device memory, both built once by the caller: the block itself (row pointers int32 [m + 1], column indices int32
 * [nnz], values float32 [nnz]) and its transpose (row pointers [n + 1], the ROW indices of the block as its column indices,
 * the values in that order).  Layout contract: nnz < 2^31, m, n < 2^31, indices in range, column indices strictly increasing
 * inside a row (no duplicates), no stored zeros needed.  An update rule touches A only through products in which a zero of
 * A contributes exactly zero (dist_nmf.py:705 via :730, :749, :883, :902; the KL quotient :806-810 is zero wherever A is), so a
 * sparse step is the dense step on the densified block up to summation order; the k x k work, the update kernels, Gram
 * matrices, clamps and normalisation are the dense entry points above, which never see A.
 * Factors enter these kernels as PACKED images [rows x KPAD], KPAD = dnmf_csr_kpad(k) = 16 / 32 / 64 / 128 / 256 floats, zero
 * padded and 16-byte aligned (dnmf_csr_pack): a gathered row is one float4 per lane whatever k is.
 * Rows with more than dnmf_csr_seg() stored entries ("long rows") are named by the caller, once per image: `long_rows`
 * [n_long] (ascending row numbers) and `long_segptr` [n_long + 1] (running count of their segments of dnmf_csr_seg() entries,
 * long_segptr[0] = 0, long_segptr[n_long] = nseg); such a row is computed segment by segment and its partial rows are added in
 * segment order.  n_long = 0: both may be NULL.  No sum is formed with atomics: results are bit-reproducible.
 * `ws`: dnmf_csr_ws_bytes(m, n, k, nseg) bytes (the larger nseg of the two images), 16-byte aligned. */
int dnmf_csr_kpad(int k);
int dnmf_csr_seg(void);
size_t dnmf_csr_ws_bytes(long m, long n, int k, int nseg);
/* P = the packed image of a factor.  transpose == 0: X is [rows x cols], cols = k (W): P[rows x KPAD].  transpose != 0: X is
 * [rows x cols], rows = k (H): P[cols x KPAD] = X^T.  (H_j.T of dist_nmf.py:730, materialised.) */
int dnmf_csr_pack(const float* X, long rows, long cols, long ldx, int transpose, float* P, void* stream);
/* out[r][0:k] = sum over the stored entries p of row r of val[p] * Fp[col[p]][0:k].  On the block's CSR with Fp = packed H^T:
 * A H^T [m x k] (global_mm(A_ij, H_j.T), dist_nmf.py:730, :883).  On the transpose's CSR with Fp = packed W and out_trans != 0
 * (out[c][r], ldo >= rows): W^T A [k x n] (global_mm(W_i.T, A_ij), :749, :902).  Empty rows give exact zeros. */
int dnmf_csr_mm(const int* rowptr, const int* col, const float* val, long rows, const float* Fp, int k, float* out, long ldo,
                int out_trans, const int* long_rows, const int* long_segptr, int n_long, int nseg, void* ws, size_t ws_bytes,
                void* stream);
/* The KL products with the quotient fused (dist_nmf.py:806-810): per stored entry d = <Lp[r], Fp[col[p]]>, q = val[p] / (d + eps),
 * out[r] += q * Fp[col[p]].  Block's CSR, Lp = packed W, Fp = packed H^T: U H^T [m x k] (:810).  Transpose's CSR, Lp = packed
 * H^T, Fp = packed W, out_trans != 0: W^T U [k x n] (:808). */
int dnmf_csr_kl_mm(const int* rowptr, const int* col, const float* val, long rows, const float* Lp, const float* Fp, int k,
                   float eps, float* out, long ldo, int out_trans, const int* long_rows, const int* long_segptr, int n_long,
                   int nseg, void* ws, size_t ws_bytes, void* stream);
/* sq[0] = ||A - W H||_F^2 (pyDNMF.py:205-218) without a dense image: sum over the stored entries of a (a - 2 d), d = <W[i], H[:, j]>,
 * plus <W^T W, H H^T> (= ||W H||^2 over ALL entries).  The two terms cancel when the fit is good, so d, the stored-entry sum, both
 * Gram matrices and their contraction are float64.  Block's CSR, Wp = packed W [m x KPAD], HTp = packed H^T [n x KPAD]. */
int dnmf_csr_resid_sqnorm(const int* rowptr, const int* col, const float* val, long m, long n, const float* Wp, const float* HTp,
                          int k, const int* long_rows, const int* long_segptr, int n_long, int nseg, double* sq, void* ws,
                          size_t ws_bytes, void* stream);

/* ---- A sparse block whose UNSTORED entries are MISSING (not observed; no reference counterpart: the reference's rules with every sum
 * restricted to the stored positions Omega of the block).  A stored zero is an observation.  Objective 'fro': sum over Omega of
 * (a - (W H))^2; 'kl': the quotient rule with both sums over Omega.  With d = <Lp[r], Fp[col[p]]> formed per stored entry p of row r:
 *     kl == 0:  num[r] = sum_p val[p] Fp[col[p]]             den[r] = sum_p d Fp[col[p]]       (A H^T and P_Omega(W H) H^T)
 *     kl != 0:  num[r] = sum_p val[p] / (d + eps) Fp[col[p]]   den[r] = sum_p Fp[col[p]]
 * On the block's CSR with Lp = packed W, Fp = packed H^T these are the two sides of the W rule (dist_nmf.py:729-732, KL :806-810 and
 * :827-830); on the transpose's CSR with Lp = packed H^T, Fp = packed W and out_trans != 0, of the H rule (:748-751, KL :846-849).  On a
 * fully stored block they are the reference's rules up to summation order.  Rows without a stored entry give exact zeros.  Same CSR,
 * packed-image and long-row arguments as dnmf_csr_kl_mm; no atomics: bit-reproducible.
 * `ws`: dnmf_csr_masked_ws_bytes(m, n, k, nseg) bytes (the larger nseg of the two images; long rows leave PAIRS of partial rows). */
size_t dnmf_csr_masked_ws_bytes(long m, long n, int k, int nseg);
/* the pair stored: num and den [rows x k] (out_trans != 0: [k x rows]) with the same leading dimension ldo -- the two halves of one
 * contiguous buffer where the sums cross ranks (one allreduce, then dnmf_csr_ratio_update) */
int dnmf_csr_masked_mm(const int* rowptr, const int* col, const float* val, long rows, const float* Lp, const float* Fp, int k,
                       float eps, int kl, float* num, float* den, long ldo, int out_trans, const int* long_rows,
                       const int* long_segptr, int n_long, int nseg, void* ws, size_t ws_bytes, void* stream);
/* the pair applied where nothing crosses ranks: X[r] = Lp[r] * num[r] / (den[r] + eps), max(., eps) if clamp != 0 (pyDNMF.py:170-172).
 * X is the factor itself (W [rows x k], or H [k x rows] with out_trans != 0) and Lp its packed copy: X is written, never read. */
int dnmf_csr_masked_update(const int* rowptr, const int* col, const float* val, long rows, const float* Lp, const float* Fp, int k,
                           float eps, int kl, int clamp, float* X, long ldx, int out_trans, const int* long_rows,
                           const int* long_segptr, int n_long, int nseg, void* ws, size_t ws_bytes, void* stream);
/* X <- X * num / (den + eps), max(., eps) if clamp != 0: the multiply-divide of dist_nmf.py:731-732, :750-751, :828-830, :847-849 on a
 * summed pair.  X [rows x cols], ldx; num, den [rows x cols], ldp. */
int dnmf_csr_ratio_update(float* X, long rows, long cols, long ldx, const float* num, const float* den, long ldp, float eps,
                          int clamp, void* stream);
/* sq[0] = ||P_Omega(A - W H)||_F^2 (pyDNMF.py:205-218 over the stored positions): sum of (a - d)^2 with d and the sum in float64, a
 * fixed number of waves and one workgroup adding their partials in a fixed order.  Block's CSR, Wp = packed W, HTp = packed H^T. */
int dnmf_csr_masked_resid_sqnorm(const int* rowptr, const int* col, const float* val, long m, long n, const float* Wp,
                                 const float* HTp, int k, const int* long_rows, const int* long_segptr, int n_long, int nseg,
                                 double* sq, void* ws, size_t ws_bytes, void* stream);

/* ---- NMFk on a sparse block: the perturbed copy and the per-column error ----
 * val_out[p] = val[p] * (1 + nv + 2 nv u) (pyDNMFk.py:42-44) on ONE CSR image of the block.  u is the uniform dnmf_perturb_uniform
 * gives the entry's position in the DENSE block: linear index L = r * ncols + c, the splitmix64 finaliser of (seed, L >> 1), its high
 * 24 bits for even L and its low 24 bits for odd L -- so the result equals dnmf_perturb_uniform on the densified block at the stored
 * positions, bit for bit, and depends on (seed, position) only.  transposed == 0: the block's own image (row index r, column index
 * c).  transposed != 0: the transpose's image (its row index is c, its column index r; rows must equal ncols); the two outputs
 * describe the same matrix.  `ncols`: the dense block's column count.  Rows of any length; no workspace. */
int dnmf_csr_perturb_uniform(const int* rowptr, const int* col, const float* val, long rows, long ncols, int transposed,
                             float noise_var, unsigned long long seed, float* val_out, void* stream);
/* num[c], den[c] (float64, c < rows) of pyDNMF.py:221-239 (`column_err`) over this rank's rows, from the TRANSPOSE's image: rows = the
 * block's column count n, cols = its row count m, Lp = packed H^T [n x KPAD], Fp = packed W [m x KPAD]; d = <H^T[c], W[r]> in float64.
 *     masked == 0:  num[c] = sum_stored a (a - 2 d) + h_c^T (W^T W) h_c,  den[c] = sum_stored a^2   (W^T W: this rank's float64 Gram
 *                   matrix, partials added in a fixed order, read through L2)
 *     masked != 0:  num[c] = sum_stored (a - d)^2,                        den[c] = sum_stored a^2   (missing='unstored')
 * A column without a stored entry gives den = 0 and num = the Gram term (masked: 0).  Long rows of the image go through segment
 * partials added in segment order; no atomics: bit-reproducible.
 * `ws`: dnmf_csr_column_err_ws_bytes(n, m, k, masked, nseg) bytes (nseg of the transpose's image), 16-byte aligned. */
size_t dnmf_csr_column_err_ws_bytes(long rows, long cols, int k, int masked, int nseg);
int dnmf_csr_column_err(const int* rowptr, const int* col, const float* val, long rows, long cols, const float* Lp, const float* Fp,
                        int k, int masked, const int* long_rows, const int* long_segptr, int n_long, int nseg, double* num,
                        double* den, void* ws, size_t ws_bytes, void* stream);

/* ---- dense data with missing entries: NaN = not observed (csrc/dnmf_masked.h) ----
 * A [m x n] (lda) is float32 and stays as handed over; an entry is observed iff it is not NaN (a zero is an observation) -- there is no
 * mask array.  With Omega the observed positions, S = W H and F = H^T (W side) or W (H side), the masked MU rules are pairs
 *     kl == 0:  num = P_Omega(A) F,              den = P_Omega(S) F       dist_nmf.py:729-732 (W), :748-751 (H), sums over Omega
 *     kl != 0:  num = P_Omega(A / (S + eps)) F,  den = P_Omega(1) F       dist_nmf.py:806-810 (the quotient), :827-849 (the rules)
 * formed tile by tile on the matrix cores: S in accumulators, one compare and two selects per element, two second products.  On a block
 * without a NaN they are the reference's rules up to summation order.  A row (column) without an observation gives exact zeros in
 * both halves.  1 <= k <= DNMF_TUNED_MAX_K; any shape and any leading dimensions (NaN in the padding is never read as data).  Partial
 * sums are added in a fixed order, no float atomics: bit-reproducible.
 * `ws`: dnmf_masked_ws_bytes(m, n, k) bytes, 16-byte aligned (0: bad shape or rank). */
size_t dnmf_masked_ws_bytes(long m, long n, int k);
/* The launch plans for an m x n block at rank k, host arithmetic only (nothing is launched): out = {tiles_per_split, nsplit, zdim,
 * rowblks_per_chunk, nchunks, nrowblk}.  W side: nsplit column splits of tiles_per_split 32-column tiles each (the last split holds
 * the rest), zdim halves of the output columns; its partial slabs take nsplit * 2 * m * KP floats.  H side: nrowblk 32-row blocks in
 * nchunks chunks of rowblks_per_chunk (the last chunk holds the rest); its slabs take nchunks * 2 * KP * ldp floats, ldp = n rounded
 * up to the column block of 4096 / KP columns.  KP = dnmf_kp(k).  Non-zero for an unsupported k, m or n < 1, or a null `out`. */
int dnmf_masked_plan(long m, long n, int k, long out[6]);
/* Workgroups (of 256 threads, one output element per thread and grid-stride trip) of the ending that adds the partial slabs, for a
 * rows x cols output: m x k on the W side, k x n on the H side.  Host arithmetic only; 0 for rows or cols < 1. */
long dnmf_masked_reduce_grid(long rows, long cols);
/* the pair stored: num, den [m x k] (W side) or [k x n] (H side) with the same leading dimension ldo -- the two halves of one contiguous
 * buffer where the sums cross ranks (one allreduce, then dnmf_csr_ratio_update) */
int dnmf_masked_aht_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                         int kl, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream);
int dnmf_masked_wta_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                         int kl, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream);
/* the pair applied where nothing crosses ranks: W <- W * num / (den + eps) (dist_nmf.py:731-732, :828-830), H alike (:750-751,
 * :847-849) with max(., eps) if clamp != 0 (pyDNMF.py:170-172); the factor is updated in place after the pass has read it */
int dnmf_masked_update_w(const float* A, long m, long n, long lda, float* W, long ldw, const float* H, long ldh, int k, float eps, int kl,
                         void* ws, size_t ws_bytes, void* stream);
int dnmf_masked_update_h(const float* A, long m, long n, long lda, const float* W, long ldw, float* H, long ldh, int k, float eps, int kl,
                         int clamp, void* ws, size_t ws_bytes, void* stream);
/* sq[0] = ||P_Omega(A - W H)||_F^2 (pyDNMF.py:205-218 over the observed positions), float64 (summed like dnmf_resid_sqnorm) */
int dnmf_masked_resid_sqnorm(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                             double* sq, void* stream);
/* out[0] = ||P_Omega(A)||_F^2, out[1] = |Omega| (the count of observed entries), both float64 */
int dnmf_masked_sqnorm(const float* A, long m, long n, long lda, double* out, void* stream);
/* num[c] = sum_{i: (i,c) in Omega} (a - S)^2, den[c] = sum_{i: (i,c) in Omega} a^2 (float64, c < n) over this rank's rows: the pieces of
 * PyNMF.column_err (pyDNMF.py:221-239) with both sums over the observed positions.  The S tile stays in MFMA accumulators; fp32 per
 * 16-row tile, float64 from there on.  Every row chunk leaves one float64 pair per column in `ws`; an ending adds them in chunk order
 * and STORES num, den (nothing is accumulated into them, no atomics: two calls are bit-identical).  A column without an observation
 * gives exactly (0, 0).  1 <= k <= DNMF_TUNED_MAX_K; any shape and any leading dimensions.
 * `ws`: dnmf_masked_column_err_ws_bytes(m, n, k) bytes, 16-byte aligned (0: bad shape or rank). */
size_t dnmf_masked_column_err_ws_bytes(long m, long n, int k);
/* Its launch plan, host arithmetic only: out = {rowblks_per_chunk, nchunks, ncolblk} -- nchunks chunks of rowblks_per_chunk 32-row
 * blocks (the last chunk holds the rest), ncolblk blocks of 128 columns; the slab takes nchunks * 2 * ncolblk * 128 doubles. */
int dnmf_masked_column_err_plan(long m, long n, int k, long out[3]);
int dnmf_masked_column_err(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, double* num,
                           double* den, void* ws, size_t ws_bytes, void* stream);
/* A whole masked MU fit on one rank as ONE call (pyDNMF.py:138-182 over the observed positions): `itr` steps of dnmf_masked_update_w
 * (iff w_update) and dnmf_masked_update_h with the clamp of H and then of W at the steps i % 10 == 0 (:155-157, :170-172),
 * normalize_features (:185-194) and sq_out = {||P_Omega(A - W H)||^2, ||P_Omega(A)||^2} (:205-218; the caller takes the square roots,
 * as after dnmf_mu_fro_fit).  Host sequencing of the launches above on `stream`: no host synchronisation inside.  One problem per call.
 * `ws`: dnmf_masked_ws_bytes_fit(m, n, k) bytes, 16-byte aligned (0: bad shape or rank). */
size_t dnmf_masked_ws_bytes_fit(long m, long n, int k);
int dnmf_masked_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int kl,
                       int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream);

/* ---- the Itakura-Saito objective (beta = 0) on dense strictly positive float32 data (csrc/dnmf_is.h) ----
 * No counterpart in the reference, whose objectives are fro and kl; the rule is the majorisation-minimisation MU of Fevotte & Idier
 * (2011), scikit-learn's for beta_loss='itakura-saito'.  With S = W H, R = 1 / (S + eps) element-wise and F = H^T (W side) or W (H side):
 *     num = (A . R . R) F,   den = R F,   X <- X . sqrt(num / (den + eps))
 * which never increases D_IS(A | S + eps) = sum (q - log q - 1), q = A . R.  The pairs have the structure of the masked ones above
 * (a tile of S in MFMA accumulators, one element-wise step, two second products that share their F fragments -- the same kernels in
 * a third mode, with dnmf_masked_plan's launch geometry but for the two choices dnmf_is_plan names) and parallel the reference's KL products (dist_nmf.py:806-810: the quotient;
 * :827-849: the rules); the element-wise step is one v_rcp_f32 and two multiplies, and there is no mask: a NaN of A is not skipped,
 * a zero of A sends the divergence to infinity (callers check A > 0).  1 <= k <= DNMF_TUNED_MAX_K; any shape and any leading dimensions
 * (padding is never read as data and adds exactly nothing: csrc/dnmf_is.h).  Partial sums are added in a fixed order, no float
 * atomics: bit-reproducible.  Bad arguments return DNMF_EINVAL with a dnmf_last_error text; the *_bytes functions return 0.
 * `ws`: dnmf_is_ws_bytes(m, n, k) bytes, 16-byte aligned, serves every entry point below but the whole fit. */
size_t dnmf_is_ws_bytes(long m, long n, int k);
/* The launch plans, host arithmetic only (nothing is launched): out[0..5] = {tiles_per_split, nsplit, zdim, rowblks_per_chunk,
 * nchunks, nrowblk} with the meaning of dnmf_masked_plan and its values, except that the H side never asks for fewer than four row
 * chunks (a workgroup is four waves, a wave per chunk; the masked plan asks for 1024 / column blocks, which is below four beyond 256
 * column blocks of 4096 / KP columns) and that zdim is 1 at KP = 128 as well (a workgroup of the W side holds all four tiles of output
 * columns, so S is formed once; the column splits are sized for 512 / rowtiles workgroups accordingly); out[6] / out[7] = workgroups of the W side's / H side's ending (256 outputs each per
 * grid-stride trip: dnmf_masked_reduce_grid(m, k) / (k, n)). */
int dnmf_is_plan(long m, long n, int k, long out[8]);
/* the pair stored: num = (A . R . R) F, den = R F, [m x k] (W side) or [k x n] (H side) with the same leading dimension ldo -- the two
 * halves of one contiguous buffer where the sums cross ranks (one allreduce, then dnmf_is_ratio_update); parallels
 * dist_nmf.py:806,810 (W side) and :806,808 (H side) */
int dnmf_is_aht_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                     float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream);
int dnmf_is_wta_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                     float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream);
/* the pair applied where nothing crosses ranks: W <- W * sqrt(num / (den + eps)) in place after the pass has read it (parallels
 * dist_nmf.py:828-830), H alike with max(., eps) if clamp != 0 (:847-849, pyDNMF.py:170-172) */
int dnmf_is_update_w(const float* A, long m, long n, long lda, float* W, long ldw, const float* H, long ldh, int k, float eps, void* ws,
                     size_t ws_bytes, void* stream);
int dnmf_is_update_h(const float* A, long m, long n, long lda, const float* W, long ldw, float* H, long ldh, int k, float eps, int clamp,
                     void* ws, size_t ws_bytes, void* stream);
/* X[r][c] <- X[r][c] * sqrt(num[r][c] / (den[r][c] + eps)), max(., eps) if clamp != 0: the rule on a stored pair (ldo: the leading
 * dimension of num and den) -- the same expression as the endings above */
int dnmf_is_ratio_update(float* X, long rows, long cols, long ldx, const float* num, const float* den, long ldo, float eps, int clamp,
                         void* stream);
/* *out (double, device) = D_IS(A | W H + eps) = sum (q - log q - 1), q = a / (s + eps), over the block.  S tiles stay in MFMA
 * accumulators (as in dnmf_masked_resid_sqnorm); fp32 per 32 x 128 tile and lane, float64 from there on, every tile's sum in its own
 * slot of `ws` and the slots added in a fixed order: two calls are bit-identical.  Parallels the residual of pyDNMF.py:205-218. */
int dnmf_is_divergence(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                       double* out, void* ws, size_t ws_bytes, void* stream);
/* div[c] (float64, c < n) = sum_i (q - log q - 1), q = a / (s + eps), over this rank's rows: the divergence above column by column.
 * No counterpart in the reference; it stands where PyNMF.column_err (pyDNMF.py:221-239) stands in an NMFk sweep (pyDNMFk.py:248) when
 * the objective is Itakura-Saito -- divided by the global row count it is a mean per entry, scale-invariant across columns.  The
 * structure of dnmf_masked_column_err: S tiles in MFMA accumulators, fp32 over the 16 rows a lane holds of a 32-row block, float64
 * from there on; every row chunk leaves one float64 per column in `ws`, an ending adds them in chunk order and STORES div (nothing
 * is accumulated into it, no atomics: two calls are bit-identical).  1 <= k <= DNMF_TUNED_MAX_K; any shape and leading dimensions.
 * `ws`: dnmf_is_column_div_ws_bytes(m, n, k) bytes, 16-byte aligned (0: bad shape or rank). */
size_t dnmf_is_column_div_ws_bytes(long m, long n, int k);
/* Its launch plan, host arithmetic only: out = {rowblks_per_chunk, nchunks, ncolblk} with the values of dnmf_masked_column_err_plan;
 * the slab takes nchunks * ncolblk * 128 doubles (one per chunk and column, not a pair). */
int dnmf_is_column_div_plan(long m, long n, int k, long out[3]);
int dnmf_is_column_div(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                       double* div, void* ws, size_t ws_bytes, void* stream);
/* A whole Itakura-Saito MU fit on one rank as ONE call (pyDNMF.py:138-182): `itr` steps of dnmf_is_update_w (iff w_update) and
 * dnmf_is_update_h with the clamp of H and then of W at the steps i % 10 == 0 (:155-157, :170-172), normalize_features (:185-194) and
 * sq_out = {||A - W H||^2, ||A||^2} (:205-218: the Frobenius pair, as after dnmf_mu_kl_fit; the caller takes the square roots).  Host
 * sequencing of the launches above on `stream`: no host synchronisation inside.  One problem per call.
 * `ws`: dnmf_is_ws_bytes_fit(m, n, k) bytes, 16-byte aligned (0: bad shape or rank). */
size_t dnmf_is_ws_bytes_fit(long m, long n, int k);
int dnmf_is_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
                   int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream);

/* ---- measurement aid (no counterpart in the reference) ----
 * Which shader clock does the GPU hold right now?  Launches ONE wave on `stream` that writes `n` pairs {s_memtime (shader
 * cycles), wall_clock64 (the constant 100 MHz reference)} into samples[2 n], sleeping `naps` x ~4 us between two pairs, and
 * returns at once.  Launched on its own stream BEFORE the work of interest, it keeps one wave slot of one CU while that work
 * runs; (d memtime / d wall) x 0.1 between consecutive pairs is the clock in GHz over that interval.  The fp32 passes of a
 * step hold about 2.0 GHz of the 2.4 GHz peak clock (full-rate fp32 MFMAs + a 4 TB/s HBM stream meet the board's power limit):
 * bench.py quotes roofline fractions against the peak clock and reports this one next to them.  1 <= n, 0 <= naps <= 1000. */
int dnmf_clock_probe(unsigned long long* samples, int n, int naps, void* stream);

#ifdef __cplusplus
}
#endif

/* the beta-divergence family (dnmf_beta_*): part of this ABI, declared in a header of its own */
#include "dnmf_beta_api.h"
/* and its per-column statistic for rank estimation (dnmf_beta_column_div*), likewise */
#include "dnmf_beta_nmfk_api.h"

#endif /* DNMF_H */
