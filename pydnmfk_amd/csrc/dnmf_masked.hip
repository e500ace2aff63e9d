// dnmf_masked.hip -- C ABI of the masked MU rules on DENSE data whose missing entries are NaN (csrc/dnmf_masked.h).  A translation unit
// of its own (see csrc/dnmf_kl.hip).  Plain launch chains: no workgroup waits for another one; no float atomics in the products.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_masked.h"

namespace {

// per-column error: 128-column blocks x row chunks (a wave per chunk and column block).  About two waves per SIMD, and at most 256
// chunks: the ending adds a column's chunk pairs one after another
struct MaskedColerrPlan { long ncolblk; long ldc; long nrowblk; long rowblks_per_chunk; long nchunks; size_t bytes; };
MaskedColerrPlan plan_masked_colerr(long m, long n) {
    MaskedColerrPlan c{};
    c.ncolblk = cdiv(n, 128);
    c.ldc = c.ncolblk * 128;
    c.nrowblk = cdiv(m, 32);
    const long want = std::min<long>(std::max<long>(1, 2048 / c.ncolblk), 256);
    c.rowblks_per_chunk = std::max<long>(1, cdiv(c.nrowblk, want));
    c.nchunks = cdiv(c.nrowblk, c.rowblks_per_chunk);
    c.bytes = (size_t)c.nchunks * 2 * c.ldc * sizeof(double);
    return c;
}

// workspace of a whole fit: the step's slabs, the partials of the column sums of W (dnmf_colsum: at most 1024 slabs of KP floats), the
// sums themselves, and three doubles {resid, ||P(A)||^2, |Omega|}
struct MaskedFitWs { size_t step; size_t part_off; size_t part_bytes; size_t cs_off; size_t sq_off; size_t total; };
MaskedFitWs masked_fit_layout(long m, long n, int k) {
    MaskedFitWs f{};
    const int kt = kt_of(k);
    const size_t kp = 32 * (size_t)kt;
    f.step = align256(std::max(plan_masked_uht(m, n, kt).bytes, plan_masked_wtu(m, n, kt).bytes));
    f.part_off = f.step;
    f.part_bytes = align256(1024 * kp * sizeof(float));
    f.cs_off = f.part_off + f.part_bytes;
    f.sq_off = f.cs_off + align256(kp * sizeof(float));
    f.total = f.sq_off + 256;
    return f;
}

int masked_reduce(const float* P, long part_stride, long half_stride, long ldp, int nparts, long rows, long cols, float* num, float* den,
                  long ldo, float* X, long ldx, float eps, int clamp, hipStream_t st, const char* who) {
    const unsigned grid = (unsigned)masked_reduce_grid(rows, cols);
    hipLaunchKernelGGL(masked_reduce_kernel, dim3(grid), dim3(256), 0, st, P, part_stride, half_stride, ldp, nparts, rows, cols, num, den, ldo,
                       X, ldx, eps, clamp);
    return check_launch(who);
}

// the W side into partial slabs, then the ending: (num, den) stored, or X = W updated in place
int masked_w_side(const char* who, const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                  float eps, int kl, float* num, float* den, long ldo, float* X, void* ws, size_t ws_bytes, void* stream) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "%s: rank k=%d unsupported (1 <= k <= %d for masked dense data)", who, k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && (X || (num && den && ldo >= k)),
            "%s: null pointer or bad shape", who);
    const MaskedUhtPlan u = plan_masked_uht(m, n, kt);
    if (!ws || ws_bytes < u.bytes || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, u.bytes);
    const int kp = 32 * kt;
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    const long half = m * kp, split = 2 * half;
    const dim3 grid((unsigned)u.rowtiles, (unsigned)u.nsplit, (unsigned)u.zdim), block(256);
    const size_t lds = 2ul * kp * BK * sizeof(float);
    hipStream_t st = S(stream);
    float* P = (float*)ws;
#define MU_CASE(KT_, JT_)                                                                                                    \
    if (kt == KT_) {                                                                                                         \
        if (fast && kl) hipLaunchKernelGGL((masked_uht_kernel<KT_, JT_, true, true>), grid, block, lds, st, a, P, split, half, u.cols_per_split);   \
        else if (fast) hipLaunchKernelGGL((masked_uht_kernel<KT_, JT_, true, false>), grid, block, lds, st, a, P, split, half, u.cols_per_split);   \
        else if (kl) hipLaunchKernelGGL((masked_uht_kernel<KT_, JT_, false, true>), grid, block, lds, st, a, P, split, half, u.cols_per_split);     \
        else hipLaunchKernelGGL((masked_uht_kernel<KT_, JT_, false, false>), grid, block, lds, st, a, P, split, half, u.cols_per_split);            \
    }
    MU_CASE(1, 1) MU_CASE(2, 2) MU_CASE(4, 2)
#undef MU_CASE
    if (int rc = check_launch(who)) return rc;
    return masked_reduce(P, split, half, kp, u.nsplit, m, k, num, den, ldo, X, ldw, eps, 0, st, who);
}

int masked_h_side(const char* who, const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                  float eps, int kl, float* num, float* den, long ldo, float* X, int clamp, void* ws, size_t ws_bytes, void* stream) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "%s: rank k=%d unsupported (1 <= k <= %d for masked dense data)", who, k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && (X || (num && den && ldo >= n)),
            "%s: null pointer or bad shape", who);
    const MaskedWtuPlan w = plan_masked_wtu(m, n, kt);
    if (!ws || ws_bytes < w.bytes || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, w.bytes);
    const int kp = 32 * kt;
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    a.ncolblk = w.ncolblk;
    const long half = (long)kp * w.ldp;
    a.P = (float*)ws; a.ldp = w.ldp; a.chunk_stride = 2 * half;
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    const dim3 grid((unsigned)(cdiv(w.nchunks, 4) * w.ncolblk)), block(256);     // 4 row chunks (waves) per workgroup
    const size_t lds = (size_t)kp * 32 * w.nt * sizeof(float);
    hipStream_t st = S(stream);
#define MH_CASE(KT_, NT_)                                                                                                    \
    if (kt == KT_) {                                                                                                         \
        if (fast && kl) hipLaunchKernelGGL((masked_wtu_kernel<KT_, NT_, true, true>), grid, block, lds, st, a, half, w.rowblks_per_chunk);    \
        else if (fast) hipLaunchKernelGGL((masked_wtu_kernel<KT_, NT_, true, false>), grid, block, lds, st, a, half, w.rowblks_per_chunk);    \
        else if (kl) hipLaunchKernelGGL((masked_wtu_kernel<KT_, NT_, false, true>), grid, block, lds, st, a, half, w.rowblks_per_chunk);      \
        else hipLaunchKernelGGL((masked_wtu_kernel<KT_, NT_, false, false>), grid, block, lds, st, a, half, w.rowblks_per_chunk);             \
    }
    MH_CASE(1, 4) MH_CASE(2, 2) MH_CASE(4, 1)
#undef MH_CASE
    if (int rc = check_launch(who)) return rc;
    return masked_reduce(a.P, a.chunk_stride, half, w.ldp, (int)w.nchunks, k, n, num, den, ldo, X, ldh, eps, clamp, st, who);
}

}  // namespace

extern "C" {

size_t dnmf_masked_ws_bytes(long m, long n, int k) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1) return 0;
    return align256(std::max(plan_masked_uht(m, n, kt).bytes, plan_masked_wtu(m, n, kt).bytes));
}

// the launch plans of both sides as numbers (host arithmetic, no GPU): what the launches above use, for callers and tests that must
// know which loops of the kernels a shape enters
int dnmf_masked_plan(long m, long n, int k, long out[6]) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "masked_plan: rank k=%d unsupported (1 <= k <= %d for masked dense data)", k, DNMF_TUNED_MAX_K);
    REQUIRE(out && m >= 1 && n >= 1, "masked_plan: null pointer or bad shape");
    const MaskedUhtPlan u = plan_masked_uht(m, n, kt);
    const MaskedWtuPlan w = plan_masked_wtu(m, n, kt);
    out[0] = u.cols_per_split / BK;     // 32-column tiles a workgroup of the W side walks (the last split may hold fewer)
    out[1] = u.nsplit;
    out[2] = u.zdim;
    out[3] = w.rowblks_per_chunk;       // 32-row blocks a wave of the H side walks (the last chunk may hold fewer)
    out[4] = w.nchunks;
    out[5] = w.nrowblk;
    return DNMF_OK;
}

// the grid of the ending (masked_reduce_kernel) for a rows x cols output, as the launches size it: rows x cols = m x k on the W side,
// k x n on the H side; the kernel takes cdiv(rows * cols, 256 * grid) grid-stride trips.  0 for rows or cols < 1.
long dnmf_masked_reduce_grid(long rows, long cols) {
    if (rows < 1 || cols < 1) return 0;
    return masked_reduce_grid(rows, cols);
}

int dnmf_masked_aht_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                         int kl, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(num && den, "masked_aht_pair: null pointer or bad shape");
    return masked_w_side("masked_aht_pair", A, m, n, lda, W, ldw, H, ldh, k, eps, kl, num, den, ldo, nullptr, ws, ws_bytes, stream);
}

int dnmf_masked_wta_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                         int kl, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(num && den, "masked_wta_pair: null pointer or bad shape");
    return masked_h_side("masked_wta_pair", A, m, n, lda, W, ldw, H, ldh, k, eps, kl, num, den, ldo, nullptr, 0, ws, ws_bytes, stream);
}

int dnmf_masked_update_w(const float* A, long m, long n, long lda, float* W, long ldw, const float* H, long ldh, int k, float eps, int kl,
                         void* ws, size_t ws_bytes, void* stream) {
    return masked_w_side("masked_update_w", A, m, n, lda, W, ldw, H, ldh, k, eps, kl, nullptr, nullptr, 0, W, ws, ws_bytes, stream);
}

int dnmf_masked_update_h(const float* A, long m, long n, long lda, const float* W, long ldw, float* H, long ldh, int k, float eps, int kl,
                         int clamp, void* ws, size_t ws_bytes, void* stream) {
    return masked_h_side("masked_update_h", A, m, n, lda, W, ldw, H, ldh, k, eps, kl, nullptr, nullptr, 0, H, clamp != 0, ws, ws_bytes, stream);
}

int dnmf_masked_resid_sqnorm(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                             double* sq, void* stream) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "masked_resid_sqnorm: rank k=%d unsupported (1 <= k <= %d for masked dense data)", k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && sq && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n, "masked_resid_sqnorm: null pointer or bad shape");
    hipStream_t st = S(stream);
    if (hipMemsetAsync(sq, 0, sizeof(double), st) != hipSuccess) return fail(DNMF_EHIP, "masked_resid_sqnorm: memset failed");
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, 0.f);
    a.out = sq;
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    const dim3 grid((unsigned)cdiv(a.nrowblk * a.ncolblk, 4)), block(256);
#define MR_CASE(KT_)                                                                                     \
    if (kt == KT_) {                                                                                     \
        if (fast) hipLaunchKernelGGL((masked_resid_kernel<KT_, true>), grid, block, 0, st, a);           \
        else hipLaunchKernelGGL((masked_resid_kernel<KT_, false>), grid, block, 0, st, a);               \
    }
    MR_CASE(1) MR_CASE(2) MR_CASE(4)
#undef MR_CASE
    return check_launch("masked_resid_sqnorm");
}

int dnmf_masked_sqnorm(const float* A, long m, long n, long lda, double* out, void* stream) {
    REQUIRE(A && out && m >= 1 && n >= 1 && lda >= n, "masked_sqnorm: null pointer or bad shape");
    hipStream_t st = S(stream);
    if (hipMemsetAsync(out, 0, 2 * sizeof(double), st) != hipSuccess) return fail(DNMF_EHIP, "masked_sqnorm: memset failed");
    const unsigned grid = (unsigned)std::min<long>(cdiv(m * n, 1024), 4096);
    hipLaunchKernelGGL(masked_sqnorm_kernel, dim3(grid), dim3(256), 0, st, A, m, n, lda, out);
    return check_launch("masked_sqnorm");
}

size_t dnmf_masked_column_err_ws_bytes(long m, long n, int k) {
    if (kt_of(k) < 0 || m < 1 || n < 1) return 0;
    return align256(plan_masked_colerr(m, n).bytes);
}

// the launch plan of dnmf_masked_column_err as numbers (host arithmetic, no GPU)
int dnmf_masked_column_err_plan(long m, long n, int k, long out[3]) {
    REQUIRE(kt_of(k) > 0, "masked_column_err_plan: rank k=%d unsupported (1 <= k <= %d for masked dense data)", k, DNMF_TUNED_MAX_K);
    REQUIRE(out && m >= 1 && n >= 1, "masked_column_err_plan: null pointer or bad shape");
    const MaskedColerrPlan c = plan_masked_colerr(m, n);
    out[0] = c.rowblks_per_chunk;       // 32-row blocks a wave walks (the last chunk may hold fewer)
    out[1] = c.nchunks;
    out[2] = c.ncolblk;                 // 128-column blocks (the last may be ragged)
    return DNMF_OK;
}

int dnmf_masked_column_err(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, double* num,
                           double* den, void* ws, size_t ws_bytes, void* stream) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "masked_column_err: rank k=%d unsupported (1 <= k <= %d for masked dense data)", k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && num && den && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n, "masked_column_err: null pointer or bad shape");
    const MaskedColerrPlan c = plan_masked_colerr(m, n);
    if (!ws || ws_bytes < c.bytes || !aligned16(ws)) return fail(DNMF_EWS, "masked_column_err: workspace %zu < %zu bytes", ws_bytes, c.bytes);
    hipStream_t st = S(stream);
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, 0.f);
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    double* P = (double*)ws;
    const dim3 grid((unsigned)cdiv(c.nchunks * c.ncolblk, 4)), block(256);
#define MC_CASE(KT_)                                                                                                            \
    if (kt == KT_) {                                                                                                            \
        if (fast) hipLaunchKernelGGL((masked_colerr_kernel<KT_, true>), grid, block, 0, st, a, P, c.ldc, c.rowblks_per_chunk);  \
        else hipLaunchKernelGGL((masked_colerr_kernel<KT_, false>), grid, block, 0, st, a, P, c.ldc, c.rowblks_per_chunk);      \
    }
    MC_CASE(1) MC_CASE(2) MC_CASE(4)
#undef MC_CASE
    if (int rc = check_launch("masked_column_err")) return rc;
    hipLaunchKernelGGL(masked_colerr_reduce_kernel, dim3((unsigned)std::min<long>(cdiv(n, 256), 4096)), dim3(256), 0, st, (const double*)P, c.ldc,
                       c.nchunks, n, num, den);
    return check_launch("masked_column_err");
}

size_t dnmf_masked_ws_bytes_fit(long m, long n, int k) {
    if (kt_of(k) < 0 || m < 1 || n < 1) return 0;
    return masked_fit_layout(m, n, k).total;
}

// pyDNMF.py:138-182 for a masked block on one rank: the launches the step loop makes, in its order, with nothing in between
int dnmf_masked_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int kl,
                       int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "masked_mu_fit: rank k=%d unsupported (1 <= k <= %d for masked dense data)", k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && sq_out && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && itr >= 0,
            "masked_mu_fit: null pointer or bad shape (m=%ld n=%ld k=%d itr=%d)", m, n, k, itr);
    const MaskedFitWs f = masked_fit_layout(m, n, k);
    if (!ws || ws_bytes < f.total || !aligned16(ws)) return fail(DNMF_EWS, "masked_mu_fit: workspace %zu < %zu bytes", ws_bytes, f.total);
    char* base = (char*)ws;
    int rc = DNMF_OK;
    for (int i = 0; i < itr; ++i) {                                                                   // pyDNMF.py:151-172
        const int clamp = (i % 10 == 0);
        if (w_update && (rc = dnmf_masked_update_w(A, m, n, lda, W, ldw, H, ldh, k, eps, kl, ws, f.step, stream))) return rc;
        if ((rc = dnmf_masked_update_h(A, m, n, lda, W, ldw, H, ldh, k, eps, kl, clamp, ws, f.step, stream))) return rc;
        if (clamp && (rc = dnmf_clamp_min(W, m, k, ldw, eps, stream))) return rc;
    }
    // normalize_features (pyDNMF.py:185-194): s = column sums of W; W /= s + eps; H *= s^T
    float* s = (float*)(base + f.cs_off);
    if ((rc = dnmf_colsum(W, m, k, ldw, s, base + f.part_off, f.part_bytes, stream))) return rc;
    if ((rc = dnmf_scale_cols_div(W, m, k, ldw, s, eps, stream))) return rc;
    if ((rc = dnmf_scale_rows_mul(H, k, n, ldh, s, stream))) return rc;
    // relative_err (pyDNMF.py:205-218) over the observed positions; the caller takes the square roots
    double* sq = (double*)(base + f.sq_off);
    if ((rc = dnmf_masked_resid_sqnorm(A, m, n, lda, W, ldw, H, ldh, k, sq, stream))) return rc;
    if ((rc = dnmf_masked_sqnorm(A, m, n, lda, sq + 1, stream))) return rc;
    if (hipMemcpyAsync(sq_out, sq, 2 * sizeof(double), hipMemcpyDeviceToDevice, S(stream)) != hipSuccess)
        return fail(DNMF_EHIP, "masked_mu_fit: copy of the squared norms failed");
    return DNMF_OK;
}

}  // extern "C"
