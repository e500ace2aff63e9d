// dnmf_is.hip -- C ABI of the Itakura-Saito MU rule on dense strictly positive data (csrc/dnmf_is.h).  A translation unit of its own
// (see csrc/dnmf_kl.hip).  Plain launch chains: no workgroup waits for another one; no float atomics in the products or the divergence.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_is.h"

namespace {

// The H side's plan: the masked one, but never fewer than four row chunks.  masked_wtu_kernel's workgroup is four waves = four chunks;
// plan_masked_wtu asks for 1024 / ncolblk of them, which is TWO at n = 16384, KP = 128 (512 column blocks of 32): half the waves of
// every workgroup returned at once and the pass ran on half the SIMDs (measured, 32768 x 16384, k = 128: 10.8 ms).  Shapes with at most
// 256 column blocks -- every shape of the masked suite -- get the masked plan unchanged.
MaskedWtuPlan plan_is_wtu(long m, long n, int kt) { return plan_masked_wtu(m, n, kt, 4); }

// The W side's plan: the masked one with ONE part of the output columns at KP = 128 (JT = KT = 4).  masked_uht_kernel<4, 2> forms every
// S tile twice, once per half of the output columns: 8 m n k flop for an IS side's 6 m n k.  With all four output tiles of both halves
// in one workgroup (128 accumulator registers, which the compiler keeps in AGPRs: 254 VGPRs + 156 AGPRs, no scratch, one wave per
// SIMD as before) S is formed once.  Up to KP = 64 nothing changes.
MaskedUhtPlan plan_is_uht(long m, long n, int kt) { return plan_masked_uht(m, n, kt, 1); }

// the divergence leaves one double per 32 x 128 tile
size_t is_div_bytes(long m, long n) { return (size_t)cdiv(m, 32) * cdiv(n, 128) * sizeof(double); }

size_t is_step_bytes(long m, long n, int kt) {
    return align256(std::max(std::max(plan_is_uht(m, n, kt).bytes, plan_is_wtu(m, n, kt).bytes), is_div_bytes(m, n)));
}

// workspace of a whole fit: the layout of dnmf_masked_mu_fit (the step's slabs, the partials of the column sums of W, the sums, and
// the two doubles {resid, ||A||^2})
struct IsFitWs { size_t step; size_t part_off; size_t part_bytes; size_t cs_off; size_t sq_off; size_t total; };
IsFitWs is_fit_layout(long m, long n, int k) {
    IsFitWs f{};
    const int kt = kt_of(k);
    const size_t kp = 32 * (size_t)kt;
    f.step = is_step_bytes(m, n, kt);
    f.part_off = f.step;
    f.part_bytes = align256(1024 * kp * sizeof(float));
    f.cs_off = f.part_off + f.part_bytes;
    f.sq_off = f.cs_off + align256(kp * sizeof(float));
    f.total = f.sq_off + 256;
    return f;
}

int is_reduce(const float* P, long part_stride, long half_stride, long ldp, int nparts, long rows, long cols, float* num, float* den,
              long ldo, float* X, long ldx, float eps, int clamp, hipStream_t st, const char* who) {
    const unsigned grid = (unsigned)masked_reduce_grid(rows, cols);
    hipLaunchKernelGGL(is_reduce_kernel, dim3(grid), dim3(256), 0, st, P, part_stride, half_stride, ldp, nparts, rows, cols, num, den, ldo, X,
                       ldx, eps, clamp);
    return check_launch(who);
}

// the W side into partial slabs (masked_uht_kernel in its IS mode), then the ending
int is_w_side(const char* who, const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
              float eps, float* num, float* den, long ldo, float* X, void* ws, size_t ws_bytes, void* stream) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "%s: rank k=%d unsupported (1 <= k <= %d for the Itakura-Saito kernels)", who, k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && (X || (num && den && ldo >= k)),
            "%s: null pointer or bad shape", who);
    const MaskedUhtPlan u = plan_is_uht(m, n, kt);
    if (!ws || ws_bytes < u.bytes || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, u.bytes);
    const int kp = 32 * kt;
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    const long half = m * kp, split = 2 * half;
    const dim3 grid((unsigned)u.rowtiles, (unsigned)u.nsplit, (unsigned)u.zdim), block(256);
    const size_t lds = 2ul * kp * BK * sizeof(float);
    hipStream_t st = S(stream);
    float* P = (float*)ws;
#define IW_CASE(KT_, JT_)                                                                                                                  \
    if (kt == KT_) {                                                                                                                       \
        if (fast) hipLaunchKernelGGL((masked_uht_kernel<KT_, JT_, true, PAIR_IS>), grid, block, lds, st, a, P, split, half, u.cols_per_split);  \
        else hipLaunchKernelGGL((masked_uht_kernel<KT_, JT_, false, PAIR_IS>), grid, block, lds, st, a, P, split, half, u.cols_per_split);      \
    }
    IW_CASE(1, 1) IW_CASE(2, 2) IW_CASE(4, 4)
#undef IW_CASE
    if (int rc = check_launch(who)) return rc;
    return is_reduce(P, split, half, kp, u.nsplit, m, k, num, den, ldo, X, ldw, eps, 0, st, who);
}

int is_h_side(const char* who, const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
              float eps, float* num, float* den, long ldo, float* X, int clamp, void* ws, size_t ws_bytes, void* stream) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "%s: rank k=%d unsupported (1 <= k <= %d for the Itakura-Saito kernels)", who, k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && (X || (num && den && ldo >= n)),
            "%s: null pointer or bad shape", who);
    const MaskedWtuPlan w = plan_is_wtu(m, n, kt);
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
#define IH_CASE(KT_, NT_)                                                                                                          \
    if (kt == KT_) {                                                                                                               \
        if (fast) hipLaunchKernelGGL((masked_wtu_kernel<KT_, NT_, true, PAIR_IS>), grid, block, lds, st, a, half, w.rowblks_per_chunk);  \
        else hipLaunchKernelGGL((masked_wtu_kernel<KT_, NT_, false, PAIR_IS>), grid, block, lds, st, a, half, w.rowblks_per_chunk);      \
    }
    IH_CASE(1, 4) IH_CASE(2, 2) IH_CASE(4, 1)
#undef IH_CASE
    if (int rc = check_launch(who)) return rc;
    return is_reduce(a.P, a.chunk_stride, half, w.ldp, (int)w.nchunks, k, n, num, den, ldo, X, ldh, eps, clamp, st, who);
}

}  // namespace

extern "C" {

size_t dnmf_is_ws_bytes(long m, long n, int k) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1) return 0;
    return is_step_bytes(m, n, kt);
}

size_t dnmf_is_ws_bytes_fit(long m, long n, int k) {
    if (kt_of(k) < 0 || m < 1 || n < 1) return 0;
    return is_fit_layout(m, n, k).total;
}

// the launch plans of both sides and of their endings as numbers (host arithmetic, no GPU): what the launches above use
int dnmf_is_plan(long m, long n, int k, long out[8]) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "is_plan: rank k=%d unsupported (1 <= k <= %d for the Itakura-Saito kernels)", k, DNMF_TUNED_MAX_K);
    REQUIRE(out && m >= 1 && n >= 1, "is_plan: null pointer or bad shape");
    const MaskedUhtPlan u = plan_is_uht(m, n, kt);
    const MaskedWtuPlan w = plan_is_wtu(m, n, kt);
    out[0] = u.cols_per_split / BK;     // 32-column tiles a workgroup of the W side walks (the last split may hold fewer)
    out[1] = u.nsplit;
    out[2] = u.zdim;
    out[3] = w.rowblks_per_chunk;       // 32-row blocks a wave of the H side walks (the last chunk may hold fewer)
    out[4] = w.nchunks;
    out[5] = w.nrowblk;
    out[6] = masked_reduce_grid(m, k);  // workgroups (256 outputs each per grid-stride trip) of the W side's ending
    out[7] = masked_reduce_grid(k, n);  // and of the H side's
    return DNMF_OK;
}

int dnmf_is_aht_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                     float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(num && den, "is_aht_pair: null pointer or bad shape");
    return is_w_side("is_aht_pair", A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, nullptr, ws, ws_bytes, stream);
}

int dnmf_is_wta_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                     float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(num && den, "is_wta_pair: null pointer or bad shape");
    return is_h_side("is_wta_pair", A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, nullptr, 0, ws, ws_bytes, stream);
}

int dnmf_is_update_w(const float* A, long m, long n, long lda, float* W, long ldw, const float* H, long ldh, int k, float eps, void* ws,
                     size_t ws_bytes, void* stream) {
    return is_w_side("is_update_w", A, m, n, lda, W, ldw, H, ldh, k, eps, nullptr, nullptr, 0, W, ws, ws_bytes, stream);
}

int dnmf_is_update_h(const float* A, long m, long n, long lda, const float* W, long ldw, float* H, long ldh, int k, float eps, int clamp,
                     void* ws, size_t ws_bytes, void* stream) {
    return is_h_side("is_update_h", A, m, n, lda, W, ldw, H, ldh, k, eps, nullptr, nullptr, 0, H, clamp != 0, ws, ws_bytes, stream);
}

int dnmf_is_ratio_update(float* X, long rows, long cols, long ldx, const float* num, const float* den, long ldo, float eps, int clamp,
                         void* stream) {
    REQUIRE(X && num && den && rows >= 1 && cols >= 1 && ldx >= cols && ldo >= cols, "is_ratio_update: null pointer or bad shape");
    const unsigned grid = (unsigned)masked_reduce_grid(rows, cols);
    hipLaunchKernelGGL(is_ratio_kernel, dim3(grid), dim3(256), 0, S(stream), X, rows, cols, ldx, num, den, ldo, eps, clamp != 0);
    return check_launch("is_ratio_update");
}

int dnmf_is_divergence(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                       double* out, void* ws, size_t ws_bytes, void* stream) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "is_divergence: rank k=%d unsupported (1 <= k <= %d for the Itakura-Saito kernels)", k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && out && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n, "is_divergence: null pointer or bad shape");
    const size_t need = is_div_bytes(m, n);
    if (!ws || ws_bytes < need || !aligned16(ws)) return fail(DNMF_EWS, "is_divergence: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = S(stream);
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    const long tiles = a.nrowblk * a.ncolblk;
    double* P = (double*)ws;
    const dim3 grid((unsigned)cdiv(tiles, 4)), block(256);
#define ID_CASE(KT_)                                                                                  \
    if (kt == KT_) {                                                                                  \
        if (fast) hipLaunchKernelGGL((is_div_kernel<KT_, true>), grid, block, 0, st, a, P);           \
        else hipLaunchKernelGGL((is_div_kernel<KT_, false>), grid, block, 0, st, a, P);               \
    }
    ID_CASE(1) ID_CASE(2) ID_CASE(4)
#undef ID_CASE
    if (int rc = check_launch("is_divergence")) return rc;
    hipLaunchKernelGGL(is_div_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)P, tiles, out);
    return check_launch("is_divergence");
}

// pyDNMF.py:138-182 under the Itakura-Saito rule on one rank: the launches the step loop makes, in its order, with nothing in between
int dnmf_is_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
                   int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "is_mu_fit: rank k=%d unsupported (1 <= k <= %d for the Itakura-Saito kernels)", k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && sq_out && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && itr >= 0,
            "is_mu_fit: null pointer or bad shape (m=%ld n=%ld k=%d itr=%d)", m, n, k, itr);
    const IsFitWs f = is_fit_layout(m, n, k);
    if (!ws || ws_bytes < f.total || !aligned16(ws)) return fail(DNMF_EWS, "is_mu_fit: workspace %zu < %zu bytes", ws_bytes, f.total);
    char* base = (char*)ws;
    int rc = DNMF_OK;
    for (int i = 0; i < itr; ++i) {                                                                   // pyDNMF.py:151-172
        const int clamp = (i % 10 == 0);
        if (w_update && (rc = dnmf_is_update_w(A, m, n, lda, W, ldw, H, ldh, k, eps, ws, f.step, stream))) return rc;
        if ((rc = dnmf_is_update_h(A, m, n, lda, W, ldw, H, ldh, k, eps, clamp, ws, f.step, stream))) return rc;
        if (clamp && (rc = dnmf_clamp_min(W, m, k, ldw, eps, stream))) return rc;
    }
    // normalize_features (pyDNMF.py:185-194): s = column sums of W; W /= s + eps; H *= s^T
    float* s = (float*)(base + f.cs_off);
    if ((rc = dnmf_colsum(W, m, k, ldw, s, base + f.part_off, f.part_bytes, stream))) return rc;
    if ((rc = dnmf_scale_cols_div(W, m, k, ldw, s, eps, stream))) return rc;
    if ((rc = dnmf_scale_rows_mul(H, k, n, ldh, s, stream))) return rc;
    // relative_err (pyDNMF.py:205-218): the Frobenius pair, as after dnmf_mu_kl_fit; the caller takes the square roots
    double* sq = (double*)(base + f.sq_off);
    if ((rc = dnmf_resid_sqnorm(A, m, n, lda, W, ldw, H, ldh, k, sq, stream))) return rc;
    if ((rc = dnmf_sqnorm(A, m, n, lda, sq + 1, stream))) return rc;
    if (hipMemcpyAsync(sq_out, sq, 2 * sizeof(double), hipMemcpyDeviceToDevice, S(stream)) != hipSuccess)
        return fail(DNMF_EHIP, "is_mu_fit: copy of the squared norms failed");
    return DNMF_OK;
}

}  // extern "C"
