// dnmf_is.hip -- C ABI of the Itakura-Saito MU rule on dense strictly positive data: the PAIR_IS mode of the pair launch path of
// csrc/dnmf_masked.h behind its ABI names, the rule on a stored pair, the divergence and its per-column form (csrc/dnmf_is.h).  A translation unit of its own
// (see csrc/dnmf_kl.hip).  Plain launch chains: no workgroup waits for another one; no float atomics in the products or the divergence.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_is.h"

namespace {

// the divergence leaves one double per 32 x 128 tile
size_t is_div_bytes(long m, long n) { return (size_t)cdiv(m, 32) * cdiv(n, 128) * sizeof(double); }

// one workspace serves a step and the divergence
size_t is_step_bytes(long m, long n, int kt) { return align256(std::max(pair_step_bytes<PAIR_IS>(m, n, kt), is_div_bytes(m, n))); }

}  // namespace

extern "C" {

size_t dnmf_is_ws_bytes(long m, long n, int k) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1) return 0;
    return is_step_bytes(m, n, kt);
}

size_t dnmf_is_ws_bytes_fit(long m, long n, int k) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1) return 0;
    return pair_fit_layout(is_step_bytes(m, n, kt), k).total;
}

// the launch plans of both sides (csrc/dnmf_masked.h) and of their endings as numbers (host arithmetic, no GPU)
int dnmf_is_plan(long m, long n, int k, long out[8]) {
    if (int rc = pair_plan_report<PAIR_IS>("is_plan", m, n, k, out)) return rc;
    out[6] = masked_reduce_grid(m, k);  // workgroups (256 outputs each per grid-stride trip) of the W side's ending
    out[7] = masked_reduce_grid(k, n);  // and of the H side's
    return DNMF_OK;
}

int dnmf_is_aht_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                     float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(num && den, "is_aht_pair: null pointer or bad shape");
    return pair_w_side<PAIR_IS>("is_aht_pair", A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, nullptr, ws, ws_bytes, stream);
}

int dnmf_is_wta_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                     float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(num && den, "is_wta_pair: null pointer or bad shape");
    return pair_h_side<PAIR_IS>("is_wta_pair", A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, nullptr, 0, ws, ws_bytes, stream);
}

int dnmf_is_update_w(const float* A, long m, long n, long lda, float* W, long ldw, const float* H, long ldh, int k, float eps, void* ws,
                     size_t ws_bytes, void* stream) {
    return pair_w_side<PAIR_IS>("is_update_w", A, m, n, lda, W, ldw, H, ldh, k, eps, nullptr, nullptr, 0, W, ws, ws_bytes, stream);
}

int dnmf_is_update_h(const float* A, long m, long n, long lda, const float* W, long ldw, float* H, long ldh, int k, float eps, int clamp,
                     void* ws, size_t ws_bytes, void* stream) {
    return pair_h_side<PAIR_IS>("is_update_h", A, m, n, lda, W, ldw, H, ldh, k, eps, nullptr, nullptr, 0, H, clamp != 0, ws, ws_bytes, stream);
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

size_t dnmf_is_column_div_ws_bytes(long m, long n, int k) {
    if (kt_of(k) < 0 || m < 1 || n < 1) return 0;
    return align256(plan_masked_colerr(m, n, 1).bytes);
}

// the launch plan of dnmf_is_column_div as numbers (host arithmetic, no GPU): the masked per-column plan
int dnmf_is_column_div_plan(long m, long n, int k, long out[3]) {
    REQUIRE(kt_of(k) > 0, "is_column_div_plan: rank k=%d unsupported (1 <= k <= %d for the Itakura-Saito kernels)", k, DNMF_TUNED_MAX_K);
    REQUIRE(out && m >= 1 && n >= 1, "is_column_div_plan: null pointer or bad shape");
    const MaskedColerrPlan c = plan_masked_colerr(m, n, 1);
    out[0] = c.rowblks_per_chunk;       // 32-row blocks a wave walks (the last chunk may hold fewer)
    out[1] = c.nchunks;
    out[2] = c.ncolblk;                 // 128-column blocks (the last may be ragged)
    return DNMF_OK;
}

int dnmf_is_column_div(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                       double* div, void* ws, size_t ws_bytes, void* stream) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "is_column_div: rank k=%d unsupported (1 <= k <= %d for the Itakura-Saito kernels)", k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && div && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n, "is_column_div: null pointer or bad shape");
    const MaskedColerrPlan c = plan_masked_colerr(m, n, 1);
    if (!ws || ws_bytes < c.bytes || !aligned16(ws)) return fail(DNMF_EWS, "is_column_div: workspace %zu < %zu bytes", ws_bytes, c.bytes);
    hipStream_t st = S(stream);
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    double* P = (double*)ws;
    const dim3 grid((unsigned)cdiv(c.nchunks * c.ncolblk, 4)), block(256);
#define IC_CASE(KT_)                                                                                                         \
    if (kt == KT_) {                                                                                                         \
        if (fast) hipLaunchKernelGGL((is_coldiv_kernel<KT_, true>), grid, block, 0, st, a, P, c.ldc, c.rowblks_per_chunk);   \
        else hipLaunchKernelGGL((is_coldiv_kernel<KT_, false>), grid, block, 0, st, a, P, c.ldc, c.rowblks_per_chunk);       \
    }
    IC_CASE(1) IC_CASE(2) IC_CASE(4)
#undef IC_CASE
    if (int rc = check_launch("is_column_div")) return rc;
    hipLaunchKernelGGL(is_coldiv_reduce_kernel, dim3((unsigned)std::min<long>(cdiv(n, 256), 4096)), dim3(256), 0, st, (const double*)P, c.ldc,
                       c.nchunks, n, div);
    return check_launch("is_column_div");
}

// a whole Itakura-Saito fit: the chain of csrc/dnmf_masked.h with the IS steps; its error is the Frobenius pair, as after dnmf_mu_kl_fit
int dnmf_is_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
                   int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream) {
    return pair_mu_fit<PAIR_IS>(
        "is_mu_fit", is_step_bytes, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, sq_out, ws, ws_bytes, stream,
        [&](size_t step) { return dnmf_is_update_w(A, m, n, lda, W, ldw, H, ldh, k, eps, ws, step, stream); },
        [&](int clamp, size_t step) { return dnmf_is_update_h(A, m, n, lda, W, ldw, H, ldh, k, eps, clamp, ws, step, stream); },
        [&](double* sq) { return dnmf_resid_sqnorm(A, m, n, lda, W, ldw, H, ldh, k, sq, stream); },
        [&](double* sq) { return dnmf_sqnorm(A, m, n, lda, sq, stream); });
}

}  // extern "C"
