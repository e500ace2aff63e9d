// dnmf_beta.hip -- C ABI of the beta-divergence MU rule on dense data, -2 <= beta <= 4: the PAIR_BETA mode of the pair launch path of
// csrc/dnmf_masked.h behind its ABI names, the rule on a stored pair, the divergence and its per-column sums (csrc/dnmf_beta.h).  A translation unit of its own
// (see csrc/dnmf_kl.hip).  Plain launch chains: no workgroup waits for another one; no float atomics in the products or the divergence.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_beta.h"

namespace {

// the divergence leaves one double per 32 x 128 tile
size_t beta_div_bytes(long m, long n) { return (size_t)cdiv(m, 32) * cdiv(n, 128) * sizeof(double); }

// one workspace serves a step and the divergence
size_t beta_step_bytes(long m, long n, int kt) { return align256(std::max(pair_step_bytes<PAIR_BETA>(m, n, kt), beta_div_bytes(m, n))); }

}  // namespace

// every entry point that takes a workspace refuses a misaligned one first (include/dnmf.h: the workspace contract), then a beta
// outside the accepted range
#define REQUIRE_BETA(who) REQUIRE(beta_ok(beta), who ": beta=%g is outside the accepted range -2 <= beta <= 4", (double)beta)

extern "C" {

size_t dnmf_beta_ws_bytes(long m, long n, int k) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1) return 0;
    return beta_step_bytes(m, n, kt);
}

size_t dnmf_beta_ws_bytes_fit(long m, long n, int k) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1) return 0;
    return pair_fit_layout(beta_step_bytes(m, n, kt), k).total;
}

// the launch plans of both sides (csrc/dnmf_masked.h) and of their endings as numbers (host arithmetic, no GPU)
int dnmf_beta_plan(long m, long n, int k, long out[8]) {
    if (int rc = pair_plan_report<PAIR_BETA>("beta_plan", m, n, k, out)) return rc;
    out[6] = masked_reduce_grid(m, k);  // workgroups (256 outputs each per grid-stride trip) of the W side's ending
    out[7] = masked_reduce_grid(k, n);  // and of the H side's
    return DNMF_OK;
}

int dnmf_beta_aht_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                       float beta, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta_aht_pair");
    REQUIRE_BETA("beta_aht_pair");
    REQUIRE(num && den, "beta_aht_pair: null pointer or bad shape");
    return pair_w_side<PAIR_BETA>("beta_aht_pair", A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, nullptr, ws, ws_bytes, stream,
                                  beta_exp(beta));
}

int dnmf_beta_wta_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                       float beta, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta_wta_pair");
    REQUIRE_BETA("beta_wta_pair");
    REQUIRE(num && den, "beta_wta_pair: null pointer or bad shape");
    return pair_h_side<PAIR_BETA>("beta_wta_pair", A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, nullptr, 0, ws, ws_bytes, stream,
                                  beta_exp(beta));
}

int dnmf_beta_update_w(const float* A, long m, long n, long lda, float* W, long ldw, const float* H, long ldh, int k, float eps,
                       float beta, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta_update_w");
    REQUIRE_BETA("beta_update_w");
    return pair_w_side<PAIR_BETA>("beta_update_w", A, m, n, lda, W, ldw, H, ldh, k, eps, nullptr, nullptr, 0, W, ws, ws_bytes, stream,
                                  beta_exp(beta));
}

int dnmf_beta_update_h(const float* A, long m, long n, long lda, const float* W, long ldw, float* H, long ldh, int k, float eps,
                       float beta, int clamp, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta_update_h");
    REQUIRE_BETA("beta_update_h");
    return pair_h_side<PAIR_BETA>("beta_update_h", A, m, n, lda, W, ldw, H, ldh, k, eps, nullptr, nullptr, 0, H, clamp != 0, ws, ws_bytes,
                                  stream, beta_exp(beta));
}

int dnmf_beta_ratio_update(float* X, long rows, long cols, long ldx, const float* num, const float* den, long ldo, float eps, float beta,
                           int clamp, void* stream) {
    REQUIRE_BETA("beta_ratio_update");
    REQUIRE(X && num && den && rows >= 1 && cols >= 1 && ldx >= cols && ldo >= cols, "beta_ratio_update: null pointer or bad shape");
    const unsigned grid = (unsigned)masked_reduce_grid(rows, cols);
    hipLaunchKernelGGL(beta_ratio_kernel, dim3(grid), dim3(256), 0, S(stream), X, rows, cols, ldx, num, den, ldo, eps, clamp != 0,
                       beta_gamma(beta));
    return check_launch("beta_ratio_update");
}

int dnmf_beta_divergence(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                         float beta, double* out, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta_divergence");
    const int kt = kt_of(k);
    REQUIRE_BETA("beta_divergence");
    REQUIRE(kt > 0, "beta_divergence: rank k=%d unsupported (1 <= k <= %d for the beta-divergence kernels)", k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && out && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n, "beta_divergence: null pointer or bad shape");
    const size_t need = beta_div_bytes(m, n);
    if (!ws || ws_bytes < need || !aligned16(ws)) return fail(DNMF_EWS, "beta_divergence: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = S(stream);
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    const long tiles = a.nrowblk * a.ncolblk;
    double* P = (double*)ws;
    const dim3 grid((unsigned)cdiv(tiles, 4)), block(256);
    const int form = beta == 1.f ? BETA_DIV_KL : (beta == 0.f ? BETA_DIV_IS : BETA_DIV_GEN);
    const float c = form == BETA_DIV_GEN ? (float)(1.0 / ((double)beta * ((double)beta - 1.0))) : 1.f;
#define BD_FORM(KT_, FAST_)                                                                                                        \
    {                                                                                                                              \
        if (form == BETA_DIV_KL) hipLaunchKernelGGL((beta_div_kernel<KT_, FAST_, BETA_DIV_KL>), grid, block, 0, st, a, P, beta, c);      \
        else if (form == BETA_DIV_IS) hipLaunchKernelGGL((beta_div_kernel<KT_, FAST_, BETA_DIV_IS>), grid, block, 0, st, a, P, beta, c); \
        else hipLaunchKernelGGL((beta_div_kernel<KT_, FAST_, BETA_DIV_GEN>), grid, block, 0, st, a, P, beta, c);                         \
    }
#define BD_CASE(KT_)                  \
    if (kt == KT_) {                  \
        if (fast) BD_FORM(KT_, true)  \
        else BD_FORM(KT_, false)      \
    }
    BD_CASE(1) BD_CASE(2) BD_CASE(4)
#undef BD_CASE
#undef BD_FORM
    if (int rc = check_launch("beta_divergence")) return rc;
    hipLaunchKernelGGL(is_div_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)P, tiles, out);
    return check_launch("beta_divergence");
}

// ---- the per-column statistic of an NMFk sweep under norm='beta' (include/dnmf_beta_nmfk_api.h): the masked per-column error's plan
// and pair slab as they are
size_t dnmf_beta_column_div_ws_bytes(long m, long n, int k) {
    if (kt_of(k) < 0 || m < 1 || n < 1) return 0;
    return align256(plan_masked_colerr(m, n, 2).bytes);
}

int dnmf_beta_column_div_plan(long m, long n, int k, long out[3]) {
    REQUIRE(kt_of(k) > 0, "beta_column_div_plan: rank k=%d unsupported (1 <= k <= %d for the beta-divergence kernels)", k, DNMF_TUNED_MAX_K);
    REQUIRE(out && m >= 1 && n >= 1, "beta_column_div_plan: null pointer or bad shape");
    const MaskedColerrPlan c = plan_masked_colerr(m, n, 2);
    out[0] = c.rowblks_per_chunk;       // 32-row blocks a wave walks (the last chunk may hold fewer)
    out[1] = c.nchunks;
    out[2] = c.ncolblk;                 // 128-column blocks (the last may be ragged)
    return DNMF_OK;
}

int dnmf_beta_column_div(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                         float beta, double* div, double* pw, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta_column_div");
    const int kt = kt_of(k);
    REQUIRE_BETA("beta_column_div");
    REQUIRE(kt > 0, "beta_column_div: rank k=%d unsupported (1 <= k <= %d for the beta-divergence kernels)", k, DNMF_TUNED_MAX_K);
    REQUIRE(A && W && H && div && pw && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n, "beta_column_div: null pointer or bad shape");
    const MaskedColerrPlan cp = plan_masked_colerr(m, n, 2);
    if (!ws || ws_bytes < cp.bytes || !aligned16(ws)) return fail(DNMF_EWS, "beta_column_div: workspace %zu < %zu bytes", ws_bytes, cp.bytes);
    hipStream_t st = S(stream);
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    double* P = (double*)ws;
    const dim3 grid((unsigned)cdiv(cp.nchunks * cp.ncolblk, 4)), block(256);
    const int form = beta == 1.f ? BETA_DIV_KL : (beta == 0.f ? BETA_DIV_IS : BETA_DIV_GEN);
    const float c = form == BETA_DIV_GEN ? (float)(1.0 / ((double)beta * ((double)beta - 1.0))) : 1.f;
#define BC_LAUNCH(KT_, FAST_, FORM_) \
    hipLaunchKernelGGL((beta_coldiv_kernel<KT_, FAST_, FORM_>), grid, block, 0, st, a, P, cp.ldc, cp.rowblks_per_chunk, beta, c)
#define BC_FORM(KT_, FAST_)                                            \
    {                                                                  \
        if (form == BETA_DIV_KL) BC_LAUNCH(KT_, FAST_, BETA_DIV_KL);   \
        else if (form == BETA_DIV_IS) BC_LAUNCH(KT_, FAST_, BETA_DIV_IS); \
        else BC_LAUNCH(KT_, FAST_, BETA_DIV_GEN);                      \
    }
#define BC_CASE(KT_)                  \
    if (kt == KT_) {                  \
        if (fast) BC_FORM(KT_, true)  \
        else BC_FORM(KT_, false)      \
    }
    BC_CASE(1) BC_CASE(2) BC_CASE(4)
#undef BC_CASE
#undef BC_FORM
#undef BC_LAUNCH
    if (int rc = check_launch("beta_column_div")) return rc;
    hipLaunchKernelGGL(masked_colerr_reduce_kernel, dim3((unsigned)std::min<long>(cdiv(n, 256), 4096)), dim3(256), 0, st, (const double*)P,
                       cp.ldc, cp.nchunks, n, div, pw);
    return check_launch("beta_column_div");
}

// a whole beta-divergence fit: the chain of csrc/dnmf_masked.h with the beta steps; its error is the Frobenius pair, as after dnmf_is_mu_fit
int dnmf_beta_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, float beta,
                     int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta_mu_fit");
    REQUIRE_BETA("beta_mu_fit");
    return pair_mu_fit<PAIR_BETA>(
        "beta_mu_fit", beta_step_bytes, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, sq_out, ws, ws_bytes, stream,
        [&](size_t step) { return dnmf_beta_update_w(A, m, n, lda, W, ldw, H, ldh, k, eps, beta, ws, step, stream); },
        [&](int clamp, size_t step) { return dnmf_beta_update_h(A, m, n, lda, W, ldw, H, ldh, k, eps, beta, clamp, ws, step, stream); },
        [&](double* sq) { return dnmf_resid_sqnorm(A, m, n, lda, W, ldw, H, ldh, k, sq, stream); },
        [&](double* sq) { return dnmf_sqnorm(A, m, n, lda, sq, stream); });
}

}  // extern "C"
