// dnmf_beta.hip -- C ABI of the beta-divergence MU rule on dense data, -2 <= beta <= 4: the PAIR_BETA mode of the pair launch path of
// csrc/dnmf_masked.h behind its ABI names, the rule on a stored pair, the divergence and its per-column sums (csrc/dnmf_beta.h).  A translation unit of its own
// (see csrc/dnmf_kl.hip).  Plain launch chains: no workgroup waits for another one; no float atomics in the products or the divergence.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_beta.h"

// every entry point that takes a workspace refuses a misaligned one first (include/dnmf.h: the workspace contract), then a beta
// outside the accepted range
#define REQUIRE_BETA(who) REQUIRE(beta_ok(beta), who ": beta=%g is outside the accepted range -2 <= beta <= 4", (double)beta)

extern "C" {

size_t dnmf_beta_ws_bytes(long m, long n, int k) { return div_ws_bytes<PAIR_BETA>(m, n, k, false); }

size_t dnmf_beta_ws_bytes_fit(long m, long n, int k) { return div_ws_bytes<PAIR_BETA>(m, n, k, true); }

int dnmf_beta_plan(long m, long n, int k, long out[8]) { return div_plan_report<PAIR_BETA>("beta_plan", m, n, k, out); }

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
    return pair_ratio_update<PAIR_BETA>("beta_ratio_update", X, rows, cols, ldx, num, den, ldo, eps, clamp, stream, beta_gamma(beta));
}

int dnmf_beta_divergence(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                         float beta, double* out, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta_divergence");
    REQUIRE_BETA("beta_divergence");
    return with_beta_term<1>(beta, [&](auto term) {
        return tile_sum("beta_divergence", PairMode<PAIR_BETA>::serves, A, m, n, lda, W, ldw, H, ldh, k, eps, term, out, ws, ws_bytes, stream);
    });
}

// ---- the per-column statistic of an NMFk sweep under norm='beta' (include/dnmf_beta_nmfk_api.h): the masked per-column error's plan
// and pair slab as they are
size_t dnmf_beta_column_div_ws_bytes(long m, long n, int k) { return col_sums_ws_bytes(m, n, k, 2); }

int dnmf_beta_column_div_plan(long m, long n, int k, long out[3]) {
    return col_sums_plan_report("beta_column_div_plan", PairMode<PAIR_BETA>::serves, m, n, k, 2, out);
}

int dnmf_beta_column_div(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                         float beta, double* div, double* pw, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta_column_div");
    REQUIRE_BETA("beta_column_div");
    return with_beta_term<2>(beta, [&](auto term) {
        return col_sums("beta_column_div", PairMode<PAIR_BETA>::serves, A, m, n, lda, W, ldw, H, ldh, k, eps, term, div, pw, ws, ws_bytes,
                        stream);
    });
}

// a whole beta-divergence fit: the chain of csrc/dnmf_masked.h with the beta steps; its error is the Frobenius pair, as after dnmf_is_mu_fit
int dnmf_beta_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, float beta,
                     int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta_mu_fit");
    REQUIRE_BETA("beta_mu_fit");
    return pair_mu_fit<PAIR_BETA>(
        "beta_mu_fit", div_step_bytes<PAIR_BETA>, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, sq_out, ws, ws_bytes, stream,
        [&](size_t step) { return dnmf_beta_update_w(A, m, n, lda, W, ldw, H, ldh, k, eps, beta, ws, step, stream); },
        [&](int clamp, size_t step) { return dnmf_beta_update_h(A, m, n, lda, W, ldw, H, ldh, k, eps, beta, clamp, ws, step, stream); },
        [&](double* sq) { return dnmf_resid_sqnorm(A, m, n, lda, W, ldw, H, ldh, k, sq, stream); },
        [&](double* sq) { return dnmf_sqnorm(A, m, n, lda, sq, stream); });
}

}  // extern "C"
