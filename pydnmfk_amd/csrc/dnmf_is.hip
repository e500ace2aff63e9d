// dnmf_is.hip -- C ABI of the Itakura-Saito MU rule on dense strictly positive data: the PAIR_IS mode of the pair launch path of
// csrc/dnmf_masked.h behind its ABI names, the rule on a stored pair, the divergence and its per-column form (csrc/dnmf_is.h).  A translation unit of its own
// (see csrc/dnmf_kl.hip).  Plain launch chains: no workgroup waits for another one; no float atomics in the products or the divergence.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_is.h"

extern "C" {

size_t dnmf_is_ws_bytes(long m, long n, int k) { return div_ws_bytes<PAIR_IS>(m, n, k, false); }

size_t dnmf_is_ws_bytes_fit(long m, long n, int k) { return div_ws_bytes<PAIR_IS>(m, n, k, true); }

int dnmf_is_plan(long m, long n, int k, long out[8]) { return div_plan_report<PAIR_IS>("is_plan", m, n, k, out); }

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
    return pair_ratio_update<PAIR_IS>("is_ratio_update", X, rows, cols, ldx, num, den, ldo, eps, clamp, stream);
}

int dnmf_is_divergence(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                       double* out, void* ws, size_t ws_bytes, void* stream) {
    return tile_sum("is_divergence", PairMode<PAIR_IS>::serves, A, m, n, lda, W, ldw, H, ldh, k, eps, IsDivTerm{}, out, ws, ws_bytes, stream);
}

size_t dnmf_is_column_div_ws_bytes(long m, long n, int k) { return col_sums_ws_bytes(m, n, k, IsDivTerm::NSUM); }

int dnmf_is_column_div_plan(long m, long n, int k, long out[3]) {
    return col_sums_plan_report("is_column_div_plan", PairMode<PAIR_IS>::serves, m, n, k, IsDivTerm::NSUM, out);
}

int dnmf_is_column_div(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                       double* div, void* ws, size_t ws_bytes, void* stream) {
    return col_sums("is_column_div", PairMode<PAIR_IS>::serves, A, m, n, lda, W, ldw, H, ldh, k, eps, IsDivTerm{}, div, nullptr, ws, ws_bytes,
                    stream);
}

// a whole Itakura-Saito fit: the chain of csrc/dnmf_masked.h with the IS steps; its error is the Frobenius pair, as after dnmf_mu_kl_fit
int dnmf_is_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
                   int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream) {
    return pair_mu_fit<PAIR_IS>(
        "is_mu_fit", div_step_bytes<PAIR_IS>, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, sq_out, ws, ws_bytes, stream,
        [&](size_t step) { return dnmf_is_update_w(A, m, n, lda, W, ldw, H, ldh, k, eps, ws, step, stream); },
        [&](int clamp, size_t step) { return dnmf_is_update_h(A, m, n, lda, W, ldw, H, ldh, k, eps, clamp, ws, step, stream); },
        [&](double* sq) { return dnmf_resid_sqnorm(A, m, n, lda, W, ldw, H, ldh, k, sq, stream); },
        [&](double* sq) { return dnmf_sqnorm(A, m, n, lda, sq, stream); });
}

}  // extern "C"
