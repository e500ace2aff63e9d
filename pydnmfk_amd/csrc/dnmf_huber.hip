// dnmf_huber.hip -- C ABI of the Huber loss by reweighted MU on dense data, delta > 0: the PAIR_HUBER mode of the pair launch path of
// csrc/dnmf_masked.h behind its ABI names, and the objective (csrc/dnmf_huber.h).  A translation unit of its own (see csrc/dnmf_kl.hip).
// Plain launch chains: no workgroup waits for another one; no float atomics in the products or the objective.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_huber.h"

// every entry point that takes a workspace refuses a misaligned one first (include/dnmf.h: the workspace contract), then a delta that is
// not a positive number
#define REQUIRE_DELTA(who) REQUIRE(huber_delta_ok(delta), who ": delta=%g is not accepted (delta > 0; inf is the Frobenius objective)", (double)delta)

extern "C" {

// ONE query for every entry point below: the whole fit's layout, whose first bytes are a step's slabs and the objective's slots
size_t dnmf_huber_ws_bytes(long m, long n, int k) { return div_ws_bytes<PAIR_HUBER>(m, n, k, true); }

int dnmf_huber_uht_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                        float delta, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "huber_uht_pair");
    REQUIRE_DELTA("huber_uht_pair");
    REQUIRE(num && den, "huber_uht_pair: null pointer or bad shape");
    return pair_w_side<PAIR_HUBER>("huber_uht_pair", A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, nullptr, ws, ws_bytes, stream,
                                   huber_exp(delta));
}

int dnmf_huber_wtu_pair(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                        float delta, float* num, float* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "huber_wtu_pair");
    REQUIRE_DELTA("huber_wtu_pair");
    REQUIRE(num && den, "huber_wtu_pair: null pointer or bad shape");
    return pair_h_side<PAIR_HUBER>("huber_wtu_pair", A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, nullptr, 0, ws, ws_bytes, stream,
                                   huber_exp(delta));
}

int dnmf_huber_update_w(const float* A, long m, long n, long lda, float* W, long ldw, const float* H, long ldh, int k, float eps,
                        float delta, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "huber_update_w");
    REQUIRE_DELTA("huber_update_w");
    return pair_w_side<PAIR_HUBER>("huber_update_w", A, m, n, lda, W, ldw, H, ldh, k, eps, nullptr, nullptr, 0, W, ws, ws_bytes, stream,
                                   huber_exp(delta));
}

int dnmf_huber_update_h(const float* A, long m, long n, long lda, const float* W, long ldw, float* H, long ldh, int k, float eps,
                        float delta, int clamp, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "huber_update_h");
    REQUIRE_DELTA("huber_update_h");
    return pair_h_side<PAIR_HUBER>("huber_update_h", A, m, n, lda, W, ldw, H, ldh, k, eps, nullptr, nullptr, 0, H, clamp != 0, ws, ws_bytes,
                                   stream, huber_exp(delta));
}

int dnmf_huber_loss(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                    float delta, double* out, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "huber_loss");
    REQUIRE_DELTA("huber_loss");
    return tile_sum("huber_loss", PairMode<PAIR_HUBER>::serves, A, m, n, lda, W, ldw, H, ldh, k, eps, HuberTerm{delta}, out, ws, ws_bytes,
                    stream);
}

// a whole Huber fit: the chain of csrc/dnmf_masked.h with the Huber steps; its error is the Frobenius pair, as after dnmf_beta_mu_fit
int dnmf_huber_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, float delta,
                      int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "huber_mu_fit");
    REQUIRE_DELTA("huber_mu_fit");
    return pair_mu_fit<PAIR_HUBER>(
        "huber_mu_fit", div_step_bytes<PAIR_HUBER>, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, sq_out, ws, ws_bytes, stream,
        [&](size_t step) { return dnmf_huber_update_w(A, m, n, lda, W, ldw, H, ldh, k, eps, delta, ws, step, stream); },
        [&](int clamp, size_t step) { return dnmf_huber_update_h(A, m, n, lda, W, ldw, H, ldh, k, eps, delta, clamp, ws, step, stream); },
        [&](double* sq) { return dnmf_resid_sqnorm(A, m, n, lda, W, ldw, H, ldh, k, sq, stream); },
        [&](double* sq) { return dnmf_sqnorm(A, m, n, lda, sq, stream); });
}

}  // extern "C"
