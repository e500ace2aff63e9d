// dnmf_weighted.hip -- C ABI of the MU pair rules under per-entry weights (include/dnmf_weighted_api.h): the kernels of
// csrc/dnmf_weighted.h behind their ABI names, for the four norms (0 fro, 1 kl, 2 is, 3 beta).  A translation unit of its own (see
// csrc/dnmf_kl.hip).  Plain launch chains: no workgroup waits for another one; no float atomics in the products or the sums.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_weighted.h"

// every entry point that takes a workspace refuses a misaligned one first (include/dnmf.h: the workspace contract), then a norm it does
// not know and, under norm 3, a beta outside the accepted range
#define REQUIRE_NORM(who)                                                                                                     \
    REQUIRE(norm >= 0 && norm <= 3, who ": norm=%d is not known (0 fro, 1 kl, 2 is, 3 beta)", norm);                          \
    REQUIRE(norm != 3 || beta_ok(beta), who ": beta=%g is outside the accepted range -2 <= beta <= 4", (double)beta)

namespace {
inline PairExp weighted_exp(int norm, float beta) { return norm == 3 ? beta_exp(beta) : PairExp{}; }
}  // namespace

extern "C" {

size_t dnmf_weighted_ws_bytes(long m, long n, int k) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1) return 0;
    return weighted_step_bytes(m, n, kt);
}

size_t dnmf_weighted_ws_bytes_fit(long m, long n, int k) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1) return 0;
    return pair_fit_layout(weighted_step_bytes(m, n, kt), k).total;
}

int dnmf_weighted_plan(long m, long n, int k, int norm, long out[8]) {
    const float beta = 0.f;
    REQUIRE_NORM("weighted_plan");
    return with_weighted_mode(norm, [&](auto mode) { return div_plan_report<mode.value>("weighted_plan", m, n, k, out); });
}

int dnmf_weighted_aht_pair(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, const float* H,
                           long ldh, int k, float eps, int norm, float beta, float* num, float* den, long ldo, void* ws, size_t ws_bytes,
                           void* stream) {
    REQUIRE_WS16(ws, "weighted_aht_pair");
    REQUIRE_NORM("weighted_aht_pair");
    REQUIRE(num && den, "weighted_aht_pair: null pointer or bad shape");
    return with_weighted_mode(norm, [&](auto mode) {
        return weighted_w_side<mode.value>("weighted_aht_pair", A, m, n, lda, V, ldv, W, ldw, H, ldh, k, eps, num, den, ldo, nullptr, ws,
                                           ws_bytes, stream, weighted_exp(norm, beta));
    });
}

int dnmf_weighted_wta_pair(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, const float* H,
                           long ldh, int k, float eps, int norm, float beta, float* num, float* den, long ldo, void* ws, size_t ws_bytes,
                           void* stream) {
    REQUIRE_WS16(ws, "weighted_wta_pair");
    REQUIRE_NORM("weighted_wta_pair");
    REQUIRE(num && den, "weighted_wta_pair: null pointer or bad shape");
    return with_weighted_mode(norm, [&](auto mode) {
        return weighted_h_side<mode.value>("weighted_wta_pair", A, m, n, lda, V, ldv, W, ldw, H, ldh, k, eps, num, den, ldo, nullptr, 0, ws,
                                           ws_bytes, stream, weighted_exp(norm, beta));
    });
}

int dnmf_weighted_update_w(const float* A, long m, long n, long lda, const float* V, long ldv, float* W, long ldw, const float* H, long ldh,
                           int k, float eps, int norm, float beta, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "weighted_update_w");
    REQUIRE_NORM("weighted_update_w");
    return with_weighted_mode(norm, [&](auto mode) {
        return weighted_w_side<mode.value>("weighted_update_w", A, m, n, lda, V, ldv, W, ldw, H, ldh, k, eps, nullptr, nullptr, 0, W, ws,
                                           ws_bytes, stream, weighted_exp(norm, beta));
    });
}

int dnmf_weighted_update_h(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, float* H, long ldh,
                           int k, float eps, int norm, float beta, int clamp, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "weighted_update_h");
    REQUIRE_NORM("weighted_update_h");
    return with_weighted_mode(norm, [&](auto mode) {
        return weighted_h_side<mode.value>("weighted_update_h", A, m, n, lda, V, ldv, W, ldw, H, ldh, k, eps, nullptr, nullptr, 0, H,
                                           clamp != 0, ws, ws_bytes, stream, weighted_exp(norm, beta));
    });
}

// sq (device) = {sum v (a - s)^2, sum v a^2} over v > 0, s = W H without eps: the weighted error pair
int dnmf_weighted_resid_sqnorm(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, const float* H,
                               long ldh, int k, double* sq, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "weighted_resid_sqnorm");
    return weighted_tile_sum("weighted_resid_sqnorm", A, m, n, lda, V, ldv, W, ldw, H, ldh, k, 0.f, WeightedErrTerm<2>{1.f}, sq, ws,
                             ws_bytes, stream);
}

// *out (device) = sum v d(a | s + eps) of the norm (kl, is, beta); under fro half the weighted squared residual (s without eps)
int dnmf_weighted_divergence(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, const float* H,
                             long ldh, int k, float eps, int norm, float beta, double* out, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "weighted_divergence");
    REQUIRE_NORM("weighted_divergence");
    auto run = [&](auto term) {
        return weighted_tile_sum("weighted_divergence", A, m, n, lda, V, ldv, W, ldw, H, ldh, k, eps, term, out, ws, ws_bytes, stream);
    };
    if (norm == 0) return run(WeightedErrTerm<1>{0.5f});
    if (norm == 1) return run(WeightedDivTerm<BETA_DIV_KL>{});
    if (norm == 2) return run(WeightedDivTerm<BETA_DIV_IS>{});
    const BetaForm bf = beta_form(beta);
    if (bf.form == BETA_DIV_KL) return run(WeightedDivTerm<BETA_DIV_KL>{});
    if (bf.form == BETA_DIV_IS) return run(WeightedDivTerm<BETA_DIV_IS>{});
    return run(WeightedDivTerm<BETA_DIV_GEN>{beta, bf.c});
}

// ---- the per-column statistic of an NMFk sweep under weights (include/dnmf_weighted_nmfk_api.h): the masked per-column error's plan
// and pair slab as they are, weighted_col_sums_kernel in the walk's place
size_t dnmf_weighted_column_div_ws_bytes(long m, long n, int k) { return col_sums_ws_bytes(m, n, k, 2); }

int dnmf_weighted_column_div_plan(long m, long n, int k, long out[3]) {
    return col_sums_plan_report("weighted_column_div_plan", "the weighted kernels", m, n, k, 2, out);
}

int dnmf_weighted_column_div(const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw, const float* H,
                             long ldh, int k, float eps, int norm, float beta, double* num, double* den, void* ws, size_t ws_bytes,
                             void* stream) {
    REQUIRE_WS16(ws, "weighted_column_div");
    REQUIRE_NORM("weighted_column_div");
    auto run = [&](auto term) {
        return weighted_col_sums("weighted_column_div", A, m, n, lda, V, ldv, W, ldw, H, ldh, k, eps, term, num, den, ws, ws_bytes, stream);
    };
    if (norm == 0) return run(WeightedColErrTerm{});
    const BetaForm bf = norm == 3 ? beta_form(beta) : BetaForm{norm == 1 ? BETA_DIV_KL : BETA_DIV_IS, 1.f};
    if (bf.form == BETA_DIV_KL) return run(WeightedColDivTerm<BETA_DIV_KL>{});
    if (bf.form == BETA_DIV_IS) return run(WeightedColDivTerm<BETA_DIV_IS>{});
    return run(WeightedColDivTerm<BETA_DIV_GEN>{beta, bf.c});
}

// a whole weighted fit: the chain of csrc/dnmf_masked.h with the weighted steps; sq_out is the weighted error pair
int dnmf_weighted_mu_fit(const float* A, long m, long n, long lda, const float* V, long ldv, float* W, long ldw, float* H, long ldh, int k,
                         float eps, int norm, float beta, int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "weighted_mu_fit");
    REQUIRE_NORM("weighted_mu_fit");
    REQUIRE(V && ldv >= n, "weighted_mu_fit: null pointer or bad shape");
    return with_weighted_mode(norm, [&](auto mode) {
        return pair_mu_fit<mode.value>(
            "weighted_mu_fit", weighted_step_bytes, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, sq_out, ws, ws_bytes, stream,
            [&](size_t step) { return dnmf_weighted_update_w(A, m, n, lda, V, ldv, W, ldw, H, ldh, k, eps, norm, beta, ws, step, stream); },
            [&](int clamp, size_t step) {
                return dnmf_weighted_update_h(A, m, n, lda, V, ldv, W, ldw, H, ldh, k, eps, norm, beta, clamp, ws, step, stream);
            },
            // both sums come from one walk, through the step's slabs (free by now) into the fit's pair of doubles
            [&](double* sq) {
                return dnmf_weighted_resid_sqnorm(A, m, n, lda, V, ldv, W, ldw, H, ldh, k, sq, ws, weighted_step_bytes(m, n, kt_of(k)), stream);
            },
            [&](double*) { return (int)DNMF_OK; });
    });
}

}  // extern "C"
