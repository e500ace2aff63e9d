// dnmf_masked.hip -- C ABI of the masked MU rules on DENSE data whose missing entries are NaN: the masked modes of the pair launch
// path of csrc/dnmf_masked.h behind their ABI names, and the error kernels of a masked block with their plans.  A translation unit
// of its own (see csrc/dnmf_kl.hip).  Plain launch chains: no workgroup waits for another one; no float atomics in the products.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_masked.h"

namespace {

// the two masked modes of the one launch path (csrc/dnmf_masked.h), picked by the ABI's `kl`
int masked_w_side(const char* who, const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                  float eps, int kl, float* num, float* den, long ldo, float* X, void* ws, size_t ws_bytes, void* stream) {
    return kl ? pair_w_side<PAIR_KL>(who, A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, X, ws, ws_bytes, stream)
              : pair_w_side<PAIR_FRO>(who, A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, X, ws, ws_bytes, stream);
}

int masked_h_side(const char* who, const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                  float eps, int kl, float* num, float* den, long ldo, float* X, int clamp, void* ws, size_t ws_bytes, void* stream) {
    return kl ? pair_h_side<PAIR_KL>(who, A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, X, clamp, ws, ws_bytes, stream)
              : pair_h_side<PAIR_FRO>(who, A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, X, clamp, ws, ws_bytes, stream);
}

}  // namespace

extern "C" {

size_t dnmf_masked_ws_bytes(long m, long n, int k) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1) return 0;
    return pair_step_bytes<PAIR_FRO>(m, n, kt);
}

int dnmf_masked_plan(long m, long n, int k, long out[6]) { return pair_plan_report<PAIR_FRO>("masked_plan", m, n, k, out); }

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

size_t dnmf_masked_column_err_ws_bytes(long m, long n, int k) { return col_sums_ws_bytes(m, n, k, MaskedErrTerm::NSUM); }

int dnmf_masked_column_err_plan(long m, long n, int k, long out[3]) {
    return col_sums_plan_report("masked_column_err_plan", PairMode<PAIR_FRO>::serves, m, n, k, MaskedErrTerm::NSUM, out);
}

int dnmf_masked_column_err(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, double* num,
                           double* den, void* ws, size_t ws_bytes, void* stream) {
    return col_sums("masked_column_err", PairMode<PAIR_FRO>::serves, A, m, n, lda, W, ldw, H, ldh, k, 0.f, MaskedErrTerm{}, num, den, ws,
                    ws_bytes, stream);
}

size_t dnmf_masked_ws_bytes_fit(long m, long n, int k) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1) return 0;
    return pair_fit_layout(pair_step_bytes<PAIR_FRO>(m, n, kt), k).total;
}

// a whole masked fit: the chain of csrc/dnmf_masked.h with the masked steps and the error over the observed positions
int dnmf_masked_mu_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int kl,
                       int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream) {
    return pair_mu_fit<PAIR_FRO>(
        "masked_mu_fit", pair_step_bytes<PAIR_FRO>, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, sq_out, ws, ws_bytes, stream,
        [&](size_t step) { return dnmf_masked_update_w(A, m, n, lda, W, ldw, H, ldh, k, eps, kl, ws, step, stream); },
        [&](int clamp, size_t step) { return dnmf_masked_update_h(A, m, n, lda, W, ldw, H, ldh, k, eps, kl, clamp, ws, step, stream); },
        [&](double* sq) { return dnmf_masked_resid_sqnorm(A, m, n, lda, W, ldw, H, ldh, k, sq, stream); },
        [&](double* sq) { return dnmf_masked_sqnorm(A, m, n, lda, sq, stream); });
}

}  // extern "C"
