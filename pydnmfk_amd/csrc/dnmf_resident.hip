// dnmf_resident.hip -- C ABI of the resident pair-rule fits (csrc/dnmf_resident.h, include/dnmf_resident_api.h): the plan of a shape as
// numbers, and the launch of a batch of whole Itakura-Saito / beta-divergence MU fits, one workgroup per problem -- or, under per-entry
// weights, of whole fro / kl / is / beta fits (pair_resident_weighted_kernel).  A translation unit of its own (see csrc/dnmf_kl.hip).
// One launch per call; no workgroup waits for another one; no workspace.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_resident.h"

namespace {

// the dynamic LDS a workgroup may ask for on the current device, and the opt-in of every instantiation up to it: once per DEVICE (a
// process may drive several GPUs, and hipFuncSetAttribute acts on the current one).  0: no device, or the query failed
constexpr int RS_MAX_DEVICES = 64;
typedef void (*ResidentKernel)(ResidentArgs);

template <int KT, bool FAST>
ResidentKernel resident_kernel(int mode) {
    return mode == DNMF_RESIDENT_IS ? pair_resident_kernel<KT, FAST, PAIR_IS> : pair_resident_kernel<KT, FAST, PAIR_BETA>;
}
ResidentKernel resident_kernel(int mode, int kp, bool fast) {
    if (kp == 16) return fast ? resident_kernel<1, true>(mode) : resident_kernel<1, false>(mode);
    return fast ? resident_kernel<2, true>(mode) : resident_kernel<2, false>(mode);
}

// the weighted kernels, by the norm of dnmf_weighted_* (0 fro, 1 kl, 2 is, 3 beta)
typedef void (*ResidentWeightedKernel)(ResidentArgs, ResidentWeights);

template <int KT, bool FAST>
ResidentWeightedKernel resident_weighted_kernel(int norm) {
    if (norm == 0) return pair_resident_weighted_kernel<KT, FAST, PAIR_FRO>;
    if (norm == 1) return pair_resident_weighted_kernel<KT, FAST, PAIR_KL>;
    return norm == 2 ? pair_resident_weighted_kernel<KT, FAST, PAIR_IS> : pair_resident_weighted_kernel<KT, FAST, PAIR_BETA>;
}
ResidentWeightedKernel resident_weighted_kernel(int norm, int kp, bool fast) {
    if (kp == 16) return fast ? resident_weighted_kernel<1, true>(norm) : resident_weighted_kernel<1, false>(norm);
    return fast ? resident_weighted_kernel<2, true>(norm) : resident_weighted_kernel<2, false>(norm);
}

size_t resident_lds_limit() {
    static size_t limit_of[RS_MAX_DEVICES];
    static bool have[RS_MAX_DEVICES] = {};
    int dev = 0, lim = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= RS_MAX_DEVICES) { clear_hip_error(); return 0; }
    if (have[dev]) return limit_of[dev];
    if (hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || lim < 0) { clear_hip_error(); return 0; }
    const size_t limit = std::min<size_t>((size_t)lim, RS_LDS_MAX);
    for (int mode : {DNMF_RESIDENT_IS, DNMF_RESIDENT_BETA})
        for (int kp : {16, 32})
            for (bool fast : {false, true}) allow_lds(resident_kernel(mode, kp, fast), limit);
    for (int norm = 0; norm < 4; ++norm)
        for (int kp : {16, 32})
            for (bool fast : {false, true}) allow_lds(resident_weighted_kernel(norm, kp, fast), limit);
    clear_hip_error();
    limit_of[dev] = limit;
    have[dev] = true;
    return limit;
}

}  // namespace

extern "C" {

int dnmf_pair_resident_plan(long m, long n, int k, long out[8]) {
    REQUIRE(out && m >= 1 && n >= 1, "pair_resident_plan: null pointer or bad shape");
    const ResidentPlan r = plan_resident(m, n, k);
    out[0] = r.eligible;
    out[1] = r.kp ? (long)std::min<size_t>(r.lds, (size_t)1 << 62) : 0;     // bytes of dynamic LDS (0: the rank is not served)
    out[2] = r.kp;
    out[3] = RS_NW;
    out[4] = cdiv(r.rowtiles, RS_NW);   // 16-row tiles the busiest wave walks in a W phase (each over all column tiles)
    out[5] = cdiv(r.coltiles, RS_NW);   // 16-column tiles the busiest wave walks in an H phase (each over all row tiles)
    out[6] = r.rowtiles;
    out[7] = r.coltiles;
    return DNMF_OK;
}

int dnmf_pair_resident_fit_batch(int mode, float beta, const float* A, long a_stride, long lda, float* W, long w_stride, long ldw, float* H,
                                 long h_stride, long ldh, long m, long n, int k, float eps, int w_update, int itr, int batch,
                                 double* sq_out, void* stream) {
    const char* who = "pair_resident_fit_batch";
    REQUIRE(mode == DNMF_RESIDENT_IS || mode == DNMF_RESIDENT_BETA, "%s: mode %d (DNMF_RESIDENT_IS or DNMF_RESIDENT_BETA)", who, mode);
    if (mode == DNMF_RESIDENT_BETA) {
        REQUIRE(beta_ok(beta), "%s: beta=%g is outside the accepted range -2 <= beta <= 4", who, (double)beta);
        if (beta == 0.f) mode = DNMF_RESIDENT_IS;          // beta = 0 IS Itakura-Saito: its kernels, its bits (as PyNMF renames it)
    }
    REQUIRE(k >= 1 && k <= RS_MAX_K, "%s: rank k=%d unsupported (1 <= k <= %d for the resident fits)", who, k, RS_MAX_K);
    REQUIRE(A && W && H && sq_out && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && itr >= 0 && batch >= 1,
            "%s: null pointer or bad shape (m=%ld n=%ld k=%d itr=%d batch=%d)", who, m, n, k, itr, batch);
    REQUIRE(batch == 1 || (a_stride >= (m - 1) * lda + n && w_stride >= (m - 1) * ldw + k && h_stride >= (long)(k - 1) * ldh + n),
            "%s: the problems of a batch overlap (strides %ld %ld %ld)", who, a_stride, w_stride, h_stride);
    const ResidentPlan r = plan_resident(m, n, k);
    if (!r.eligible) return DNMF_RESIDENT_NOT_TAKEN;
    hipStream_t st = S(stream);
    if (r.lds > resident_lds_limit()) return DNMF_RESIDENT_NOT_TAKEN;      // the device's own limit: not taken rather than a failed launch
    ResidentArgs a{};
    a.A = A; a.a_stride = batch == 1 ? 0 : a_stride; a.lda = lda;
    a.W = W; a.w_stride = batch == 1 ? 0 : w_stride; a.ldw = ldw;
    a.H = H; a.h_stride = batch == 1 ? 0 : h_stride; a.ldh = ldh;
    a.m = (int)m; a.n = (int)n; a.k = k; a.eps = eps; a.w_update = w_update; a.itr = itr; a.sq = sq_out;
    if (mode == DNMF_RESIDENT_BETA) { const PairExp px = beta_exp(beta); a.pexp = px.e; a.gamma = px.gamma; }
    else a.gamma = 1.f;
    // the 16-byte loads of A: every row of every problem starts on a 16-byte boundary and holds whole vectors.  The choice changes how
    // A is fetched, never a sum: both forms give the same bits
    const bool fast = aligned16(A) && lda % 4 == 0 && n % 4 == 0 && a.a_stride % 4 == 0;
    hipLaunchKernelGGL(resident_kernel(mode, r.kp, fast), dim3((unsigned)batch), dim3(RS_T), r.lds, st, a);
    return check_launch(who);
}

int dnmf_pair_resident_weighted_fit_batch(int norm, float beta, const float* A, long a_stride, long lda, const float* V, long v_stride,
                                          long ldv, float* W, long w_stride, long ldw, float* H, long h_stride, long ldh, long m, long n,
                                          int k, float eps, int w_update, int itr, int batch, double* sq_out, void* stream) {
    const char* who = "pair_resident_weighted_fit_batch";
    REQUIRE(norm >= 0 && norm <= 3, "%s: norm=%d is not known (0 fro, 1 kl, 2 is, 3 beta)", who, norm);
    if (norm == 3) {
        REQUIRE(beta_ok(beta), "%s: beta=%g is outside the accepted range -2 <= beta <= 4", who, (double)beta);
        if (beta == 0.f) norm = 2;                         // beta = 0 IS Itakura-Saito: its kernels, its bits
    }
    REQUIRE(k >= 1 && k <= RS_MAX_K, "%s: rank k=%d unsupported (1 <= k <= %d for the resident fits)", who, k, RS_MAX_K);
    REQUIRE(A && V && W && H && sq_out && m >= 1 && n >= 1 && lda >= n && ldv >= n && ldw >= k && ldh >= n && itr >= 0 && batch >= 1,
            "%s: null pointer or bad shape (m=%ld n=%ld k=%d itr=%d batch=%d)", who, m, n, k, itr, batch);
    // (v_stride = 0: every problem reads the one V -- a sweep perturbs the data and keeps the weights)
    REQUIRE(batch == 1 || (a_stride >= (m - 1) * lda + n && w_stride >= (m - 1) * ldw + k && h_stride >= (long)(k - 1) * ldh + n &&
                           (v_stride == 0 || v_stride >= (m - 1) * ldv + n)),
            "%s: the problems of a batch overlap (strides %ld %ld %ld %ld)", who, a_stride, v_stride, w_stride, h_stride);
    const ResidentPlan r = plan_resident(m, n, k);
    if (!r.eligible) return DNMF_RESIDENT_NOT_TAKEN;
    hipStream_t st = S(stream);
    if (r.lds > resident_lds_limit()) return DNMF_RESIDENT_NOT_TAKEN;
    ResidentArgs a{};
    a.A = A; a.a_stride = batch == 1 ? 0 : a_stride; a.lda = lda;
    a.W = W; a.w_stride = batch == 1 ? 0 : w_stride; a.ldw = ldw;
    a.H = H; a.h_stride = batch == 1 ? 0 : h_stride; a.ldh = ldh;
    a.m = (int)m; a.n = (int)n; a.k = k; a.eps = eps; a.w_update = w_update; a.itr = itr; a.sq = sq_out;
    if (norm == 3) { const PairExp px = beta_exp(beta); a.pexp = px.e; a.gamma = px.gamma; }
    else a.gamma = 1.f;
    const ResidentWeights w{V, batch == 1 ? 0 : v_stride, ldv};
    // the 16-byte loads: they must hold for the rows of V as for the rows of A (one FAST for both; the bits do not depend on it)
    const bool fast = aligned16(A) && lda % 4 == 0 && n % 4 == 0 && a.a_stride % 4 == 0 && aligned16(V) && ldv % 4 == 0 && w.v_stride % 4 == 0;
    hipLaunchKernelGGL(resident_weighted_kernel(norm, r.kp, fast), dim3((unsigned)batch), dim3(RS_T), r.lds, st, a, w);
    return check_launch(who);
}

}  // extern "C"
