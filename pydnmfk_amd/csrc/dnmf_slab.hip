// dnmf_slab.hip -- C ABI of the slab pair-rule fits (csrc/dnmf_slab.h, include/dnmf_slab_api.h): the plan of a shape as numbers, and the
// whole Itakura-Saito / beta-divergence fits -- or, under per-entry weights, fro / kl / is / beta fits -- of a batch of same-shape problems:
// per step one W-phase and one H-phase launch for ALL problems, then one finish launch.  A translation unit of its own (see
// csrc/dnmf_kl.hip).  No workgroup waits for another one; no workspace.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_slab.h"

namespace {

typedef void (*SlabStepW)(SlabArgs, int);
typedef void (*SlabStepH)(SlabArgs, int, int);
typedef void (*SlabFinish)(SlabArgs, int);
struct SlabKernels { SlabStepW w; SlabStepH h; SlabFinish fin; };

// fast_w: the 16-byte loads of the W phase (rows of A, of V, of H);  fast_h: those of the H phase (rows of W);  fast_a: the finish's (A, V)
template <int KT, int MODE, bool WT>
SlabKernels slab_kernels(bool fast_w, bool fast_h, bool fast_a) {
    return SlabKernels{fast_w ? pair_slab_w_kernel<KT, true, MODE, WT> : pair_slab_w_kernel<KT, false, MODE, WT>,
                       fast_h ? pair_slab_h_kernel<KT, true, MODE, WT> : pair_slab_h_kernel<KT, false, MODE, WT>,
                       fast_a ? pair_slab_finish_kernel<KT, true, WT> : pair_slab_finish_kernel<KT, false, WT>};
}
template <int MODE, bool WT>
SlabKernels slab_kernels(int kp, bool fast_w, bool fast_h, bool fast_a) {
    if (kp == 16) return slab_kernels<1, MODE, WT>(fast_w, fast_h, fast_a);
    return kp == 32 ? slab_kernels<2, MODE, WT>(fast_w, fast_h, fast_a) : slab_kernels<4, MODE, WT>(fast_w, fast_h, fast_a);
}
// pair: PAIR_FRO / PAIR_KL (weighted alone), PAIR_IS, PAIR_BETA
SlabKernels slab_kernels(int pair, bool weighted, int kp, bool fast_w, bool fast_h, bool fast_a) {
    if (weighted) {
        if (pair == PAIR_FRO) return slab_kernels<PAIR_FRO, true>(kp, fast_w, fast_h, fast_a);
        if (pair == PAIR_KL) return slab_kernels<PAIR_KL, true>(kp, fast_w, fast_h, fast_a);
        return pair == PAIR_IS ? slab_kernels<PAIR_IS, true>(kp, fast_w, fast_h, fast_a) : slab_kernels<PAIR_BETA, true>(kp, fast_w, fast_h, fast_a);
    }
    return pair == PAIR_IS ? slab_kernels<PAIR_IS, false>(kp, fast_w, fast_h, fast_a) : slab_kernels<PAIR_BETA, false>(kp, fast_w, fast_h, fast_a);
}

inline bool rows16(const float* X, long ld, long stride) { return aligned16(X) && ld % 4 == 0 && stride % 4 == 0; }

// the checks both entry points share (before any HIP call), then the launches: pair_mu_fit's order of operations
int slab_fit(const char* who, int pair, float beta, const float* A, long a_stride, long lda, const float* V, long v_stride, long ldv,
             float* W, long w_stride, long ldw, float* H, long h_stride, long ldh, long m, long n, int k, float eps, int w_update, int itr,
             int batch, double* sq_out, void* stream) {
    const bool weighted = V != nullptr;
    REQUIRE(k >= 1 && k <= SL_MAX_K, "%s: rank k=%d unsupported (1 <= k <= %d for the slab fits)", who, k, SL_MAX_K);
    REQUIRE(A && W && H && sq_out && m >= 1 && n >= 1 && m <= SL_MAX_DIM && n <= SL_MAX_DIM && lda >= n && ldw >= k && ldh >= n &&
                itr >= 0 && batch >= 1 && batch <= 65535 && (!weighted || ldv >= n),
            "%s: null pointer or bad shape (m=%ld n=%ld k=%d itr=%d batch=%d)", who, m, n, k, itr, batch);
    // (v_stride = 0: every problem reads the one V -- a sweep perturbs the data and keeps the weights)
    REQUIRE(batch == 1 || (a_stride >= (m - 1) * lda + n && w_stride >= (m - 1) * ldw + k && h_stride >= (long)(k - 1) * ldh + n &&
                           (!weighted || v_stride == 0 || v_stride >= (m - 1) * ldv + n)),
            "%s: the problems of a batch overlap (strides %ld %ld %ld %ld)", who, a_stride, v_stride, w_stride, h_stride);
    const SlabPlan r = plan_slab(m, n, k);
    hipStream_t st = S(stream);
    SlabArgs a{};
    a.A = A; a.a_stride = batch == 1 ? 0 : a_stride; a.lda = lda;
    a.V = V; a.v_stride = batch == 1 ? 0 : v_stride; a.ldv = ldv;
    a.W = W; a.w_stride = batch == 1 ? 0 : w_stride; a.ldw = ldw;
    a.H = H; a.h_stride = batch == 1 ? 0 : h_stride; a.ldh = ldh;
    a.m = (int)m; a.n = (int)n; a.k = k; a.eps = eps; a.sq = sq_out;
    if (pair == PAIR_BETA) { const PairExp px = beta_exp(beta); a.pexp = px.e; a.gamma = px.gamma; }
    else a.gamma = 1.f;
    // the 16-byte loads: every row of every problem starts on a 16-byte boundary and holds whole vectors.  The choice changes how an
    // operand is fetched, never a sum: both forms give the same bits
    const bool fast_a = n % 4 == 0 && rows16(A, lda, a.a_stride) && (!weighted || rows16(V, ldv, a.v_stride));
    const bool fast_w = fast_a && rows16(H, ldh, a.h_stride);
    const bool fast_h = k % 4 == 0 && rows16(W, ldw, a.w_stride);
    const SlabKernels kn = slab_kernels(pair, weighted, r.kp, fast_w, fast_h, fast_a);
    const dim3 gw((unsigned)r.row_slabs, 1, (unsigned)batch), gh((unsigned)r.col_slabs, 1, (unsigned)batch);
    int pending = 0;                                                           // W = max(W, eps) of a clamp step, not yet in global W
    for (int i = 0; i < itr; ++i) {
        const int clamp = (i % 10 == 0);
        if (w_update) {
            hipLaunchKernelGGL(kn.w, gw, dim3(SL_T), r.lds_w, st, a, pending);
            pending = 0;
        }
        hipLaunchKernelGGL(kn.h, gh, dim3(SL_T), r.lds_h, st, a, clamp, pending);
        if (clamp) pending = 1;
    }
    hipLaunchKernelGGL(kn.fin, dim3((unsigned)batch), dim3(SL_FIN_T), 0, st, a, pending);
    return check_launch(who);
}

}  // namespace

extern "C" {

int dnmf_pair_slab_plan(long m, long n, int k, long out[8]) {
    REQUIRE(out && m >= 1 && n >= 1, "pair_slab_plan: null pointer or bad shape");
    const SlabPlan r = plan_slab(m, n, k);
    out[0] = r.eligible;
    out[1] = (long)std::max(r.lds_w, r.lds_h);      // bytes of dynamic LDS of the larger phase (0: the rank is not served)
    out[2] = r.kp;
    out[3] = SL_NW;
    out[4] = r.row_slabs;                            // workgroups of a W phase per problem
    out[5] = r.col_slabs;                            // workgroups of an H phase per problem
    out[6] = r.w_panels;                             // panels of H each of the former walks
    out[7] = r.h_panels;                             // panels of W each of the latter walks
    return DNMF_OK;
}

int dnmf_pair_slab_fit_batch(int mode, float beta, const float* A, long a_stride, long lda, float* W, long w_stride, long ldw, float* H,
                             long h_stride, long ldh, long m, long n, int k, float eps, int w_update, int itr, int batch, double* sq_out,
                             void* stream) {
    const char* who = "pair_slab_fit_batch";
    REQUIRE(mode == DNMF_SLAB_IS || mode == DNMF_SLAB_BETA, "%s: mode %d (DNMF_SLAB_IS or DNMF_SLAB_BETA)", who, mode);
    if (mode == DNMF_SLAB_BETA) {
        REQUIRE(beta_ok(beta), "%s: beta=%g is outside the accepted range -2 <= beta <= 4", who, (double)beta);
        if (beta == 0.f) mode = DNMF_SLAB_IS;              // beta = 0 IS Itakura-Saito: its kernels, its bits (as PyNMF renames it)
    }
    return slab_fit(who, mode == DNMF_SLAB_IS ? PAIR_IS : PAIR_BETA, beta, A, a_stride, lda, nullptr, 0, 0, W, w_stride, ldw, H, h_stride,
                    ldh, m, n, k, eps, w_update, itr, batch, sq_out, stream);
}

int dnmf_pair_slab_weighted_fit_batch(int norm, float beta, const float* A, long a_stride, long lda, const float* V, long v_stride, long ldv,
                                      float* W, long w_stride, long ldw, float* H, long h_stride, long ldh, long m, long n, int k, float eps,
                                      int w_update, int itr, int batch, double* sq_out, void* stream) {
    const char* who = "pair_slab_weighted_fit_batch";
    REQUIRE(norm >= 0 && norm <= 3, "%s: norm=%d is not known (0 fro, 1 kl, 2 is, 3 beta)", who, norm);
    if (norm == 3) {
        REQUIRE(beta_ok(beta), "%s: beta=%g is outside the accepted range -2 <= beta <= 4", who, (double)beta);
        if (beta == 0.f) norm = 2;                         // beta = 0 IS Itakura-Saito: its kernels, its bits
    }
    REQUIRE(V, "%s: null pointer (the weights)", who);
    static const int pair_of[4] = {PAIR_FRO, PAIR_KL, PAIR_IS, PAIR_BETA};
    return slab_fit(who, pair_of[norm], beta, A, a_stride, lda, V, v_stride, ldv, W, w_stride, ldw, H, h_stride, ldh, m, n, k, eps, w_update,
                    itr, batch, sq_out, stream);
}

}  // extern "C"
