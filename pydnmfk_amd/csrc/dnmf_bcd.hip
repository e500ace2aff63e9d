// dnmf_bcd.hip -- C ABI of the BCD method (csrc/dnmf_bcd.h): the step primitives a host choreography sequences between its grid
// exchanges, and the whole single-rank fit.  A translation unit of its own (see csrc/dnmf_kl.hip).
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_bcd.h"

namespace {

inline unsigned ew_grid(long total) { return (unsigned)std::max<long>(1, std::min<long>(cdiv(total, 256), 256L * 32)); }

// per-problem workspace slice (a batched fit holds `batch` of them, slice z = problem z):
//                    [ step workspace (dnmf_ws_bytes) | W_old | Wm | AHT | AHT kept | H_old | Hm | W^T A | G_h | G_h kept | G_w |
//                      s (KP floats) | column-sum partials | state block | squared norms ]
// m x k buffers have ld = k, k x n buffers ld = n, Gram buffers are KP x KP
struct BcdWs { size_t step, wo, wm, aht, ahtk, ho, hm, wta, gh, ghk, gw, s, part, st, sq, total; };

BcdWs bcd_layout(long m, long n, int k) {
    BcdWs L{};
    const int kp = dnmf_kp(k);
    const size_t mk = align256((size_t)m * k * sizeof(float)), kn = align256((size_t)k * n * sizeof(float));
    const size_t g = align256((size_t)kp * kp * sizeof(float));
    size_t o = align256(dnmf_ws_bytes(m, n, k));
    L.step = o;
    L.wo = o; o += mk;
    L.wm = o; o += mk;
    L.aht = o; o += mk;
    L.ahtk = o; o += mk;
    L.ho = o; o += kn;
    L.hm = o; o += kn;
    L.wta = o; o += kn;
    L.gh = o; o += g;
    L.ghk = o; o += g;
    L.gw = o; o += g;
    L.s = o; o += align256((size_t)kp * sizeof(float));
    L.part = o; o += align256((size_t)cdiv(m, BCD_ROWS) * k * sizeof(float));
    L.st = o; o += align256(BCD_NSLOTS * sizeof(double));
    L.sq = o; o += 256;
    L.total = o;
    return L;
}

int pg_launch(bool hs, const float* Xm, long ldx, const float* P, long ldp, const float* G, long R, int k, const double* st, float* X,
              long ldo, float* part, hipStream_t s) {
    const dim3 grid((unsigned)cdiv(R, BCD_ROWS), (unsigned)cdiv(cdiv(k, BCD_CG), 4));
    const int kp = dnmf_kp(k);
    if (hs) DNMF_LAUNCH(bcd_pg_kernel<true>, grid, dim3(256), 0, s, Xm, ldx, P, ldp, G, kp, R, k, st, (int)BCD_LH, X, ldo, part);
    else DNMF_LAUNCH(bcd_pg_kernel<false>, grid, dim3(256), 0, s, Xm, ldx, P, ldp, G, kp, R, k, st, (int)BCD_LW, X, ldo, part);
    return check_launch(hs ? "bcd_update_h" : "bcd_update_w");
}

}  // namespace

extern "C" {

size_t dnmf_bcd_ws_bytes_w(long m, int k) {
    if (m < 1 || k < 1 || k > DNMF_MAX_K) return 0;
    return (size_t)cdiv(m, BCD_ROWS) * k * sizeof(float);
}

size_t dnmf_bcd_ws_bytes(long m, long n, int k) {
    if (m < 1 || n < 1 || k < 1 || k > DNMF_MAX_K || dnmf_ws_bytes(m, n, k) == 0) return 0;
    return bcd_layout(m, n, k).total;
}

size_t dnmf_bcd_ws_bytes_fit(long m, long n, int k, int batch) {
    if (batch < 1) return 0;
    return (size_t)batch * dnmf_bcd_ws_bytes(m, n, k);
}

int dnmf_bcd_state_init(double* st, const double* sq, void* stream) {
    REQUIRE(st && sq, "bcd_state_init: null pointer");
    DNMF_LAUNCH(bcd_state_init_kernel, dim3(1), dim3(64), 0, S(stream), st, sq);
    return check_launch("bcd_state_init");
}

int dnmf_bcd_init_factor(const float* X0, long rows, long cols, long ld0, float* Xold, long ldo, float* Xm, long ldm, const double* st,
                         int which, void* stream) {
    REQUIRE(X0 && Xold && Xm && st && rows >= 1 && cols >= 1 && ld0 >= cols && ldo >= cols && ldm >= cols && (which == 0 || which == 1),
            "bcd_init_factor: bad arguments");
    DNMF_LAUNCH(bcd_init_factor_kernel, dim3(ew_grid(rows * cols)), dim3(256), 0, S(stream), X0, rows, cols, ld0, Xold, ldo, Xm, ldm,
                       st, which == 0 ? (int)BCD_SW : (int)BCD_SH);
    return check_launch("bcd_init_factor");
}

int dnmf_bcd_lipschitz(const float* G, int k, double* st, int which, void* stream) {
    const int kp = dnmf_kp(k);
    REQUIRE(G && st && kp > 0 && (which == 0 || which == 1), "bcd_lipschitz: bad arguments (k %d)", k);
    DNMF_LAUNCH(bcd_lipschitz_kernel, dim3(1), dim3(256), 0, S(stream), G, kp, k, st, which == 0 ? (int)BCD_LW : (int)BCD_LH);
    return check_launch("bcd_lipschitz");
}

int dnmf_bcd_update_w(const float* Wm, long ldwm, const float* AHT, long ldaht, const float* G, long m, int k, const double* st, float* W,
                      long ldw, float* s, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "bcd_update_w");
    REQUIRE(Wm && AHT && G && st && W && s && ws && m >= 1 && k >= 1 && k <= DNMF_MAX_K && ldwm >= k && ldaht >= k && ldw >= k,
            "bcd_update_w: bad arguments (m %ld, k %d)", m, k);
    REQUIRE(W != Wm, "bcd_update_w: W must not alias Wm (the step reads Wm rows other workgroups write)");
    if (ws_bytes < dnmf_bcd_ws_bytes_w(m, k)) return fail(DNMF_EWS, "bcd_update_w: workspace %zu < %zu", ws_bytes, dnmf_bcd_ws_bytes_w(m, k));
    hipStream_t st_ = S(stream);
    float* part = (float*)ws;
    int rc;
    if ((rc = pg_launch(false, Wm, ldwm, AHT, ldaht, G, m, k, st, W, ldw, part, st_))) return rc;
    DNMF_LAUNCH(bcd_colsum_kernel, dim3((unsigned)k), dim3(256), 0, st_, part, cdiv(m, BCD_ROWS), k, s);
    return check_launch("bcd_colsum");
}

int dnmf_bcd_scale_cols(float* W, long m, int k, long ldw, const float* s, void* stream) {
    REQUIRE(W && s && m >= 1 && k >= 1 && ldw >= k, "bcd_scale_cols: bad arguments");
    DNMF_LAUNCH(bcd_scale_cols_kernel, dim3(ew_grid(m * (long)k)), dim3(256), 0, S(stream), W, m, k, ldw, s);
    return check_launch("bcd_scale_cols");
}

int dnmf_bcd_update_h(const float* Hm, long ldhm, const float* WTA, long ldwta, const float* G, int k, long n, const double* st, float* H,
                      long ldh, void* stream) {
    REQUIRE(Hm && WTA && G && st && H && n >= 1 && k >= 1 && k <= DNMF_MAX_K && ldhm >= n && ldwta >= n && ldh >= n,
            "bcd_update_h: bad arguments (k %d, n %ld)", k, n);
    REQUIRE(H != Hm, "bcd_update_h: H must not alias Hm");
    return pg_launch(true, Hm, ldhm, WTA, ldwta, G, n, k, st, H, ldh, nullptr, S(stream));
}

int dnmf_bcd_decide(double* st, const double* sq, void* stream) {
    REQUIRE(st && sq, "bcd_decide: null pointer");
    DNMF_LAUNCH(bcd_decide_kernel, dim3(1), dim3(64), 0, S(stream), st, sq);
    return check_launch("bcd_decide");
}

int dnmf_bcd_extrapolate(float* W, long ldw, float* Wold, long ldwo, float* Wm, long ldwm, long m, float* H, long ldh, float* Hold,
                         long ldho, float* Hm, long ldhm, long n, int k, float* AHT, long ldaht, float* AHTk, long ldahtk, float* G,
                         float* Gk, const double* st, void* stream) {
    const int kp = dnmf_kp(k);
    REQUIRE(W && Wold && Wm && H && Hold && Hm && AHT && AHTk && G && Gk && st && m >= 1 && n >= 1 && kp > 0 && ldw >= k && ldwo >= k &&
            ldwm >= k && ldh >= n && ldho >= n && ldhm >= n && ldaht >= k && ldahtk >= k, "bcd_extrapolate: bad arguments");
    BcdJobs J{};
    J.j[0] = BcdJob{W, Wold, Wm, m, k, ldw, ldwo, ldwm, 0, (int)BCD_WW};
    J.j[1] = BcdJob{H, Hold, Hm, k, n, ldh, ldho, ldhm, 0, (int)BCD_WH};
    J.j[2] = BcdJob{AHT, AHTk, nullptr, m, k, ldaht, ldahtk, 0, 1, 0};
    J.j[3] = BcdJob{G, Gk, nullptr, kp, kp, kp, kp, 0, 1, 0};
    J.n = 4;
    const long big = std::max(m * (long)k, (long)k * n);
    DNMF_LAUNCH(bcd_extrapolate_kernel, dim3(ew_grid(big), 4), dim3(256), 0, S(stream), J, st);
    return check_launch("bcd_extrapolate");
}

// One rank: `itr` BCD iterations (one update(), dist_nmf.py:967-1047), then the clamp iff (itr - 1) % 10 == 0 (PyNMF.fit runs ONE
// trip with i = itr - 1, pyDNMF.py:151-156), normalize_features (:185-194) and the squared norms of relative_err (:205-218).
// batch > 1: the same launch sequence, laid out for problem 0, with every launch covering all problems (blockIdx.z = problem; csrc/
// dnmf_common.h "batched launches").  Each problem's state block and squared norms sit in its own workspace slice, so the problems
// of one batch accept or restart independently in the same iteration: nothing the host issues depends on a decision.
int dnmf_bcd_fro_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
                     int itr, int batch, long a_stride, long w_stride, long h_stride, double* sq_out, void* ws, size_t ws_bytes,
                     void* stream) {
    (void)w_update;                                                          // (W is always updated: dist_nmf.py:967 ignores W_update)
    REQUIRE_WS16(ws, "bcd_fro_fit");
    REQUIRE(A && W && H && sq_out && ws && m >= 1 && n >= 1 && k >= 1 && k <= DNMF_MAX_K && lda >= n && ldw >= k && ldh >= n && itr >= 1 &&
            batch >= 1, "bcd_fro_fit: bad arguments (m %ld, n %ld, k %d, itr %d, batch %d)", m, n, k, itr, batch);
    const size_t need = dnmf_bcd_ws_bytes(m, n, k);
    REQUIRE(need != 0, "bcd_fro_fit: unsupported shape (m %ld, n %ld, k %d)", m, n, k);
    if (ws_bytes < (size_t)batch * need) return fail(DNMF_EWS, "bcd_fro_fit: workspace %zu < %d x %zu", ws_bytes, batch, need);
    const BcdWs L = bcd_layout(m, n, k);
    BatchCtx* ctx = dnmf_batch_();
    if (ctx->B != 1) return fail(DNMF_EINVAL, "bcd_fro_fit: called inside a batched fit");
    BatchGuard guard(ctx);
    if (int frc = batch_families(ctx, "bcd_fro_fit", batch, A, sizeof(float), m, n, lda, a_stride, W, ldw, w_stride, H, ldh, h_stride, k, ws,
                                 L.total)) return frc;
    char* b = (char*)ws;
    const int kp = dnmf_kp(k);
    float *Wo = (float*)(b + L.wo), *Wm = (float*)(b + L.wm), *AHT = (float*)(b + L.aht), *AHTk = (float*)(b + L.ahtk);
    float *Ho = (float*)(b + L.ho), *Hm = (float*)(b + L.hm), *WTA = (float*)(b + L.wta);
    float *Gh = (float*)(b + L.gh), *Ghk = (float*)(b + L.ghk), *Gw = (float*)(b + L.gw), *s = (float*)(b + L.s);
    double *st = (double*)(b + L.st), *sq = (double*)(b + L.sq);
    void* part = b + L.part;
    const size_t part_bytes = L.st - L.part;
    const size_t step = L.step;
    hipStream_t hs = S(stream);
    int rc;
    // initWandH (dist_nmf.py:947-965)
    if ((rc = dnmf_sqnorm(A, m, n, lda, sq, stream))) return rc;
    if ((rc = dnmf_sqnorm(W, m, k, ldw, sq + 1, stream))) return rc;
    if ((rc = dnmf_sqnorm(H, k, n, ldh, sq + 2, stream))) return rc;
    if ((rc = dnmf_bcd_state_init(st, sq, stream))) return rc;
    if ((rc = dnmf_bcd_init_factor(W, m, k, ldw, Wo, k, Wm, k, st, 0, stream))) return rc;
    if ((rc = dnmf_bcd_init_factor(H, k, n, ldh, Ho, n, Hm, n, st, 1, stream))) return rc;
    if ((rc = dnmf_gram_hht(Ho, k, n, n, Gh, ws, step, stream))) return rc;
    if ((rc = dnmf_aht(A, m, n, lda, Ho, k, n, AHT, k, stream))) return rc;
    // the kept products of every problem: one copy each, the slices `L.total` apart as the rows of a two-dimensional copy
    const size_t gbytes = (size_t)kp * kp * sizeof(float), ahtbytes = (size_t)m * k * sizeof(float);
    if (batch == 1 ? (hipMemcpyAsync(Ghk, Gh, gbytes, hipMemcpyDeviceToDevice, hs) != hipSuccess ||
                      hipMemcpyAsync(AHTk, AHT, ahtbytes, hipMemcpyDeviceToDevice, hs) != hipSuccess)
                   : (hipMemcpy2DAsync(Ghk, L.total, Gh, L.total, gbytes, (size_t)batch, hipMemcpyDeviceToDevice, hs) != hipSuccess ||
                      hipMemcpy2DAsync(AHTk, L.total, AHT, L.total, ahtbytes, (size_t)batch, hipMemcpyDeviceToDevice, hs) != hipSuccess))
        return fail(DNMF_EHIP, "bcd_fro_fit: copy of the kept products failed");
    for (int i = 0; i < itr; ++i) {                                                              // :977-1047
        if ((rc = dnmf_bcd_lipschitz(Gh, k, st, 0, stream))) return rc;
        if ((rc = dnmf_bcd_update_w(Wm, k, AHT, k, Gh, m, k, st, W, ldw, s, part, part_bytes, stream))) return rc;
        if ((rc = dnmf_bcd_scale_cols(W, m, k, ldw, s, stream))) return rc;
        if ((rc = dnmf_wta_gram(A, m, n, lda, W, k, ldw, WTA, n, Gw, ws, step, stream))) return rc;
        if ((rc = dnmf_bcd_lipschitz(Gw, k, st, 1, stream))) return rc;
        if ((rc = dnmf_bcd_update_h(Hm, n, WTA, n, Gw, k, n, st, H, ldh, stream))) return rc;
        if ((rc = dnmf_gram_hht(H, k, n, ldh, Gh, ws, step, stream))) return rc;
        if ((rc = dnmf_aht(A, m, n, lda, H, k, ldh, AHT, k, stream))) return rc;
        if ((rc = dnmf_resid_sqnorm_ws(A, m, n, lda, W, ldw, H, ldh, k, sq + 3, ws, step, stream))) return rc;
        if ((rc = dnmf_bcd_decide(st, sq + 3, stream))) return rc;
        if ((rc = dnmf_bcd_extrapolate(W, ldw, Wo, k, Wm, k, m, H, ldh, Ho, n, Hm, n, n, k, AHT, k, AHTk, k, Gh, Ghk, st, stream))) return rc;
    }
    if ((itr - 1) % 10 == 0) {                                                                   // pyDNMF.py:155-157
        if ((rc = dnmf_clamp_min(H, k, n, ldh, eps, stream))) return rc;
        if ((rc = dnmf_clamp_min(W, m, k, ldw, eps, stream))) return rc;
    }
    // normalize_features (pyDNMF.py:185-194) and relative_err (:205-218), as the other whole fits
    if ((rc = dnmf_colsum(W, m, k, ldw, s, ws, step, stream))) return rc;
    if ((rc = dnmf_scale_cols_div(W, m, k, ldw, s, eps, stream))) return rc;
    if ((rc = dnmf_scale_rows_mul(H, k, n, ldh, s, stream))) return rc;
    // a single fit writes its pair where the caller wants it; the problems of a batch write theirs in their slices (sq[4], sq[5]), gathered
    // into sq_out[z][2] by one copy
    double* fin = batch == 1 ? sq_out : sq + 4;
    if ((rc = dnmf_resid_sqnorm_ws(A, m, n, lda, W, ldw, H, ldh, k, fin, ws, step, stream))) return rc;
    if ((rc = dnmf_sqnorm(A, m, n, lda, fin + 1, stream))) return rc;
    if (batch > 1 && hipMemcpy2DAsync(sq_out, 2 * sizeof(double), fin, L.total, 2 * sizeof(double), (size_t)batch, hipMemcpyDeviceToDevice,
                                      hs) != hipSuccess)
        return fail(DNMF_EHIP, "bcd_fro_fit: copy of the squared norms failed");
    return DNMF_OK;
}

}  // extern "C"
