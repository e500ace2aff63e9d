// dnmf_f64_div.hip -- the entry points of the float64 Itakura-Saito and beta-divergence family (include/dnmf_f64_div_api.h):
// dnmf_is_f64_* and dnmf_beta_f64_*, one implementation each side; the kernels and their plans are csrc/dnmf_f64_div.h.
// Plain launch chains on the caller's stream: pair kernel, then the ending; no workgroup waits for another.
#include "dnmf_f64_div.h"

namespace {

// what a norm / beta chooses before anything is launched: the element-wise mode of the pair, the rule's exponent, the objective's form
struct DivMode { int pm; PowArgs pa; int rule; double gamma; int form; double beta, c; };
inline bool beta64_ok(double beta) { return beta >= -2.0 && beta <= 4.0; }      // (the padding argument; a NaN compares false)
inline DivMode div_mode_is() { return DivMode{PM_IS, PowArgs{-2.0, 2, 1, 0}, RULE64_SQRT, 0.5, DIV64_IS, 0.0, 1.0}; }
inline DivMode div_mode_beta(double beta) {
    if (beta == 0.0) return div_mode_is();                               // beta = 0 IS the Itakura-Saito pair, rule and objective
    DivMode d;
    const double e = beta - 2.0, h = 2.0 * e;
    d.pa = PowArgs{e, 0, 0, 0};
    if (h == std::nearbyint(h)) {                                        // 2 (beta - 2) an integer in [-8, 4]: multiplies, rcp, rsq
        const int hi = (int)h, ah = hi < 0 ? -hi : hi;
        d.pm = PM_HALF;
        d.pa.ipow = ah / 2; d.pa.inv = hi < 0; d.pa.odd = ah % 2;
    } else d.pm = PM_GEN;
    d.gamma = beta < 1.0 ? 1.0 / (2.0 - beta) : (beta <= 2.0 ? 1.0 : 1.0 / (beta - 1.0));
    d.rule = d.gamma == 1.0 ? RULE64_QUOT : (d.gamma == 0.5 ? RULE64_SQRT : RULE64_POW);
    d.form = beta == 1.0 ? DIV64_KL : DIV64_GEN;
    d.beta = beta;
    d.c = d.form == DIV64_GEN ? 1.0 / (beta * (beta - 1.0)) : 1.0;
    return d;
}

inline unsigned end_grid(long rows, long cols) { return (unsigned)std::min<long>(cdiv(rows * cols, 256), 8192); }

struct Operands { const double* A; long m, n, lda; const double* W; long ldw; const double* H; long ldh; int k; double eps; };

#define PM_CASE(LAUNCH) do { if (md.pm == PM_IS) LAUNCH(PM_IS); else if (md.pm == PM_HALF) LAUNCH(PM_HALF); else LAUNCH(PM_GEN); } while (0)

// the W side's pair into its slabs of `ws` (ws[split][half][m][kp])
int launch_div_uht(const char* who, const Operands& o, const DivMode& md, const DivUhtPlan& p, double* ws, hipStream_t st) {
    if (!(buf_ok(o.lda, 16 * DIV64_RT) && buf_ok(o.ldw, 16 * DIV64_RT) && buf_ok(o.ldh, o.k)))
        return fail(DNMF_EINVAL, "%s: a row pitch beyond the 2 GiB window of the float64 operand loads", who);
    const dim3 grid(p.gx, (unsigned)p.nsplit);
    const long half = o.m * p.kp;
#define UHT_L(NT_, VEC_, PM_) hipLaunchKernelGGL((f64_div_uht_kernel<NT_, DIV64_RT, VEC_, PM_, div64_uht_d(NT_)>), grid, dim3(256), 0, st, o.A, o.lda, o.m, o.n, o.W, o.ldw, \
                                                 o.H, o.ldh, o.k, o.eps, md.pa, ws, (long)p.kp, 2 * half, half, p.cps)
#define UHT_NT1(PM_) do { if (p.vec) UHT_L(1, true, PM_); else UHT_L(1, false, PM_); } while (0)
#define UHT_NT2(PM_) do { if (p.vec) UHT_L(2, true, PM_); else UHT_L(2, false, PM_); } while (0)
#define UHT_NT4(PM_) do { if (p.vec) UHT_L(4, true, PM_); else UHT_L(4, false, PM_); } while (0)
    if (p.nt == 1) PM_CASE(UHT_NT1); else if (p.nt == 2) PM_CASE(UHT_NT2); else PM_CASE(UHT_NT4);
#undef UHT_NT4
#undef UHT_NT2
#undef UHT_NT1
#undef UHT_L
    return check_launch(who);
}

// the H side's pair into its slabs of `ws` (ws[chunk][half][kp][ldp])
int launch_div_wtu(const char* who, const Operands& o, const DivMode& md, const DivWtuPlan& p, double* ws, hipStream_t st) {
    if (!(buf_ok(o.lda, 16) && buf_ok(o.ldw, 16) && buf_ok(o.ldh, o.k)))
        return fail(DNMF_EINVAL, "%s: a row pitch beyond the 2 GiB window of the float64 operand loads", who);
    const dim3 grid(p.gx);
    const long half = (long)p.kp * p.ldp;
#define WTU_L(NT_, VEC_, PM_) hipLaunchKernelGGL((f64_div_wtu_kernel<NT_, div64_ct(NT_), VEC_, PM_>), grid, dim3(256), 0, st, o.A, o.lda, o.m, o.n, o.W, o.ldw, \
                                                 o.H, o.ldh, o.k, o.eps, md.pa, p.rows_per_chunk, p.ncolblk, p.nwaves, ws, 2 * half, half, p.ldp)
#define WTU_NT1(PM_) do { if (p.vec) WTU_L(1, true, PM_); else WTU_L(1, false, PM_); } while (0)
#define WTU_NT2(PM_) do { if (p.vec) WTU_L(2, true, PM_); else WTU_L(2, false, PM_); } while (0)
#define WTU_NT4(PM_) do { if (p.vec) WTU_L(4, true, PM_); else WTU_L(4, false, PM_); } while (0)
    if (p.nt == 1) PM_CASE(WTU_NT1); else if (p.nt == 2) PM_CASE(WTU_NT2); else PM_CASE(WTU_NT4);
#undef WTU_NT4
#undef WTU_NT2
#undef WTU_NT1
#undef WTU_L
    return check_launch(who);
}

// one side, pair kernel and ending: X != nullptr applies the rule to X (the side's factor, after the pass has read it), otherwise the
// pair is stored to (num, den)
int div64_side(const char* who, bool wside, const Operands& o, const DivMode& md, double* X, long ldx, int clamp, double* num, double* den, long ldo,
               void* ws, size_t ws_bytes, hipStream_t st) {
    double* slab = (double*)ws;
    long rows, cols, ldp, stride, half; int nslab, rc;
    if (wside) {
        const DivUhtPlan p = plan_div_uht(o.m, o.n, o.k);
        rows = o.m; cols = o.k; ldp = p.kp; half = o.m * p.kp; stride = 2 * half; nslab = (int)p.nsplit;
        if (ws_bytes < (size_t)p.nsplit * stride * sizeof(double)) return fail(DNMF_EWS, "%s: workspace too small", who);
        rc = launch_div_uht(who, o, md, p, slab, st);
    } else {
        const DivWtuPlan p = plan_div_wtu(o.m, o.n, o.k);
        rows = o.k; cols = o.n; ldp = p.ldp; half = (long)p.kp * p.ldp; stride = 2 * half; nslab = (int)p.nchunks;
        if (ws_bytes < (size_t)p.nchunks * stride * sizeof(double)) return fail(DNMF_EWS, "%s: workspace too small", who);
        rc = launch_div_wtu(who, o, md, p, slab, st);
    }
    if (rc) return rc;
    const dim3 grid(end_grid(rows, cols));
    if (X) hipLaunchKernelGGL(f64_pair_end_kernel<true>, grid, dim3(256), 0, st, (const double*)slab, (const double*)slab + half, stride, ldp, nslab, rows, cols,
                              X, ldx, (double*)nullptr, (double*)nullptr, 0L, o.eps, md.rule, md.gamma, clamp);
    else hipLaunchKernelGGL(f64_pair_end_kernel<false>, grid, dim3(256), 0, st, (const double*)slab, (const double*)slab + half, stride, ldp, nslab, rows, cols,
                            (double*)nullptr, 0L, num, den, ldo, o.eps, md.rule, md.gamma, 0);
    return check_launch(who);
}

#define DIV_OPERANDS_OK(extra) (A && W && H && ws && m >= 1 && n >= 1 && k >= 1 && k <= DIV64_MAX_K && lda >= n && ldw >= k && ldh >= n && (extra))

int div64_pair(const char* who, bool wside, const DivMode& md, const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh,
               int k, double eps, double* num, double* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQ(DIV_OPERANDS_OK(num && den && ldo >= (wside ? (long)k : n)), "%s: bad arguments (1 <= k <= %d)", who, DIV64_MAX_K);
    return div64_side(who, wside, Operands{A, m, n, lda, W, ldw, H, ldh, k, eps}, md, nullptr, 0, 0, num, den, ldo, ws, ws_bytes, ST(stream));
}
int div64_update(const char* who, bool wside, const DivMode& md, const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh,
                 int k, double eps, int clamp, void* ws, size_t ws_bytes, void* stream) {
    REQ(DIV_OPERANDS_OK(true), "%s: bad arguments (1 <= k <= %d)", who, DIV64_MAX_K);
    return div64_side(who, wside, Operands{A, m, n, lda, W, ldw, H, ldh, k, eps}, md, wside ? (double*)W : (double*)H, wside ? ldw : ldh, clamp, nullptr, nullptr,
                      0, ws, ws_bytes, ST(stream));
}
int div64_ratio(const char* who, const DivMode& md, double* X, long rows, long cols, long ldx, const double* num, const double* den, long ldo, double eps,
                int clamp, void* stream) {
    REQ(X && num && den && rows >= 1 && cols >= 1 && ldx >= cols && ldo >= cols, "%s: bad arguments", who);
    hipLaunchKernelGGL(f64_pair_end_kernel<true>, dim3(end_grid(rows, cols)), dim3(256), 0, ST(stream), num, den, 0L, ldo, 1, rows, cols, X, ldx,
                       (double*)nullptr, (double*)nullptr, 0L, eps, md.rule, md.gamma, clamp);
    return check_launch(who);
}
int div64_objective(const char* who, const DivMode& md, const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k,
                    double eps, double* out, void* ws, size_t ws_bytes, void* stream) {
    REQ(DIV_OPERANDS_OK(out != nullptr), "%s: bad arguments (1 <= k <= %d)", who, DIV64_MAX_K);
    const DivSumPlan p = plan_div_sum(m, n, k);
    const long nparts = (long)p.gx * p.gy;
    if (ws_bytes < (size_t)nparts * sizeof(double)) return fail(DNMF_EWS, "%s: workspace too small", who);
    hipStream_t st = ST(stream);
    const dim3 grid(p.gx, p.gy);
#define SUM_L(KS_, FORM_) hipLaunchKernelGGL((f64_div_sum_kernel<KS_, FORM_>), grid, dim3(256), 0, st, A, lda, m, n, W, ldw, H, ldh, k, eps, md.beta, md.c, p.cpw, (double*)ws)
#define SUM_KS(FORM_) do { if (p.ks == 4) SUM_L(4, FORM_); else if (p.ks == 8) SUM_L(8, FORM_); else SUM_L(16, FORM_); } while (0)
    if (md.form == DIV64_KL) SUM_KS(DIV64_KL); else if (md.form == DIV64_IS) SUM_KS(DIV64_IS); else SUM_KS(DIV64_GEN);
#undef SUM_KS
#undef SUM_L
    hipLaunchKernelGGL(f64_sum_final_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, (int)nparts, out);
    return check_launch(who);
}

#define BETA_OK(who) REQ(beta64_ok(beta), who ": beta = %g is outside -2 <= beta <= 4", beta)

}  // namespace

extern "C" {

size_t dnmf_is_f64_ws_bytes(long m, long n, int k) { return div64_ws_bytes(m, n, k); }
size_t dnmf_beta_f64_ws_bytes(long m, long n, int k) { return div64_ws_bytes(m, n, k); }

// num = (A . R . R) H^T, den = R H^T, R = 1 / (W H + eps)  (the W side of csrc/dnmf_is.h; parallels dist_nmf.py:806, :810)
int dnmf_is_f64_aht_pair(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps, double* num,
                         double* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "is f64 aht_pair");
    return div64_pair("is f64 aht_pair", true, div_mode_is(), A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, ws, ws_bytes, stream);
}
// num = W^T (A . R . R), den = W^T R  (the H side; parallels dist_nmf.py:806, :808)
int dnmf_is_f64_wta_pair(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps, double* num,
                         double* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "is f64 wta_pair");
    return div64_pair("is f64 wta_pair", false, div_mode_is(), A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, ws, ws_bytes, stream);
}
// W <- W . sqrt(num / (den + eps))  (parallels dist_nmf.py:828-830)
int dnmf_is_f64_update_w(const double* A, long m, long n, long lda, double* W, long ldw, const double* H, long ldh, int k, double eps, void* ws,
                         size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "is f64 update_w");
    return div64_update("is f64 update_w", true, div_mode_is(), A, m, n, lda, W, ldw, H, ldh, k, eps, 0, ws, ws_bytes, stream);
}
// H <- H . sqrt(num / (den + eps)), max(., eps) if clamp  (parallels dist_nmf.py:847-849, pyDNMF.py:170-172)
int dnmf_is_f64_update_h(const double* A, long m, long n, long lda, const double* W, long ldw, double* H, long ldh, int k, double eps, int clamp, void* ws,
                         size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "is f64 update_h");
    return div64_update("is f64 update_h", false, div_mode_is(), A, m, n, lda, W, ldw, H, ldh, k, eps, clamp, ws, ws_bytes, stream);
}
// X <- X . sqrt(num / (den + eps)), max(., eps) if clamp: the rule on a stored pair, the function of the endings above
int dnmf_is_f64_ratio_update(double* X, long rows, long cols, long ldx, const double* num, const double* den, long ldo, double eps, int clamp, void* stream) {
    return div64_ratio("is f64 ratio_update", div_mode_is(), X, rows, cols, ldx, num, den, ldo, eps, clamp, stream);
}
// *out = D_IS(A | W H + eps) = sum (q - log q - 1), q = a / (s + eps)  (parallels the residual of pyDNMF.py:205-218)
int dnmf_is_f64_divergence(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps, double* out,
                           void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "is f64 divergence");
    return div64_objective("is f64 divergence", div_mode_is(), A, m, n, lda, W, ldw, H, ldh, k, eps, out, ws, ws_bytes, stream);
}

// num = (A . P) H^T, den = (S' . P) H^T, S' = W H + eps, P = S'^(beta - 2)  (the W side of csrc/dnmf_beta.h)
int dnmf_beta_f64_aht_pair(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps, double beta,
                           double* num, double* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta f64 aht_pair");
    BETA_OK("beta f64 aht_pair");
    return div64_pair("beta f64 aht_pair", true, div_mode_beta(beta), A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, ws, ws_bytes, stream);
}
// num = W^T (A . P), den = W^T (S' . P)  (the H side)
int dnmf_beta_f64_wta_pair(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps, double beta,
                           double* num, double* den, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta f64 wta_pair");
    BETA_OK("beta f64 wta_pair");
    return div64_pair("beta f64 wta_pair", false, div_mode_beta(beta), A, m, n, lda, W, ldw, H, ldh, k, eps, num, den, ldo, ws, ws_bytes, stream);
}
// W <- W . (num / (den + eps))^gamma(beta)  (Fevotte & Idier 2011; gamma as in csrc/dnmf_beta.h)
int dnmf_beta_f64_update_w(const double* A, long m, long n, long lda, double* W, long ldw, const double* H, long ldh, int k, double eps, double beta, void* ws,
                           size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta f64 update_w");
    BETA_OK("beta f64 update_w");
    return div64_update("beta f64 update_w", true, div_mode_beta(beta), A, m, n, lda, W, ldw, H, ldh, k, eps, 0, ws, ws_bytes, stream);
}
// H <- H . (num / (den + eps))^gamma(beta), max(., eps) if clamp  (pyDNMF.py:170-172)
int dnmf_beta_f64_update_h(const double* A, long m, long n, long lda, const double* W, long ldw, double* H, long ldh, int k, double eps, double beta, int clamp,
                           void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta f64 update_h");
    BETA_OK("beta f64 update_h");
    return div64_update("beta f64 update_h", false, div_mode_beta(beta), A, m, n, lda, W, ldw, H, ldh, k, eps, clamp, ws, ws_bytes, stream);
}
// X <- X . (num / (den + eps))^gamma(beta), max(., eps) if clamp: the rule on a stored pair; gamma = 1 is the plain quotient
int dnmf_beta_f64_ratio_update(double* X, long rows, long cols, long ldx, const double* num, const double* den, long ldo, double eps, double beta, int clamp,
                               void* stream) {
    BETA_OK("beta f64 ratio_update");
    return div64_ratio("beta f64 ratio_update", div_mode_beta(beta), X, rows, cols, ldx, num, den, ldo, eps, clamp, stream);
}
// *out = D_beta(A | W H + eps); beta = 1: sum a log(a / s') - a + s' (s' where a = 0); beta = 0: the Itakura-Saito sum; a^beta is 0 at a = 0
int dnmf_beta_f64_divergence(const double* A, long m, long n, long lda, const double* W, long ldw, const double* H, long ldh, int k, double eps, double beta,
                             double* out, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "beta f64 divergence");
    BETA_OK("beta f64 divergence");
    return div64_objective("beta f64 divergence", div_mode_beta(beta), A, m, n, lda, W, ldw, H, ldh, k, eps, out, ws, ws_bytes, stream);
}

}  // extern "C"
