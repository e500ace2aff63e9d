// dnmf_csr.hip -- C ABI of the sparse (CSR) data block: packed factor images, the gather products, the KL products with the
// quotient fused, the residual's closed form, the passes of a block whose unstored entries are missing, and NMFk's perturbed copy and
// per-column error (csrc/dnmf_csr.h).  A translation unit of its own (see csrc/dnmf_kl.hip).
// Plain launch chains: no workgroup waits for another one.
#include <cmath>
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_csr.h"

namespace {

inline int csr_kpad_of(int k) {
    if (k < 1 || k > DNMF_MAX_K) return -1;
    return k <= 16 ? 16 : (k <= 32 ? 32 : (k <= 64 ? 64 : (k <= 128 ? 128 : 256)));
}

inline int gram_chunks(long rows, int k) {
    const long nt = cdiv(k, 16) * cdiv(k, 16);
    return (int)std::max<long>(1, std::min<long>(cdiv(rows, 512), std::max<long>(8, 256 / nt)));
}

inline long resid_waves(long rows) { return std::min<long>(round_up(std::max<long>(rows, 1), 4), CSR_RESID_WAVES); }

struct ResidWs { size_t gw, gh, dpart, total; int ncw, nch; long nw; };

ResidWs resid_layout(long rows, long cols, int k, long nseg) {
    ResidWs L{};
    L.ncw = gram_chunks(rows, k);
    L.nch = gram_chunks(cols, k);
    L.nw = resid_waves(rows);
    size_t o = 0;
    L.gw = o; o += align256((size_t)L.ncw * k * k * sizeof(double));
    L.gh = o; o += align256((size_t)L.nch * k * k * sizeof(double));
    L.dpart = o; o += align256((size_t)(L.nw + nseg) * sizeof(double));
    L.total = o;
    return L;
}

struct CsrArgs {
    const int* rowptr; const int* col; const float* val; long rows;
    const float* L; const float* F; int k; float eps; float* out; long ldo; int out_trans;
    const int* long_rows; const int* long_segptr; int n_long; int nseg; float* part;
    float* out2 = nullptr; int clamp = 0;              // masked passes: the denominator's half of the pair / the clamp of the fused ending
};

template <int G, int MODE>
int csr_launch(const CsrArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((csr_rows_kernel<G, MODE>), dim3((unsigned)cdiv(a.rows, 4)), dim3(256), 0, st, a.rowptr, a.col, a.val, a.rows, a.L,
                       a.F, a.k, a.eps, a.out, a.ldo, a.out_trans, (float*)nullptr, 0);
    if (a.n_long > 0) {
        hipLaunchKernelGGL((csr_long_kernel<G, MODE>), dim3((unsigned)cdiv(a.nseg, 4)), dim3(256), 0, st, a.rowptr, a.col, a.val, a.L, a.F,
                           a.eps, a.long_rows, a.long_segptr, a.n_long, a.part, (double*)nullptr);
        hipLaunchKernelGGL(csr_long_reduce_kernel, dim3((unsigned)a.n_long), dim3(4 * G), 0, st, (const float*)a.part, 4 * G, a.long_rows,
                           a.long_segptr, a.k, a.out, a.ldo, a.out_trans);
    }
    return check_launch(MODE ? "csr_kl_mm" : "csr_mm");
}

// masked passes (MODE 3: Frobenius, 4: KL): the pair [num | den] is stored (END = CSR_END_STORE) or applied to the factor `out`
template <int G, int MODE, int END>
int csr_masked_launch(const CsrArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((csr_rows_kernel<G, MODE, END>), dim3((unsigned)cdiv(a.rows, 4)), dim3(256), 0, st, a.rowptr, a.col, a.val, a.rows, a.L,
                       a.F, a.k, a.eps, a.out, a.ldo, a.out_trans, a.out2, a.clamp);
    if (a.n_long > 0) {
        hipLaunchKernelGGL((csr_long_kernel<G, MODE>), dim3((unsigned)cdiv(a.nseg, 4)), dim3(256), 0, st, a.rowptr, a.col, a.val, a.L, a.F,
                           a.eps, a.long_rows, a.long_segptr, a.n_long, a.part, (double*)nullptr);
        hipLaunchKernelGGL((csr_long_reduce_pair_kernel<END>), dim3((unsigned)a.n_long), dim3(4 * G), 0, st, (const float*)a.part, 4 * G,
                           a.long_rows, a.long_segptr, a.L, a.k, a.eps, a.clamp, a.out, a.out2, a.ldo, a.out_trans);
    }
    return check_launch(END == CSR_END_STORE ? "csr_masked_mm" : "csr_masked_update");
}

template <int MODE, int END>
int csr_masked_dispatch(const CsrArgs& a, hipStream_t st) {
    switch (csr_kpad_of(a.k)) {
        case 16: return csr_masked_launch<4, MODE, END>(a, st);
        case 32: return csr_masked_launch<8, MODE, END>(a, st);
        case 64: return csr_masked_launch<16, MODE, END>(a, st);
        case 128: return csr_masked_launch<32, MODE, END>(a, st);
        default: return csr_masked_launch<64, MODE, END>(a, st);
    }
}

template <int G>
int masked_resid_launch(const int* rowptr, const int* col, const float* val, long rows, const float* Wp, const float* HTp, const int* long_rows,
                        const int* long_segptr, int n_long, int nseg, double* dpart, long nw, hipStream_t st) {
    hipLaunchKernelGGL((csr_resid_rows_kernel<G, CSR_M_RESID>), dim3((unsigned)(nw / 4)), dim3(256), 0, st, rowptr, col, val, rows, Wp, HTp, dpart);
    if (n_long > 0)
        hipLaunchKernelGGL((csr_long_kernel<G, CSR_M_RESID>), dim3((unsigned)cdiv(nseg, 4)), dim3(256), 0, st, rowptr, col, val, Wp, HTp, 0.f,
                           long_rows, long_segptr, n_long, (float*)nullptr, dpart + nw);
    return check_launch("csr_masked_resid_sqnorm");
}

// workspace of the masked passes: the partial PAIRS of the long rows, or the residual's float64 partials
inline size_t masked_ws_need(long rows, int k, long nseg) {
    const size_t pairs = align256((size_t)nseg * 2 * csr_kpad_of(k) * sizeof(float));
    const size_t dparts = align256((size_t)(resid_waves(rows) + nseg) * sizeof(double));
    return std::max<size_t>(256, std::max(pairs, dparts));
}

template <int MODE>
int csr_dispatch(const CsrArgs& a, hipStream_t st) {
    switch (csr_kpad_of(a.k)) {
        case 16: return csr_launch<4, MODE>(a, st);
        case 32: return csr_launch<8, MODE>(a, st);
        case 64: return csr_launch<16, MODE>(a, st);
        case 128: return csr_launch<32, MODE>(a, st);
        default: return csr_launch<64, MODE>(a, st);
    }
}

template <int G>
int resid_launch(const int* rowptr, const int* col, const float* val, long rows, const float* Wp, const float* HTp, const int* long_rows,
                 const int* long_segptr, int n_long, int nseg, double* dpart, long nw, hipStream_t st) {
    hipLaunchKernelGGL((csr_resid_rows_kernel<G>), dim3((unsigned)(nw / 4)), dim3(256), 0, st, rowptr, col, val, rows, Wp, HTp, dpart);
    if (n_long > 0)
        hipLaunchKernelGGL((csr_long_kernel<G, 2>), dim3((unsigned)cdiv(nseg, 4)), dim3(256), 0, st, rowptr, col, val, Wp, HTp, 0.f, long_rows,
                           long_segptr, n_long, (float*)nullptr, dpart + nw);
    return check_launch("csr_resid_sqnorm");
}

// workspace of dnmf_csr_column_err: the Gram partials of W and their sum (zero meaning only), then one float64 PAIR per segment
struct ColerrWs { size_t gpart, gram, dpart, total; int nc; };

ColerrWs colerr_layout(long frows, int k, long nseg, bool masked) {
    ColerrWs L{};
    L.nc = masked ? 0 : gram_chunks(frows, k);
    size_t o = 0;
    L.gpart = o; o += align256((size_t)L.nc * k * k * sizeof(double));
    L.gram = o; o += masked ? 0 : align256((size_t)k * k * sizeof(double));
    L.dpart = o; o += align256((size_t)nseg * 2 * sizeof(double));
    L.total = std::max<size_t>(256, o);
    return L;
}

template <int G, bool MASKED>
int colerr_launch(const int* rowptr, const int* col, const float* val, long rows, const float* Lp, const float* Fp, int k, const double* Gm,
                  const int* long_rows, const int* long_segptr, int n_long, int nseg, double* dpart, double* num, double* den, hipStream_t st) {
    hipLaunchKernelGGL((csr_colerr_rows_kernel<G, MASKED>), dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, st, rowptr, col, val, rows, Lp, Fp, k,
                       Gm, num, den);
    if (n_long > 0) {
        hipLaunchKernelGGL((csr_colerr_long_kernel<G, MASKED>), dim3((unsigned)cdiv(nseg, 4)), dim3(256), 0, st, rowptr, col, val, Lp, Fp,
                           long_rows, long_segptr, n_long, dpart);
        hipLaunchKernelGGL(csr_colerr_long_reduce_kernel, dim3((unsigned)n_long), dim3(64), 0, st, (const double*)dpart, long_rows,
                           long_segptr, Lp, 4 * G, k, Gm, num, den);
    }
    return check_launch("csr_column_err");
}

template <bool MASKED, typename... Args>
int colerr_dispatch(int kpad, Args... a) {
    switch (kpad) {
        case 16: return colerr_launch<4, MASKED>(a...);
        case 32: return colerr_launch<8, MASKED>(a...);
        case 64: return colerr_launch<16, MASKED>(a...);
        case 128: return colerr_launch<32, MASKED>(a...);
        default: return colerr_launch<64, MASKED>(a...);
    }
}

int check_common(const char* who, const int* rowptr, const int* col, const float* val, long rows, int k, const int* long_rows,
                 const int* long_segptr, int n_long, int nseg) {
    if (!rowptr || rows < 1 || rows >= (1L << 31)) return fail(DNMF_EINVAL, "%s: null row pointers or bad row count %ld (1 <= rows < 2^31)", who, rows);
    if (csr_kpad_of(k) < 0) return fail(DNMF_EINVAL, "%s: rank k=%d unsupported (1 <= k <= %d)", who, k, DNMF_MAX_K);
    if (n_long < 0 || nseg < 0 || (n_long > 0 && (!long_rows || !long_segptr || nseg < n_long)))
        return fail(DNMF_EINVAL, "%s: bad long-row lists (n_long=%d, segments=%d)", who, n_long, nseg);
    (void)col; (void)val;        // (null for a block without stored entries: never dereferenced then)
    return DNMF_OK;
}

}  // namespace

extern "C" {

int dnmf_csr_kpad(int k) { return csr_kpad_of(k); }

int dnmf_csr_seg(void) { return CSR_SEG; }

size_t dnmf_csr_ws_bytes(long rows, long cols, int k, int nseg) {
    if (rows < 1 || cols < 1 || nseg < 0 || csr_kpad_of(k) < 0) return 0;
    const size_t part = align256((size_t)nseg * csr_kpad_of(k) * sizeof(float));
    return std::max<size_t>(256, std::max(part, resid_layout(rows, cols, k, nseg).total));
}

int dnmf_csr_pack(const float* X, long rows, long cols, long ldx, int transpose, float* P, void* stream) {
    REQUIRE(X && P && rows >= 1 && cols >= 1 && ldx >= cols && aligned16(P), "csr_pack: null / misaligned pointer or bad shape");
    const int k = (int)(transpose ? rows : cols);
    REQUIRE((transpose ? rows : cols) <= DNMF_MAX_K, "csr_pack: rank %ld unsupported (1 <= k <= %d)", transpose ? rows : cols, DNMF_MAX_K);
    const int kpad = csr_kpad_of(k);
    if (transpose) {
        REQUIRE(cols < (1L << 31), "csr_pack: %ld columns (must be < 2^31)", cols);
        hipLaunchKernelGGL(csr_pack_t_kernel, dim3((unsigned)cdiv(cols, 32), (unsigned)cdiv(kpad, 32)), dim3(256), 0, S(stream), X, k, cols,
                           ldx, P, kpad);
    } else {
        const long quads = rows * (kpad / 4);
        hipLaunchKernelGGL(csr_pack_kernel, dim3((unsigned)std::min<long>(cdiv(quads, 256), 8192)), dim3(256), 0, S(stream), X, rows, k, ldx,
                           P, kpad);
    }
    return check_launch("csr_pack");
}

int dnmf_csr_mm(const int* rowptr, const int* col, const float* val, long rows, const float* Fp, int k, float* out, long ldo, int out_trans,
                const int* long_rows, const int* long_segptr, int n_long, int nseg, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_common("csr_mm", rowptr, col, val, rows, k, long_rows, long_segptr, n_long, nseg)) return rc;
    REQUIRE(Fp && out && aligned16(Fp) && ldo >= (out_trans ? rows : (long)k), "csr_mm: null / misaligned operand or ld too small");
    const size_t need = (size_t)nseg * csr_kpad_of(k) * sizeof(float);
    if (n_long > 0 && (!ws || ws_bytes < need || !aligned16(ws))) return fail(DNMF_EWS, "csr_mm: workspace %zu < %zu bytes", ws_bytes, need);
    const CsrArgs a{rowptr, col, val, rows, nullptr, Fp, k, 0.f, out, ldo, out_trans, long_rows, long_segptr, n_long, nseg, (float*)ws};
    return csr_dispatch<0>(a, S(stream));
}

int dnmf_csr_kl_mm(const int* rowptr, const int* col, const float* val, long rows, const float* Lp, const float* Fp, int k, float eps,
                   float* out, long ldo, int out_trans, const int* long_rows, const int* long_segptr, int n_long, int nseg, void* ws,
                   size_t ws_bytes, void* stream) {
    if (int rc = check_common("csr_kl_mm", rowptr, col, val, rows, k, long_rows, long_segptr, n_long, nseg)) return rc;
    REQUIRE(Lp && Fp && out && aligned16(Lp) && aligned16(Fp) && ldo >= (out_trans ? rows : (long)k),
            "csr_kl_mm: null / misaligned operand or ld too small");
    const size_t need = (size_t)nseg * csr_kpad_of(k) * sizeof(float);
    if (n_long > 0 && (!ws || ws_bytes < need || !aligned16(ws))) return fail(DNMF_EWS, "csr_kl_mm: workspace %zu < %zu bytes", ws_bytes, need);
    const CsrArgs a{rowptr, col, val, rows, Lp, Fp, k, eps, out, ldo, out_trans, long_rows, long_segptr, n_long, nseg, (float*)ws};
    return csr_dispatch<1>(a, S(stream));
}

int dnmf_csr_resid_sqnorm(const int* rowptr, const int* col, const float* val, long rows, long cols, const float* Wp, const float* HTp,
                          int k, const int* long_rows, const int* long_segptr, int n_long, int nseg, double* sq, void* ws, size_t ws_bytes,
                          void* stream) {
    if (int rc = check_common("csr_resid_sqnorm", rowptr, col, val, rows, k, long_rows, long_segptr, n_long, nseg)) return rc;
    REQUIRE(Wp && HTp && sq && cols >= 1 && cols < (1L << 31) && aligned16(Wp) && aligned16(HTp), "csr_resid_sqnorm: null / misaligned operand or bad shape");
    const ResidWs L = resid_layout(rows, cols, k, nseg);
    if (!ws || ws_bytes < L.total || !aligned16(ws)) return fail(DNMF_EWS, "csr_resid_sqnorm: workspace %zu < %zu bytes", ws_bytes, L.total);
    hipStream_t st = S(stream);
    const int kpad = csr_kpad_of(k);
    double* gw = (double*)((char*)ws + L.gw);
    double* gh = (double*)((char*)ws + L.gh);
    double* dpart = (double*)((char*)ws + L.dpart);
    const unsigned tiles = (unsigned)(cdiv(k, 16) * cdiv(k, 16));
    hipLaunchKernelGGL(csr_gram_f64_kernel, dim3((unsigned)L.ncw, tiles), dim3(256), 0, st, Wp, rows, kpad, k, cdiv(rows, L.ncw), gw);
    hipLaunchKernelGGL(csr_gram_f64_kernel, dim3((unsigned)L.nch, tiles), dim3(256), 0, st, HTp, cols, kpad, k, cdiv(cols, L.nch), gh);
    int rc;
    switch (kpad) {
        case 16: rc = resid_launch<4>(rowptr, col, val, rows, Wp, HTp, long_rows, long_segptr, n_long, nseg, dpart, L.nw, st); break;
        case 32: rc = resid_launch<8>(rowptr, col, val, rows, Wp, HTp, long_rows, long_segptr, n_long, nseg, dpart, L.nw, st); break;
        case 64: rc = resid_launch<16>(rowptr, col, val, rows, Wp, HTp, long_rows, long_segptr, n_long, nseg, dpart, L.nw, st); break;
        case 128: rc = resid_launch<32>(rowptr, col, val, rows, Wp, HTp, long_rows, long_segptr, n_long, nseg, dpart, L.nw, st); break;
        default: rc = resid_launch<64>(rowptr, col, val, rows, Wp, HTp, long_rows, long_segptr, n_long, nseg, dpart, L.nw, st); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(csr_resid_final_kernel, dim3(1), dim3(256), 0, st, (const double*)gw, L.ncw, (const double*)gh, L.nch, k,
                       (const double*)dpart, L.nw + (n_long > 0 ? nseg : 0), sq);
    return check_launch("csr_resid_sqnorm");
}

size_t dnmf_csr_masked_ws_bytes(long rows, long cols, int k, int nseg) {
    if (rows < 1 || cols < 1 || nseg < 0 || csr_kpad_of(k) < 0) return 0;
    return masked_ws_need(std::max(rows, cols), k, nseg);
}

// The Frobenius rule W <- W * (A H^T) / (W H H^T + eps) (dist_nmf.py:729-732; H: :748-751) and the KL rule W <- W * (U H^T) / (rowsum(H) + eps)
// with U = A / (W H + eps) (dist_nmf.py:806-810, :827-830; H: :846-849), both sums of the numerator AND of the denominator restricted to
// the stored positions: num and den of a row, stored as a pair
int dnmf_csr_masked_mm(const int* rowptr, const int* col, const float* val, long rows, const float* Lp, const float* Fp, int k, float eps,
                       int kl, float* num, float* den, long ldo, int out_trans, const int* long_rows, const int* long_segptr, int n_long,
                       int nseg, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_common("csr_masked_mm", rowptr, col, val, rows, k, long_rows, long_segptr, n_long, nseg)) return rc;
    REQUIRE(Lp && Fp && num && den && aligned16(Lp) && aligned16(Fp) && ldo >= (out_trans ? rows : (long)k),
            "csr_masked_mm: null / misaligned operand or ld too small");
    const size_t need = (size_t)nseg * 2 * csr_kpad_of(k) * sizeof(float);
    if (n_long > 0 && (!ws || ws_bytes < need || !aligned16(ws))) return fail(DNMF_EWS, "csr_masked_mm: workspace %zu < %zu bytes", ws_bytes, need);
    CsrArgs a{rowptr, col, val, rows, Lp, Fp, k, eps, num, ldo, out_trans, long_rows, long_segptr, n_long, nseg, (float*)ws};
    a.out2 = den;
    return kl ? csr_masked_dispatch<CSR_M_KL, CSR_END_STORE>(a, S(stream)) : csr_masked_dispatch<CSR_M_FRO, CSR_END_STORE>(a, S(stream));
}

// The same two rules (dist_nmf.py:729-732 / :748-751; :827-830 / :846-849) applied where nothing crosses ranks: the wave that owns row r
// holds Lp[r] (the packed copy of the factor's row) and writes X[r] = Lp[r] * num / (den + eps), max(., eps) with `clamp` (pyDNMF.py:170-172)
int dnmf_csr_masked_update(const int* rowptr, const int* col, const float* val, long rows, const float* Lp, const float* Fp, int k, float eps,
                           int kl, int clamp, float* X, long ldx, int out_trans, const int* long_rows, const int* long_segptr, int n_long,
                           int nseg, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_common("csr_masked_update", rowptr, col, val, rows, k, long_rows, long_segptr, n_long, nseg)) return rc;
    REQUIRE(Lp && Fp && X && aligned16(Lp) && aligned16(Fp) && ldx >= (out_trans ? rows : (long)k),
            "csr_masked_update: null / misaligned operand or ld too small");
    const size_t need = (size_t)nseg * 2 * csr_kpad_of(k) * sizeof(float);
    if (n_long > 0 && (!ws || ws_bytes < need || !aligned16(ws))) return fail(DNMF_EWS, "csr_masked_update: workspace %zu < %zu bytes", ws_bytes, need);
    CsrArgs a{rowptr, col, val, rows, Lp, Fp, k, eps, X, ldx, out_trans, long_rows, long_segptr, n_long, nseg, (float*)ws};
    a.clamp = clamp != 0;
    return kl ? csr_masked_dispatch<CSR_M_KL, CSR_END_UPDATE>(a, S(stream)) : csr_masked_dispatch<CSR_M_FRO, CSR_END_UPDATE>(a, S(stream));
}

// X <- X * num / (den + eps) (the multiply-divide of dist_nmf.py:731-732, :750-751, :828-830, :847-849) after the pair was summed over ranks
int dnmf_csr_ratio_update(float* X, long rows, long cols, long ldx, const float* num, const float* den, long ldp, float eps, int clamp,
                          void* stream) {
    REQUIRE(X && num && den && rows >= 1 && cols >= 1 && ldx >= cols && ldp >= cols, "csr_ratio_update: null pointer or bad shape");
    const bool vec = aligned16(X) && aligned16(num) && aligned16(den) && cols % 4 == 0 && ldx % 4 == 0 && ldp % 4 == 0;
    const long total = rows * (vec ? cols / 4 : cols);
    const unsigned grid = (unsigned)std::min<long>(cdiv(total, 256), 8192);
    if (vec) hipLaunchKernelGGL((csr_ratio_kernel<4>), dim3(grid), dim3(256), 0, S(stream), X, rows, cols, ldx, num, den, ldp, eps, clamp != 0);
    else hipLaunchKernelGGL((csr_ratio_kernel<1>), dim3(grid), dim3(256), 0, S(stream), X, rows, cols, ldx, num, den, ldp, eps, clamp != 0);
    return check_launch("csr_ratio_update");
}

// sq[0] = ||P_Omega(A - W H)||_F^2 (pyDNMF.py:205-218 with the sum restricted to the stored positions): sum of (a - d)^2 in float64
int dnmf_csr_masked_resid_sqnorm(const int* rowptr, const int* col, const float* val, long rows, long cols, const float* Wp, const float* HTp,
                                 int k, const int* long_rows, const int* long_segptr, int n_long, int nseg, double* sq, void* ws,
                                 size_t ws_bytes, void* stream) {
    if (int rc = check_common("csr_masked_resid_sqnorm", rowptr, col, val, rows, k, long_rows, long_segptr, n_long, nseg)) return rc;
    REQUIRE(Wp && HTp && sq && cols >= 1 && cols < (1L << 31) && aligned16(Wp) && aligned16(HTp),
            "csr_masked_resid_sqnorm: null / misaligned operand or bad shape");
    const long nw = resid_waves(rows);
    const size_t need = (size_t)(nw + nseg) * sizeof(double);
    if (!ws || ws_bytes < need || !aligned16(ws)) return fail(DNMF_EWS, "csr_masked_resid_sqnorm: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = S(stream);
    double* dpart = (double*)ws;
    int rc;
    switch (csr_kpad_of(k)) {
        case 16: rc = masked_resid_launch<4>(rowptr, col, val, rows, Wp, HTp, long_rows, long_segptr, n_long, nseg, dpart, nw, st); break;
        case 32: rc = masked_resid_launch<8>(rowptr, col, val, rows, Wp, HTp, long_rows, long_segptr, n_long, nseg, dpart, nw, st); break;
        case 64: rc = masked_resid_launch<16>(rowptr, col, val, rows, Wp, HTp, long_rows, long_segptr, n_long, nseg, dpart, nw, st); break;
        case 128: rc = masked_resid_launch<32>(rowptr, col, val, rows, Wp, HTp, long_rows, long_segptr, n_long, nseg, dpart, nw, st); break;
        default: rc = masked_resid_launch<64>(rowptr, col, val, rows, Wp, HTp, long_rows, long_segptr, n_long, nseg, dpart, nw, st); break;
    }
    if (rc) return rc;
    // (no Gram term: zero chunks of both Gram matrices, k = 0)
    hipLaunchKernelGGL(csr_resid_final_kernel, dim3(1), dim3(256), 0, st, (const double*)nullptr, 0, (const double*)nullptr, 0, 0,
                       (const double*)dpart, nw + (n_long > 0 ? nseg : 0), sq);
    return check_launch("csr_masked_resid_sqnorm");
}

// ---- NMFk on a sparse block
// The perturbed copy of pyDNMFk.py:42-44 (`sample.randM`: X * (1 + nv + 2 nv U)) on ONE CSR image: val_out[p] = val[p] * factor of the
// entry's position in the dense block, the factor of dnmf_perturb_uniform (csrc/dnmf_stream.h).  `transposed`: the image is the
// transpose's (its row index is the block's column); `ncols`: the dense block's column count.
int dnmf_csr_perturb_uniform(const int* rowptr, const int* col, const float* val, long rows, long ncols, int transposed, float noise_var,
                             unsigned long long seed, float* val_out, void* stream) {
    REQUIRE(rowptr && rows >= 1 && rows < (1L << 31), "csr_perturb_uniform: null row pointers or bad row count %ld (1 <= rows < 2^31)", rows);
    REQUIRE(ncols >= 1 && ncols < (1L << 31), "csr_perturb_uniform: %ld columns of the dense block (1 <= ncols < 2^31)", ncols);
    REQUIRE(!transposed || rows == ncols, "csr_perturb_uniform: the transpose's image has %ld rows, the dense block %ld columns", rows, ncols);
    REQUIRE(val_out, "csr_perturb_uniform: null destination");
    REQUIRE(std::isfinite(noise_var) && noise_var >= 0.f, "csr_perturb_uniform: noise_var %g (finite, >= 0)", (double)noise_var);
    (void)col; (void)val;        // (null for a block without stored entries: never dereferenced then)
    hipLaunchKernelGGL(csr_perturb_uniform_kernel, dim3((unsigned)std::min<long>(cdiv(rows, 4), 1L << 16)), dim3(256), 0, S(stream), rowptr,
                       col, val, rows, ncols, transposed != 0, noise_var, seed, val_out);
    return check_launch("csr_perturb_uniform");
}

size_t dnmf_csr_column_err_ws_bytes(long rows, long cols, int k, int masked, int nseg) {
    if (rows < 1 || cols < 1 || nseg < 0 || csr_kpad_of(k) < 0) return 0;
    return colerr_layout(cols, k, nseg, masked != 0).total;
}

// The per-column sums of pyDNMF.py:221-239 (`column_err`) over this rank's rows, on the TRANSPOSE's image (rows = the block's
// columns, cols = the block's rows): Lp = packed H^T [rows x KPAD], Fp = packed W [cols x KPAD].
int dnmf_csr_column_err(const int* rowptr, const int* col, const float* val, long rows, long cols, const float* Lp, const float* Fp, int k,
                        int masked, const int* long_rows, const int* long_segptr, int n_long, int nseg, double* num, double* den, void* ws,
                        size_t ws_bytes, void* stream) {
    if (int rc = check_common("csr_column_err", rowptr, col, val, rows, k, long_rows, long_segptr, n_long, nseg)) return rc;
    REQUIRE(Lp && Fp && num && den && cols >= 1 && cols < (1L << 31) && aligned16(Lp) && aligned16(Fp),
            "csr_column_err: null / misaligned operand or bad shape");
    const ColerrWs L = colerr_layout(cols, k, nseg, masked != 0);
    const size_t need = masked ? (size_t)nseg * 2 * sizeof(double) : L.total;
    if ((need > 0 || n_long > 0) && (!ws || ws_bytes < need || !aligned16(ws)))
        return fail(DNMF_EWS, "csr_column_err: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = S(stream);
    const int kpad = csr_kpad_of(k);
    double* dpart = ws ? (double*)((char*)ws + L.dpart) : nullptr;
    if (masked)
        return colerr_dispatch<true>(kpad, rowptr, col, val, rows, Lp, Fp, k, (const double*)nullptr, long_rows, long_segptr, n_long, nseg,
                                     dpart, num, den, st);
    double* gpart = (double*)((char*)ws + L.gpart);
    double* Gm = (double*)((char*)ws + L.gram);
    const unsigned tiles = (unsigned)(cdiv(k, 16) * cdiv(k, 16));
    hipLaunchKernelGGL(csr_gram_f64_kernel, dim3((unsigned)L.nc, tiles), dim3(256), 0, st, Fp, cols, kpad, k, cdiv(cols, L.nc), gpart);
    hipLaunchKernelGGL(csr_gram_sum_kernel, dim3((unsigned)cdiv(k * k, 256)), dim3(256), 0, st, (const double*)gpart, L.nc, k * k, Gm);
    return colerr_dispatch<false>(kpad, rowptr, col, val, rows, Lp, Fp, k, (const double*)Gm, long_rows, long_segptr, n_long, nseg, dpart, num,
                                  den, st);
}

}  // extern "C"
