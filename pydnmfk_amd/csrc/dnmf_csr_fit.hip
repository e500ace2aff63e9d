// dnmf_csr_fit.hip -- whole MU fits of sparse (CSR) data blocks, one problem or a batch that shares one pattern: `itr` update steps, the
// final normalisation and the two squared norms of the relative error in ONE library call (include/dnmf_csr_fit_api.h).  Replaces the
// Python loop of PyNMF.fit over a SparseBlock on one rank and, batched, the one-by-one perturbation fits of an NMFk sweep over sparse data.
// The passes over the stored entries are the batched kernels of csrc/dnmf_csr_batch.h (one index read per tile of problems,
// problem-interleaved packed images); everything that never sees A -- Gram matrices, update rules, clamps, sums, normalisation -- is a
// launch of the per-step entry points under the batch state of csrc/dnmf_fit.hip (blockIdx.z = problem, bit-identical to single
// launches), in the order the step loop issues them.  A translation unit of its own (see csrc/dnmf_kl.hip).
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_csr_batch.h"

namespace {

// [ batch x slice | image of W | image of H^T ];  a slice: [ G | product | x | scratch | long-row partials | gw | gh | dpart | sq ]
struct CsrFitWs {
    int kpad, G, bt, tiles, kp, ncw, nch;
    long nw;
    size_t g, prod, x, scratch, scratch_bytes, part, gw, gh, dpart, sq, slice, wimg, himg, wimg_bytes, himg_bytes, total;
};

bool csr_fit_shape_ok(long m, long n, int k, int batch) {
    return m >= 1 && n >= 1 && m < (1L << 31) && n < (1L << 31) && csr_kpad_of(k) > 0 && batch >= 1;
}

CsrFitWs csr_fit_layout(long m, long n, int k, int batch, long nseg) {
    CsrFitWs L{};
    L.kpad = csr_kpad_of(k); L.G = L.kpad / 4; L.bt = batch == 1 ? 1 : csrb_bt(L.kpad); L.tiles = (int)cdiv(batch, L.bt); L.kp = dnmf_kp(k);
    L.ncw = gram_chunks(m, k); L.nch = gram_chunks(n, k); L.nw = resid_waves(m);
    size_t o = 0;
    L.g = o; o += align256((size_t)L.kp * L.kp * sizeof(float));
    L.prod = o; o += align256((size_t)std::max(m, n) * k * sizeof(float));                 // A H^T / U H^T (m x k), W^T A / W^T U (k x n)
    L.x = o; o += align256((size_t)L.kp * sizeof(float));                                  // row sums of H, column sums of W
    L.scratch_bytes = align256(std::max(dnmf_ws_bytes(k, n, k), dnmf_ws_bytes(m, k, k)));  // what the Gram and column-sum launches ask for
    L.scratch = o; o += L.scratch_bytes;
    L.part = o; o += align256((size_t)nseg * 2 * L.kpad * sizeof(float));                  // partial rows or pairs of the long rows
    L.gw = o; o += align256((size_t)L.ncw * k * k * sizeof(double));
    L.gh = o; o += align256((size_t)L.nch * k * k * sizeof(double));
    L.dpart = o; o += align256((size_t)(L.nw + nseg) * sizeof(double));
    L.sq = o; o += 256;
    L.slice = o;
    L.wimg_bytes = align256((size_t)L.tiles * m * L.bt * L.kpad * sizeof(float));
    L.himg_bytes = align256((size_t)L.tiles * n * L.bt * L.kpad * sizeof(float));
    L.wimg = (size_t)batch * L.slice;
    L.himg = L.wimg + L.wimg_bytes;
    L.total = L.himg + L.himg_bytes;
    return L;
}

// one image of the pattern as a pass reads it: the block's (rows = m, L = W, F = H^T) or its transpose's (rows = n, L = H^T, F = W)
struct CsrSide {
    const int* rowptr; const int* col; const float* val; long rows; const float* Limg; const float* Fimg; long frows;
    const int* long_rows; const int* long_segptr; int n_long, nseg, out_trans;
};
struct CsrPass {
    CsrSide s; long vstride; int batch, tiles, k; float eps; float* out; float* out2; long ostride, ldo; int clamp;
    float* part; double* dpart; long slice;
};

template <int MODE, int END>
struct PassLaunch {
    template <int G, bool ONE>
    static int run(const CsrPass& p, hipStream_t st) {
        constexpr int BT = ONE ? 1 : csrb_bt(4 * G);
        const CsrSide& s = p.s;
        hipLaunchKernelGGL((csrb_rows_kernel<G, MODE, END, BT>), dim3((unsigned)cdiv(s.rows, 4), 1, (unsigned)p.tiles), dim3(256), 0, st, s.rowptr,
                           s.col, s.val, p.vstride, s.rows, p.batch, s.Limg, s.Fimg, s.frows, p.k, p.eps, p.out, p.out2, p.ostride, p.ldo,
                           s.out_trans, p.clamp);
        if (s.n_long > 0) {
            hipLaunchKernelGGL((csrb_long_kernel<G, MODE, BT>), dim3((unsigned)cdiv(s.nseg, 4), 1, (unsigned)p.tiles), dim3(256), 0, st, s.rowptr,
                               s.col, s.val, p.vstride, s.rows, p.batch, s.Limg, s.Fimg, s.frows, p.eps, s.long_rows, s.long_segptr, s.n_long,
                               p.part, (double*)nullptr, p.slice);
            if (MODE == CSR_M_FRO || MODE == CSR_M_KL)
                hipLaunchKernelGGL((csrb_long_reduce_pair_kernel<END>), dim3((unsigned)s.n_long, (unsigned)p.batch), dim3(4 * G), 0, st,
                                   (const float*)p.part, p.slice, 4 * G, s.long_rows, s.long_segptr, s.Limg, s.rows, BT, p.k, p.eps, p.clamp,
                                   p.out, p.out2, p.ostride, p.ldo, s.out_trans);
            else
                hipLaunchKernelGGL(csrb_long_reduce_kernel, dim3((unsigned)s.n_long, (unsigned)p.batch), dim3(4 * G), 0, st, (const float*)p.part,
                                   p.slice, 4 * G, s.long_rows, s.long_segptr, p.k, p.out, p.ostride, p.ldo, s.out_trans);
        }
        return check_launch("csr_mu_fit_batch: pass over the stored entries");
    }
};

// the float64 partials of the residual: resid_waves(rows) per problem from the rows, one per segment behind them
template <int MODE>
struct ResidLaunch {
    template <int G, bool ONE>
    static int run(const CsrPass& p, hipStream_t st, long nw) {
        constexpr int BT = ONE ? 1 : csrb_bt(4 * G);
        const CsrSide& s = p.s;
        hipLaunchKernelGGL((csrb_resid_rows_kernel<G, MODE, BT>), dim3((unsigned)(nw / 4), 1, (unsigned)p.tiles), dim3(256), 0, st, s.rowptr, s.col,
                           s.val, p.vstride, s.rows, p.batch, s.Limg, s.Fimg, s.frows, p.dpart, p.slice);
        if (s.n_long > 0)
            hipLaunchKernelGGL((csrb_long_kernel<G, MODE, BT>), dim3((unsigned)cdiv(s.nseg, 4), 1, (unsigned)p.tiles), dim3(256), 0, st, s.rowptr,
                               s.col, s.val, p.vstride, s.rows, p.batch, s.Limg, s.Fimg, s.frows, 0.f, s.long_rows, s.long_segptr, s.n_long,
                               (float*)nullptr, p.dpart + nw, p.slice);
        return check_launch("csr_mu_fit_batch: residual");
    }
};

// ONE: a single problem runs the kernels at BT = 1 -- its images are the plain packed images, nothing is interleaved with absent problems
template <typename F, bool ONE, typename... A>
int by_kpad_bt(int kpad, A&&... a) {
    switch (kpad) {
        case 16: return F::template run<4, ONE>(a...);
        case 32: return F::template run<8, ONE>(a...);
        case 64: return F::template run<16, ONE>(a...);
        case 128: return F::template run<32, ONE>(a...);
        default: return F::template run<64, ONE>(a...);
    }
}
template <typename F, typename... A>
int by_kpad(int kpad, const CsrPass& p, A&&... a) {
    return p.batch == 1 ? by_kpad_bt<F, true>(kpad, p, a...) : by_kpad_bt<F, false>(kpad, p, a...);
}

int pass_any(int norm, int missing, const CsrPass& p, hipStream_t st) {
    const int kpad = csr_kpad_of(p.k);
    if (missing) return norm ? by_kpad<PassLaunch<CSR_M_KL, CSR_END_UPDATE>>(kpad, p, st) : by_kpad<PassLaunch<CSR_M_FRO, CSR_END_UPDATE>>(kpad, p, st);
    return norm ? by_kpad<PassLaunch<CSR_KL_MM, CSR_END_STORE>>(kpad, p, st) : by_kpad<PassLaunch<CSR_MM, CSR_END_STORE>>(kpad, p, st);
}

}  // namespace

extern "C" {

int dnmf_csr_fit_plan(long m, long n, int k, int batch, long out[6]) {
    REQUIRE(out, "csr_fit_plan: null pointer");
    REQUIRE(csr_fit_shape_ok(m, n, k, batch), "csr_fit_plan: bad shape (m=%ld n=%ld k=%d batch=%d; 1 <= m, n < 2^31, 1 <= k <= %d, batch >= 1)", m,
            n, k, batch, DNMF_MAX_K);
    const CsrFitWs L = csr_fit_layout(m, n, k, batch, 0);
    out[0] = L.kpad; out[1] = L.G; out[2] = L.bt; out[3] = L.tiles; out[4] = (long)L.wimg_bytes; out[5] = (long)L.himg_bytes;
    return DNMF_OK;
}

size_t dnmf_csr_fit_ws_bytes(long m, long n, int k, int batch, int nseg_max) {
    if (!csr_fit_shape_ok(m, n, k, batch) || nseg_max < 0) return 0;
    return csr_fit_layout(m, n, k, batch, nseg_max).total;
}

int dnmf_csr_mu_fit_batch(long m, long n, int k, int batch, long nnz, const int* crow, const int* col, const int* long_rows,
                          const int* long_segptr, int n_long, int nseg, const int* t_crow, const int* t_col, const int* t_long_rows,
                          const int* t_long_segptr, int t_n_long, int t_nseg, const float* val, const float* t_val, long val_stride, float* W,
                          long ldw, long w_stride, float* H, long ldh, long h_stride, int norm, int missing, float eps, int w_update, int itr,
                          void* ws, size_t ws_bytes, double* sq_out, void* stream) {
    // ---- refusals, before any HIP call
    REQUIRE(batch >= 1, "csr_mu_fit_batch: batch=%d (at least one problem)", batch);
    REQUIRE(csr_kpad_of(k) > 0, "csr_mu_fit_batch: rank k=%d unsupported (1 <= k <= %d)", k, DNMF_MAX_K);
    REQUIRE(m >= 1 && n >= 1 && m < (1L << 31) && n < (1L << 31) && nnz >= 1 && nnz < (1L << 31),
            "csr_mu_fit_batch: bad shape (m=%ld n=%ld nnz=%ld; 1 <= m, n, nnz < 2^31)", m, n, nnz);
    REQUIRE(crow && col && t_crow && t_col && val && t_val && W && H && sq_out && ws, "csr_mu_fit_batch: null pointer");
    REQUIRE((norm == 0 || norm == 1) && (missing == 0 || missing == 1) && itr >= 0,
            "csr_mu_fit_batch: norm=%d (0 fro, 1 kl), missing=%d (0 zero, 1 unstored), itr=%d", norm, missing, itr);
    REQUIRE(ldw >= k && ldh >= n && aligned16(val) && aligned16(t_val), "csr_mu_fit_batch: leading dimension too small or misaligned values");
    REQUIRE(n_long >= 0 && nseg >= 0 && t_n_long >= 0 && t_nseg >= 0 && (n_long == 0 || (long_rows && long_segptr && nseg >= n_long)) &&
                (t_n_long == 0 || (t_long_rows && t_long_segptr && t_nseg >= t_n_long)),
            "csr_mu_fit_batch: bad long-row lists (n_long=%d / %d, segments=%d / %d)", n_long, t_n_long, nseg, t_nseg);
    REQUIRE(batch == 1 || (val_stride >= nnz && val_stride % 4 == 0), "csr_mu_fit_batch: val_stride=%ld (a multiple of 4, >= nnz=%ld)", val_stride, nnz);
    REQUIRE(aligned16(ws), "csr_mu_fit_batch: the workspace must start on a 16-byte boundary");
    const long nsegmax = std::max(nseg, t_nseg);
    const CsrFitWs L = csr_fit_layout(m, n, k, batch, nsegmax);
    REQUIRE(ws_bytes >= L.total, "csr_mu_fit_batch: workspace %zu < %zu bytes", ws_bytes, L.total);
    BatchCtx* ctx = dnmf_batch_();
    REQUIRE(ctx->B == 1, "csr_mu_fit_batch: called inside a batched fit");
    BatchGuard guard(ctx);
    // the families of the launches that never see the pattern: the value arrays (one 1 x nnz matrix each: ||A||^2), W, H, the slices
    if (batch > 1) {
        const BatchFam fam[4] = {{(unsigned long)val, (unsigned long)val + (size_t)nnz * 4, val_stride * 4},
                                 {(unsigned long)W, (unsigned long)W + ((size_t)(m - 1) * ldw + k) * 4, w_stride * 4},
                                 {(unsigned long)H, (unsigned long)H + ((size_t)(k - 1) * ldh + n) * 4, h_stride * 4},
                                 {(unsigned long)ws, (unsigned long)ws + L.slice, (long)L.slice}};
        for (int i = 0; i < 4; ++i) {
            if (fam[i].stride % 16 != 0 || fam[i].stride < 0 || (unsigned long)fam[i].stride < fam[i].hi - fam[i].lo)
                return fail(DNMF_EINVAL, "csr_mu_fit_batch: stride of operand %d (%ld bytes) must be a multiple of 16 bytes and span one problem (%lu bytes)",
                            i, fam[i].stride, fam[i].hi - fam[i].lo);
            for (int j = 0; j < i; ++j)
                if (overlap(fam[i], fam[j])) return fail(DNMF_EINVAL, "csr_mu_fit_batch: operands %d and %d overlap", j, i);
            ctx->tab.f[i] = fam[i];
        }
        ctx->tab.n = 4;
        ctx->B = batch;
    } else {
        val_stride = w_stride = h_stride = 0;
    }

    hipStream_t st = S(stream);
    char* base = (char*)ws;
    float* G = (float*)(base + L.g);
    float* prod = (float*)(base + L.prod);
    float* x = (float*)(base + L.x);
    void* scratch = base + L.scratch;
    float* Wimg = (float*)(base + L.wimg);
    float* Himg = (float*)(base + L.himg);
    const long slice = (long)L.slice;
    const CsrSide block{crow, col, val, m, Wimg, Himg, n, long_rows, long_segptr, n_long, nseg, 0};
    const CsrSide trans{t_crow, t_col, t_val, n, Himg, Wimg, m, t_long_rows, t_long_segptr, t_n_long, t_nseg, 1};
    CsrPass p{};
    p.vstride = val_stride; p.batch = batch; p.tiles = L.tiles; p.k = k; p.eps = eps; p.part = (float*)(base + L.part);
    p.dpart = (double*)(base + L.dpart); p.slice = slice;

    bool w_stale = true, h_stale = true;                 // the images against the factors
    auto pack = [&]() -> int {
        if (w_stale) {
            const long quads = m * (L.kpad / 4);
            hipLaunchKernelGGL(csrb_pack_kernel, dim3((unsigned)std::min<long>(cdiv(quads, 256), 8192), (unsigned)batch), dim3(256), 0, st,
                               (const float*)W, w_stride, m, k, ldw, Wimg, L.kpad, L.bt);
        }
        if (h_stale)
            hipLaunchKernelGGL(csrb_pack_t_kernel, dim3((unsigned)cdiv(n, 32), (unsigned)cdiv(L.kpad, 32), (unsigned)batch), dim3(256), 0, st,
                               (const float*)H, h_stride, k, n, ldh, Himg, L.kpad, L.bt);
        w_stale = h_stale = false;
        return check_launch("csr_mu_fit_batch: pack");
    };
    // the product of a side into the slices (zero meaning), or the rule applied to the factor stack itself (missing)
    auto side = [&](bool h_side, int clamp) -> int {
        p.s = h_side ? trans : block;
        p.clamp = clamp;
        if (missing) {
            p.out = h_side ? H : W; p.out2 = nullptr;
            p.ostride = (h_side ? h_stride : w_stride) * (long)sizeof(float);
            p.ldo = h_side ? ldh : ldw;
        } else {
            p.out = prod; p.out2 = nullptr; p.ostride = slice; p.ldo = h_side ? n : (long)k;
        }
        return pass_any(norm, missing, p, st);
    };

    int rc = DNMF_OK;
    for (int i = 0; i < itr && !rc; ++i) {                                               // pyDNMF.py:151-172
        const int clamp = (i % 10 == 0);
        if (w_update) {
            if (!missing && !norm && (rc = dnmf_gram_hht(H, k, n, ldh, G, scratch, L.scratch_bytes, stream))) break;     // dist_nmf.py:729
            if (!missing && norm && (rc = dnmf_rowsum(H, k, n, ldh, x, stream))) break;                                  // :827
            if ((rc = pack()) || (rc = side(false, 0))) break;
            if (!missing) {
                if (!norm) rc = dnmf_mu_update_w(W, m, k, ldw, prod, k, G, eps, stream);                                 // :731-732
                else rc = dnmf_kl_update_w(W, m, k, ldw, prod, k, x, eps, stream);                                       // :828-830
                if (rc) break;
            }
            w_stale = true;
        }
        if (!missing && !norm && (rc = dnmf_gram_wtw(W, m, k, ldw, G, scratch, L.scratch_bytes, stream))) break;         // :705
        if (!missing && norm && (rc = dnmf_colsum(W, m, k, ldw, x, scratch, L.scratch_bytes, stream))) break;            // :846
        if ((rc = pack()) || (rc = side(true, clamp))) break;
        if (!missing) {
            if (!norm) rc = dnmf_mu_update_h(H, k, n, ldh, prod, n, G, eps, clamp, stream);                              // :750-751
            else rc = dnmf_kl_update_h(H, k, n, ldh, prod, n, x, eps, clamp, stream);                                    // :847-849
            if (rc) break;
        }
        h_stale = true;
        if (clamp) {                                                                                                     // pyDNMF.py:170-172
            if ((rc = dnmf_clamp_min(W, m, k, ldw, eps, stream))) break;
            w_stale = true;
        }
    }
    if (rc) return rc;
    // normalize_features (pyDNMF.py:185-194)
    if ((rc = dnmf_colsum(W, m, k, ldw, x, scratch, L.scratch_bytes, stream))) return rc;
    if ((rc = dnmf_scale_cols_div(W, m, k, ldw, x, eps, stream))) return rc;
    if ((rc = dnmf_scale_rows_mul(H, k, n, ldh, x, stream))) return rc;
    w_stale = h_stale = true;
    // relative_err (pyDNMF.py:205-218): the residual's closed form (or, missing, its sum over the stored positions), and sum A^2
    if ((rc = pack())) return rc;
    double* gw = (double*)(base + L.gw);
    double* gh = (double*)(base + L.gh);
    double* sq = (double*)(base + L.sq);
    p.s = block;
    if (!missing) {
        const unsigned tiles16 = (unsigned)(cdiv(k, 16) * cdiv(k, 16));
        hipLaunchKernelGGL(csrb_gram_f64_kernel, dim3((unsigned)L.ncw, tiles16, (unsigned)batch), dim3(256), 0, st, (const float*)Wimg, m, L.kpad,
                           L.bt, k, cdiv(m, L.ncw), gw, slice);
        hipLaunchKernelGGL(csrb_gram_f64_kernel, dim3((unsigned)L.nch, tiles16, (unsigned)batch), dim3(256), 0, st, (const float*)Himg, n, L.kpad,
                           L.bt, k, cdiv(n, L.nch), gh, slice);
        if ((rc = by_kpad<ResidLaunch<CSR_RESID>>(L.kpad, p, st, L.nw))) return rc;
        hipLaunchKernelGGL(csrb_resid_final_kernel, dim3((unsigned)batch), dim3(256), 0, st, (const double*)gw, L.ncw, (const double*)gh, L.nch, k,
                           (const double*)p.dpart, L.nw + (n_long > 0 ? nseg : 0), sq, slice);
    } else {
        if ((rc = by_kpad<ResidLaunch<CSR_M_RESID>>(L.kpad, p, st, L.nw))) return rc;
        hipLaunchKernelGGL(csrb_resid_final_kernel, dim3((unsigned)batch), dim3(256), 0, st, (const double*)nullptr, 0, (const double*)nullptr, 0, 0,
                           (const double*)p.dpart, L.nw + (n_long > 0 ? nseg : 0), sq, slice);
    }
    if ((rc = check_launch("csr_mu_fit_batch: residual"))) return rc;
    if ((rc = dnmf_sqnorm(val, 1, nnz, nnz, sq + 1, stream))) return rc;
    if (hipMemcpy2DAsync(sq_out, 2 * sizeof(double), sq, L.slice, 2 * sizeof(double), (size_t)batch, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return fail(DNMF_EHIP, "csr_mu_fit_batch: copy of the squared norms failed");
    return DNMF_OK;
}

}  // extern "C"
