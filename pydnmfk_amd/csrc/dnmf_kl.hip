// dnmf_kl.hip -- C ABI of the NN-form kernels (residual / per-column error, the two KL products: csrc/dnmf_nn.h).  A translation
// unit of its own: this kernel family compiles as long as the rest together, so it builds side by side with csrc/dnmf.hip.
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_nt.h"
#include "dnmf_stream.h"
#include "dnmf_nn.h"

// the 16-wide kernels for k <= 16 live in csrc/dnmf_kl16.hip (own compiler flags); 1 = not applicable
__attribute__((visibility("hidden"))) int dnmf_kl16_uht_(const float* A, long m, long n, long lda, const float* W, long ldw,
                                                         const float* H, long ldh, long hblk, int k, float eps, float* UHT,
                                                         long ldo, void* ws, size_t ws_bytes, void* stream);
__attribute__((visibility("hidden"))) int dnmf_kl16_wtu_(const float* A, long m, long n, long lda, const float* W, long ldw,
                                                         const float* H, long ldh, int k, float eps, float* WTU, long ldo,
                                                         void* ws, size_t ws_bytes, void* stream);

// the software-pipelined U H^T for whole 128-row tiles (csrc/dnmf_kluht.hip)
__attribute__((visibility("hidden"))) int dnmf_kl_uht_pipe_(const float* A, long rowtiles, long n, long lda, const float* W, long ldw,
                                                            const float* H, long ldh, long hblk, long hextra, int kt, float eps,
                                                            float* out, long ldo, long split_stride, long cols_per_split,
                                                            int nsplit, void* stream);

// csrc/dnmf_wide.hip: ranks 128 < k <= 256
#define HID __attribute__((visibility("hidden")))
HID int dnmf_wide_quot_(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps, float* U,
                        long ldu, void* stream);
HID int dnmf_wide_resid_(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, double* out,
                         void* stream);
HID int dnmf_wide_column_err_(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, double* num,
                              double* den, void* stream);
#undef HID

namespace {
// The KL products of a wide rank: U = A / (W H + eps) materialised at the END of the caller's workspace (dnmf_ws_bytes reserves the
// image for k > 128), then the tuned contraction on U.  uht: U H^T; else W^T U.
int wide_kl_product(bool uht, const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps,
                    float* out, long ldo, void* ws, size_t ws_bytes, void* stream) {
    const long ldu = round_up(n, 4);
    const size_t ub = align256((size_t)m * ldu * sizeof(float));
    if (!ws || ws_bytes < ub) return fail(DNMF_EWS, "kl product (k = %d): workspace %zu < %zu (the quotient image)", k, ws_bytes, ub);
    const size_t inner = (ws_bytes - ub) & ~size_t(255);
    float* U = (float*)((char*)ws + inner);
    if (int rc = dnmf_wide_quot_(A, m, n, lda, W, ldw, H, ldh, k, eps, U, ldu, stream)) return rc;
    return uht ? dnmf_aht(U, m, n, ldu, H, k, ldh, out, ldo, stream) : dnmf_wta(U, m, n, ldu, W, k, ldw, out, ldo, ws, inner, stream);
}
}  // namespace

extern "C" {

static NnArgs nn_args(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                      int k, float eps) {
    NnArgs a{};
    a.A = A; a.lda = lda; a.m = m; a.n = n; a.W = W; a.ldw = ldw; a.H = H; a.ldh = ldh; a.k = k; a.eps = eps;
    a.nrowblk = cdiv(m, 32); a.ncolblk = (int)cdiv(n, 128);
    a.kreal = k;
    return a;
}

}  // extern "C"
namespace {
// ---- selectors: every choice the entry points of this file make between kernels, template arguments and grids, as a function of the
// shape, the pitches, the operands' addresses modulo 16 (off16) and the workspace size.  The entry points launch from these and
// dnmf_dense_plan reports them (dnmf_dense_plan_kl_ below).  `ea`: bytes per element of A.  offws: the workspace's address modulo 16.
struct Fac { unsigned offw; long ldw; unsigned offh; long ldh; int k; };      // the factors as the kernels will see them
inline bool fac_friendly(const Fac& f, int kp) { return f.k == kp && f.offw == 0 && f.ldw % 4 == 0 && f.offh == 0 && f.ldh % 4 == 0; }   // = pad_factors' test
// (the images sit at multiples of 256 bytes behind the workspace base: they have its address modulo 16, `offws`; the query takes 0)
inline Fac fac_padded(long n, int kp, unsigned offws) { return Fac{offws, kp, offws, round_up(n, 4), kp}; }
inline bool a_vec(unsigned offa, size_t ea, long lda, long n) { return offa % (4 * ea) == 0 && lda % 4 == 0 && n % 4 == 0; }
inline bool fac_fast(const Fac& f) { return f.offw == 0 && f.offh == 0 && f.ldw % 4 == 0 && f.k % 4 == 0 && f.ldh % 4 == 0; }

// the residual: resid_lds_kernel<KT, true, TA> (H staged through LDS, waves walking row chunks) when the block is big enough to give
// every wave a chunk of several row blocks, else resid_kernel<KT, FAST, TA> (one tile per wave)
struct ResidSel { bool pad, fast, lds; Fac f; long rpc, nchunks; int ncolblk; unsigned grid; };
inline ResidSel select_resid(long m, long n, int kt, size_t ea, unsigned offa, long lda, Fac f, bool allow_pad, size_t ws_bytes,
                             unsigned offws = 0) {
    ResidSel s{};
    const int kp = 32 * kt;
    const bool big = n >= 128 && m >= 4096;
    s.pad = allow_pad && a_vec(offa, ea, lda, n) && big && !fac_friendly(f, kp) && ws_bytes >= pad_bytes(m, n, kp);
    s.f = s.pad ? fac_padded(n, kp, offws) : f;
    s.fast = a_vec(offa, ea, lda, n) && fac_fast(s.f);
    s.ncolblk = (int)cdiv(n, 128);
    const long nrowblk = cdiv(m, 32);
    s.lds = s.fast && s.f.k % 32 == 0 && big;
    if (s.lds) {
        TnPlan pl = plan_tn(m, n, kt, 4);
        const long nch = std::max<long>(1, pl.nchunks / 2);           // one wave per SIMD (1024 waves): half of plan_tn's round
        pl.rows_per_chunk = round_up(cdiv(m, nch), 32);
        s.rpc = std::max<long>(1, round_up(pl.rows_per_chunk, 32) / 32);
        s.nchunks = cdiv(nrowblk, s.rpc);
        s.grid = (unsigned)(cdiv(s.nchunks, 4) * s.ncolblk);
    } else {
        s.rpc = 1;
        s.nchunks = nrowblk;
        s.grid = (unsigned)cdiv(nrowblk * s.ncolblk, 4);
    }
    return s;
}

// the per-column error: colerr_kernel<KT, FAST, TA>, about 8 waves per SIMD in flight, every wave walking a chunk of row blocks of its
// 128-column block
struct ColerrSel { bool fast; long rpc, nchunks; int ncolblk; unsigned grid; };
inline ColerrSel select_colerr(long m, long n, size_t ea, unsigned offa, long lda, const Fac& f) {
    ColerrSel s;
    const long nrowblk = cdiv(m, 32);
    s.ncolblk = (int)cdiv(n, 128);
    s.fast = a_vec(offa, ea, lda, n) && fac_fast(f);
    s.rpc = std::max<long>(1, cdiv(nrowblk * s.ncolblk, 8192));
    s.nchunks = cdiv(nrowblk, s.rpc);
    s.grid = (unsigned)cdiv(s.nchunks * s.ncolblk, 4);
    return s;
}

// W^T U at 16 < k <= 128: kl_wtu_kernel<KT, NT, FAST> on row chunks, then the reduction of the chunk slabs
struct KlWtuSel { bool ews, pad, fast; Fac f; KlWtuPlan plan; size_t pbytes, need; unsigned grid; };
inline KlWtuSel select_kl_wtu(long m, long n, int k, int kt, unsigned offa, long lda, Fac f, bool allow_pad, size_t ws_bytes,
                              unsigned offws = 0) {
    KlWtuSel s{};
    const int kp = 32 * kt;
    s.plan = plan_kl_wtu(m, n, kt);
    s.pbytes = (size_t)s.plan.nchunks * s.plan.tn.ldp * kp * sizeof(float);
    s.need = s.pbytes + reduce_scratch_bytes((int)s.plan.nchunks, k, n);
    s.ews = ws_bytes < s.need;
    s.pad = allow_pad && a_vec(offa, 4, lda, n) && offa == 0 && !fac_friendly(f, kp) && ws_bytes >= align256(s.need) + pad_bytes(m, n, kp);
    s.f = s.pad ? fac_padded(n, kp, offws) : f;
    s.fast = offa == 0 && a_vec(offa, 4, lda, n) && fac_fast(s.f);
    s.grid = (unsigned)(cdiv(s.plan.nchunks, 4) * s.plan.tn.ncolblk);
    return s;
}

// U H^T at 16 < k <= 128 (and what the 16-wide kernel leaves).  Whole 128-row tiles of a friendly problem (aligned rows, k = KP or padded
// to it, whole 32-column tiles, 2 GiB descriptor windows) go to the software-pipelined kernel (kl_uht_pipe_kernel<KT, .>); a ragged
// last row tile -- or everything else -- to kl_uht_kernel<KT, FAST>.  Same arithmetic in the same order: the two are bit identical.
// hblk > 0: H as column blocks; a column split must not straddle a block: cols_per_split divides hblk.
// ews: 0 fine, 1 the split slabs do not fit the workspace, 2 not even one split per block does.
struct KlUhtSel { int ews; bool pad, fast, pipe; Fac f; UhtPlan u; size_t pbytes, need; long rowtile0, rest; };
inline KlUhtSel select_kl_uht(long m, long n, int k, int kt, unsigned offa, long lda, Fac f, long hblk, unsigned offo, long ldo, bool allow_pad,
                              size_t ws_bytes, unsigned offws = 0) {
    KlUhtSel s{};
    const int kp = 32 * kt;
    s.u = plan_uht(m, n, kt);
    if (hblk) {
        const long nb = n / hblk;
        long sp = std::max<long>(1, (s.u.nsplit + nb / 2) / nb);
        auto fits = [&](long q) { return hblk % q == 0 && (hblk / q) % BK == 0 &&
                                         (size_t)(nb * q) * m * kp * sizeof(float) + reduce_scratch_bytes((int)(nb * q), (int)m, k) <= ws_bytes; };
        while (sp > 1 && !fits(sp)) --sp;
        if (!fits(sp) && nb * sp > 1) { s.ews = 2; return s; }
        s.u.cols_per_split = hblk / sp;
        s.u.nsplit = (int)(nb * sp);
    }
    const bool split = s.u.nsplit > 1;
    s.pbytes = split ? (size_t)s.u.nsplit * m * kp * sizeof(float) : 0;
    s.need = s.pbytes + reduce_scratch_bytes(s.u.nsplit, (int)m, k);
    if (split && ws_bytes < s.need) { s.ews = 1; return s; }
    const bool a16 = offa == 0 && lda % 4 == 0 && n % 4 == 0;
    const bool room = ws_bytes >= align256(s.need) + pad_bytes(m, n, kp);
    if (allow_pad && a16 && room)
        s.pad = hblk ? !(f.k == kp && f.offw == 0 && f.ldw % 4 == 0 && f.offh == 0) : !fac_friendly(f, kp);
    s.f = s.pad ? fac_padded(n, kp, offws) : f;
    const long ldout = split ? kp : ldo;
    const int out_cols = split ? kp : k;
    s.fast = a16 && fac_fast(s.f) && (split ? offws == 0 : offo == 0) && ldout % 4 == 0;      // (split slabs start at the workspace base)
    auto window = [](long rows, long ld, long cols) { return (rows * ld + cols) * 4 < 0x7fffffffL; };
    s.pipe = s.fast && s.f.k == kp && m >= 128 && n % BK == 0 && s.u.cols_per_split % BK == 0 && out_cols >= kp &&
             window(128, lda, s.u.cols_per_split) && window(kp, s.f.ldh, s.u.cols_per_split);
    s.rowtile0 = s.pipe ? m / 128 : 0;
    s.rest = cdiv(m, 128) - s.rowtile0;
    return s;
}
// the reductions of the two KL products: column-split slabs [nsplit][m][KP] -> m x k; chunk slabs [nchunks][KP][ldp] -> k x n
inline ReduceShape reduce_shape_kl_uht(long m, int kp, int nsplit, int k) { return ReduceShape{m * kp, kp, nsplit, (int)m, k, (int)m, k}; }
inline ReduceShape reduce_shape_kl_wtu(const KlWtuPlan& pl, int kp, int k, long n) {
    return ReduceShape{pl.tn.ldp * kp, pl.tn.ldp, (int)pl.nchunks, k, n, k, n};
}
}  // namespace
namespace {
// ws (optional): with room for the zero-padded factor images (pad_bytes: every dnmf_ws_bytes workspace has it) a rank that is
// not a whole number of 32-wide tiles -- every k an NMFk sweep visits -- runs the LDS-staged kernel on [m x KP] / [KP x n]
// images instead of the predicated one-tile-per-wave kernel (round 4: 0.645 -> ~0.39 ms at 32768 x 16384, k = 16; zero
// columns of W / rows of H add nothing to W H).
template <typename TA>
int resid_sqnorm_impl(const TA* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                      int k, double* out, void* stream, void* ws = nullptr, size_t ws_bytes = 0) {
    REQUIRE_WS16(ws, "resid_sqnorm");
    if (wide_k(k)) {
        REQUIRE((std::is_same<TA, float>::value) && A && W && H && out && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n,
                "resid_sqnorm: bad arguments (k = %d: float32 data)", k);
        return dnmf_wide_resid_(reinterpret_cast<const float*>(A), m, n, lda, W, ldw, H, ldh, k, out, stream);
    }
    const int kt = kt_of(k);
    REQUIRE(kt > 0 && A && W && H && out && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n, "resid_sqnorm: bad arguments");
    hipStream_t st = S(stream);
    if (batch_memset(out, 0, sizeof(double), st) != hipSuccess) return fail(DNMF_EHIP, "resid_sqnorm: memset failed");
    const Fac f0{off16(W), ldw, off16(H), ldh, k};
    ResidSel sel = select_resid(m, n, kt, sizeof(TA), off16(A), lda, f0, ws != nullptr, ws_bytes, off16(ws));
    if (sel.pad && !pad_factors(W, ldw, H, ldh, k, m, n, 32 * kt, ws, ws_bytes, 0, st))      // (the copy could not be launched: as without a workspace)
        sel = select_resid(m, n, kt, sizeof(TA), off16(A), lda, f0, false, 0);
    NnArgs a = nn_args(reinterpret_cast<const float*>(A), m, n, lda, W, ldw, H, ldh, k, 0.f);
    a.out = out;
    const bool fast = sel.fast;
    hipStream_t stq = st;
    if (sel.lds) {
        const long rpc = sel.rpc;
        a.ncolblk = sel.ncolblk;
        const dim3 grid2(sel.grid), block2(256);
        const size_t lds = (size_t)(32 * kt) * 128 * sizeof(float);
#define RL_CASE(KT_)                                                                                 \
        if (kt == KT_) {                                                                             \
            static bool once = false;                                                                \
            if (!once) { allow_lds(resid_lds_kernel<KT_, true, TA>, lds); once = true; }              \
            DNMF_LAUNCH((resid_lds_kernel<KT_, true, TA>), grid2, block2, lds, stq, a, rpc);  \
        }
        RL_CASE(1) RL_CASE(2) RL_CASE(4)
#undef RL_CASE
        return check_launch("resid_sqnorm(lds)");
    }
    const dim3 grid(sel.grid), block(256);
#define RS_CASE(KT_)                                                                  \
    if (kt == KT_) {                                                                   \
        if (fast) DNMF_LAUNCH((resid_kernel<KT_, true, TA>), grid, block, 0, st, a); \
        else DNMF_LAUNCH((resid_kernel<KT_, false, TA>), grid, block, 0, st, a);    \
    }
    RS_CASE(1) RS_CASE(2) RS_CASE(4)
#undef RS_CASE
    return check_launch("resid_sqnorm");
}
}  // namespace
extern "C" {

int dnmf_resid_sqnorm(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                      int k, double* out, void* stream) {
    return resid_sqnorm_impl<float>(A, m, n, lda, W, ldw, H, ldh, k, out, stream);
}
int dnmf_resid_sqnorm_bf16a(const void* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                            int k, double* out, void* stream) {
    return resid_sqnorm_impl<bf16_t>((const bf16_t*)A, m, n, lda, W, ldw, H, ldh, k, out, stream);
}
int dnmf_resid_sqnorm_ws(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                         int k, double* out, void* ws, size_t ws_bytes, void* stream) {
    return resid_sqnorm_impl<float>(A, m, n, lda, W, ldw, H, ldh, k, out, stream, ws, ws_bytes);
}
int dnmf_resid_sqnorm_ws_bf16a(const void* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh,
                               int k, double* out, void* ws, size_t ws_bytes, void* stream) {
    return resid_sqnorm_impl<bf16_t>((const bf16_t*)A, m, n, lda, W, ldw, H, ldh, k, out, stream, ws, ws_bytes);
}

}  // extern "C"
namespace {
template <typename TA>
int column_err_impl(const TA* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                    double* num, double* den, void* stream) {
    if (wide_k(k)) {
        REQUIRE((std::is_same<TA, float>::value) && A && W && H && num && den && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n,
                "column_err: bad arguments (k = %d: float32 data)", k);
        return dnmf_wide_column_err_(reinterpret_cast<const float*>(A), m, n, lda, W, ldw, H, ldh, k, num, den, stream);
    }
    const int kt = kt_of(k);
    REQUIRE(kt > 0 && A && W && H && num && den && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n, "column_err: bad arguments");
    hipStream_t st = S(stream);
    NnArgs a = nn_args(reinterpret_cast<const float*>(A), m, n, lda, W, ldw, H, ldh, k, 0.f);
    const ColerrSel sel = select_colerr(m, n, sizeof(TA), off16(A), lda, Fac{off16(W), ldw, off16(H), ldh, k});
    const bool fast = sel.fast;
    const long rpc = sel.rpc;
    const dim3 grid(sel.grid), block(256);
#define CE_CASE(KT_)                                                                             \
    if (kt == KT_) {                                                                             \
        if (fast) DNMF_LAUNCH((colerr_kernel<KT_, true, TA>), grid, block, 0, st, a, num, den, rpc); \
        else DNMF_LAUNCH((colerr_kernel<KT_, false, TA>), grid, block, 0, st, a, num, den, rpc);    \
    }
    CE_CASE(1) CE_CASE(2) CE_CASE(4)
#undef CE_CASE
    return check_launch("column_err");
}
}  // namespace
extern "C" {

int dnmf_column_err(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                    double* num, double* den, void* stream) {
    return column_err_impl<float>(A, m, n, lda, W, ldw, H, ldh, k, num, den, stream);
}
int dnmf_column_err_bf16a(const void* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                          double* num, double* den, void* stream) {
    return column_err_impl<bf16_t>((const bf16_t*)A, m, n, lda, W, ldw, H, ldh, k, num, den, stream);
}

}  // extern "C"
namespace {

// H as column blocks [n / hblk][k][hblk] -> one zero-padded contiguous image [kp x round_up(n, 4)] (and W -> [m x kp]) at the
// end of the workspace: the block-aware twin of pad_factors for ranks / alignments the interior paths do not take
bool pad_factors_hblocks(const float*& W, long& ldw, const float*& H, long& ldh, long hblk, int& k, long m, long n, int kp,
                         void* ws, size_t ws_bytes, size_t own_need, hipStream_t st) {
    const size_t pb = pad_bytes(m, n, kp);
    if (!ws || ws_bytes < align256(own_need) + pb) return false;
    char* base = (char*)ws + align256(own_need);
    float* Wp = (float*)base;
    const long ldhp = round_up(n, 4);
    float* Hp = (float*)(base + align256((size_t)m * kp * sizeof(float)));
    if (hipMemsetAsync(Wp, 0, (size_t)m * kp * sizeof(float), st) != hipSuccess) return false;
    if (hipMemcpy2DAsync(Wp, (size_t)kp * sizeof(float), W, (size_t)ldw * sizeof(float), (size_t)k * sizeof(float), (size_t)m,
                         hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
    if (hipMemsetAsync(Hp, 0, (size_t)kp * ldhp * sizeof(float), st) != hipSuccess) return false;
    for (long q = 0; q * hblk < n; ++q)
        if (hipMemcpy2DAsync(Hp + q * hblk, (size_t)ldhp * sizeof(float), H + q * k * hblk, (size_t)hblk * sizeof(float),
                             (size_t)hblk * sizeof(float), (size_t)k, hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
    W = Wp; ldw = kp; H = Hp; ldh = ldhp; k = kp;
    return true;
}

// hblk = 0: H is one k x n matrix (ldh).  hblk > 0: H is the stack of n / hblk column blocks [q][k][hblk] (ldh = hblk).
int kl_uht_impl(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, long hblk, int k,
                float eps, float* UHT, long ldo, void* ws, size_t ws_bytes, void* stream) {   // (W, ldw, H, ldh, k may be re-pointed at padded copies)
    REQUIRE_WS16(ws, "kl_uht");
    if (wide_k(k)) {
        REQUIRE(!hblk && A && W && H && UHT && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && ldo >= k,
                "kl_uht: bad arguments (k = %d; H as column blocks: k <= %d)", k, DNMF_TUNED_MAX_K);
        return wide_kl_product(true, A, m, n, lda, W, ldw, H, ldh, k, eps, UHT, ldo, ws, ws_bytes, stream);
    }
    const int kt = kt_of(k);
    REQUIRE(kt > 0 && A && W && H && UHT && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldo >= k, "kl_uht: bad arguments");
    REQUIRE(hblk ? (ldh == hblk && n % hblk == 0 && hblk % BK == 0) : ldh >= n, "kl_uht: bad H layout (ldh %ld, block %ld, n %ld)", ldh, hblk, n);
    const int kp = 32 * kt;
    const int k_out = k;                                   // columns of UHT the caller gets
    if (int rc16 = dnmf_kl16_uht_(A, m, n, lda, W, ldw, H, ldh, hblk, k, eps, UHT, ldo, ws, ws_bytes, stream); rc16 != 1) return rc16;
    const Fac f0{off16(W), ldw, off16(H), ldh, k};
    const size_t wsb = ws ? ws_bytes : 0;
    KlUhtSel sel = select_kl_uht(m, n, k, kt, off16(A), lda, f0, hblk, off16(UHT), ldo, true, wsb, off16(ws));
    if (sel.ews == 2) return fail(DNMF_EWS, "kl_uht: workspace %zu too small for %ld column blocks", ws_bytes, n / hblk);
    if (sel.ews) return fail(DNMF_EWS, "kl_uht: workspace %zu < %zu", ws_bytes, sel.need);
    if (sel.pad) {
        const bool done = hblk ? pad_factors_hblocks(W, ldw, H, ldh, hblk, k, m, n, kp, ws, ws_bytes, sel.need, S(stream))
                               : pad_factors(W, ldw, H, ldh, k, m, n, kp, ws, ws_bytes, sel.need, S(stream));
        if (done) hblk = 0;                                // (the padded image is one matrix)
        else sel = select_kl_uht(m, n, k_out, kt, off16(A), lda, f0, hblk, off16(UHT), ldo, false, wsb, off16(ws));      // (a copy could not be made)
    }
    const UhtPlan& u = sel.u;
    const size_t pbytes = sel.pbytes;
    NnArgs a = nn_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    a.kreal = k_out;                                       // (k may be the padded rank by now)
    a.hblk = hblk; a.hextra = hblk ? (long)k * hblk - hblk : 0;
    const bool split = u.nsplit > 1;
    float* out = split ? (float*)ws : UHT;
    const long ldout = split ? kp : ldo;
    const int out_cols = split ? kp : k_out;
    const bool fast = sel.fast;
    hipStream_t st = S(stream);
    const long rowtile0 = sel.rowtile0;
    if (sel.pipe)
        if (int rcp = dnmf_kl_uht_pipe_(A, rowtile0, n, lda, W, ldw, H, ldh, hblk, a.hextra, kt, eps, out, ldout, (long)m * kp,
                                        u.cols_per_split, u.nsplit, stream); rcp) return rcp;
    a.rowtile0 = rowtile0;
    const dim3 grid((unsigned)sel.rest, (unsigned)u.nsplit), block(256);
    const size_t lds = 2ul * kp * BK * sizeof(float);
    if (grid.x > 0) {
#define UH_CASE(KT_)                                                                                                  \
    if (kt == KT_) {                                                                                                  \
        if (fast) DNMF_LAUNCH((kl_uht_kernel<KT_, true>), grid, block, lds, st, a, out, ldout, (long)m * kp,    \
                                     u.cols_per_split, out_cols);                                                     \
        else DNMF_LAUNCH((kl_uht_kernel<KT_, false>), grid, block, lds, st, a, out, ldout, (long)m * kp,        \
                                u.cols_per_split, out_cols);                                                          \
    }
    UH_CASE(1) UH_CASE(2) UH_CASE(4)
#undef UH_CASE
    }
    int rc = check_launch("kl_uht");
    if (rc || !split) return rc;
    return launch_reduce((const float*)ws, reduce_shape_kl_uht(m, kp, u.nsplit, k_out), UHT, ldo, (float*)((char*)ws + pbytes), st);
}

}  // namespace
extern "C" {

int dnmf_kl_uht(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                float eps, float* UHT, long ldo, void* ws, size_t ws_bytes, void* stream) {
    return kl_uht_impl(A, m, n, lda, W, ldw, H, ldh, 0, k, eps, UHT, ldo, ws, ws_bytes, stream);
}

size_t dnmf_ws_bytes_hblocks(long m, long n, int k, long nh) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1 || nh < 1 || n % nh) return 0;
    const int kp = 32 * kt;
    // a column split never straddles a block: at least n / nh splits, at most twice the planner's count
    const UhtPlan u = plan_uht(m, n, kt);
    const long nb = n / nh, nsp = nb * std::max<long>(1, (u.nsplit + nb / 2) / nb);
    const size_t slabs = (size_t)nsp * m * kp * sizeof(float) + reduce_scratch_bytes((int)nsp, (int)m, k);
    return std::max(dnmf_ws_bytes(m, n, k), align256(slabs) + pad_bytes(m, n, kp));
}

int dnmf_kl_uht_hblocks(const float* A, long m, long n, long lda, const float* W, long ldw, const float* Hs, long nh, int k,
                        float eps, float* UHT, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(nh >= 1, "kl_uht_hblocks: bad block width");
    return kl_uht_impl(A, m, n, lda, W, ldw, Hs, nh, nh, k, eps, UHT, ldo, ws, ws_bytes, stream);
}

int dnmf_kl_wtu(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                float eps, float* WTU, long ldo, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "kl_wtu");
    if (wide_k(k)) {
        REQUIRE(A && W && H && WTU && ws && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && ldo >= n, "kl_wtu: bad arguments");
        return wide_kl_product(false, A, m, n, lda, W, ldw, H, ldh, k, eps, WTU, ldo, ws, ws_bytes, stream);
    }
    const int kt = kt_of(k);
    REQUIRE(kt > 0 && A && W && H && WTU && ws && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && ldo >= n, "kl_wtu: bad arguments");
    const int kp = 32 * kt;
    const Fac f0{off16(W), ldw, off16(H), ldh, k};
    KlWtuSel sel = select_kl_wtu(m, n, k, kt, off16(A), lda, f0, true, ws_bytes, off16(ws));
    const KlWtuPlan& plan = sel.plan;
    const int nt = plan.nt;
    const TnPlan& p = plan.tn;
    const long rowblks_per_chunk = plan.rowblks_per_chunk;
    const long nchunks = plan.nchunks;
    const size_t pbytes = sel.pbytes, need = sel.need;
    if (sel.ews) return fail(DNMF_EWS, "kl_wtu: workspace %zu < %zu", ws_bytes, need);
    const int k_out = k;                                   // rows of WTU the caller gets
    if (int rc16 = dnmf_kl16_wtu_(A, m, n, lda, W, ldw, H, ldh, k, eps, WTU, ldo, ws, ws_bytes, stream); rc16 != 1) return rc16;
    if (sel.pad && !pad_factors(W, ldw, H, ldh, k, m, n, kp, ws, ws_bytes, need, S(stream)))      // (the copy could not be launched)
        sel = select_kl_wtu(m, n, k, kt, off16(A), lda, f0, false, ws_bytes, off16(ws));
    NnArgs a = nn_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    a.kreal = k_out;
    a.ncolblk = p.ncolblk;
    a.P = (float*)ws; a.ldp = p.ldp; a.chunk_stride = p.ldp * kp;
    const bool fast = sel.fast;
    const dim3 grid(sel.grid), block(256);   // 4 row chunks (waves) per workgroup
    const size_t lds = (size_t)kp * 32 * nt * sizeof(float);                   // the H block of the workgroup's columns
    hipStream_t st = S(stream);
#define WU_CASE(KT_, NT_)                                                                                         \
    if (kt == KT_) {                                                                                              \
        if (fast) DNMF_LAUNCH((kl_wtu_kernel<KT_, NT_, true>), grid, block, lds, st, a, rowblks_per_chunk); \
        else DNMF_LAUNCH((kl_wtu_kernel<KT_, NT_, false>), grid, block, lds, st, a, rowblks_per_chunk);    \
    }
    WU_CASE(1, 4) WU_CASE(2, 2) WU_CASE(4, 2)
#undef WU_CASE
    int rc = check_launch("kl_wtu");
    if (rc) return rc;
    return launch_reduce((const float*)ws, reduce_shape_kl_wtu(plan, kp, k_out, n), WTU, ldo, (float*)((char*)ws + pbytes), st);
}

}  // extern "C"

// =============================================================================================== the launch-plan query (this file's entry points)
// Library-internal: dnmf_dense_plan (csrc/dnmf.hip) forwards the KL products, the residual and the per-column error here, and
// dnmf_dense_plan_variants appends this file's variants.  ld / off: pitches and addresses modulo 16 of {A, W, H, out}, resolved.
__attribute__((visibility("hidden"))) int dnmf_dense_plan_kl_(int op, int bf16a, long m, long n, int k, const long* ld, const unsigned* off,
                                                              size_t ws_bytes, long* out);
__attribute__((visibility("hidden"))) int dnmf_dense_variants_kl_(long* rows, int cap, int nrows);
// csrc/dnmf_kl16.hip: the 16-wide kernels' part (1 = the 16-wide kernel does not apply: the 32-wide selectors answer)
__attribute__((visibility("hidden"))) int dnmf_kl16_plan_(int uht, long m, long n, int k, const long* ld, const unsigned* off, long hblk,
                                                          size_t ws_bytes, long* out);
__attribute__((visibility("hidden"))) int dnmf_kl16_variants_(long* rows, int cap, int nrows);

namespace {
void report_reduce_kl(long* out, const ReduceSel& r) {
    out[DNMF_DENSE_PLAN_REDUCE] = r.kind;
    out[DNMF_DENSE_PLAN_SLICES] = r.kind == REDUCE_TWO_STAGE ? r.ny : 0;
}
}  // namespace

int dnmf_dense_plan_kl_(int op, int bf16a, long m, long n, int k, const long* ld, const unsigned* off, size_t ws_bytes, long* out) {
    const int kt = kt_of(k), kp = 32 * kt;
    const size_t ea = bf16a ? 2 : 4;
    const Fac f{off[1], ld[1], off[2], ld[2], k};
    switch (op) {
    case DNMF_DENSE_OP_KL_UHT: case DNMF_DENSE_OP_KL_UHT_HBLOCKS: {
        REQUIRE(!bf16a, "dense_plan: the KL products take float32 data");
        const long hblk = op == DNMF_DENSE_OP_KL_UHT_HBLOCKS ? ld[2] : 0;
        REQUIRE(!hblk || (n % hblk == 0 && hblk % BK == 0), "dense_plan: bad H layout (block %ld, n %ld)", hblk, n);
        if (int rc16 = dnmf_kl16_plan_(1, m, n, k, ld, off, hblk, ws_bytes, out); rc16 != 1) return rc16;
        const KlUhtSel s = select_kl_uht(m, n, k, kt, off[0], ld[0], f, hblk, off[3], ld[3], true, ws_bytes);
        if (s.ews) break;
        out[DNMF_DENSE_PLAN_FAMILY] = s.pipe ? DNMF_DENSE_FAM_KL_UHT_PIPE : DNMF_DENSE_FAM_KL_UHT;
        out[DNMF_DENSE_PLAN_KT] = kt; out[DNMF_DENSE_PLAN_FAST] = s.fast; out[DNMF_DENSE_PLAN_MODE] = s.pad;
        out[DNMF_DENSE_PLAN_EDGE] = s.pipe && s.rest > 0;              // kl_uht_kernel follows for the ragged last row tile
        out[DNMF_DENSE_PLAN_GRID_X] = s.pipe ? s.rowtile0 : s.rest; out[DNMF_DENSE_PLAN_GRID_Y] = s.u.nsplit; out[DNMF_DENSE_PLAN_BLOCK] = 256;
        out[DNMF_DENSE_PLAN_COUNT] = s.u.nsplit; out[DNMF_DENSE_PLAN_PER] = s.u.cols_per_split;
        out[DNMF_DENSE_PLAN_NK] = cdiv(std::min<long>(s.u.cols_per_split, n), BK);
        out[DNMF_DENSE_PLAN_AUX] = s.rest;
        if (s.u.nsplit > 1) report_reduce_kl(out, select_reduce(reduce_shape_kl_uht(m, kp, s.u.nsplit, k), 0, off[3], ld[3]));
        break;
    }
    case DNMF_DENSE_OP_KL_WTU: {
        REQUIRE(!bf16a, "dense_plan: the KL products take float32 data");
        {
            const KlWtuSel s0 = select_kl_wtu(m, n, k, kt, off[0], ld[0], f, true, ws_bytes);
            if (s0.ews) break;                                          // (the entry point refuses before it tries the 16-wide kernel)
        }
        if (int rc16 = dnmf_kl16_plan_(0, m, n, k, ld, off, 0, ws_bytes, out); rc16 != 1) return rc16;
        const KlWtuSel s = select_kl_wtu(m, n, k, kt, off[0], ld[0], f, true, ws_bytes);
        if (s.ews) break;
        out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_KL_WTU;
        out[DNMF_DENSE_PLAN_KT] = kt; out[DNMF_DENSE_PLAN_FAST] = s.fast; out[DNMF_DENSE_PLAN_MODE] = s.pad; out[DNMF_DENSE_PLAN_NT] = s.plan.nt;
        out[DNMF_DENSE_PLAN_GRID_X] = s.grid; out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 256;
        out[DNMF_DENSE_PLAN_COUNT] = s.plan.nchunks; out[DNMF_DENSE_PLAN_PER] = 32 * s.plan.rowblks_per_chunk;
        const long rows_last = m - (s.plan.nchunks - 1) * 32 * s.plan.rowblks_per_chunk;
        out[DNMF_DENSE_PLAN_B0_FULL] = std::min(m, 32 * s.plan.rowblks_per_chunk) / 32; out[DNMF_DENSE_PLAN_B0_TAIL] = std::min(m, 32 * s.plan.rowblks_per_chunk) % 32;
        out[DNMF_DENSE_PLAN_BL_FULL] = rows_last / 32; out[DNMF_DENSE_PLAN_BL_TAIL] = rows_last % 32;
        report_reduce_kl(out, select_reduce(reduce_shape_kl_wtu(s.plan, kp, k, n), 0, off[3], ld[3]));
        break;
    }
    case DNMF_DENSE_OP_RESID_SQNORM: {
        const ResidSel s = select_resid(m, n, kt, ea, off[0], ld[0], f, ws_bytes > 0, ws_bytes);
        out[DNMF_DENSE_PLAN_FAMILY] = s.lds ? DNMF_DENSE_FAM_RESID_LDS : DNMF_DENSE_FAM_RESID;
        out[DNMF_DENSE_PLAN_KT] = kt; out[DNMF_DENSE_PLAN_FAST] = s.fast; out[DNMF_DENSE_PLAN_MODE] = s.pad;
        out[DNMF_DENSE_PLAN_GRID_X] = s.grid; out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 256;
        out[DNMF_DENSE_PLAN_COUNT] = s.nchunks; out[DNMF_DENSE_PLAN_PER] = 32 * s.rpc;
        break;
    }
    case DNMF_DENSE_OP_COLUMN_ERR: {
        const ColerrSel s = select_colerr(m, n, ea, off[0], ld[0], f);
        out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_COLERR;
        out[DNMF_DENSE_PLAN_KT] = kt; out[DNMF_DENSE_PLAN_FAST] = s.fast;
        out[DNMF_DENSE_PLAN_GRID_X] = s.grid; out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 256;
        out[DNMF_DENSE_PLAN_COUNT] = s.nchunks; out[DNMF_DENSE_PLAN_PER] = 32 * s.rpc;
        break;
    }
    default: return fail(DNMF_EINVAL, "dense_plan: unknown op %d", op);
    }
    return DNMF_OK;
}

// this file's variants, each from its selector called over its discrete input domain (rows as dnmf_dense_plan_variants writes them)
int dnmf_dense_variants_kl_(long* rows, int cap, int nrows) {
    auto emit = [&](long fam, long kt, long fast, long mode, long nt, long edge, long b16) {
        const long r[DNMF_DENSE_VARIANT_LEN] = {fam, kt, fast, mode, 0, nt, 0, edge, 0, b16};
        if (rows && nrows < cap) for (int i = 0; i < DNMF_DENSE_VARIANT_LEN; ++i) rows[(long)nrows * DNMF_DENSE_VARIANT_LEN + i] = r[i];
        ++nrows;
    };
    for (int kt : {1, 2, 4}) {
        const int kp = 32 * kt;
        for (unsigned o : {0u, 4u})
            for (int k : {kp, kp - 4})
                for (size_t wsb : {(size_t)0, ~(size_t)0 >> 1}) {                          // without and with room for the padded images
                    const Fac f{o, kp + 4, o, 516, k};
                    for (long m : {4224L, 4196L, 100L}) {                                  // whole row tiles, a ragged one, below one tile
                        const KlUhtSel u = select_kl_uht(m, 512, k, kt, o, 516, f, 0, o, kp + 4, true, wsb);
                        if (!u.ews) emit(u.pipe ? DNMF_DENSE_FAM_KL_UHT_PIPE : DNMF_DENSE_FAM_KL_UHT, kt, u.fast, u.pad, 0, u.pipe && u.rest > 0, 0);
                        const KlWtuSel w = select_kl_wtu(m, 512, k, kt, o, 516, f, true, wsb);
                        if (!w.ews) emit(DNMF_DENSE_FAM_KL_WTU, kt, w.fast, w.pad, w.plan.nt, 0, 0);
                        for (size_t ea : {(size_t)4, (size_t)2}) {
                            const ResidSel r = select_resid(m, 512, kt, ea, o, 520, f, wsb > 0, wsb);
                            emit(r.lds ? DNMF_DENSE_FAM_RESID_LDS : DNMF_DENSE_FAM_RESID, kt, r.fast, r.pad, 0, 0, ea == 2);
                            const ColerrSel c = select_colerr(m, 512, ea, o, 520, f);
                            emit(DNMF_DENSE_FAM_COLERR, kt, c.fast, 0, 0, 0, ea == 2);
                        }
                    }
                }
    }
    return dnmf_kl16_variants_(rows, cap, nrows);
}
