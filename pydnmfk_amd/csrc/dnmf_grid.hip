// dnmf_grid.hip -- whole steps of a rank of a 1D or 2D grid, sequenced INSIDE the library: kernels -> collective -> kernels on the
// caller's stream with no host code in between (pydnmfk_amd/dist_nmf.py is the choreography they mirror).  MU / Frobenius, MU / KL
// and HALS / Frobenius, each on 1D grids (dnmf_*_step_1d) and on 2D grids (dnmf_*_step_2d); the Frobenius steps also with
// bf16-stored A.  The collectives are the communicator's (csrc/dnmf_comm.h).  A host that is not PyTorch (the reference's mpi4py
// driver) gets the packed single allreduce and the overlapped H phase through these entry points; the PyTorch
// host can use them instead of torch.distributed (params.exchange = 'native').
#include "dnmf_comm.h"
#include "dnmf_host.h"

namespace {

// the entry points that touch A, for fp32 and for bf16-stored A (params.precision = 'bfloat16': Frobenius mu / hals)
template <typename TA> struct AOps;
template <> struct AOps<float> {
    static constexpr bool f32 = true;
    static int aht(const float* A, long m, long n, long lda, const float* H, int k, long ldh, float* o, long ldo, void* s) { return dnmf_aht(A, m, n, lda, H, k, ldh, o, ldo, s); }
    static int wta(const float* A, long m, long n, long lda, const float* W, int k, long ldw, float* o, long ldo, void* ws, size_t wb, void* s) { return dnmf_wta(A, m, n, lda, W, k, ldw, o, ldo, ws, wb, s); }
    static int wta_gram(const float* A, long m, long n, long lda, const float* W, int k, long ldw, float* o, long ldo, float* G, void* ws, size_t wb, void* s) { return dnmf_wta_gram(A, m, n, lda, W, k, ldw, o, ldo, G, ws, wb, s); }
    static int ahtw(const float* A, long m, long n, long lda, const float* H, int k, long ldh, const float* G, float* W, long ldw, float eps, void* s) { return dnmf_aht_update_w(A, m, n, lda, H, k, ldh, G, W, ldw, eps, s); }
};
template <> struct AOps<bf16_t> {
    static constexpr bool f32 = false;
    static int aht(const bf16_t* A, long m, long n, long lda, const float* H, int k, long ldh, float* o, long ldo, void* s) { return dnmf_aht_bf16a(A, m, n, lda, H, k, ldh, o, ldo, s); }
    static int wta(const bf16_t* A, long m, long n, long lda, const float* W, int k, long ldw, float* o, long ldo, void* ws, size_t wb, void* s) { return dnmf_wta_bf16a(A, m, n, lda, W, k, ldw, o, ldo, ws, wb, s); }
    static int wta_gram(const bf16_t* A, long m, long n, long lda, const float* W, int k, long ldw, float* o, long ldo, float* G, void* ws, size_t wb, void* s) { return dnmf_wta_gram_bf16a(A, m, n, lda, W, k, ldw, o, ldo, G, ws, wb, s); }
    static int ahtw(const bf16_t* A, long m, long n, long lda, const float* H, int k, long ldh, const float* G, float* W, long ldw, float eps, void* s) { return dnmf_aht_update_w_bf16a(A, m, n, lda, H, k, ldh, G, W, ldw, eps, s); }
};

// ================================================================================================ 1D grids
// workspace of the 1D steps: [kernel scratch of dnmf_ws_bytes | G (KP x KP) | packed exchange buffer | k doubles: HALS norms]
struct Ws1d { size_t g_off, x_off, ss2_off, total; };
Ws1d ws1d_layout(long m_l, long n_l, int k) {
    const int kp = 32 * kt_of(k);
    Ws1d w;
    size_t kws = std::max(dnmf_ws_bytes(m_l, n_l, k), dnmf_ws_bytes(m_l, k, k));   // kernel scratch: the whole block (and the HALS sweep's), every chunk width of the
    for (int nch = 2; nch <= MAX_CHUNKS; ++nch) {                 // overlapped H phase (the chunking of W^T A depends on the width)
        const long cw = (cdiv(n_l, nch) + 63) / 64 * 64;
        if (cw >= n_l) continue;
        kws = std::max(kws, dnmf_ws_bytes(m_l, cw, k));
        if (n_l % cw) kws = std::max(kws, dnmf_ws_bytes(m_l, n_l % cw, k));
    }
    w.g_off = align256(kws);
    w.x_off = w.g_off + align256((size_t)kp * kp * sizeof(float));
    const size_t big = std::max((size_t)k * n_l, (size_t)m_l * k);
    // one packed message [product | pad | KP x KP] or up to MAX_CHUNKS chunk messages, each padded to 64 floats; the norms behind them
    w.ss2_off = w.x_off + (pad64(big) + (size_t)MAX_CHUNKS * 64 + (size_t)kp * kp + 128) * sizeof(float);
    w.total = align256(w.ss2_off + DNMF_MAX_K * sizeof(double));
    return w;
}

// What the 1D steps share: the argument checks, the carved workspace, which phase exchanges, the packed message.
struct Step1d {
    dnmf_comm* c; hipStream_t st; int kp; size_t kws; float *G, *X; double* ss2;   // kernel scratch: [0, kws) of the workspace

    int init(const char* what, const void* A, long m_l, long n_l, const float* W, const float* H, int k, void* ws, size_t ws_bytes,
             dnmf_comm* comm, void* stream) {
        REQUIRE_WS16(ws, what);
        const int kt = kt_of(k);
        REQUIRE(kt > 0 && A && W && H && ws && comm && m_l >= 1 && n_l >= 1, "%s: bad arguments", what);
        REQUIRE(comm->p_r == 1 || comm->p_c == 1, "%s: a %d x %d grid is 2D", what, comm->p_r, comm->p_c);
        const Ws1d L = ws1d_layout(m_l, n_l, k);
        if (ws_bytes < L.total) return fail(DNMF_EWS, "%s: workspace %zu < %zu", what, ws_bytes, L.total);
        char* base = (char*)ws;
        c = comm; st = S(stream); kp = 32 * kt; kws = L.g_off;
        G = (float*)(base + L.g_off); X = (float*)(base + L.x_off); ss2 = (double*)(base + L.ss2_off);
        return DNMF_OK;
    }
    // which axis exchanges: the W phase when W is replicated, the H phase when H is (always: a 1 x 1 grid acts as a row grid)
    bool w_exchanges() const { return c->p_c != 1; }
    bool h_exchanges() const { return c->p_r != 1 || c->always; }
    // [big | pad to 64 floats | small] at the head of the exchange buffer: ONE message of `count` floats
    struct Packed { float *big, *small; size_t count; };
    Packed packed(size_t big, size_t small) const { return Packed{X, X + pad64(big), pad64(big) + small}; }
};

// One MU / Frobenius step of a rank of a 1D grid (dist_nmf.py:716-771 with the exchanges of :681,:707).  p_c == 1: A and W
// are row blocks, H is replicated -- the W phase is the fused local kernel, the H phase ONE allreduce of the packed
// [W^T A (k x n_l) | pad | W^T W (KP x KP)] message (or `overlap_chunks` column chunks: W^T A of chunk c+1 is computed on
// the caller's stream while chunk c is reduced on the communicator's stream; chunk 0 carries W^T W).  p_r == 1: the mirror
// image (A and H column blocks, W replicated, [A H^T | H H^T] reduced).
template <typename TA>
int mu_fro_step_1d_impl(const TA* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k,
                        float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    Step1d s;
    int rc;
    if ((rc = s.init("mu_fro_step_1d", A, m_l, n_l, W, H, k, ws, ws_bytes, c, stream))) return rc;
    const size_t kws = s.kws, gram = (size_t)s.kp * s.kp;
    hipStream_t st = s.st;
    if (w_update) {                                               // Fro_MU_update_W :716-732
        if (!s.w_exchanges()) {
            if ((rc = dnmf_gram_hht(H, k, n_l, ldh, s.G, ws, kws, stream))) return rc;
            if ((rc = AOps<TA>::ahtw(A, m_l, n_l, lda, H, k, ldh, s.G, W, ldw, eps, stream))) return rc;
        } else {
            const Step1d::Packed p = s.packed((size_t)m_l * k, gram);          // [A H^T | H H^T]
            if ((rc = dnmf_gram_hht(H, k, n_l, ldh, p.small, ws, kws, stream))) return rc;
            if ((rc = AOps<TA>::aht(A, m_l, n_l, lda, H, k, ldh, p.big, k, stream))) return rc;
            if ((rc = dnmf_allreduce_f32_(c, G_WORLD, p.big, p.count, st))) return rc;
            if ((rc = dnmf_mu_update_w(W, m_l, k, ldw, p.big, k, p.small, eps, stream))) return rc;
        }
    }
    int nch = (c->p_c == 1 && s.h_exchanges()) ? c->overlap_chunks : 1;       // Fro_MU_update_H :736-751
    if (nch > 1 && n_l / 64 < nch) nch = (int)std::max<long>(1, n_l / 64);
    if (nch <= 1) {
        const Step1d::Packed p = s.packed((size_t)k * n_l, gram);              // [W^T A | W^T W]
        if ((rc = AOps<TA>::wta_gram(A, m_l, n_l, lda, W, k, ldw, p.big, n_l, p.small, ws, kws, stream))) return rc;
        if (s.h_exchanges() && (rc = dnmf_allreduce_f32_(c, G_WORLD, p.big, p.count, st))) return rc;
        if ((rc = dnmf_mu_update_h(H, k, n_l, ldh, p.big, n_l, p.small, eps, clamp, stream))) return rc;
    } else {
        const long cw = (cdiv(n_l, nch) + 63) / 64 * 64;          // chunk width: ceil(n_l / nch) rounded up to 64 columns
        const Step1d::Packed p0 = s.packed((size_t)k * std::min(cw, n_l), gram);   // chunk 0: [W^T A chunk | W^T W] in one message
        if ((rc = dnmf_gram_wtw(W, m_l, k, ldw, p0.small, ws, kws, stream))) return rc;
        size_t off = 0;
        float* chunk_ptr[MAX_CHUNKS]; long c0s[MAX_CHUNKS], c1s[MAX_CHUNKS];
        int nq = 0;
        for (long c0 = 0; c0 < n_l; c0 += cw, ++nq) {             // the later chunks: messages of their own behind it
            const long c1 = std::min(n_l, c0 + cw);
            const size_t span = nq == 0 ? p0.count : pad64((size_t)k * (c1 - c0));
            float* AtW = s.X + off;
            if ((rc = AOps<TA>::wta(A + c0, m_l, c1 - c0, lda, W, k, ldw, AtW, c1 - c0, ws, kws, stream))) return rc;
            HIP_OK(hipEventRecord(c->ready[nq], st), "mu_fro_step_1d: event record");
            HIP_OK(hipStreamWaitEvent(c->xstream, c->ready[nq], 0), "mu_fro_step_1d: stream wait");
            if ((rc = dnmf_allreduce_f32_(c, G_WORLD, AtW, span, c->xstream))) return rc;
            HIP_OK(hipEventRecord(c->done[nq], c->xstream), "mu_fro_step_1d: event record");
            chunk_ptr[nq] = AtW; c0s[nq] = c0; c1s[nq] = c1;
            off += span;
        }
        for (int q = 0; q < nq; ++q) {
            HIP_OK(hipStreamWaitEvent(st, c->done[q], 0), "mu_fro_step_1d: stream wait");
            if ((rc = dnmf_mu_update_h(H + c0s[q], k, c1s[q] - c0s[q], ldh, chunk_ptr[q], c1s[q] - c0s[q], p0.small, eps, clamp, stream))) return rc;
        }
    }
    if (clamp) return dnmf_clamp_min(W, m_l, k, ldw, eps, stream);
    return DNMF_OK;
}

// One MU / KL step of a rank of a 1D grid (dist_nmf.py:813-869; exchanges :797,:707): [U H^T | rowsum(H)] is reduced when
// W is replicated (p_r == 1), [W^T U | colsum(W)] when H is (p_c == 1).
int mu_kl_step_1d_impl(const float* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k,
                       float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    Step1d s;
    int rc;
    if ((rc = s.init("mu_kl_step_1d", A, m_l, n_l, W, H, k, ws, ws_bytes, c, stream))) return rc;
    const size_t kws = s.kws;
    if (w_update) {                                               // KL_MU_update_W :813-830
        const Step1d::Packed p = s.packed((size_t)m_l * k, (size_t)k);         // [U H^T | rowsum(H)]
        if ((rc = dnmf_rowsum(H, k, n_l, ldh, p.small, stream))) return rc;
        if ((rc = dnmf_kl_uht(A, m_l, n_l, lda, W, ldw, H, ldh, k, eps, p.big, k, ws, kws, stream))) return rc;
        if (s.w_exchanges() && (rc = dnmf_allreduce_f32_(c, G_WORLD, p.big, p.count, s.st))) return rc;
        if ((rc = dnmf_kl_update_w(W, m_l, k, ldw, p.big, k, p.small, eps, stream))) return rc;
    }
    const Step1d::Packed p = s.packed((size_t)k * n_l, (size_t)k);             // KL_MU_update_H :832-849: [W^T U | colsum(W)]
    if ((rc = dnmf_colsum(W, m_l, k, ldw, p.small, ws, kws, stream))) return rc;
    if ((rc = dnmf_kl_wtu(A, m_l, n_l, lda, W, ldw, H, ldh, k, eps, p.big, n_l, ws, kws, stream))) return rc;
    if (s.h_exchanges() && (rc = dnmf_allreduce_f32_(c, G_WORLD, p.big, p.count, s.st))) return rc;
    if ((rc = dnmf_kl_update_h(H, k, n_l, ldh, p.big, n_l, p.small, eps, clamp, stream))) return rc;
    if (clamp) return dnmf_clamp_min(W, m_l, k, ldw, eps, stream);
    return DNMF_OK;
}

// One HALS / Frobenius step of a rank of a 1D grid (FRO_HALS_update, dist_nmf.py:873-934): products and Gram matrices as in the
// MU step (one packed allreduce per phase along the split axis), the W sweep column by column -- with row-sharded W (p_r > 1)
// the 8-byte sum of squares of every column is allreduced between the column kernels (utils.py:388-391), with local norms
// (p_r == 1) it is the persistent sweep, or k column launches when `column_sweep` != 0 -- then the H sweep.  `clamp`:
// H = max(H, eps), W = max(W, eps) afterwards (pyDNMF.py:170-172).
template <typename TA>
int hals_fro_step_1d_impl(const TA* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k,
                          float eps, int w_update, int clamp, int column_sweep, void* ws, size_t ws_bytes, dnmf_comm_t* c,
                          void* stream) {
    Step1d s;
    int rc;
    if ((rc = s.init("hals_fro_step_1d", A, m_l, n_l, W, H, k, ws, ws_bytes, c, stream))) return rc;
    const size_t kws = s.kws, gram = (size_t)s.kp * s.kp;
    if (w_update) {                                               // FRO_HALS_update_W :873-891
        const Step1d::Packed p = s.packed((size_t)m_l * k, gram);              // [A H^T | H H^T]
        if ((rc = dnmf_gram_hht(H, k, n_l, ldh, p.small, ws, kws, stream))) return rc;                 // :882
        if ((rc = AOps<TA>::aht(A, m_l, n_l, lda, H, k, ldh, p.big, k, stream))) return rc;            // :883
        if (s.w_exchanges() && (rc = dnmf_allreduce_f32_(c, G_WORLD, p.big, p.count, s.st))) return rc;
        // :884-891.  W's rows are spread over the ranks exactly when the H phase exchanges
        if (s.h_exchanges()) rc = dnmf_hals_sweep_exchanged_(c, W, m_l, k, ldw, p.big, k, p.small, eps, s.ss2, ws, kws, stream, column_sweep);
        else rc = dnmf_hals_sweep_local_(W, m_l, k, ldw, p.big, k, p.small, eps, column_sweep, s.ss2, ws, kws, stream);
        if (rc) return rc;
    }
    const Step1d::Packed p = s.packed((size_t)k * n_l, gram);                  // FRO_HALS_update_H :893-909: [W^T A | W^T W]
    if ((rc = AOps<TA>::wta_gram(A, m_l, n_l, lda, W, k, ldw, p.big, n_l, p.small, ws, kws, stream))) return rc;   // :902-903
    if (s.h_exchanges() && (rc = dnmf_allreduce_f32_(c, G_WORLD, p.big, p.count, s.st))) return rc;
    if ((rc = dnmf_hals_update_h(H, k, n_l, ldh, p.big, n_l, p.small, eps, stream))) return rc;        // :905-909
    if (clamp) {
        if ((rc = dnmf_clamp_min(H, k, n_l, ldh, eps, stream))) return rc;
        return dnmf_clamp_min(W, m_l, k, ldw, eps, stream);
    }
    return DNMF_OK;
}

// ================================================================================================ 2D grids
// slices of a block over the members of a sub-communicator follow the reference's partition rule (utils.py:36-41): the first
// total % p members hold one item more
struct Split {
    int p; long base, rem;
    long count(int q) const { return base + (q < rem ? 1 : 0); }
    long start(int q) const { return (long)q * base + std::min<long>(q, rem); }
    long maxc() const { return base + (rem > 0 ? 1 : 0); }
    bool equal() const { return rem == 0; }
};
inline Split split_of(long total, int p) { return Split{p, total / p, total % p}; }

// workspace of the 2D steps: kernel scratch | G | the exchange buffers (sized for the padded, ragged form) | sums | HALS norms
struct Ws2d { size_t g_off, hs_off, hj_off, v_off, vp_off, sw_off, wp_off, wg_off, wi_off, y_off, yb_off, sh_off, x_off, ss2_off, total; };
Ws2d ws2d_layout(long m_l, long n_l, int k, int p_r, int p_c) {
    const int kp = 32 * kt_of(k);
    const Split ws = split_of(m_l, p_c), hs = split_of(n_l, p_r);
    const long mw = ws.maxc(), nh = hs.maxc();
    size_t kws = std::max(dnmf_ws_bytes(m_l, n_l, k), dnmf_ws_bytes(m_l, std::max<long>(1, hs.base), k));
    kws = std::max(kws, dnmf_ws_bytes(ws.maxc(), k, k));            // (the HALS W sweep on the rank's slice)
    if (hs.equal() && hs.base % 32 == 0) kws = std::max(kws, dnmf_ws_bytes_hblocks(m_l, n_l, k, hs.base));
    Ws2d w;
    size_t o = align256(kws);
    auto take = [&](size_t floats) { const size_t at = o; o += align256(floats * sizeof(float)); return at; };
    w.g_off = take((size_t)kp * kp);
    w.hs_off = take((size_t)p_r * k * nh + (size_t)k * nh);     // gathered H slices [p_r][k nh] (+ this rank's padded send block)
    w.hj_off = take((size_t)k * n_l);                           // H_j assembled (ragged / narrow slices)
    w.v_off = take((size_t)m_l * k);                            // A H^T or U H^T of the block
    w.vp_off = take((size_t)p_c * mw * k);                      // ... laid out at the pitch of the largest W slice
    w.sw_off = take((size_t)mw * k);                            // this rank's slice of the reduced product
    w.wp_off = take((size_t)mw * k);                            // this rank's W slice, padded
    w.wg_off = take((size_t)p_c * mw * k);                      // gathered W slices
    w.wi_off = take((size_t)m_l * k);                           // W_i assembled
    w.y_off = take((size_t)k * n_l);                            // full-width H-phase product
    w.yb_off = take((size_t)p_r * k * nh);                      // ... as member blocks
    w.sh_off = take((size_t)k * nh);
    w.x_off = take(128);                                        // factor sums (KL)
    w.ss2_off = take(2 * DNMF_MAX_K);                           // k doubles: the HALS norms
    w.total = o;
    return w;
}

int check_2d(const char* what, const dnmf_comm* c, long m_l, long n_l, long m_w, long n_h, long ldw, long ldh, int k) {
    if (c->p_r * c->p_c != c->nranks) return fail(DNMF_EINVAL, "%s: communicator grid %d x %d", what, c->p_r, c->p_c);
    const int i = c->rank / c->p_c, j = c->rank % c->p_c;
    const Split ws = split_of(m_l, c->p_c), hs = split_of(n_l, c->p_r);
    if (m_l < c->p_c || n_l < c->p_r || m_w != ws.count(j) || n_h != hs.count(i) || ldw != k || ldh != n_h)
        return fail(DNMF_EINVAL, "%s: factor slices off the partition rule or strided (A %ld x %ld on %d x %d at (%d, %d): W slice %ld x %d "
                    "ld %ld, expected %ld rows; H slice %d x %ld ld %ld, expected %ld columns): use the host choreography",
                    what, m_l, n_l, c->p_r, c->p_c, i, j, m_w, k, ldw, ws.count(j), k, n_h, ldh, hs.count(i));
    return DNMF_OK;
}

#define COPY2D(dst, dpitch, src, spitch, width, height, what)                                                                   \
    HIP_OK(hipMemcpy2DAsync((dst), (size_t)(dpitch) * sizeof(float), (src), (size_t)(spitch) * sizeof(float),                   \
                            (size_t)(width) * sizeof(float), (size_t)(height), hipMemcpyDeviceToDevice, st), what)
#define COPY1D(dst, src, count, what) \
    HIP_OK(hipMemcpyAsync((dst), (src), (size_t)(count) * sizeof(float), hipMemcpyDeviceToDevice, st), what)

// The exchanges and the two products of a 2D step, shared by the Frobenius and the KL form.  How H_j reaches the kernels mirrors
// gather_H / _product_scattered_to_H of pydnmfk_amd/dist_nmf.py exactly (the same kernels on the same operand shapes: same bits):
//   blocked  equal slices of whole 32-column tiles, p_r > 1: the allgather's receive buffer [p_r][k][n_h] IS the operand
//   else     H_j (k x n_l) is assembled from the (padded) slices
//   sliced   equal slices of whole 16-byte vectors: the H-phase product is formed slice by slice into the reduce-scatter's
//            send buffer; else one full-width product, cut into member blocks at the pitch of the largest slice
struct Grid2d {
    dnmf_comm* c; hipStream_t st; int k, i, j; long m_l, n_l, m_w, n_h; Split ws, hs; bool blocked, sliced;
    char* base; Ws2d L;
    float* at(size_t off) const { return (float*)(base + off); }

    // `f32`: bf16-stored A has no column-block form of A H^T
    int init(const char* what, const void* A, long m_l_, long n_l_, long lda, const float* W, long m_w_, long ldw, const float* H,
             long n_h_, long ldh, int k_, void* wsp, size_t ws_bytes, dnmf_comm* comm, void* stream, bool f32) {
        REQUIRE_WS16(wsp, what);
        REQUIRE(kt_of(k_) > 0 && A && W && H && wsp && comm && m_l_ >= 1 && n_l_ >= 1 && lda >= n_l_, "%s: bad arguments", what);
        if (int rc = check_2d(what, comm, m_l_, n_l_, m_w_, n_h_, ldw, ldh, k_)) return rc;
        c = comm; st = S(stream); k = k_; i = c->rank / c->p_c; j = c->rank % c->p_c;
        m_l = m_l_; n_l = n_l_; m_w = m_w_; n_h = n_h_;
        ws = split_of(m_l, c->p_c); hs = split_of(n_l, c->p_r);
        blocked = f32 && c->p_r > 1 && hs.equal() && n_h % 32 == 0;
        sliced = hs.equal() && n_h % 4 == 0;
        L = ws2d_layout(m_l, n_l, k, c->p_r, c->p_c);
        if (ws_bytes < L.total) return fail(DNMF_EWS, "%s: workspace %zu < %zu", what, ws_bytes, L.total);
        base = (char*)wsp;
        return DNMF_OK;
    }

    // H_j from the row group: returns the operand pointer (*hb = leading dimension, or the block width when blocked)
    int gather_h(const float* H, const float** Hop, long* hb) {
        float* Hs = at(L.hs_off);
        const long nh = hs.maxc();
        int rc;
        if (c->p_r == 1) { *Hop = H; *hb = n_l; return DNMF_OK; }                                        // (one member: its slice is H_j)
        if (hs.equal()) {
            if ((rc = dnmf_allgather_f32_(c, G_ROW, H, Hs, (size_t)k * n_h, st))) return rc;
            if (blocked) { *Hop = Hs; *hb = n_h; return DNMF_OK; }
        } else {                                                                                          // ragged: blocks padded to the largest
            float* mine = Hs + (size_t)c->p_r * k * nh;
            COPY1D(mine, H, (size_t)k * n_h, "gather_h: pad");
            if ((rc = dnmf_allgather_f32_(c, G_ROW, mine, Hs, (size_t)k * nh, st))) return rc;
        }
        float* Hj = at(L.hj_off);
        const size_t pitch = hs.equal() ? (size_t)k * n_h : (size_t)k * nh;
        for (int q = 0; q < c->p_r; ++q)
            COPY2D(Hj + hs.start(q), n_l, Hs + q * pitch, hs.count(q), hs.count(q), k, "gather_h: assemble");
        *Hop = Hj; *hb = n_l;
        return DNMF_OK;
    }
    // W_i (m_l x k) from the column group
    int gather_w(const float* W, const float** Wi_out) {
        int rc;
        if (c->p_c == 1) { *Wi_out = W; return DNMF_OK; }
        float* Wi = at(L.wi_off);
        if (ws.equal()) {
            if ((rc = dnmf_allgather_f32_(c, G_COL, W, Wi, (size_t)m_w * k, st))) return rc;
        } else {
            float *Wp = at(L.wp_off), *Wg = at(L.wg_off);
            const size_t pitch = (size_t)ws.maxc() * k;
            COPY1D(Wp, W, (size_t)m_w * k, "gather_w: pad");
            if ((rc = dnmf_allgather_f32_(c, G_COL, Wp, Wg, pitch, st))) return rc;
            for (int q = 0; q < c->p_c; ++q) COPY1D(Wi + ws.start(q) * k, Wg + q * pitch, (size_t)ws.count(q) * k, "gather_w: assemble");
        }
        *Wi_out = Wi;
        return DNMF_OK;
    }
    // reduce-scatter of V (m_l x k) over the column group -> this rank's m_w x k slice
    int scatter_to_w(const float* V, const float** out) {
        int rc;
        if (c->p_c == 1) { *out = V; return DNMF_OK; }
        float* Sw = at(L.sw_off);
        if (ws.equal()) {
            if ((rc = dnmf_reduce_scatter_f32_(c, G_COL, V, Sw, (size_t)m_w * k, j, st))) return rc;
        } else {
            float* Vp = at(L.vp_off);
            const size_t pitch = (size_t)ws.maxc() * k;
            for (int q = 0; q < c->p_c; ++q) COPY1D(Vp + q * pitch, V + ws.start(q) * k, (size_t)ws.count(q) * k, "scatter_to_w: pad");
            if ((rc = dnmf_reduce_scatter_f32_(c, G_COL, Vp, Sw, pitch, j, st))) return rc;
        }
        *out = Sw;
        return DNMF_OK;
    }
    // reduce-scatter of the H-phase product over the row group -> this rank's k x n_h slice.  sliced: Yb holds the member
    // blocks already; else Y (k x n_l) is cut into blocks at the pitch of the largest slice first.
    int scatter_to_h(const float* Y, const float** out) {
        int rc;
        float *Yb = at(L.yb_off), *Sh = at(L.sh_off);
        if (c->p_r == 1) { *out = sliced ? Yb : Y; return DNMF_OK; }
        size_t pitch = (size_t)k * n_h;
        if (!sliced) {
            pitch = (size_t)k * hs.maxc();
            for (int q = 0; q < c->p_r; ++q)
                COPY2D(Yb + q * pitch, hs.count(q), Y + hs.start(q), n_l, hs.count(q), k, "scatter_to_h: blocks");
        }
        if ((rc = dnmf_reduce_scatter_f32_(c, G_ROW, Yb, Sh, pitch, i, st))) return rc;
        *out = Sh;
        return DNMF_OK;
    }
    // the leading dimension of what scatter_to_h returned
    long h_pitch() const { return (c->p_r == 1 && !sliced) ? n_l : n_h; }

    // V (m_l x k) = A H_j^T, H as gather_h returned it (AH_glob, dist_nmf.py:198)
    template <typename TA> int aht(const TA* A, long lda, const float* Hop, long hb, float* V) const {
        if constexpr (AOps<TA>::f32)
            if (blocked) return dnmf_aht_hblocks(A, m_l, n_l, lda, Hop, hb, k, V, k, st);
        return AOps<TA>::aht(A, m_l, n_l, lda, Hop, k, hb, V, k, st);
    }
    // W_i^T A (ATW_glob :166).  sliced: slice by slice into Yb -- member q's k x n_h block is contiguous; else full width into Y
    template <typename TA> int wta(const TA* A, long lda, const float* Wi, float* Y, float* Yb, void* wsp, size_t kws) const {
        if (!sliced) return AOps<TA>::wta(A, m_l, n_l, lda, Wi, k, k, Y, n_l, wsp, kws, st);
        for (int q = 0; q < c->p_r; ++q)
            if (int rc = AOps<TA>::wta(A + q * n_h, m_l, n_h, lda, Wi, k, k, Yb + (size_t)q * k * n_h, n_h, wsp, kws, st)) return rc;
        return DNMF_OK;
    }
};

// What tells the two Frobenius steps of a 2D grid apart: how each phase ends once its product and Gram matrix are this rank's
struct MuRule {
    static constexpr const char* name = "mu_fro_step_2d";
    static constexpr bool clamps_h = false;                        // (dnmf_mu_update_h clamps)
    static int w_end(const Grid2d& g, float* W, long ldw, const float* AH, const float* G, float eps, void*, size_t) {
        return dnmf_mu_update_w(W, g.m_w, g.k, ldw, AH, g.k, G, eps, g.st);                               // :244-245
    }
    static int h_end(const Grid2d& g, float* H, long ldh, const float* AtW, const float* G, float eps, int clamp) {
        return dnmf_mu_update_h(H, g.k, g.n_h, ldh, AtW, g.h_pitch(), G, eps, clamp, g.st);               // :224-225
    }
};
struct HalsRule {       // the column norms of the W sweep are summed over ALL ranks (every rank holds other rows of W)
    static constexpr const char* name = "hals_fro_step_2d";
    static constexpr bool clamps_h = true;
    static int w_end(const Grid2d& g, float* W, long ldw, const float* AH, const float* G, float eps, void* ws, size_t kws) {
        double* ss2 = reinterpret_cast<double*>(g.base + g.L.ss2_off);
        if (g.c->nranks > 1) return dnmf_hals_sweep_exchanged_(g.c, W, g.m_w, g.k, ldw, AH, g.k, G, eps, ss2, ws, kws, g.st);   // :428-434
        return dnmf_hals_sweep_local_(W, g.m_w, g.k, ldw, AH, g.k, G, eps, 0, ss2, ws, kws, g.st);
    }
    static int h_end(const Grid2d& g, float* H, long ldh, const float* AtW, const float* G, float eps, int) {
        return dnmf_hals_update_h(H, g.k, g.n_h, ldh, AtW, g.h_pitch(), G, eps, g.st);                    // :449-452
    }
};

// One Frobenius step of a rank of a p_r x p_c grid -- MU (nmf_algorithms_2D.update, dist_nmf.py:207-263) or HALS (FRO_HALS_update,
// :411-470), with global_gram :107-117, AH_glob :186-205, ATW_glob :154-172: the rank holds A_ij (m_l x n_l), its slice W_ij
// (m_w x k) of the grid row's W_i and its slice H_ij (k x n_h) of the grid column's H_j.  Row group = the p_r ranks of its grid
// column (they share H_j's columns), column group = the p_c ranks of its grid row (they share W_i's rows).
template <typename TA, typename RULE>
int fro_step_2d_impl(const TA* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh,
                     int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    Grid2d g;
    int rc;
    if ((rc = g.init(RULE::name, A, m_l, n_l, lda, W, m_w, ldw, H, n_h, ldh, k, ws, ws_bytes, c, stream, AOps<TA>::f32))) return rc;
    const int kp = 32 * kt_of(k);
    const size_t kws = g.L.g_off, gram = (size_t)kp * kp;
    float *G = g.at(g.L.g_off), *V = g.at(g.L.v_off), *Y = g.at(g.L.y_off), *Yb = g.at(g.L.yb_off);
    if (w_update) {                                                // Fro_MU_update_W :227-245, FRO_HALS_update_W :411-434
        if ((rc = dnmf_gram_hht(H, k, n_h, ldh, G, ws, kws, stream))) return rc;
        if ((rc = dnmf_allreduce_f32_(c, G_WORLD, G, gram, g.st))) return rc;                             // global_gram :114
        const float *Hop, *AH; long hb;
        if ((rc = g.gather_h(H, &Hop, &hb))) return rc;                                                   // AH_glob :195-197
        if ((rc = g.aht(A, lda, Hop, hb, V))) return rc;                                                  // :198, H as received
        if ((rc = g.scatter_to_w(V, &AH))) return rc;                                                     // :202
        if ((rc = RULE::w_end(g, W, ldw, AH, G, eps, ws, kws))) return rc;
    }
    if ((rc = dnmf_gram_wtw(W, m_w, k, ldw, G, ws, kws, stream))) return rc;                              // Fro_MU_update_H :207-225, FRO_HALS_update_H :436-452
    if ((rc = dnmf_allreduce_f32_(c, G_WORLD, G, gram, g.st))) return rc;
    const float *Wi, *AtW;
    if ((rc = g.gather_w(W, &Wi))) return rc;                                                             // ATW_glob :163-165
    if ((rc = g.wta(A, lda, Wi, Y, Yb, ws, kws))) return rc;                                              // :166
    if ((rc = g.scatter_to_h(Y, &AtW))) return rc;                                                        // :169-171
    if ((rc = RULE::h_end(g, H, ldh, AtW, G, eps, clamp))) return rc;
    if (clamp && RULE::clamps_h && (rc = dnmf_clamp_min(H, k, n_h, ldh, eps, stream))) return rc;
    if (clamp) return dnmf_clamp_min(W, m_w, k, ldw, eps, stream);
    return DNMF_OK;
}

// The same for MU / KL (dist_nmf.py:351-407 with sum_axis :346-349, gather_W_H :268-291, UHT_glob :330-343, WTU_glob :294-318)
int mu_kl_step_2d_impl(const float* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh,
                       int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    Grid2d g;
    int rc;
    if ((rc = g.init("mu_kl_step_2d", A, m_l, n_l, lda, W, m_w, ldw, H, n_h, ldh, k, ws, ws_bytes, c, stream, true))) return rc;
    const size_t kws = g.L.g_off;
    float *V = g.at(g.L.v_off), *Y = g.at(g.L.y_off), *Yb = g.at(g.L.yb_off), *x = g.at(g.L.x_off);
    hipStream_t st = g.st;
    // H_j: gathered once per step (the W phase changes W, not H)
    const float* Hop; long hb;
    if ((rc = g.gather_h(H, &Hop, &hb))) return rc;                                                       // gather_W_H :283-287
    const float* Wi;
    if (w_update) {                                                // KL_MU_update_W :351-369
        if ((rc = dnmf_rowsum(H, k, n_h, ldh, x, stream))) return rc;
        if ((rc = dnmf_allreduce_f32_(c, G_WORLD, x, (size_t)k, st))) return rc;                          // sum_axis :346-349
        if ((rc = g.gather_w(W, &Wi))) return rc;                                                         // :276-280
        if (g.blocked) rc = dnmf_kl_uht_hblocks(A, m_l, n_l, lda, Wi, k, Hop, hb, k, eps, V, k, ws, kws, stream);   // :337-338
        else rc = dnmf_kl_uht(A, m_l, n_l, lda, Wi, k, Hop, hb, k, eps, V, k, ws, kws, stream);
        if (rc) return rc;
        const float* UHT;
        if ((rc = g.scatter_to_w(V, &UHT))) return rc;                                                    // :340
        if ((rc = dnmf_kl_update_w(W, m_w, k, ldw, UHT, k, x, eps, stream))) return rc;                   // :369
    }
    if ((rc = dnmf_colsum(W, m_w, k, ldw, x, ws, kws, stream))) return rc;                                // KL_MU_update_H :371-389
    if ((rc = dnmf_allreduce_f32_(c, G_WORLD, x, (size_t)k, st))) return rc;
    if ((rc = g.gather_w(W, &Wi))) return rc;                                                             // :387
    if (g.sliced && c->p_r > 1) {
        // WTU_glob :311-312.  Round 5: ONE full-width product, then the k x n_l result is cut into the reduce-scatter's member blocks
        // (scatter_to_h) -- p_r sliced launches that wrote the blocks directly cost 4.19 ms against 3.97 + 0.04 ms on the config-4
        // block (each slice pays its own partial slabs and tail; tools/dbg/kl_slices.py).  The product wants H_j as one matrix:
        // assembled from the gathered blocks (k x n_l floats, one copy per member).
        if (g.blocked) {
            float* Hj = g.at(g.L.hj_off);
            for (int q = 0; q < c->p_r; ++q)
                COPY2D(Hj + (size_t)q * n_h, n_l, Hop + (size_t)q * k * n_h, n_h, n_h, k, "mu_kl_step_2d: assemble H_j");
            Hop = Hj; hb = n_l;
        }
        if ((rc = dnmf_kl_wtu(A, m_l, n_l, lda, Wi, k, Hop, hb, k, eps, Y, n_l, ws, kws, stream))) return rc;
        g.sliced = false;                                          // (scatter_to_h cuts Y into the member blocks)
    } else if (g.sliced) {                                         // one member: its "slice" is the whole width, written where the update reads it
        if ((rc = dnmf_kl_wtu(A, m_l, n_h, lda, Wi, k, Hop, g.blocked ? n_h : hb, k, eps, Yb, n_h, ws, kws, stream))) return rc;
    } else if ((rc = dnmf_kl_wtu(A, m_l, n_l, lda, Wi, k, Hop, hb, k, eps, Y, n_l, ws, kws, stream))) return rc;
    const float* WTU;
    if ((rc = g.scatter_to_h(Y, &WTU))) return rc;                                                        // :314-316
    if ((rc = dnmf_kl_update_h(H, k, n_h, ldh, WTU, g.h_pitch(), x, eps, clamp, stream))) return rc;      // :389
    if (clamp) return dnmf_clamp_min(W, m_w, k, ldw, eps, stream);
    return DNMF_OK;
}

}  // namespace

// ================================================================================================ the C ABI (include/dnmf.h)
extern "C" {

size_t dnmf_ws_bytes_1d(long m_l, long n_l, int k) {
    if (kt_of(k) < 0 || m_l < 1 || n_l < 1) return 0;
    return ws1d_layout(m_l, n_l, k).total;
}
size_t dnmf_ws_bytes_2d(long m_l, long n_l, int k, int p_r, int p_c) {
    if (kt_of(k) < 0 || p_r < 1 || p_c < 1 || m_l < p_c || n_l < p_r) return 0;
    return ws2d_layout(m_l, n_l, k, p_r, p_c).total;
}

int dnmf_mu_fro_step_1d(const float* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    return mu_fro_step_1d_impl<float>(A, m_l, n_l, lda, W, ldw, H, ldh, k, eps, w_update, clamp, ws, ws_bytes, c, stream);
}
int dnmf_mu_fro_step_1d_bf16a(const void* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    return mu_fro_step_1d_impl<bf16_t>((const bf16_t*)A, m_l, n_l, lda, W, ldw, H, ldh, k, eps, w_update, clamp, ws, ws_bytes, c, stream);
}
int dnmf_mu_kl_step_1d(const float* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    return mu_kl_step_1d_impl(A, m_l, n_l, lda, W, ldw, H, ldh, k, eps, w_update, clamp, ws, ws_bytes, c, stream);
}
int dnmf_hals_fro_step_1d(const float* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update, int clamp, int column_sweep, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    return hals_fro_step_1d_impl<float>(A, m_l, n_l, lda, W, ldw, H, ldh, k, eps, w_update, clamp, column_sweep, ws, ws_bytes, c, stream);
}
int dnmf_hals_fro_step_1d_bf16a(const void* A, long m_l, long n_l, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update, int clamp, int column_sweep, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    return hals_fro_step_1d_impl<bf16_t>((const bf16_t*)A, m_l, n_l, lda, W, ldw, H, ldh, k, eps, w_update, clamp, column_sweep, ws, ws_bytes, c, stream);
}
int dnmf_mu_fro_step_2d(const float* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh, int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    return fro_step_2d_impl<float, MuRule>(A, m_l, n_l, lda, W, m_w, ldw, H, n_h, ldh, k, eps, w_update, clamp, ws, ws_bytes, c, stream);
}
int dnmf_mu_fro_step_2d_bf16a(const void* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh, int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    return fro_step_2d_impl<bf16_t, MuRule>((const bf16_t*)A, m_l, n_l, lda, W, m_w, ldw, H, n_h, ldh, k, eps, w_update, clamp, ws, ws_bytes, c, stream);
}
int dnmf_mu_kl_step_2d(const float* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh, int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    return mu_kl_step_2d_impl(A, m_l, n_l, lda, W, m_w, ldw, H, n_h, ldh, k, eps, w_update, clamp, ws, ws_bytes, c, stream);
}
int dnmf_hals_fro_step_2d(const float* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh, int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    return fro_step_2d_impl<float, HalsRule>(A, m_l, n_l, lda, W, m_w, ldw, H, n_h, ldh, k, eps, w_update, clamp, ws, ws_bytes, c, stream);
}
int dnmf_hals_fro_step_2d_bf16a(const void* A, long m_l, long n_l, long lda, float* W, long m_w, long ldw, float* H, long n_h, long ldh, int k, float eps, int w_update, int clamp, void* ws, size_t ws_bytes, dnmf_comm_t* c, void* stream) {
    return fro_step_2d_impl<bf16_t, HalsRule>((const bf16_t*)A, m_l, n_l, lda, W, m_w, ldw, H, n_h, ldh, k, eps, w_update, clamp, ws, ws_bytes, c, stream);
}

}  // extern "C"
