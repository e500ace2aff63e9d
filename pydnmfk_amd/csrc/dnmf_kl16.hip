// dnmf_kl16.hip -- launchers of the 16-wide KL kernels (csrc/dnmf_kl16.h).  A translation unit of its own because it is
// compiled with -mllvm -amdgpu-mfma-vgpr-form (pydnmfk_amd/build.py): MFMA accumulators in VGPRs, so that the division
// between the two products reads and writes them in place.  The other units keep hipcc's heuristic (their k = 128 kernels
// need the AGPR half of the register file).
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_kl16.h"

// Library-internal (called from csrc/dnmf_kl.hip).  Return 1 when the 16-wide kernel does not apply (the caller goes on to
// the 32-wide kernels with its arguments untouched), else the launch status.
__attribute__((visibility("hidden"))) int dnmf_kl16_uht_(const float* A, long m, long n, long lda, const float* W, long ldw,
                                                         const float* H, long ldh, long hblk, int k, float eps, float* UHT,
                                                         long ldo, void* ws, size_t ws_bytes, void* stream);
__attribute__((visibility("hidden"))) int dnmf_kl16_wtu_(const float* A, long m, long n, long lda, const float* W, long ldw,
                                                         const float* H, long ldh, int k, float eps, float* WTU, long ldo,
                                                         void* ws, size_t ws_bytes, void* stream);

// Library-internal: this file's part of the launch-plan query (dnmf_dense_plan -> csrc/dnmf_kl.hip -> here) and of the variant list.
// ld / off: pitches and addresses modulo 16 of {A, W, H, out}.  Return 1 when the 16-wide kernel does not apply.
__attribute__((visibility("hidden"))) int dnmf_kl16_plan_(int uht, long m, long n, int k, const long* ld, const unsigned* off, long hblk,
                                                          size_t ws_bytes, long* out);
__attribute__((visibility("hidden"))) int dnmf_kl16_variants_(long* rows, int cap, int nrows);

constexpr long WINDOW = 0x7fffffffL;          // the kernels address a tile / a chunk through one 2 GiB buffer descriptor

namespace {
// ---- selectors: whether the 16-wide kernel applies, whether the factors are first copied into images padded to 16 (pad_factors), the
// splits / chunks and the reduction.  The launchers below launch from these and the query reports them.  off*: addresses modulo 16.
inline bool friendly16(unsigned offw, long ldw, unsigned offh, long ldh, int k) {
    return k == 16 && offw == 0 && ldw % 4 == 0 && offh == 0 && ldh % 4 == 0;
}
inline bool pad16_fits(long m, long n, size_t need16, size_t ws_bytes) { return ws_bytes >= align256(need16) + pad_bytes(m, n, 16); }   // = pad_factors' test

// U H^T.  hblk > 0: H is the stack of n / hblk column blocks [q][k][hblk] (ldh = hblk); taken only with k = 16 and aligned factors
// (other ranks go to the caller's block-aware padding and come back as one matrix).  direct: one split of full rank into an aligned
// output is stored without slabs.  ws_bytes: 0 without a workspace.
struct Kl16UhtSel { bool applies, pad, direct; UhtPlan u; size_t pb16, need16; unsigned gx; };
inline Kl16UhtSel select_kl16_uht(long m, long n, int k, unsigned offa, long lda, unsigned offw, long ldw, unsigned offh, long ldh, long hblk,
                                  unsigned offo, long ldo, size_t ws_bytes) {
    Kl16UhtSel s{};
    if (!(k <= 16 && offa == 0 && lda % 4 == 0 && n % BK == 0 && m <= 0x7fffffffL)) return s;
    const bool friendly = friendly16(offw, ldw, offh, ldh, k);
    if (hblk && !friendly) return s;
    const long ldh_img = friendly ? ldh : round_up(n, 4);
    if (128 * lda * 4 + n * 4 >= WINDOW || 16 * ldh_img * 4 + n * 4 >= WINDOW) return s;
    // column splits: rowtiles x nsplit workgroups, at most ONE resident round (4 workgroups per CU by registers and LDS) --
    // a second, partly filled round would run at a fraction of the memory parallelism (see plan_wtu16)
    const long rowtiles = cdiv(m, 128);
    long ns = std::max<long>(1, 1024 / rowtiles);
    ns = std::min<long>(ns, std::max<long>(1, n / 256));
    s.u.cols_per_split = round_up(cdiv(n, ns), BK);
    s.u.nsplit = (int)cdiv(n, s.u.cols_per_split);
    if (hblk) {                                        // a column split must not straddle a block of H
        const long nb = n / hblk;
        long sp = std::max<long>(1, ns / nb);
        while (sp > 1 && !(hblk % sp == 0 && (hblk / sp) % BK == 0)) --sp;
        s.u.cols_per_split = hblk / sp;
        s.u.nsplit = (int)(nb * sp);
    }
    s.direct = s.u.nsplit == 1 && k == 16 && offo == 0 && ldo % 4 == 0;
    s.pb16 = s.direct ? 0 : (size_t)s.u.nsplit * m * 16 * sizeof(float);
    s.need16 = s.pb16 + reduce_scratch_bytes(s.u.nsplit, (int)m, k);
    if (!s.direct && !(ws_bytes > 0 && ws_bytes >= s.need16)) return s;
    s.pad = !friendly;
    if (s.pad && !pad16_fits(m, n, s.need16, ws_bytes)) return s;
    s.gx = (unsigned)cdiv(m, 128);
    s.applies = true;
    return s;
}

// W^T U: kl_wtu16_kernel on the row chunks of plan_wtu16, then the reduction of the chunk slabs
struct Kl16WtuSel { bool applies, pad; Tn16Plan q; size_t pb16, need16; unsigned gx; };
inline Kl16WtuSel select_kl16_wtu(long m, long n, int k, unsigned offa, long lda, unsigned offw, long ldw, unsigned offh, long ldh,
                                  size_t ws_bytes) {
    Kl16WtuSel s{};
    if (!(k <= 16 && offa == 0 && lda % 4 == 0 && n % 64 == 0)) return s;
    s.q = plan_wtu16(m, n);
    const bool friendly = friendly16(offw, ldw, offh, ldh, k);
    const long ldw_img = friendly ? ldw : 16;
    if ((s.q.rows_per_chunk + 16) * lda * 4 + 1024 >= WINDOW || (s.q.rows_per_chunk + 16) * ldw_img * 4 >= WINDOW) return s;
    s.pb16 = (size_t)s.q.nchunks * 16 * n * sizeof(float);
    s.need16 = s.pb16 + reduce_scratch_bytes(s.q.nchunks, k, n);
    if (!(ws_bytes > 0 && ws_bytes >= s.need16)) return s;
    s.pad = !friendly;
    if (s.pad && !pad16_fits(m, n, s.need16, ws_bytes)) return s;
    s.gx = (unsigned)cdiv((long)s.q.nchunks * s.q.ncolblk, 4);
    s.applies = true;
    return s;
}
// the reductions that follow (launcher and query)
inline ReduceShape reduce_shape_kl16_uht(const Kl16UhtSel& s, long m, int k) { return ReduceShape{m * 16, 16, s.u.nsplit, (int)m, k, (int)m, k}; }
inline ReduceShape reduce_shape_kl16_wtu(const Kl16WtuSel& s, long n, int k) { return ReduceShape{16 * n, n, s.q.nchunks, k, n, k, n}; }
}  // namespace

int dnmf_kl16_uht_(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, long hblk, int k,
                   float eps, float* UHT, long ldo, void* ws, size_t ws_bytes, void* stream) {
    const Kl16UhtSel sel = select_kl16_uht(m, n, k, off16(A), lda, off16(W), ldw, off16(H), ldh, hblk, off16(UHT), ldo, ws ? ws_bytes : 0);
    if (!sel.applies) return 1;
    hipStream_t st = S(stream);
    const UhtPlan& u = sel.u;
    const int k_out = k;
    const bool direct = sel.direct;
    const size_t pb16 = sel.pb16;
    if (sel.pad && !pad_factors(W, ldw, H, ldh, k, m, n, 16, ws, ws_bytes, sel.need16, st)) return 1;
    Kl16Args a{};
    a.A = A; a.lda = lda; a.m = m; a.n = n; a.W = W; a.ldw = ldw; a.H = H; a.ldh = ldh; a.eps = eps;
    a.P = direct ? UHT : (float*)ws; a.ldp = direct ? ldo : 16; a.chunk_stride = direct ? 0 : m * 16;
    a.cols_per_split = u.cols_per_split;
    a.hblk = hblk; a.hextra = hblk ? (long)16 * hblk - hblk : 0;
    DNMF_LAUNCH(kl_uht16_kernel, dim3(sel.gx, (unsigned)u.nsplit), dim3(256), kl_uht16_lds_bytes(), st, a);
    int rc = check_launch("kl_uht16");
    if (rc || direct) return rc;
    return launch_reduce((const float*)ws, reduce_shape_kl16_uht(sel, m, k_out), UHT, ldo, (float*)((char*)ws + pb16), st);
}

int dnmf_kl16_wtu_(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                   float eps, float* WTU, long ldo, void* ws, size_t ws_bytes, void* stream) {
    const Kl16WtuSel sel = select_kl16_wtu(m, n, k, off16(A), lda, off16(W), ldw, off16(H), ldh, ws ? ws_bytes : 0);
    if (!sel.applies) return 1;
    hipStream_t st = S(stream);
    const Tn16Plan& q = sel.q;
    const int k_out = k;
    const size_t pb16 = sel.pb16;
    if (sel.pad && !pad_factors(W, ldw, H, ldh, k, m, n, 16, ws, ws_bytes, sel.need16, st)) return 1;
    Kl16Args a{};
    a.A = A; a.lda = lda; a.m = m; a.n = n; a.W = W; a.ldw = ldw; a.H = H; a.ldh = ldh; a.eps = eps;
    a.P = (float*)ws; a.ldp = n; a.chunk_stride = 16 * n;
    a.rows_per_chunk = q.rows_per_chunk; a.nchunks = q.nchunks; a.ncolblk = q.ncolblk;
    DNMF_LAUNCH(kl_wtu16_kernel, dim3(sel.gx), dim3(256), 0, st, a);
    int rc = check_launch("kl_wtu16");
    if (rc) return rc;
    return launch_reduce((const float*)ws, reduce_shape_kl16_wtu(sel, n, k_out), WTU, ldo, (float*)((char*)ws + pb16), st);
}

// ---- the launch-plan query of the two entry points above (fields: include/dnmf.h)
int dnmf_kl16_plan_(int uht, long m, long n, int k, const long* ld, const unsigned* off, long hblk, size_t ws_bytes, long* out) {
    if (uht) {
        const Kl16UhtSel s = select_kl16_uht(m, n, k, off[0], ld[0], off[1], ld[1], off[2], ld[2], hblk, off[3], ld[3], ws_bytes);
        if (!s.applies) return 1;
        out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_KL16_UHT;
        out[DNMF_DENSE_PLAN_KT] = 1; out[DNMF_DENSE_PLAN_FAST] = 1; out[DNMF_DENSE_PLAN_MODE] = s.pad; out[DNMF_DENSE_PLAN_EDGE] = s.direct;
        out[DNMF_DENSE_PLAN_GRID_X] = s.gx; out[DNMF_DENSE_PLAN_GRID_Y] = s.u.nsplit; out[DNMF_DENSE_PLAN_BLOCK] = 256;
        out[DNMF_DENSE_PLAN_COUNT] = s.u.nsplit; out[DNMF_DENSE_PLAN_PER] = s.u.cols_per_split;
        out[DNMF_DENSE_PLAN_NK] = cdiv(std::min<long>(s.u.cols_per_split, n), BK);
        out[DNMF_DENSE_PLAN_AUX] = m % 128;                            // rows of the ragged last row tile
        if (!s.direct) {
            const ReduceSel r = select_reduce(reduce_shape_kl16_uht(s, m, k), 0, off[3], ld[3]);
            out[DNMF_DENSE_PLAN_REDUCE] = r.kind; out[DNMF_DENSE_PLAN_SLICES] = r.kind == REDUCE_TWO_STAGE ? r.ny : 0;
        }
        return 0;
    }
    const Kl16WtuSel s = select_kl16_wtu(m, n, k, off[0], ld[0], off[1], ld[1], off[2], ld[2], ws_bytes);
    if (!s.applies) return 1;
    out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_KL16_WTU;
    out[DNMF_DENSE_PLAN_KT] = 1; out[DNMF_DENSE_PLAN_FAST] = 1; out[DNMF_DENSE_PLAN_MODE] = s.pad;
    out[DNMF_DENSE_PLAN_GRID_X] = s.gx; out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 256;
    out[DNMF_DENSE_PLAN_COUNT] = s.q.nchunks; out[DNMF_DENSE_PLAN_PER] = s.q.rows_per_chunk;
    const long r0 = std::min(m, s.q.rows_per_chunk), rl = m - (long)(s.q.nchunks - 1) * s.q.rows_per_chunk;
    out[DNMF_DENSE_PLAN_B0_FULL] = r0 / 16; out[DNMF_DENSE_PLAN_B0_TAIL] = r0 % 16;      // 16-row blocks (two per trip) and the ragged tail
    out[DNMF_DENSE_PLAN_BL_FULL] = rl / 16; out[DNMF_DENSE_PLAN_BL_TAIL] = rl % 16;
    const ReduceSel r = select_reduce(reduce_shape_kl16_wtu(s, n, k), 0, off[3], ld[3]);
    out[DNMF_DENSE_PLAN_REDUCE] = r.kind; out[DNMF_DENSE_PLAN_SLICES] = r.kind == REDUCE_TWO_STAGE ? r.ny : 0;
    return 0;
}

// this file's variants {family, KT, FAST, MODE = padded, PF, NT, V, EDGE = direct store, NTEMP, bf16}: the selectors over friendly and
// ragged factors, one and several splits, an aligned and an unaligned output, without and with a workspace
int dnmf_kl16_variants_(long* rows, int cap, int nrows) {
    auto emit = [&](long fam, long mode, long edge) {
        const long r[DNMF_DENSE_VARIANT_LEN] = {fam, 1, 1, mode, 0, 0, 0, edge, 0, 0};
        if (rows && nrows < cap) for (int i = 0; i < DNMF_DENSE_VARIANT_LEN; ++i) rows[(long)nrows * DNMF_DENSE_VARIANT_LEN + i] = r[i];
        ++nrows;
    };
    for (int k : {16, 12})
        for (unsigned o : {0u, 4u})
            for (size_t wsb : {(size_t)0, ~(size_t)0 >> 1})
                for (long n : {128L, 1024L}) {
                    for (unsigned oo : {0u, 4u}) {                    // the output's own alignment decides the direct store
                        const Kl16UhtSel u = select_kl16_uht(300, n, k, 0, n + 4, o, 20, o, n + 4, 0, oo, 20, wsb);
                        if (u.applies) emit(DNMF_DENSE_FAM_KL16_UHT, u.pad, u.direct);
                    }
                    const Kl16WtuSel w = select_kl16_wtu(300, n, k, 0, n + 4, o, 20, o, n + 4, wsb);
                    if (w.applies) emit(DNMF_DENSE_FAM_KL16_WTU, w.pad, 0);
                }
    return nrows;
}
