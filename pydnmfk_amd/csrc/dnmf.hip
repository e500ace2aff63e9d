// dnmf.hip -- MI355X (gfx950 / CDNA4) kernels + C ABI for the distributed-NMF multiplicative-update path.
//
// Written for gfx950 only: 64-wide wavefronts, fp32-input MFMA (v_mfma_f32_32x32x2_f32, exact fp32 = an
// fmaf chain), 160 KiB LDS per CU, 8 XCDs.  See DESIGN.md for the data layout and per-kernel rooflines and
// include/dnmf.h for the reference lines each entry point replaces.
//
// Two GEMM forms carry the whole path (k = NMF rank, padded to KP = 32*KT):
//   NT form  C[i][j] = sum_c X[i][c] * Y[j][c]   contraction index contiguous in both operands
//            -> A H^T (K2), H H^T (K1), W (H H^T) (K3).  X is streamed through LDS (the MFMA operand
//               layout puts the 32 rows of a tile across lanes, so a transpose is unavoidable).
//   TN form  C[j][c] = sum_i X[i][j] * Y[i][c]   contraction index is the row of both operands
//            -> W^T A (K6), W^T W (K5), (W^T W) H (K7).  Operands go global -> VGPR directly in MFMA
//               layout with 16-byte coalesced loads; no LDS, no barriers.
// MFMA 32x32x2 f32 operand maps (lane l, li = l & 31, h = l >> 5):
//   A-operand: A[i = li][kk = h]   B-operand: B[kk = h][j = li]
//   C/D: col = li, row = (reg & 3) + 8 * (reg >> 2) + 4 * h   (reg in [0,16))
// The contraction order inside a tile and the output row/column order inside a tile are permuted freely
// (sums are order-agnostic up to fp32 rounding; outputs are written to their true addresses).
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_nt.h"
#include "dnmf_tn.h"
#include "dnmf_stream.h"
#include "dnmf_update.h"
#include "dnmf_nn.h"
#include "dnmf_k16.h"

// csrc/dnmf_wide.hip: the k x k products of ranks 128 < k <= 256
#define HID __attribute__((visibility("hidden")))
HID int dnmf_wide_mu_update_w_(float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G, long ldg, float eps, void* stream);
HID int dnmf_wide_mu_update_h_(float* H, int k, long n, long ldh, const float* AtW, long ldatw, const float* G, long ldg, float eps, int clamp,
                               void* stream);
// csrc/dnmf_kl.hip: its part of the launch-plan query
HID int dnmf_dense_plan_kl_(int op, int bf16a, long m, long n, int k, const long* ld, const unsigned* off, size_t ws_bytes, long* out);
HID int dnmf_dense_variants_kl_(long* rows, int cap, int nrows);
// csrc/dnmf_timg.hip: the W phase from a bound transposed image of A (1 = not applicable)
HID int dnmf_wimage_try_(const float* A, long m, long n, long lda, const float* H, int k, long ldh, const float* G, float* W, long ldw, float eps,
                         void* stream);
#undef HID

char* dnmf_errbuf_() {
    static thread_local char buf[DNMF_ERRBUF] = "";
    return buf;
}

BatchCtx* dnmf_batch_() {
    static thread_local BatchCtx ctx = {1, {}};
    return &ctx;
}

namespace {

// ---- selectors: every choice an entry point of this file makes between kernels, template arguments and grids, as a function of the
// shape, the pitches and the operands' addresses modulo 16 (off16).  The launchers below launch from these and dnmf_dense_plan reports
// them, so the query cannot drift from the dispatch.  `ea`: bytes per element of A (4: float, 2: bfloat16).
constexpr int DENSE_BM = 128;                                        // rows of an nt_kernel / nt16_kernel workgroup, every rank
inline unsigned nt_grid_x(long nrows) { return (unsigned)cdiv(nrows, DENSE_BM); }                           // row tiles of the NT kernels
inline unsigned tn_grid(long nchunks, long ncolblk) { return (unsigned)cdiv(nchunks * ncolblk, 4); }         // a wave per (chunk, column block), 4 per workgroup
// 32-bit tile offsets of the updates' buffer accesses: the entry points refuse pitches beyond these
inline bool update_w_pitch_ok(long ldw, long ldah) { return ldw < (1L << 23) && ldah < (1L << 23); }
// (27 + 4) rows of a 32-row block plus the column part stay below 2 GiB
inline bool update_h_pitch_ok(long ldh, long ldatw) { return ldh < (1L << 24) && ldatw < (1L << 24); }
inline bool rows16(unsigned off, long ld, size_t ea) { return off == 0 && (ld * ea) % 16 == 0; }             // = a_rows16
inline bool vec4(unsigned off, long ld, long cols) { return off == 0 && ld % 4 == 0 && cols % 4 == 0; }
// NT form: 16-byte loads from A and H
inline bool nt_fast(unsigned offa, long lda, size_t ea, unsigned offh, long ldh, long n) { return rows16(offa, lda, ea) && vec4(offh, ldh, n); }
inline bool nt16_applies(int k, bool fast, long n, bool b16) { return k <= 16 && fast && n % (b16 ? 64 : 32) == 0; }
// PF code of nt_kernel (launch_nt_inst explains the codes); wgs: workgroups of the launch
inline int nt_pf(bool fast_ks1, int mode, bool store_all, bool f32, long wgs) {
    if (!(fast_ks1 && (mode == NT_FUSED_W || !store_all))) return 1;
    if (!f32) return 5;                                              // bf16 X: one 64-wide tile in flight
    // 13 = 10 with three tiles in flight: chosen when the grid has at most one workgroup per CU (a 32768-row
    // shard = the per-GPU work of the 8-GPU configuration), where a single wave per SIMD has to cover the HBM latency
    return wgs <= 256 ? 13 : 10;
}

// TN form (W^T A): the 16-wide kernel, its riding Gram, or the 32-wide kernel; fam < 0: the workspace is too small
enum { WTA_TN16 = 0, WTA_TN = 1, WTA_EWS = -1 };
struct WtaSel { int fam; bool fast, ride; int nt; Tn16Plan q; TnPlan p; size_t pb, need; };
inline WtaSel select_wta(long m, long n, int k, int kt, size_t ea, unsigned offa, long lda, unsigned offw, long ldw, size_t ws_bytes, bool gram) {
    WtaSel s{};
    const int V = ea == 2 ? 8 : 4;
    if (k <= 16 && rows16(offa, lda, ea) && n % (16 * V) == 0) {     // rank k <= 16: 16-byte aligned rows of A, whole column blocks, workspace permitting
        s.q = plan_tn16(m, n, V);
        s.pb = (size_t)s.q.nchunks * 16 * n * sizeof(float);
        if (s.pb + reduce_scratch_bytes(s.q.nchunks, k, n) <= ws_bytes) {
            const size_t gb = (size_t)s.q.nchunks * 256 * sizeof(float);            // partial Gram tiles behind the slabs
            s.fam = WTA_TN16;
            s.fast = true;
            s.ride = gram && reduce_slices(s.q.nchunks) == 1 && s.pb + gb <= ws_bytes;
            s.need = s.pb + reduce_scratch_bytes(s.q.nchunks, k, n);
            return s;
        }
    }
    s.nt = tn_nt(kt);
    s.p = plan_tn(m, n, kt, s.nt, 256, wta_waves(m, n, kt, ea));
    s.pb = (size_t)s.p.nchunks * s.p.chunk_stride * sizeof(float);
    s.need = s.pb + reduce_scratch_bytes(s.p.nchunks, k, n);
    s.fam = ws_bytes < s.need ? WTA_EWS : WTA_TN;
    // the streamed A is read 4 elements per lane, W only KT per lane (1 float for k <= 32): W's alignment need is KT-wide
    s.fast = offa % (4 * ea) == 0 && lda % 4 == 0 && n % 4 == 0 && offw % (4 * kt) == 0 && ldw % kt == 0 && k % kt == 0;
    return s;
}
// W^T W streams only W (m x k): with 256-row chunks a 32768-row shard gives 128 waves on 32 CUs and the launch is one long
// latency chain; 128-row chunks spread it over the chip (28.8 -> 21.5 us at 32768 rows, 30.2 -> 22.2 us at 65536, k = 64)
// but cost a second reduction stage on tall matrices (34 -> 42 us at 262144 rows), which keep 256.
inline long gram_min_rows(long m) { return m <= 131072 ? 128 : 256; }
struct GramWtwSel { bool fast, ews; int nt; TnPlan p; size_t pb, need; };
inline GramWtwSel select_gram_wtw(long m, int k, int kt, unsigned offw, long ldw, size_t ws_bytes) {
    GramWtwSel s;
    s.nt = kt == 4 ? 2 : kt;        // NT column sets per wave (KT = 4 uses 2 column blocks of 64 to bound registers)
    s.p = plan_tn(m, 32 * kt, kt, s.nt, gram_min_rows(m));
    s.pb = (size_t)s.p.nchunks * s.p.chunk_stride * sizeof(float);
    s.need = s.pb + reduce_scratch_bytes(s.p.nchunks, 32 * kt, 32 * kt);
    s.ews = ws_bytes < s.need;
    s.fast = vec4(offw, ldw, k);
    return s;
}

// the reductions of this file's entry points: a Gram's partial tiles ([nsplit] of `stride` floats, pitch ldp -> KP x KP, zero padded);
// the 16-row slabs of tn16_kernel; the chunk slabs of tn_kernel
inline ReduceShape reduce_shape_gram(long stride, long ldp, int nsplit, int k, int kp) { return ReduceShape{stride, ldp, nsplit, k, k, kp, kp}; }
inline ReduceShape reduce_shape_wta16(const Tn16Plan& q, int k, long n) { return ReduceShape{16 * n, n, q.nchunks, k, n, k, n}; }
inline ReduceShape reduce_shape_wta(const TnPlan& p, int k, long n) { return ReduceShape{p.chunk_stride, p.ldp, p.nchunks, k, n, k, n}; }

// the W update: 16-row wave tiles (update_w16_kernel; dnmf_mu_update_w explains when) or 32-row tiles (update_w_seq_kernel<KT, V, OCC, EDGE>)
// waves per workgroup and waves per SIMD of update_w16_kernel<KT, NWV, OCC>: the selector reports them and the launcher instantiates with them
constexpr int w16_nwv(int kt) { return kt == 4 ? 8 : 4; }
constexpr int w16_occ(int kt) { return kt == 4 ? 4 : 8; }
struct UpdWSel { bool w16, edge; int kt, v, occ, nwv; unsigned grid; long tiles; };
inline UpdWSel select_update_w(long m, int k, int kt, unsigned offw, long ldw, unsigned offah, long ldah) {
    UpdWSel s;
    const bool fast = offw == 0 && offah == 0 && ldw % 4 == 0 && ldah % 4 == 0 && k % 4 == 0;
    s.kt = kt;
    s.v = fast ? 4 : 1;
    s.w16 = fast && k == 32 * kt && m % 16 == 0 && 16 * ldw * 4 + k * 4 < 0x7fffffffL && 16 * ldah * 4 + k * 4 < 0x7fffffffL;
    if (s.w16) {
        s.nwv = w16_nwv(kt);
        s.occ = w16_occ(kt);
        s.tiles = m / 16;
        s.edge = false;
        s.grid = (unsigned)std::min<long>(cdiv(s.tiles, s.nwv), kt == 1 ? (1L << 30) : 1024L);
    } else {
        // waves per SIMD requested from the compiler (3.2 GB pass, k = 64: 3 / 4 / 5 / 6 -> 4.68 / 4.72 / 4.76 / 4.67 TB/s;
        // k = 128 holds 120 registers: 4)
        s.nwv = upd_waves(kt);
        s.occ = kt == 4 ? 4 : 5;
        s.tiles = cdiv(m, 32);
        s.edge = !(k == 32 * kt && m % 32 == 0);
        s.grid = upd_grid(s.tiles, kt);
    }
    return s;
}

// the H update: update_h_seq_kernel<KT, NT, OCC, EDGE> and its nontemporal form <KT, 2, OCC, false, 2, 2> (dnmf_mu_update_h explains)
struct UpdHSel { bool edge, nontemporal; int kt, nt, occ; unsigned grid; long tiles; };
inline UpdHSel select_update_h(int k, long n, int kt, unsigned offh, long ldh, unsigned offs, long ldatw) {
    UpdHSel s;
    const bool even = offh % 8 == 0 && offs % 8 == 0 && ldh % 2 == 0 && ldatw % 2 == 0 && n % 2 == 0;
    s.kt = kt;
    s.nt = (even && k == 32 * kt && n % 64 == 0 && n / 64 >= 1024) ? 2 : 1;
    s.occ = s.nt == 2 ? (kt == 4 ? 2 : 3) : 4;
    s.tiles = cdiv(n, 32 * s.nt);
    s.grid = upd_grid(s.tiles, kt);
    s.edge = !(k == 32 * kt && n % (32 * s.nt) == 0);
    // a long H that cannot stay cached (>= 64 MiB) streams with nontemporal loads and stores: 4.87 -> 5.07 TB/s at
    // 64 x 2^22 (each line is touched by exactly one instruction here; the W-side kernel touches a line four times
    // and loses a factor of two with the same hint, so it keeps the default policy)
    s.nontemporal = s.nt == 2 && !s.edge && (double)k * n * sizeof(float) >= 64.0 * (1 << 20);
    return s;
}

// element-wise pass (dnmf_stream.h): 16-byte vectors when X (and S) allow it; a long-row or a patch launch; `stream`: a matrix that
// cannot stay in the caches until it is touched again (>= 256 MiB) is streamed with nontemporal loads and stores: 5.5 -> 6.1 TB/s on
// the 1 GiB operands of the isolation pass; smaller factors (the W and H of a step are re-read by the next kernel) keep the default
// policy.  bad: neither a long-row nor a patch shape.
struct EwSel { bool vec, longrow, stream, bad; int txs; unsigned gx, gy; };
inline EwSel select_ew(int op, long rows, long cols, unsigned offx, long ldx, bool has_s, unsigned offs, long lds_, bool has_x, unsigned offv) {
    constexpr int U = 4;
    EwSel s{};
    s.vec = vec4(offx, ldx, cols) && (!has_s || (offs == 0 && lds_ % 4 == 0)) &&
            (!has_x || op == EW_ROWS_MUL || op == EW_KL_BYROW || offv == 0);
    const long cvecs = s.vec ? cols / 4 : cols;
    s.stream = s.vec && (double)rows * cols * sizeof(float) >= 256.0 * (1 << 20);
    if (cvecs > 256 && rows <= 65535) {
        s.longrow = true;
        s.gx = (unsigned)cdiv(cvecs, 256 * U);
        s.gy = (unsigned)rows;
        return s;
    }
    if (cvecs > 256) { s.bad = true; return s; }
    while (s.txs < 8 && (1L << s.txs) < cvecs) ++s.txs;
    s.gx = (unsigned)cdiv(rows, (256 >> s.txs) * U);
    s.gy = 1;
    return s;
}

// the squared norm: sqnorm_kernel<FAST, TA>, a grid-stride loop over 4-element vectors (FAST) or elements, at most 2048 workgroups
struct SqnormSel { bool fast; unsigned grid; long trips; };
inline SqnormSel select_sqnorm(long m, long n, size_t ea, unsigned offa, long lda) {
    SqnormSel s;
    s.fast = offa % (4 * ea) == 0 && lda % 4 == 0 && n % 4 == 0;
    const long work = s.fast ? m * (n / 4) : m * n;
    s.grid = (unsigned)std::min<long>(cdiv(work, 256), 2048);
    s.trips = cdiv(work, 256L * s.grid);
    return s;
}

template <int KT, int MT, int NW, int KS, bool FAST, int MODE, int PF, typename TX>
int launch_nt_pf(const NtArgs& a, int nsplit, hipStream_t st) {
    constexpr int BM = 32 * MT * (NW / KS);
    constexpr size_t lds32 = 2ul * (BM + 32 * KT) * BK * sizeof(float);                     // fp32 tiles (also the W.G loop)
    constexpr size_t lds16 = 2ul * (BM * BK + 32 * KT * BKH) * sizeof(float);               // bf16 X: [X raw | Y 64 wide]
    constexpr size_t lds = std::is_same<TX, bf16_t>::value ? (lds16 > lds32 ? lds16 : lds32) : lds32;
    static bool once = false;
    if (!once) { allow_lds(nt_kernel<KT, MT, NW, KS, FAST, MODE, PF, TX>, lds); once = true; }
    static_assert(BM == DENSE_BM, "the plan query reports 128-row workgroups");
    DNMF_LAUNCH((nt_kernel<KT, MT, NW, KS, FAST, MODE, PF, TX>), dim3(nt_grid_x(a.nrows), (unsigned)nsplit),
                       dim3(64 * NW), lds, st, a);
    return check_launch("nt_kernel");
}

template <int KT, int MT, int NW, int KS, bool FAST, int MODE, typename TX>
int launch_nt_inst(const NtArgs& a, int nsplit, hipStream_t st) {
    // PF code -- what the interior tiles of the streamed operand do:
    //   1  loads of k-tile t+1 issued at the top of tile t, tiles in order (also the generic / edge path)
    //   5  1 + every workgroup starts at a different k-tile (rotated order) + nontemporal loads of A (bf16 X)
    //   7  5 with LDS-DMA staging (global_load_lds: no staging VGPRs, no ds_write) -- measured, not kept
    //  10  5 with TWO k-tiles in flight and a branch-free loop (nt_mainloop_p2) -- fp32 X; grids of at most one
    //      workgroup per CU take three tiles in flight (nt_mainloop_p3t, code 13)
    // Measured on MI355X (tools/kbench.py, k = 64, n = 8192; ms at 262144 / 65536 / 32768 rows):
    //   1: 2.54 / 0.82 / -     5: 2.42-2.49 / 0.76 / 0.44     7: +-2 % of 5     10: 2.43-2.47 / 0.76 / 0.40
    // HBM reads per launch at 262144 rows (PMC): 8.67 GB for 1, 10.99 GB with the rotation alone (the streamed A evicts
    // H from L2), 8.47 GB with the nontemporal hint on top.  What did NOT help (measured, not kept): a prefetch
    // distance of 2 with conditional loads (hipcc then drains vmcnt(0) at every join: 0-18 % slower), fragment reads
    // one group ahead in a second register set (-0..4 %), 8-wave workgroups with two contraction slices (+-3 %),
    // 64-row tiles, capping workgroups per CU through the LDS request (+-5 %), loads issued for PAIRS of adjacent tiles
    // (256 B per row per visit, two register super-sets: the held clock rose 1.92 -> 1.99 GHz -- fewer DRAM row
    // activations -- but 208 registers leave two workgroups per CU, MFMA busy 85 -> 81 %, net +-2 %), and an NT form
    // WITHOUT LDS in the style of the TN kernel (lane (li, h) loads 16 B of its own row of X and of the factor, four
    // consecutive steps consume each row's 128-B line from L1): correct, but a load instruction then touches 32 rows x
    // 32 B and the texture-address unit, not the matrix pipe, paces the kernel -- 2.6x SLOWER at k = 32 and k = 64 (MFMA
    // busy 21-31 %, HBM reads 1.8x algorithmic).  The transpose of X has to go through LDS.  With A cache-resident the same
    // kernel reaches 103 / 118 / 128 TFLOP/s at 32768 / 65536 / 262144 rows against 82-89 / 91 / 113 from HBM -- with
    // IDENTICAL cycle counts (PMC): the difference is the core clock the chip holds (1.8-2.0 GHz with the HBM stream,
    // 2.2-2.4 GHz without), i.e. power, not the instruction schedule (measured ceilings).
    constexpr int BM = 32 * MT * (NW / KS);
    constexpr bool F32 = std::is_same<TX, float>::value;
    const int pf = nt_pf(FAST && KS == 1, MODE, a.store_all != 0, F32, cdiv(a.nrows, BM) * nsplit);
    if constexpr (FAST && KS == 1) {
        if constexpr (F32) {
            if (pf == 13) return launch_nt_pf<KT, MT, NW, KS, FAST, MODE, 13, TX>(a, nsplit, st);
            if (pf == 10) return launch_nt_pf<KT, MT, NW, KS, FAST, MODE, 10, TX>(a, nsplit, st);
        } else {
            if (pf == 5) return launch_nt_pf<KT, MT, NW, KS, FAST, MODE, 5, TX>(a, nsplit, st);
        }
    }
    return launch_nt_pf<KT, MT, NW, KS, FAST, MODE, 1, TX>(a, nsplit, st);
}

// Tile configuration per padded rank (KT = KP/32).  The kernel template also supports 8-wave workgroups with two contraction slices per row group (KS = 2: same
// tile, twice the waves per SIMD); measured within +-3 % of the 4-wave form at every shard size and not instantiated.
template <int MODE, typename TX = float>
int launch_nt(int kt, bool fast, const NtArgs& a, int nsplit, hipStream_t st) {
#define NT_CASE(KT_, MT_, NW_, KS_)                                                               \
    return fast ? launch_nt_inst<KT_, MT_, NW_, KS_, true, MODE, TX>(a, nsplit, st)                \
                : launch_nt_inst<KT_, MT_, NW_, KS_, false, MODE, TX>(a, nsplit, st);
    // 128-row tiles for every rank.  (k <= 32 used 256-row tiles, MT = 2, in an earlier version: equal at 262144 rows,
    // 1.8x slower at 32768 rows where it left half the CUs without a workgroup.  256-row tiles at k = 64, and 32-row
    // workgroups for the slab-wise one-pass experiment of round 2, were measured and not kept: docs/history/DESIGN_r01-r05.md.)
    if (kt == 1) { NT_CASE(1, 1, 4, 1) }
    if (kt == 2) { NT_CASE(2, 1, 4, 1) }
    if (kt == 4) { NT_CASE(4, 1, 4, 1) }
#undef NT_CASE
    return fail(DNMF_EINVAL, "unsupported k tile %d", kt);
}

inline int nt_rows_per_tile(int) { return 128; }

template <int MODE, typename TY = float>
int launch_tn(int kt, bool fast, const TnArgs& a, hipStream_t st) {
    const dim3 grid(tn_grid(a.nchunks, a.ncolblk)), block(256);
    // nontemporal loads of the streamed operand (A): +2 % at 262144 rows, +7 % at 65536 rows, slightly less HBM
    // traffic (the reused W rows stay in L2).
#define TN_CASE(KT_, NT_)                                                                                \
    if (kt == KT_) {                                                                                     \
        if (fast) DNMF_LAUNCH((tn_kernel<KT_, NT_, true, MODE, true, TY>), grid, block, 0, st, a);       \
        else DNMF_LAUNCH((tn_kernel<KT_, NT_, false, MODE, false, TY>), grid, block, 0, st, a);          \
        return check_launch("tn_kernel");                                                                \
    }
    TN_CASE(1, 4)
    TN_CASE(2, 4)
    TN_CASE(4, 2)
#undef TN_CASE
    return fail(DNMF_EINVAL, "unsupported k tile %d", kt);
}

struct SplitPlan { int nsplit; long cols_per_split; };

SplitPlan plan_gram_nt(long n) {
    SplitPlan s;
    // each workgroup walks its k-tiles as one latency chain: 128 columns (4 tiles) while that still gives at most 64
    // partial tiles (one reduction stage) -- 14.0 -> 8.8 us at n = 8192 -- else 256
    s.cols_per_split = n <= 64 * 128 ? 128 : 256;
    if (n > 256 * 512) s.cols_per_split = round_up(cdiv(n, 512), BK);
    s.nsplit = (int)std::max<long>(1, cdiv(n, s.cols_per_split));
    return s;
}


// element-wise pass (dnmf_stream.h): 16-byte vectors when X (and S) allow it; a long-row or a patch launch
template <int OP>
int launch_ew(float* X, long rows, long cols, long ldx, const float* Sm, long lds_, const float* x, float eps, int clamp,
              const char* what, hipStream_t st) {
    const EwSel sel = select_ew(OP, rows, cols, off16(X), ldx, Sm != nullptr, off16(Sm), lds_, x != nullptr, off16(x));
    const bool vec = sel.vec;
    if (sel.longrow) {                                        // long rows
        const dim3 grid(sel.gx, sel.gy);
        if (sel.stream) {
            DNMF_LAUNCH((ew_kernel<OP, 4, true, true>), grid, dim3(256), 0, st, X, rows, cols, ldx, Sm, lds_, x, eps, clamp, 0);
            return check_launch(what);
        }
        if (vec) DNMF_LAUNCH((ew_kernel<OP, 4, true>), grid, dim3(256), 0, st, X, rows, cols, ldx, Sm, lds_, x, eps, clamp, 0);
        else DNMF_LAUNCH((ew_kernel<OP, 1, true>), grid, dim3(256), 0, st, X, rows, cols, ldx, Sm, lds_, x, eps, clamp, 0);
        return check_launch(what);
    }
    if (sel.bad) return fail(DNMF_EINVAL, "%s: %ld rows x %ld columns: neither a long-row nor a patch shape", what, rows, cols);
    const int txs = sel.txs;
    const dim3 grid(sel.gx);
    if (sel.stream) {
        DNMF_LAUNCH((ew_kernel<OP, 4, false, true>), grid, dim3(256), 0, st, X, rows, cols, ldx, Sm, lds_, x, eps, clamp, txs);
        return check_launch(what);
    }
    if (vec) DNMF_LAUNCH((ew_kernel<OP, 4, false>), grid, dim3(256), 0, st, X, rows, cols, ldx, Sm, lds_, x, eps, clamp, txs);
    else DNMF_LAUNCH((ew_kernel<OP, 1, false>), grid, dim3(256), 0, st, X, rows, cols, ldx, Sm, lds_, x, eps, clamp, txs);
    return check_launch(what);
}

}  // namespace
// csrc/dnmf_team.hip: the one-pass MU/Frobenius step (16 < k <= 32, n a multiple of 512 up to 4096)
__attribute__((visibility("hidden"))) size_t dnmf_team_ws_bytes_(long m, long n, int k);
__attribute__((visibility("hidden"))) int dnmf_team_fro_(const float* A, long m, long n, long lda, float* W, long ldw, const float* H, long ldh,
                                                          const float* G, int k, float eps, void* part, size_t part_bytes, void* stream,
                                                          const float** P_out, int* nparts, const float** Pg_out, int* kp_out);
namespace {

struct WsLayout {
    size_t g_off, s_off, x_off, part_off, total;  // G [KP*KP] | S = AtW / AH / UHT / WTU | x [KP] | partials
};

size_t partial_bytes(long m, long n, int k) {
    if (wide_k(k))      // the panel calls of the contractions and of the Gram blocks + the m x n quotient image of the KL products
        return align256(std::max(std::max(partial_bytes(m, n, WIDE_PANEL), (size_t)256 * HALS_MAX_WG * sizeof(unsigned long long) + 256 * sizeof(double)),
                                 std::max(partial_bytes(m, WIDE_PANEL, WIDE_PANEL), partial_bytes(WIDE_PANEL, n, WIDE_PANEL)))) +
               align256((size_t)m * round_up(n, 4) * sizeof(float));
    const int kt = kt_of(k), kp = 32 * kt;
    size_t b = 0;
    if (k <= 16 && n % 64 == 0) {   // tn16 partial slabs (fp32: V = 4; bf16: V = 8 has fewer column blocks, more chunks)
        for (int v = 4; v <= 8; v += 4) {
            if (n % (16 * v)) continue;
            Tn16Plan q = plan_tn16(m, n, v);
            b = std::max(b, (size_t)q.nchunks * 16 * n * sizeof(float) + reduce_scratch_bytes(q.nchunks, k, n) + GRAM_RIDE_BYTES);
        }
        const Tn16Plan w = plan_wtu16(m, n);                        // kl_wtu16 partial slabs
        b = std::max(b, (size_t)w.nchunks * 16 * n * sizeof(float) + reduce_scratch_bytes(w.nchunks, k, n));
    }
    {   // wta / kl_wtu: A [m x n]
        TnPlan p = plan_tn(m, n, kt, tn_nt(kt));
        b = std::max(b, (size_t)p.nchunks * p.chunk_stride * sizeof(float) + reduce_scratch_bytes(p.nchunks, k, n));
        const KlWtuPlan q = plan_kl_wtu(m, n, kt);
        b = std::max(b, (size_t)q.nchunks * q.tn.ldp * kp * sizeof(float) + reduce_scratch_bytes((int)q.nchunks, k, n));
    }
    {   // gram W^T W: Y = W [m x k]
        TnPlan p = plan_tn(m, kp, kt, kt == 4 ? 2 : kt, gram_min_rows(m));
        b = std::max(b, (size_t)p.nchunks * p.chunk_stride * sizeof(float) + reduce_scratch_bytes(p.nchunks, kp, kp));
    }
    {   // gram H H^T
        SplitPlan s = plan_gram_nt(n);
        b = std::max(b, (size_t)s.nsplit * nt_rows_per_tile(kt) * kp * sizeof(float) + reduce_scratch_bytes(s.nsplit, kp, kp));
    }
    {   // kl_uht column-split slabs
        const long rowtiles = cdiv(m, 128);
        const int nsp = plan_uht(m, n, kt).nsplit;
        if (nsp > 1) b = std::max(b, (size_t)nsp * m * kp * sizeof(float) + reduce_scratch_bytes(nsp, (int)m, k));
        if (k <= 16) {   // kl_uht16: 16-wide slabs, also for a single split (ranks below 16 go through the slab)
            const long ns16 = std::min<long>(std::max<long>(1, 1024 / rowtiles), std::max<long>(1, n / 256));
            const int nsp16 = (int)cdiv(n, round_up(cdiv(n, ns16), BK));
            b = std::max(b, (size_t)nsp16 * m * 16 * sizeof(float) + reduce_scratch_bytes(nsp16, (int)m, k));
        }
    }
    b = std::max(b, (size_t)1024 * kp * sizeof(float));  // colsum partials (at most 1024 slabs)
    b = std::max(b, dnmf_team_ws_bytes_(m, n, k));       // one-pass MU/FRO step: the teams' partials + the granule ring (csrc/dnmf_team.hip)
    // HALS W sweep: slots + norms + the m x KP block T of its first pass (only when the sweep is asked for a factor of
    // this shape, i.e. n == k: dnmf_hals_sweep_w is called with dnmf_ws_bytes(m, k, k))
    b = std::max(b, align256((size_t)kp * HALS_MAX_WG * sizeof(unsigned long long) + (size_t)kp * sizeof(double)) +
                        (n == k ? (size_t)m * kp * sizeof(float) : 0));
    return b;
}

WsLayout ws_layout(long m, long n, int k) {
    const int kp = kp_of(k);
    WsLayout w;
    w.g_off = 0;
    w.s_off = align256((size_t)kp * kp * sizeof(float));
    const size_t s_elems = std::max((size_t)k * round_up(n, 4), (size_t)m * round_up(k, 4));
    w.x_off = w.s_off + align256(s_elems * sizeof(float));
    w.part_off = w.x_off + align256((size_t)kp * sizeof(float));
    // + room for the zero-padded factor images of the KL products (pad_factors) at the end of the partial area
    w.total = w.part_off + align256(partial_bytes(m, n, k)) + pad_bytes(m, n, kp);
    return w;
}

}  // namespace

// =============================================================================================== C ABI
// Process-wide: may kernels whose workgroups WAIT FOR EACH OTHER run (the whole fits of small problems, the persistent HALS W sweep
// -- local and across ranks --, the one-pass MU/FRO team kernel)?  They need every workgroup of a launch resident at once, i.e. the GPU
// to themselves; off, every path takes its launch-chain form (same update rules, no residency needed).  dnmf_set_persistent.
static int g_persistent_on = 1;
__attribute__((visibility("hidden"))) int dnmf_persistent_on_() { return g_persistent_on; }
__attribute__((visibility("hidden"))) void dnmf_persistent_set_(int on) { g_persistent_on = on; }
__attribute__((visibility("hidden"))) void dnmf_ws_offsets_(long m, long n, int k, size_t out[5]);
void dnmf_ws_offsets_(long m, long n, int k, size_t out[5]) {   // library-internal (csrc/dnmf_split.hip)
    const WsLayout L = ws_layout(m, n, k);
    out[0] = L.g_off; out[1] = L.s_off; out[2] = L.x_off; out[3] = L.part_off; out[4] = L.total;
}

extern "C" {

const char* dnmf_last_error(void) { return dnmf_errbuf_(); }
int dnmf_set_persistent(int on) {
    const int was = dnmf_persistent_on_();
    dnmf_persistent_set_(on != 0);
    return was;
}
int dnmf_version(void) { return 100; }
int dnmf_kp(int k) { return kp_of(k); }

size_t dnmf_ws_bytes(long m, long n, int k) {
    if (kp_of(k) < 0 || m < 1 || n < 1) return 0;
    return ws_layout(m, n, k).total;
}


}  // extern "C"
namespace {
template <typename TA>
int aht_impl(const TA* A, long m, long n, long lda, const float* H, int k, long ldh, float* AH, long ldah, void* stream, long hblk = 0);
template <typename TA>
int wta_impl(const TA* A, long m, long n, long lda, const float* W, int k, long ldw, float* AtW, long ldatw, void* ws, size_t ws_bytes, void* stream,
             float* G = nullptr);
// Gram matrices of a wide rank: the zero-padded 256 x 256 buffer, filled block by block with the tuned contractions
// (H_p H_q^T = "A H^T" with A = H_p; W_p^T W_q = "W^T A" with A = W_q)
int wide_gram(bool hht, const float* F, long len, int k, long ld, float* G, void* ws, size_t ws_bytes, void* stream) {
    if (batch_memset(G, 0, (size_t)256 * 256 * sizeof(float), S(stream)) != hipSuccess) return fail(DNMF_EHIP, "gram: memset failed");
    for (int p = 0; p < 2; ++p)
        for (int q = 0; q < 2; ++q) {
            const int kx = p ? k - WIDE_PANEL : WIDE_PANEL, ky = q ? k - WIDE_PANEL : WIDE_PANEL;
            float* blk = G + (long)p * WIDE_PANEL * 256 + q * WIDE_PANEL;
            int rc;
            if (hht) rc = aht_impl<float>(F + (long)p * WIDE_PANEL * ld, kx, len, ld, F + (long)q * WIDE_PANEL * ld, ky, ld, blk, 256, stream);
            else rc = wta_impl<float>(F + q * WIDE_PANEL, len, ky, ld, F + p * WIDE_PANEL, kx, ld, blk, 256, ws, ws_bytes, stream);
            if (rc) return rc;
        }
    return DNMF_OK;
}
}  // namespace
extern "C" {

int dnmf_gram_hht(const float* H, int k, long n, long ldh, float* G, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "gram_hht");
    if (wide_k(k)) {
        REQUIRE(H && G && n >= 1 && ldh >= n, "gram_hht: bad arguments (k=%d n=%ld)", k, n);
        return wide_gram(true, H, n, k, ldh, G, ws, ws_bytes, stream);
    }
    const int kt = kt_of(k);
    REQUIRE(kt > 0 && H && G && ws && n >= 1 && ldh >= n, "gram_hht: bad arguments (k=%d n=%ld)", k, n);
    const int kp = 32 * kt;
    const SplitPlan sp = plan_gram_nt(n);
    const long tile_rows = nt_rows_per_tile(kt);
    const size_t pbytes = (size_t)sp.nsplit * tile_rows * kp * sizeof(float);
    const size_t need = pbytes + reduce_scratch_bytes(sp.nsplit, kp, kp);
    if (ws_bytes < need) return fail(DNMF_EWS, "gram_hht: workspace %zu < %zu", ws_bytes, need);
    NtArgs a{};
    a.X = H; a.ldx = ldh; a.nrows = k; a.ncols = n;
    a.Y = H; a.ldy = ldh; a.yrows = k;
    a.cols_per_split = sp.cols_per_split;
    a.out = (float*)ws; a.ldo = kp; a.split_stride = tile_rows * kp; a.store_all = 1;
    const bool fast = nt_fast(off16(H), ldh, sizeof(float), off16(H), ldh, n);
    int rc = launch_nt<NT_STORE>(kt, fast, a, sp.nsplit, S(stream));
    if (rc) return rc;
    return launch_reduce((const float*)ws, reduce_shape_gram(tile_rows * kp, kp, sp.nsplit, k, kp), G, kp, (float*)((char*)ws + pbytes), S(stream));
}

int dnmf_gram_wtw(const float* W, long m, int k, long ldw, float* G, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "gram_wtw");
    if (wide_k(k)) {
        REQUIRE(W && G && ws && m >= 1 && ldw >= k, "gram_wtw: bad arguments (k=%d m=%ld)", k, m);
        return wide_gram(false, W, m, k, ldw, G, ws, ws_bytes, stream);
    }
    const int kt = kt_of(k);
    REQUIRE(kt > 0 && W && G && ws && m >= 1 && ldw >= k, "gram_wtw: bad arguments (k=%d m=%ld)", k, m);
    const int kp = 32 * kt;
    // TN form with X = Y = W
    const GramWtwSel sel = select_gram_wtw(m, k, kt, off16(W), ldw, ws_bytes);
    const TnPlan& p = sel.p;
    const size_t pbytes = sel.pb, need = sel.need;
    if (sel.ews) return fail(DNMF_EWS, "gram_wtw: workspace %zu < %zu", ws_bytes, need);
    TnArgs a{};
    a.X = W; a.ldx = ldw; a.xcols = k; a.Y = W; a.ldy = ldw; a.ycols = k;
    a.nrows = m; a.rows_per_chunk = p.rows_per_chunk; a.nchunks = p.nchunks; a.ncolblk = p.ncolblk;
    a.P = (float*)ws; a.chunk_stride = p.chunk_stride; a.ldp = p.ldp;
    const bool fast = sel.fast;
    const dim3 grid(tn_grid(a.nchunks, a.ncolblk)), block(256);
    hipStream_t st = S(stream);
#define GRAM_CASE(KT_, NT_)                                                                          \
    if (kt == KT_) {                                                                                 \
        if (fast) DNMF_LAUNCH((tn_kernel<KT_, NT_, true, TN_PARTIAL>), grid, block, 0, st, a); \
        else DNMF_LAUNCH((tn_kernel<KT_, NT_, false, TN_PARTIAL>), grid, block, 0, st, a);    \
    }
    GRAM_CASE(1, 1) GRAM_CASE(2, 2) GRAM_CASE(4, 2)
#undef GRAM_CASE
    int rc = check_launch("gram_wtw");
    if (rc) return rc;
    return launch_reduce((const float*)ws, reduce_shape_gram(p.chunk_stride, p.ldp, p.nchunks, k, kp), G, kp, (float*)((char*)ws + pbytes), st);
}

}  // extern "C"  (typed implementations shared by the fp32 and the bf16-A entry points)
namespace {
// alignment the vector path needs from A: 16 B for fp32 rows, 8 B for bf16 rows (4 elements per lane either way)

// rank k <= 16 with aligned operands and a column count that is a whole number of k-tiles: the 16-wide kernel.
// Returns 1 when not applicable (caller falls through to the 32-wide kernels), else the launch status.
template <int MODE, typename TA>
int try_nt16(const NtArgs& a, bool fast, long n, int k, hipStream_t st) {
    constexpr bool b16 = std::is_same<TA, bf16_t>::value;
    if (!nt16_applies(k, fast, n, b16)) return 1;
    DNMF_LAUNCH((nt16_kernel<TA, MODE>), dim3(nt_grid_x(a.nrows)), dim3(256), nt16_lds_bytes(b16), st, a);
    return check_launch("nt16_kernel");
}

// hblk = 0: H is one k x n matrix (ldh).  hblk > 0 (fp32 A): H is the stack of n / hblk column blocks [q][k][hblk], ldh = hblk.
template <typename TA>
int aht_impl(const TA* A, long m, long n, long lda, const float* H, int k, long ldh, float* AH, long ldah,
             void* stream, long hblk) {
    if (wide_k(k)) {                                               // A H^T splits exactly along the rows of H: two passes over A
        REQUIRE(!hblk && H && AH && ldah >= k && ldh >= n, "aht: bad arguments (k = %d; H as column blocks: k <= %d)", k, DNMF_TUNED_MAX_K);
        if (int rc = aht_impl<TA>(A, m, n, lda, H, WIDE_PANEL, ldh, AH, ldah, stream, 0)) return rc;
        return aht_impl<TA>(A, m, n, lda, H + (long)WIDE_PANEL * ldh, k - WIDE_PANEL, ldh, AH + WIDE_PANEL, ldah, stream, 0);
    }
    const int kt = kt_of(k);
    REQUIRE(kt > 0 && A && H && AH && m >= 1 && n >= 1 && lda >= n && ldah >= k, "aht: bad arguments");
    REQUIRE(hblk ? (ldh == hblk && n % hblk == 0 && hblk % BK == 0 && (n / 16) * (hblk / 16) < (1L << 32)) : ldh >= n,
            "aht: bad H layout (ldh %ld, block %ld, n %ld)", ldh, hblk, n);
    NtArgs a{};
    a.X = A; a.ldx = lda; a.nrows = m; a.ncols = n;
    a.Y = H; a.ldy = ldh; a.yrows = k;
    if (hblk) {
        const unsigned long units = (unsigned long)(hblk / 16);
        a.yb = YBlk{(unsigned)(((1UL << 32) + units - 1) / units), (long)(k - 1) * hblk};
    }
    a.cols_per_split = round_up(n, BK);
    a.out = AH; a.ldo = ldah; a.split_stride = 0; a.store_all = 0;
    const bool fast = nt_fast(off16(A), lda, sizeof(TA), off16(H), ldh, n);
    if (int rc16 = try_nt16<NT_STORE, TA>(a, fast, n, k, S(stream)); rc16 != 1) return rc16;
    return launch_nt<NT_STORE, TA>(kt, fast, a, 1, S(stream));
}

template <typename TA>
int aht_update_w_impl(const TA* A, long m, long n, long lda, const float* H, int k, long ldh, const float* G,
                      float* W, long ldw, float eps, void* stream) {
    REQUIRE(!wide_k(k), "aht_update_w: the fused form takes k <= %d (dnmf_aht followed by dnmf_mu_update_w beyond it)", DNMF_TUNED_MAX_K);
    const int kt = kt_of(k);
    REQUIRE(kt > 0 && A && H && G && W && m >= 1 && n >= 1 && lda >= n && ldh >= n && ldw >= k, "aht_update_w: bad arguments");
    // a transposed image of this very block bound to the calling thread (dnmf_wimage_bind): the TN-form W phase of
    // csrc/dnmf_timg.hip where its plan takes it -- bit-equal to the kernel below, so the choice never shows in the results
    if constexpr (std::is_same<TA, float>::value)
        if (int rci = dnmf_wimage_try_(A, m, n, lda, H, k, ldh, G, W, ldw, eps, stream); rci != 1) return rci;
    NtArgs a{};
    a.X = A; a.ldx = lda; a.nrows = m; a.ncols = n;
    a.Y = H; a.ldy = ldh; a.yrows = k;
    a.cols_per_split = round_up(n, BK);
    a.W = W; a.ldw = ldw; a.G = G; a.eps = eps; a.k = k;
    const bool fast = nt_fast(off16(A), lda, sizeof(TA), off16(H), ldh, n);
    a.wfast = vec4(off16(W), ldw, k);
    if (int rc16 = try_nt16<NT_FUSED_W, TA>(a, fast, n, k, S(stream)); rc16 != 1) return rc16;
    return launch_nt<NT_FUSED_W, TA>(kt, fast, a, 1, S(stream));
}
}  // namespace
extern "C" {

int dnmf_aht(const float* A, long m, long n, long lda, const float* H, int k, long ldh, float* AH, long ldah,
             void* stream) {
    return aht_impl<float>(A, m, n, lda, H, k, ldh, AH, ldah, stream);
}
int dnmf_aht_hblocks(const float* A, long m, long n, long lda, const float* Hs, long nh, int k, float* AH, long ldah,
                     void* stream) {
    REQUIRE(nh >= 1, "aht_hblocks: bad block width");
    return aht_impl<float>(A, m, n, lda, Hs, k, nh, AH, ldah, stream, nh);
}
int dnmf_aht_bf16a(const void* A, long m, long n, long lda, const float* H, int k, long ldh, float* AH, long ldah,
                   void* stream) {
    return aht_impl<bf16_t>((const bf16_t*)A, m, n, lda, H, k, ldh, AH, ldah, stream);
}
int dnmf_aht_update_w(const float* A, long m, long n, long lda, const float* H, int k, long ldh, const float* G,
                      float* W, long ldw, float eps, void* stream) {
    return aht_update_w_impl<float>(A, m, n, lda, H, k, ldh, G, W, ldw, eps, stream);
}
int dnmf_aht_update_w_bf16a(const void* A, long m, long n, long lda, const float* H, int k, long ldh, const float* G,
                            float* W, long ldw, float eps, void* stream) {
    return aht_update_w_impl<bf16_t>((const bf16_t*)A, m, n, lda, H, k, ldh, G, W, ldw, eps, stream);
}

}  // extern "C"
namespace {
template <int KT, int V, int OCC>
int launch_update_w_seq(const UpdWSel& sel, float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G, float eps, hipStream_t st) {
    constexpr size_t lds = (size_t)(32 * KT) * (32 * KT + 4) * sizeof(float);
    static bool once = false;
    if (!once) { allow_lds(update_w_seq_kernel<KT, V, OCC, false>, lds); allow_lds(update_w_seq_kernel<KT, V, OCC, true>, lds); once = true; }
    // one tile per wave (the kernel's tile loop only matters beyond 2^31 workgroups): measured on the 3.2 GB pass at
    // k = 64, workgroups that loop over tiles (256 x OCC of them, G staged once each) 4.5 TB/s, one tile per wave 4.75
    const unsigned grid = sel.grid;
    constexpr unsigned T = 64 * upd_waves(KT);
    if (!sel.edge)
        DNMF_LAUNCH((update_w_seq_kernel<KT, V, OCC, false>), dim3(grid), dim3(T), lds, st, W, m, k, ldw, AH, ldah, G, eps, (float*)nullptr, 0L);
    else
        DNMF_LAUNCH((update_w_seq_kernel<KT, V, OCC, true>), dim3(grid), dim3(T), lds, st, W, m, k, ldw, AH, ldah, G, eps, (float*)nullptr, 0L);
    return check_launch("mu_update_w");
}
}  // namespace
extern "C" {

int dnmf_mu_update_w(float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G, float eps,
                     void* stream) {
    if (wide_k(k)) {
        REQUIRE(W && AH && G && m >= 1 && ldw >= k && ldah >= k, "mu_update_w: bad arguments");
        return dnmf_wide_mu_update_w_(W, m, k, ldw, AH, ldah, G, 256, eps, stream);
    }
    const int kt = kt_of(k);
    REQUIRE(kt > 0 && W && AH && G && m >= 1 && ldw >= k && ldah >= k, "mu_update_w: bad arguments");
    REQUIRE(update_w_pitch_ok(ldw, ldah), "mu_update_w: leading dimension beyond the 32-bit tile offsets");
    const UpdWSel sel = select_update_w(m, k, kt, off16(W), ldw, off16(AH), ldah);
    hipStream_t st = S(stream);
    // 16-row wave tiles (update_w16_kernel; round 5): full ranks, whole tiles, aligned rows, 2 GiB descriptor windows.  Measured on
    // the isolation pass (k x 2^22): k = 32: 0.346 -> 0.310 ms (0.58 -> 0.65 of HBM), k = 64: 0.759 -> 0.632
    // (0.53 -> 0.64), k = 128: 1.49 -> 1.40 (0.54 -> 0.58: the matrix work of 2 n k^2 flops bounds that one).  Workgroups walk
    // their tiles grid-stride; capped at 1024 workgroups from k = 64 on (G staged once per several tiles: 0.648 -> 0.632 at
    // k = 64), one tile per wave at k = 32.
    if (sel.w16) {
        auto run = [&](auto kt_c) {
            constexpr int KT_ = decltype(kt_c)::value, NWV_ = w16_nwv(KT_), OCC_ = w16_occ(KT_);
            constexpr size_t lds = (size_t)(32 * KT_) * (32 * KT_ + 4) * sizeof(float);
            static bool once = false;
            if (!once) { allow_lds(update_w16_kernel<KT_, NWV_, OCC_>, lds); once = true; }
            DNMF_LAUNCH((update_w16_kernel<KT_, NWV_, OCC_>), dim3(sel.grid), dim3(64 * NWV_), lds, st, W, m, ldw, AH, ldah, G, eps);
            return check_launch("mu_update_w(16)");
        };
        using std::integral_constant;
        if (kt == 1) return run(integral_constant<int, 1>{});
        if (kt == 2) return run(integral_constant<int, 2>{});
        return run(integral_constant<int, 4>{});
    }
    const bool fast = sel.v == 4;
    if (kt == 1) return fast ? launch_update_w_seq<1, 4, 5>(sel, W, m, k, ldw, AH, ldah, G, eps, st) : launch_update_w_seq<1, 1, 5>(sel, W, m, k, ldw, AH, ldah, G, eps, st);
    if (kt == 2) return fast ? launch_update_w_seq<2, 4, 5>(sel, W, m, k, ldw, AH, ldah, G, eps, st) : launch_update_w_seq<2, 1, 5>(sel, W, m, k, ldw, AH, ldah, G, eps, st);
    return fast ? launch_update_w_seq<4, 4, 4>(sel, W, m, k, ldw, AH, ldah, G, eps, st) : launch_update_w_seq<4, 1, 4>(sel, W, m, k, ldw, AH, ldah, G, eps, st);
}

}  // extern "C"
namespace {
// G != nullptr: also G = W^T W (KP x KP, zero padded; dist_nmf.py:705) -- for k <= 16 inside the same two launches (the wave of
// column block 0 of every row chunk accumulates it, the reduction launch sums the partial tiles), otherwise dnmf_gram_wtw first.
template <typename TA>
int wta_impl(const TA* A, long m, long n, long lda, const float* W, int k, long ldw, float* AtW, long ldatw,
             void* ws, size_t ws_bytes, void* stream, float* G) {
    REQUIRE_WS16(ws, "wta");
    if (wide_k(k)) {                                               // W^T A splits exactly along the columns of W: two passes over A
        REQUIRE(W && AtW && ws && ldw >= k && ldatw >= n, "wta: bad arguments (k = %d)", k);
        if (G) if (int rc = dnmf_gram_wtw(W, m, k, ldw, G, ws, ws_bytes, stream)) return rc;
        if (int rc = wta_impl<TA>(A, m, n, lda, W, WIDE_PANEL, ldw, AtW, ldatw, ws, ws_bytes, stream, nullptr)) return rc;
        return wta_impl<TA>(A, m, n, lda, W + WIDE_PANEL, k - WIDE_PANEL, ldw, AtW + (long)WIDE_PANEL * ldatw, ldatw, ws, ws_bytes, stream, nullptr);
    }
    const int kt = kt_of(k);
    REQUIRE(kt > 0 && A && W && AtW && ws && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldatw >= n, "wta: bad arguments");
    const int kp = 32 * kt;
    auto gram_first = [&]() { return G ? dnmf_gram_wtw(W, m, k, ldw, G, ws, ws_bytes, stream) : DNMF_OK; };
    const WtaSel sel = select_wta(m, n, k, kt, sizeof(TA), off16(A), lda, off16(W), ldw, ws_bytes, G != nullptr);
    if (sel.fam == WTA_TN16) {   // rank k <= 16: 16-wide kernel (16-byte aligned rows of A, whole column blocks, workspace permitting)
        const Tn16Plan& q = sel.q;
        const size_t pb = sel.pb;
        TnArgs a{};
        a.X = W; a.ldx = ldw; a.xcols = k; a.Y = A; a.ldy = lda; a.ycols = n;
        a.nrows = m; a.rows_per_chunk = q.rows_per_chunk; a.nchunks = q.nchunks; a.ncolblk = q.ncolblk;
        a.P = (float*)ws; a.chunk_stride = 16 * n; a.ldp = n;
        const bool ride = sel.ride;
        int rc;
        if (!ride && (rc = gram_first())) return rc;
        hipStream_t st = S(stream);
        const dim3 grid16(tn_grid(q.nchunks, q.ncolblk));
        if (ride) {
            a.Pg = (float*)((char*)ws + pb);
            DNMF_LAUNCH((tn16_kernel<TA, true>), grid16, dim3(256), 0, st, a);
        } else {
            DNMF_LAUNCH((tn16_kernel<TA>), grid16, dim3(256), 0, st, a);
        }
        if ((rc = check_launch("tn16_kernel"))) return rc;
        const GramTail gt{a.Pg, G, 16, k, kp, q.nchunks};
        return launch_reduce((const float*)ws, reduce_shape_wta16(q, k, n), AtW, ldatw, (float*)((char*)ws + pb), st, ride ? &gt : nullptr);
    }
    const TnPlan& p = sel.p;
    const size_t pbytes = sel.pb, need = sel.need;
    if (sel.fam == WTA_EWS) return fail(DNMF_EWS, "wta: workspace %zu < %zu", ws_bytes, need);
    TnArgs a{};
    a.X = W; a.ldx = ldw; a.xcols = k; a.Y = A; a.ldy = lda; a.ycols = n;
    a.nrows = m; a.rows_per_chunk = p.rows_per_chunk; a.nchunks = p.nchunks; a.ncolblk = p.ncolblk;
    a.P = (float*)ws; a.chunk_stride = p.chunk_stride; a.ldp = p.ldp;
    // (the riding Gram was also built for the 32-wide kernel at 16 < k <= 32: no gain -- 0.3707 vs 0.3706 ms per iteration at
    // 65536 x 4096, k = 32, where the two launches it saves cost 6 us -- so these ranks keep dnmf_gram_wtw)
    int rc;
    if ((rc = gram_first())) return rc;
    if ((rc = launch_tn<TN_PARTIAL, TA>(kt, sel.fast, a, S(stream)))) return rc;
    return launch_reduce((const float*)ws, reduce_shape_wta(p, k, n), AtW, ldatw, (float*)((char*)ws + pbytes), S(stream));
}
}  // namespace
extern "C" {

int dnmf_wta(const float* A, long m, long n, long lda, const float* W, int k, long ldw, float* AtW, long ldatw,
             void* ws, size_t ws_bytes, void* stream) {
    return wta_impl<float>(A, m, n, lda, W, k, ldw, AtW, ldatw, ws, ws_bytes, stream);
}
int dnmf_wta_bf16a(const void* A, long m, long n, long lda, const float* W, int k, long ldw, float* AtW, long ldatw,
                   void* ws, size_t ws_bytes, void* stream) {
    return wta_impl<bf16_t>((const bf16_t*)A, m, n, lda, W, k, ldw, AtW, ldatw, ws, ws_bytes, stream);
}

int dnmf_wta_gram(const float* A, long m, long n, long lda, const float* W, int k, long ldw, float* AtW, long ldatw, float* G,
                  void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(G, "wta_gram: null Gram buffer");
    return wta_impl<float>(A, m, n, lda, W, k, ldw, AtW, ldatw, ws, ws_bytes, stream, G);
}
int dnmf_wta_gram_bf16a(const void* A, long m, long n, long lda, const float* W, int k, long ldw, float* AtW, long ldatw,
                        float* G, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE(G, "wta_gram: null Gram buffer");
    return wta_impl<bf16_t>((const bf16_t*)A, m, n, lda, W, k, ldw, AtW, ldatw, ws, ws_bytes, stream, G);
}

}  // extern "C"
namespace {
template <int KT, int NT, int OCC>
int launch_update_h_seq(const UpdHSel& sel, float* H, int k, long n, long ldh, const float* AtW, long ldatw, const float* G, float eps, int clamp,
                        hipStream_t st) {
    constexpr size_t lds = (size_t)(32 * KT) * (32 * KT + 4) * sizeof(float);
    static bool once = false;
    if (!once) { allow_lds(update_h_seq_kernel<KT, NT, OCC, false>, lds); allow_lds(update_h_seq_kernel<KT, NT, OCC, true>, lds); once = true; }
    const unsigned grid = sel.grid;
    constexpr unsigned T = 64 * upd_waves(KT);
    if constexpr (NT == 2) {
        if (sel.nontemporal) {
            static bool once2 = false;
            if (!once2) { allow_lds(update_h_seq_kernel<KT, NT, OCC, false, 2, 2>, lds); once2 = true; }
            DNMF_LAUNCH((update_h_seq_kernel<KT, NT, OCC, false, 2, 2>), dim3(grid), dim3(T), lds, st, H, k, n, ldh, AtW, ldatw, G, eps, clamp);
            return check_launch("mu_update_h");
        }
    }
    if (!sel.edge)
        DNMF_LAUNCH((update_h_seq_kernel<KT, NT, OCC, false>), dim3(grid), dim3(T), lds, st, H, k, n, ldh, AtW, ldatw, G, eps, clamp);
    else
        DNMF_LAUNCH((update_h_seq_kernel<KT, NT, OCC, true>), dim3(grid), dim3(T), lds, st, H, k, n, ldh, AtW, ldatw, G, eps, clamp);
    return check_launch("mu_update_h");
}
}  // namespace
extern "C" {

int dnmf_mu_update_h(float* H, int k, long n, long ldh, const float* AtW, long ldatw, const float* G, float eps,
                     int clamp, void* stream) {
    if (wide_k(k)) {
        REQUIRE(H && AtW && G && n >= 1 && ldh >= n && ldatw >= n, "mu_update_h: bad arguments");
        return dnmf_wide_mu_update_h_(H, k, n, ldh, AtW, ldatw, G, 256, eps, clamp, stream);
    }
    const int kt = kt_of(k);
    REQUIRE(kt > 0 && H && AtW && G && n >= 1 && ldh >= n && ldatw >= n, "mu_update_h: bad arguments");
    REQUIRE(update_h_pitch_ok(ldh, ldatw), "mu_update_h: leading dimension beyond the 32-bit tile offsets");
    const UpdHSel sel = select_update_h(k, n, kt, off16(H), ldh, off16(AtW), ldatw);
    hipStream_t st = S(stream);
    // variant code = 10 * NT (columns per lane) + waves per SIMD requested from the compiler.  Measured on the 3.2 GB pass
    // (k x 2^22): k = 64: 14 / 16 -> 4.76 / 4.78 TB/s, 23 -> 4.97, 24 (spills) -> 4.0; k = 32: 14 -> 4.93, 23 -> 5.26;
    // k = 128: 14 -> 3.44, 23 -> 2.58.  Two columns per lane (256 B per row and wave) stream better but need 8-byte
    // aligned rows, and a short H (fewer than 1024 such tiles: a latency chain on a few CUs) keeps 32-column tiles.
    // k = 128 (round 4): LDS holds two workgroups per CU there whatever the registers allow (66 KiB of G each), so the two-column
    // tile at TWO waves per SIMD (200 registers, no spills) costs no occupancy and halves the accesses per byte: 4.25 -> 4.5 TB/s on
    // the 6.4 GB pass (variant 23 spills there: 2.4 TB/s)
    if (sel.nt == 2) {
        if (kt == 1) return launch_update_h_seq<1, 2, 3>(sel, H, k, n, ldh, AtW, ldatw, G, eps, clamp, st);
        if (kt == 2) return launch_update_h_seq<2, 2, 3>(sel, H, k, n, ldh, AtW, ldatw, G, eps, clamp, st);
        return launch_update_h_seq<4, 2, 2>(sel, H, k, n, ldh, AtW, ldatw, G, eps, clamp, st);
    }
    if (kt == 1) return launch_update_h_seq<1, 1, 4>(sel, H, k, n, ldh, AtW, ldatw, G, eps, clamp, st);
    if (kt == 2) return launch_update_h_seq<2, 1, 4>(sel, H, k, n, ldh, AtW, ldatw, G, eps, clamp, st);
    return launch_update_h_seq<4, 1, 4>(sel, H, k, n, ldh, AtW, ldatw, G, eps, clamp, st);
}

int dnmf_clamp_min(float* X, long rows, long cols, long ldx, float eps, void* stream) {
    REQUIRE(X && rows >= 1 && cols >= 1 && ldx >= cols, "clamp_min: bad arguments");
    return launch_ew<EW_CLAMP>(X, rows, cols, ldx, nullptr, 0, nullptr, eps, 0, "clamp", S(stream));
}

int dnmf_scale_cols_div(float* W, long m, int k, long ldw, const float* s, float eps, void* stream) {
    REQUIRE(W && s && m >= 1 && k >= 1 && ldw >= k, "scale_cols_div: bad arguments");
    return launch_ew<EW_COLS_DIV>(W, m, k, ldw, nullptr, 0, s, eps, 0, "scale_cols_div", S(stream));
}

int dnmf_scale_rows_mul(float* H, int k, long n, long ldh, const float* s, void* stream) {
    REQUIRE(H && s && n >= 1 && k >= 1 && ldh >= n, "scale_rows_mul: bad arguments");
    return launch_ew<EW_ROWS_MUL>(H, k, n, ldh, nullptr, 0, s, 0.f, 0, "scale_rows_mul", S(stream));
}

}  // extern "C"
namespace {
// one wave that samples the shader clock while other kernels run (include/dnmf.h: dnmf_clock_probe)
__global__ __launch_bounds__(64) void clock_probe_kernel(unsigned long long* buf, int n, int naps) {
    if (threadIdx.x != 0) return;
    for (int i = 0; i < n; ++i) {
        const unsigned long long c = __builtin_amdgcn_s_memtime(), w = wall_clock64();
        __builtin_nontemporal_store(c, &buf[2 * i]);
        __builtin_nontemporal_store(w, &buf[2 * i + 1]);
        for (int s = 0; s < naps; ++s) __builtin_amdgcn_s_sleep(127);       // 127 x 64 cycles
    }
}

template <typename TA>
int sqnorm_impl(const TA* A, long m, long n, long lda, double* out, void* stream) {
    REQUIRE(A && out && m >= 1 && n >= 1 && lda >= n, "sqnorm: bad arguments");
    hipStream_t st = S(stream);
    if (batch_memset(out, 0, sizeof(double), st) != hipSuccess) return fail(DNMF_EHIP, "sqnorm: memset failed");
    const SqnormSel sel = select_sqnorm(m, n, sizeof(TA), off16(A), lda);
    const bool fast = sel.fast;
    const unsigned grid = sel.grid;
    if (fast) DNMF_LAUNCH((sqnorm_kernel<true, TA>), dim3(grid), dim3(256), 0, st, A, m, n, lda, out);
    else DNMF_LAUNCH((sqnorm_kernel<false, TA>), dim3(grid), dim3(256), 0, st, A, m, n, lda, out);
    return check_launch("sqnorm");
}
}  // namespace
extern "C" {

int dnmf_sqnorm(const float* A, long m, long n, long lda, double* out, void* stream) {
    return sqnorm_impl<float>(A, m, n, lda, out, stream);
}
int dnmf_sqnorm_bf16a(const void* A, long m, long n, long lda, double* out, void* stream) {
    return sqnorm_impl<bf16_t>((const bf16_t*)A, m, n, lda, out, stream);
}

// X_per = X * (1 + nv + 2 nv U[0,1)) in one pass (pyDNMFk.py:42-44); `bf16` != 0: X and X_per are bfloat16 (config 5's storage)
int dnmf_perturb_uniform(const void* X, void* X_per, long rows, long cols, long ldx, long ldo, float noise_var,
                         unsigned long long seed, int bf16, void* stream) {
    REQUIRE(X && X_per && rows >= 1 && cols >= 1 && ldx >= cols && ldo >= cols, "perturb_uniform: bad arguments (cols %ld, ld %ld / %ld)", cols, ldx, ldo);
    hipStream_t st = S(stream);
    // rows of 16-byte aligned vectors of 8 elements: the vector kernel; anything else: one element per thread, SAME values
    const bool vec = cols % 8 == 0 && ldx % 8 == 0 && ldo % 8 == 0 && aligned16(X) && aligned16(X_per);
    const long total = vec ? rows * (cols / 8) : rows * cols;
    const unsigned grid = (unsigned)std::min<long>(cdiv(total, 256), 256L * 32);
    if (vec) {
        if (bf16) hipLaunchKernelGGL(perturb_uniform_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)X, (bf16_t*)X_per, rows, cols, ldx, ldo, noise_var, seed);
        else hipLaunchKernelGGL(perturb_uniform_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)X, (float*)X_per, rows, cols, ldx, ldo, noise_var, seed);
    } else {
        if (bf16) hipLaunchKernelGGL(perturb_uniform_any_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)X, (bf16_t*)X_per, rows, cols, ldx, ldo, noise_var, seed);
        else hipLaunchKernelGGL(perturb_uniform_any_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)X, (float*)X_per, rows, cols, ldx, ldo, noise_var, seed);
    }
    return check_launch("perturb_uniform");
}

int dnmf_clock_probe(unsigned long long* samples, int n, int naps, void* stream) {
    REQUIRE(samples && n >= 1 && naps >= 0 && naps <= 1000, "clock_probe: bad arguments");
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, S(stream), samples, n, naps);
    return check_launch("clock_probe");
}

int dnmf_rowsum(const float* H, int k, long n, long ldh, float* x, void* stream) {
    REQUIRE(H && x && k >= 1 && n >= 1 && ldh >= n, "rowsum: bad arguments");
    DNMF_LAUNCH(rowsum_kernel, dim3(k), dim3(1024), 0, S(stream), H, n, ldh, x);
    return check_launch("rowsum");
}

int dnmf_colsum(const float* W, long m, int k, long ldw, float* x, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "colsum");
    const int kp = kp_of(k);
    REQUIRE(kp > 0 && W && x && ws && m >= 1 && ldw >= k, "colsum: bad arguments");
    // slabs of 128 rows (a 32768-row shard gives 256 workgroups; 1024-row slabs left it on 32 CUs: 116 us for 16 MiB),
    // at most 1024 slabs; the partials are summed in slab order by one small launch
    const long rows_per_blk = std::max<long>(128, round_up(cdiv(m, 1024), 8));
    const int nblk = (int)cdiv(m, rows_per_blk);
    if (ws_bytes < (size_t)nblk * kp * sizeof(float)) return fail(DNMF_EWS, "colsum: workspace too small");
    DNMF_LAUNCH(colsum_partial_kernel, dim3(nblk), dim3(256), 0, S(stream), W, m, k, ldw, rows_per_blk, (float*)ws, kp);
    DNMF_LAUNCH(colsum_final_kernel, dim3(1), dim3(1024), 0, S(stream), (const float*)ws, nblk, kp, k, x);
    return check_launch("colsum");
}

int dnmf_kl_update_w(float* W, long m, int k, long ldw, const float* Sm, long lds_, const float* x, float eps,
                     void* stream) {
    REQUIRE(W && Sm && x && m >= 1 && k >= 1 && ldw >= k && lds_ >= k, "kl_update_w: bad arguments");
    return launch_ew<EW_KL_BYCOL>(W, m, k, ldw, Sm, lds_, x, eps, 0, "kl_update_w", S(stream));
}

int dnmf_kl_update_h(float* H, int k, long n, long ldh, const float* Sm, long lds_, const float* x, float eps,
                     int clamp, void* stream) {
    REQUIRE(H && Sm && x && n >= 1 && k >= 1 && ldh >= n && lds_ >= n, "kl_update_h: bad arguments");
    return launch_ew<EW_KL_BYROW>(H, k, n, ldh, Sm, lds_, x, eps, clamp, "kl_update_h", S(stream));
}

}  // extern "C"
namespace {
template <typename TA>
int mu_fro_step_impl(const TA* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k,
                     float eps, int w_update, int clamp, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "mu_fro_step");
    REQUIRE(kp_of(k) > 0 && A && W && H && ws && m >= 1 && n >= 1, "mu_fro_step: bad arguments");
    const WsLayout L = ws_layout(m, n, k);
    if (ws_bytes < L.total) return fail(DNMF_EWS, "mu_fro_step: workspace %zu < %zu", ws_bytes, L.total);
    char* base = (char*)ws;
    float* G = (float*)(base + L.g_off);
    float* Sb = (float*)(base + L.s_off);
    void* part = base + L.part_off;
    const size_t part_bytes = L.total - L.part_off;
    int rc;
    if constexpr (std::is_same<TA, float>::value) {
        // 16 < k <= 32 on whole 512-column pieces: ONE pass over A (csrc/dnmf_team.h) -- the W update of a row block and its share of
        // W^T A while the block is on chip; H H^T before, W^T W after and the H update are the launches of the two-pass sequence
        if (w_update && dnmf_team_ws_bytes_(m, n, k)) {
            if ((rc = dnmf_gram_hht(H, k, n, ldh, G, part, part_bytes, stream))) return rc;
            const float *P = nullptr, *Pg = nullptr;
            int nparts = 0, tkp = 32;
            rc = dnmf_team_fro_(A, m, n, lda, W, ldw, H, ldh, G, k, eps, part, part_bytes, stream, &P, &nparts, &Pg, &tkp);
            if (rc < 0) return rc;
            if (rc == DNMF_OK) {
                // the teams' partials of W^T A -> S, and in the same launch the teams' partial Gram tiles -> G = W_new^T W_new (:748; the
                // kernel read H H^T from G: it has finished -- same stream)
                const long ldatw = round_up(n, 4);
                const GramTail gt{Pg, G, tkp, k, 32, nparts};
                if ((rc = launch_reduce(P, (long)tkp * n, n, nparts, Sb, ldatw, k, n, k, n, nullptr, S(stream), &gt))) return rc;
                if ((rc = dnmf_mu_update_h(H, k, n, ldh, Sb, ldatw, G, eps, clamp, stream))) return rc;
                if (clamp) return dnmf_clamp_min(W, m, k, ldw, eps, stream);
                return DNMF_OK;
            }
            w_update = -1;                                                            // H H^T is in G already
        }
    }
    if (w_update) {                                                                   // dist_nmf.py:716-732
        if (w_update > 0 && (rc = dnmf_gram_hht(H, k, n, ldh, G, part, part_bytes, stream))) return rc;
        if (wide_k(k)) {                                             // beyond the fused kernel's rank: the product, then the update
            const long ldah = round_up(k, 4);
            if ((rc = aht_impl<TA>(A, m, n, lda, H, k, ldh, Sb, ldah, stream, 0))) return rc;
            if ((rc = dnmf_mu_update_w(W, m, k, ldw, Sb, ldah, G, eps, stream))) return rc;
        } else if ((rc = aht_update_w_impl<TA>(A, m, n, lda, H, k, ldh, G, W, ldw, eps, stream))) return rc;
    }
    const long ldatw = round_up(n, 4);                                                // dist_nmf.py:736-751
    if ((rc = wta_impl<TA>(A, m, n, lda, W, k, ldw, Sb, ldatw, part, part_bytes, stream, G))) return rc;   // + W^T W (:705)
    if ((rc = dnmf_mu_update_h(H, k, n, ldh, Sb, ldatw, G, eps, clamp, stream))) return rc;
    if (clamp) return dnmf_clamp_min(W, m, k, ldw, eps, stream);                      // pyDNMF.py:155-157
    return DNMF_OK;
}
}  // namespace
extern "C" {

int dnmf_mu_fro_step(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k,
                     float eps, int w_update, int clamp, void* ws, size_t ws_bytes, void* stream) {
    return mu_fro_step_impl<float>(A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, clamp, ws, ws_bytes, stream);
}
int dnmf_mu_fro_step_bf16a(const void* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k,
                           float eps, int w_update, int clamp, void* ws, size_t ws_bytes, void* stream) {
    return mu_fro_step_impl<bf16_t>((const bf16_t*)A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, clamp, ws, ws_bytes, stream);
}

int dnmf_mu_kl_step(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps,
                    int w_update, int clamp, void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "mu_kl_step");
    REQUIRE(kp_of(k) > 0 && A && W && H && ws && m >= 1 && n >= 1, "mu_kl_step: bad arguments");
    const WsLayout L = ws_layout(m, n, k);
    if (ws_bytes < L.total) return fail(DNMF_EWS, "mu_kl_step: workspace %zu < %zu", ws_bytes, L.total);
    char* base = (char*)ws;
    float* Sb = (float*)(base + L.s_off);
    float* x = (float*)(base + L.x_off);
    void* part = base + L.part_off;
    const size_t part_bytes = L.total - L.part_off;
    int rc;
    if (w_update) {                                                                   // dist_nmf.py:813-830
        const long ldu = round_up(k, 4);
        if ((rc = dnmf_rowsum(H, k, n, ldh, x, stream))) return rc;
        if ((rc = dnmf_kl_uht(A, m, n, lda, W, ldw, H, ldh, k, eps, Sb, ldu, part, part_bytes, stream))) return rc;
        if ((rc = dnmf_kl_update_w(W, m, k, ldw, Sb, ldu, x, eps, stream))) return rc;
    }
    const long ldo = round_up(n, 4);                                                  // dist_nmf.py:832-849
    if ((rc = dnmf_colsum(W, m, k, ldw, x, part, part_bytes, stream))) return rc;
    if ((rc = dnmf_kl_wtu(A, m, n, lda, W, ldw, H, ldh, k, eps, Sb, ldo, part, part_bytes, stream))) return rc;
    if ((rc = dnmf_kl_update_h(H, k, n, ldh, Sb, ldo, x, eps, clamp, stream))) return rc;
    if (clamp) return dnmf_clamp_min(W, m, k, ldw, eps, stream);
    return DNMF_OK;
}

}  // extern "C"

// =============================================================================================== the launch-plan query
namespace {
// full register batches and rows left to the predicated tail loop of a row chunk of `rows` rows (tn_mainloop: batches of 8 rows on the
// FAST path only; tn16_body: batches of 16 rows)
inline void chunk_trips(long rows, int batch, bool pipelined, long* full, long* tail) {
    *full = pipelined ? rows / batch : 0;
    *tail = rows - *full * batch;
}
inline void report_chunks(long* out, long m, long rpc, int nchunks, int batch, bool pipelined) {
    out[DNMF_DENSE_PLAN_COUNT] = nchunks;
    out[DNMF_DENSE_PLAN_PER] = rpc;
    chunk_trips(std::min(rpc, m), batch, pipelined, &out[DNMF_DENSE_PLAN_B0_FULL], &out[DNMF_DENSE_PLAN_B0_TAIL]);
    chunk_trips(m - (long)(nchunks - 1) * rpc, batch, pipelined, &out[DNMF_DENSE_PLAN_BL_FULL], &out[DNMF_DENSE_PLAN_BL_TAIL]);
}
inline void report_reduce(long* out, const ReduceSel& r) {
    out[DNMF_DENSE_PLAN_REDUCE] = r.kind;
    out[DNMF_DENSE_PLAN_SLICES] = r.kind == REDUCE_TWO_STAGE ? r.ny : 0;
}
// the NT form: X nrows x ncols against Y yrows x ncols in `nsplit` column splits of `cps`.  The interior / window tests are the ones
// nt_mainloop and nt_mainloop_b16 (csrc/dnmf_nt.h) make per workgroup on the device, repeated here for every (row tile, split).
void report_nt(long* out, int mode, bool store_all, bool b16, bool fast, bool wfast, int k, long nrows, long ncols, long ldx, long ldy, long cps,
               int nsplit, long hblk) {
    const int tile = b16 ? 64 : 32;
    if (nt16_applies(k, fast, ncols, b16)) {
        out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_NT16;
        out[DNMF_DENSE_PLAN_KT] = 1; out[DNMF_DENSE_PLAN_FAST] = 1; out[DNMF_DENSE_PLAN_MODE] = mode;
        out[DNMF_DENSE_PLAN_GRID_X] = nt_grid_x(nrows); out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 256;
        out[DNMF_DENSE_PLAN_COUNT] = 1; out[DNMF_DENSE_PLAN_PER] = cps;
        out[DNMF_DENSE_PLAN_NK] = out[DNMF_DENSE_PLAN_AUX] = ncols / tile;
        out[DNMF_DENSE_PLAN_WFAST] = wfast;
        return;
    }
    const int kt = kt_of(k), kp = 32 * kt;
    const long rowtiles = nt_grid_x(nrows);
    const int pf = nt_pf(fast, mode, store_all, !b16, rowtiles * nsplit);
    out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_NT;
    out[DNMF_DENSE_PLAN_KT] = kt; out[DNMF_DENSE_PLAN_FAST] = fast; out[DNMF_DENSE_PLAN_MODE] = mode; out[DNMF_DENSE_PLAN_PF] = pf;
    out[DNMF_DENSE_PLAN_GRID_X] = rowtiles; out[DNMF_DENSE_PLAN_GRID_Y] = nsplit; out[DNMF_DENSE_PLAN_BLOCK] = 256;
    out[DNMF_DENSE_PLAN_COUNT] = nsplit; out[DNMF_DENSE_PLAN_PER] = cps;
    out[DNMF_DENSE_PLAN_WFAST] = wfast;
    long interior = 0, eligible = 0;
    for (int s = 0; s < nsplit; ++s) {
        const long cbeg = (long)s * cps, cend = std::min(cbeg + cps, ncols), w = cend - cbeg;
        if (s == 0) out[DNMF_DENSE_PLAN_NK] = cdiv(w, tile);
        if (s == nsplit - 1) out[DNMF_DENSE_PLAN_AUX] = cdiv(w, tile);
        if (!(fast && w % tile == 0 && (b16 || k >= kp))) continue;
        interior += nrows / nt_rows_per_tile(kt);
        const long yoff = hblk ? (cend - 1) / hblk * ((long)(k - 1) * hblk) : 0;
        const bool bufok = (nt_rows_per_tile(kt) * ldx + w) * 4 < 0x7fffffffL && ((long)kp * ldy + w + yoff) * 4 < 0x7fffffffL;
        if (bufok && (pf == 10 || pf == 13)) eligible += nrows / nt_rows_per_tile(kt);
    }
    out[DNMF_DENSE_PLAN_INTERIOR] = interior;
    out[DNMF_DENSE_PLAN_ELIGIBLE] = eligible;
}
}  // namespace

extern "C" int dnmf_dense_plan(int op, int bf16a, long m, long n, int k, const long* ld, const int* align, size_t ws_bytes, int ew_op,
                               long out[DNMF_DENSE_PLAN_LEN]) {
    REQUIRE(out && op >= DNMF_DENSE_OP_AHT && op <= DNMF_DENSE_OP_SQNORM && m >= 1 && n >= 1 && k >= 1 && k <= DNMF_MAX_K,
            "dense_plan: null output, unknown op or bad shape (op=%d m=%ld n=%ld k=%d)", op, m, n, k);
    for (int i = 0; i < DNMF_DENSE_PLAN_LEN; ++i) out[i] = 0;
    auto L = [&](int i, long packed) { return ld && ld[i] > 0 ? ld[i] : packed; };
    auto O = [&](int i) { return align ? (unsigned)(align[i] & 15) : 0u; };
    const size_t ea = bf16a ? 2 : 4;
    if (op == DNMF_DENSE_OP_EW) {                                    // a matrix of m rows and n columns; operands X, S, x
        REQUIRE(ew_op >= EW_CLAMP && ew_op <= EW_KL_BYCOL, "dense_plan: bad element-wise op %d", ew_op);
        const bool has_s = ew_op == EW_KL_BYROW || ew_op == EW_KL_BYCOL, has_x = ew_op != EW_CLAMP;
        const EwSel s = select_ew(ew_op, m, n, O(0), L(0, n), has_s, O(1), L(1, n), has_x, O(2));
        if (s.bad) return DNMF_OK;                                   // family NONE: the entry point refuses the shape
        out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_EW;
        out[DNMF_DENSE_PLAN_V] = s.vec ? 4 : 1; out[DNMF_DENSE_PLAN_MODE] = s.longrow; out[DNMF_DENSE_PLAN_NTEMP] = s.stream;
        out[DNMF_DENSE_PLAN_GRID_X] = s.gx; out[DNMF_DENSE_PLAN_GRID_Y] = s.gy; out[DNMF_DENSE_PLAN_BLOCK] = 256;
        out[DNMF_DENSE_PLAN_AUX] = s.txs;
        return DNMF_OK;
    }
    if (op == DNMF_DENSE_OP_SQNORM) {                                // operand A
        const SqnormSel s = select_sqnorm(m, n, ea, O(0), L(0, n));
        out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_SQNORM;
        out[DNMF_DENSE_PLAN_FAST] = s.fast; out[DNMF_DENSE_PLAN_GRID_X] = s.grid; out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 256;
        out[DNMF_DENSE_PLAN_AUX] = s.trips;
        return DNMF_OK;
    }
    if (wide_k(k)) {       // 128 < k <= 256: two panels of the tuned kernels (query k = 128 and k - 128) and the plain kernels of csrc/dnmf_wide.hip
        REQUIRE(op != DNMF_DENSE_OP_AHT_HBLOCKS && op != DNMF_DENSE_OP_AHT_UPDATE_W, "dense_plan: this entry point takes k <= %d", DNMF_TUNED_MAX_K);
        out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_WIDE;
        out[DNMF_DENSE_PLAN_COUNT] = (op == DNMF_DENSE_OP_GRAM_HHT || op == DNMF_DENSE_OP_GRAM_WTW) ? 4 : 2;
        out[DNMF_DENSE_PLAN_PER] = WIDE_PANEL;
        // the launch of the plain kernel the op runs besides (or, for the updates, instead of) its panel calls
        const bool rows_w = op == DNMF_DENSE_OP_MU_UPDATE_W;
        if (rows_w || op == DNMF_DENSE_OP_KL_UHT || op == DNMF_DENSE_OP_KL_WTU || op == DNMF_DENSE_OP_RESID_SQNORM ||
            op == DNMF_DENSE_OP_COLUMN_ERR) {                       // wide_nn_rows_kernel: W G over the k columns, or W H over the n columns of A
            const WideRowsGrid g = wide_rows_grid(rows_w, m, rows_w ? k : n);
            out[DNMF_DENSE_PLAN_GRID_X] = g.gx; out[DNMF_DENSE_PLAN_GRID_Y] = g.gy; out[DNMF_DENSE_PLAN_BLOCK] = 256;
            out[DNMF_DENSE_PLAN_AUX] = cdiv(g.cpw, 16);
        } else if (op == DNMF_DENSE_OP_MU_UPDATE_H) {               // wide_upd_h_kernel
            out[DNMF_DENSE_PLAN_GRID_X] = wide_upd_h_grid(n); out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 256;
            out[DNMF_DENSE_PLAN_AUX] = cdiv(k, 16);
        }
        return DNMF_OK;
    }
    const int kt = kt_of(k), kp = 32 * kt;
    if (op >= DNMF_DENSE_OP_KL_UHT) {                                // operands A, W, H, out: csrc/dnmf_kl.hip answers
        const long lds4[4] = {L(0, n), L(1, k), L(2, n), L(3, op == DNMF_DENSE_OP_KL_WTU ? n : k)};
        const unsigned offs4[4] = {O(0), O(1), O(2), O(3)};
        return dnmf_dense_plan_kl_(op, bf16a, m, n, k, lds4, offs4, ws_bytes, out);
    }
    switch (op) {
    case DNMF_DENSE_OP_AHT: case DNMF_DENSE_OP_AHT_HBLOCKS: case DNMF_DENSE_OP_AHT_UPDATE_W: {      // operands A, H, W (the fused form)
        const bool blocks = op == DNMF_DENSE_OP_AHT_HBLOCKS;
        REQUIRE(!(blocks && bf16a), "dense_plan: aht_hblocks takes float32 data");
        const long lda = L(0, n), ldh = L(1, n), hblk = blocks ? ldh : 0;
        REQUIRE(!blocks || (n % hblk == 0 && hblk % BK == 0), "dense_plan: bad H layout (block %ld, n %ld)", hblk, n);
        const bool fused = op == DNMF_DENSE_OP_AHT_UPDATE_W;
        report_nt(out, fused ? NT_FUSED_W : NT_STORE, false, bf16a != 0, nt_fast(O(0), lda, ea, O(1), ldh, n), fused && vec4(O(2), L(2, k), k), k, m, n,
                  lda, ldh, round_up(n, BK), 1, hblk);
        break;
    }
    case DNMF_DENSE_OP_GRAM_HHT: {                                   // operand H (k x n)
        const long ldh = L(0, n);
        const SplitPlan sp = plan_gram_nt(n);
        report_nt(out, NT_STORE, true, false, nt_fast(O(0), ldh, sizeof(float), O(0), ldh, n), false, k, k, n, ldh, ldh, sp.cols_per_split, sp.nsplit, 0);
        report_reduce(out, select_reduce(reduce_shape_gram(nt_rows_per_tile(kt) * kp, kp, sp.nsplit, k, kp), 0, 0, kp));
        break;
    }
    case DNMF_DENSE_OP_GRAM_WTW: {                                   // operand W (m x k)
        const GramWtwSel s = select_gram_wtw(m, k, kt, O(0), L(0, k), ws_bytes);
        if (s.ews) break;
        out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_TN;
        out[DNMF_DENSE_PLAN_KT] = kt; out[DNMF_DENSE_PLAN_FAST] = s.fast; out[DNMF_DENSE_PLAN_NT] = s.nt; out[DNMF_DENSE_PLAN_NTEMP] = 0;
        out[DNMF_DENSE_PLAN_GRID_X] = tn_grid(s.p.nchunks, s.p.ncolblk); out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 256;
        report_chunks(out, m, s.p.rows_per_chunk, s.p.nchunks, 8, s.fast);
        report_reduce(out, select_reduce(reduce_shape_gram(s.p.chunk_stride, s.p.ldp, s.p.nchunks, k, kp), 0, 0, kp));
        break;
    }
    case DNMF_DENSE_OP_WTA: case DNMF_DENSE_OP_WTA_GRAM: {           // operands A, W, AtW
        const WtaSel s = select_wta(m, n, k, kt, ea, O(0), L(0, n), O(1), L(1, k), ws_bytes, op == DNMF_DENSE_OP_WTA_GRAM);
        if (s.fam == WTA_EWS) break;
        const long ldatw = L(2, n);
        if (s.fam == WTA_TN16) {
            out[DNMF_DENSE_PLAN_FAMILY] = s.ride ? DNMF_DENSE_FAM_TN16_GRAM : DNMF_DENSE_FAM_TN16;
            out[DNMF_DENSE_PLAN_KT] = 1; out[DNMF_DENSE_PLAN_FAST] = 1; out[DNMF_DENSE_PLAN_V] = bf16a ? 8 : 4; out[DNMF_DENSE_PLAN_NTEMP] = 1;
            out[DNMF_DENSE_PLAN_GRID_X] = tn_grid(s.q.nchunks, s.q.ncolblk); out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 256;
            report_chunks(out, m, s.q.rows_per_chunk, s.q.nchunks, 16, true);
            report_reduce(out, select_reduce(reduce_shape_wta16(s.q, k, n), 0, O(2), ldatw));
        } else {
            out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_TN;
            out[DNMF_DENSE_PLAN_KT] = kt; out[DNMF_DENSE_PLAN_FAST] = s.fast; out[DNMF_DENSE_PLAN_NT] = s.nt; out[DNMF_DENSE_PLAN_NTEMP] = s.fast;
            out[DNMF_DENSE_PLAN_GRID_X] = tn_grid(s.p.nchunks, s.p.ncolblk); out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 256;
            report_chunks(out, m, s.p.rows_per_chunk, s.p.nchunks, 8, s.fast);
            report_reduce(out, select_reduce(reduce_shape_wta(s.p, k, n), 0, O(2), ldatw));
        }
        break;
    }
    case DNMF_DENSE_OP_MU_UPDATE_W: {                                // operands W, AH (m x k; n ignored)
        const long ldw = L(0, k), ldah = L(1, k);
        if (!update_w_pitch_ok(ldw, ldah)) break;
        const UpdWSel s = select_update_w(m, k, kt, O(0), ldw, O(1), ldah);
        out[DNMF_DENSE_PLAN_FAMILY] = s.w16 ? DNMF_DENSE_FAM_UPDATE_W16 : DNMF_DENSE_FAM_UPDATE_W_SEQ;
        out[DNMF_DENSE_PLAN_KT] = kt; out[DNMF_DENSE_PLAN_FAST] = s.v == 4; out[DNMF_DENSE_PLAN_V] = s.v; out[DNMF_DENSE_PLAN_EDGE] = s.edge;
        out[DNMF_DENSE_PLAN_OCC] = s.occ;
        out[DNMF_DENSE_PLAN_GRID_X] = s.grid; out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 64 * s.nwv;
        out[DNMF_DENSE_PLAN_COUNT] = s.tiles; out[DNMF_DENSE_PLAN_PER] = s.w16 ? 16 : 32;
        out[DNMF_DENSE_PLAN_AUX] = cdiv(s.tiles, (long)s.grid * s.nwv);
        break;
    }
    case DNMF_DENSE_OP_MU_UPDATE_H: {                                // operands H, AtW (k x n; m ignored)
        const long ldh = L(0, n), ldatw = L(1, n);
        if (!update_h_pitch_ok(ldh, ldatw)) break;
        const UpdHSel s = select_update_h(k, n, kt, O(0), ldh, O(1), ldatw);
        out[DNMF_DENSE_PLAN_FAMILY] = DNMF_DENSE_FAM_UPDATE_H_SEQ;
        out[DNMF_DENSE_PLAN_KT] = kt; out[DNMF_DENSE_PLAN_NT] = s.nt; out[DNMF_DENSE_PLAN_EDGE] = s.edge; out[DNMF_DENSE_PLAN_NTEMP] = s.nontemporal;
        out[DNMF_DENSE_PLAN_OCC] = s.occ;
        out[DNMF_DENSE_PLAN_GRID_X] = s.grid; out[DNMF_DENSE_PLAN_GRID_Y] = 1; out[DNMF_DENSE_PLAN_BLOCK] = 64 * upd_waves(kt);
        out[DNMF_DENSE_PLAN_COUNT] = s.tiles; out[DNMF_DENSE_PLAN_PER] = 32 * s.nt;
        out[DNMF_DENSE_PLAN_AUX] = cdiv(s.tiles, (long)s.grid * upd_waves(kt));
        break;
    }
    default: break;
    }
    return DNMF_OK;
}

// Every variant the selectors can return: each selector is called over its whole discrete input domain (every rank tile, both
// alignments, both sides of each of its thresholds) and what it answers is written as one row {family, KT, FAST, MODE, PF, NT, V, EDGE,
// NTEMP, bf16 A}; rows repeat.  Returns the number of rows (at most `cap` are written).  tests/test_dense_plan.py holds the reach table
// of the exact tests against this list.
extern "C" int dnmf_dense_plan_variants(long* rows, int cap) {
    int nrows = 0;
    auto emit = [&](long fam, long kt, long fast, long mode, long pf, long nt, long v, long edge, long ntemp, long b16) {
        const long r[DNMF_DENSE_VARIANT_LEN] = {fam, kt, fast, mode, pf, nt, v, edge, ntemp, b16};
        if (rows && nrows < cap) for (int i = 0; i < DNMF_DENSE_VARIANT_LEN; ++i) rows[(long)nrows * DNMF_DENSE_VARIANT_LEN + i] = r[i];
        ++nrows;
    };
    for (int b16 = 0; b16 < 2; ++b16)                                 // k = 16: the 16-wide kernels where their predicates take them
        for (int fast = 0; fast < 2; ++fast) {
            for (int mode = NT_STORE; mode <= NT_FUSED_W; ++mode)
                for (long n : {128L, 100L})
                    if (nt16_applies(16, fast != 0, n, b16 != 0)) emit(DNMF_DENSE_FAM_NT16, 1, 1, mode, 0, 0, 0, 0, 0, b16);
            for (int gram = 0; gram < 2; ++gram)
                for (size_t wsb : {(size_t)2 * 16 * 128 * 4, ~size_t(0)}) {            // the slabs alone; room for the riding Gram
                    const WtaSel s = select_wta(300, 128, 16, 1, b16 ? 2 : 4, fast ? 0 : 4, 136, 0, 20, wsb, gram != 0);
                    if (s.fam == WTA_TN16) emit(s.ride ? DNMF_DENSE_FAM_TN16_GRAM : DNMF_DENSE_FAM_TN16, 1, 1, 0, 0, 0, b16 ? 8 : 4, 0, 1, b16);
                }
        }
    for (int kt : {1, 2, 4}) {
        const int kp = 32 * kt;
        for (int fast = 0; fast < 2; ++fast) {
            for (int b16 = 0; b16 < 2; ++b16)
                for (int mode = NT_STORE; mode <= NT_FUSED_W; ++mode)
                    for (int store_all = 0; store_all < (mode == NT_STORE && !b16 ? 2 : 1); ++store_all)       // (store_all: H H^T, float32)
                        for (long wgs : {256L, 257L}) emit(DNMF_DENSE_FAM_NT, kt, fast, mode, nt_pf(fast, mode, store_all, !b16, wgs), 0, 0, 0, 0, b16);
            const unsigned off = fast ? 0 : 4;
            for (size_t ea : {(size_t)4, (size_t)2}) {
                const WtaSel s = select_wta(300, 132, kp, kt, ea, off, 136, off, kp + 4, ~size_t(0), false);
                emit(DNMF_DENSE_FAM_TN, kt, s.fast, 0, 0, s.nt, 0, 0, s.fast, ea == 2);
            }
            const GramWtwSel g = select_gram_wtw(300, kp, kt, off, kp + 4, ~size_t(0));
            emit(DNMF_DENSE_FAM_TN, kt, g.fast, 0, 0, g.nt, 0, 0, 0, 0);
            for (int k : {kp, kp - 4})
                for (long m : {64L, 48L, 40L}) {                      // whole 32-row tiles, whole 16-row tiles, neither
                    const UpdWSel s = select_update_w(m, k, kt, off, kp + 4, off, kp + 4);
                    emit(s.w16 ? DNMF_DENSE_FAM_UPDATE_W16 : DNMF_DENSE_FAM_UPDATE_W_SEQ, kt, s.v == 4, 0, 0, 0, s.v, s.edge, 0, 0);
                }
            for (int k : {kp, kp - 4})
                for (long n : {96L, 100L, 65536L, 65536L + 32, (long)(64.0 * (1 << 20) / (4 * kp))}) {      // NT = 1 whole / ragged; NT = 2; 64 MiB
                    const UpdHSel s = select_update_h(k, n, kt, off, n + 4, off, n + 4);
                    emit(DNMF_DENSE_FAM_UPDATE_H_SEQ, kt, 0, 0, 0, s.nt, 0, s.edge, s.nontemporal, 0);
                }
        }
    }
    for (unsigned off : {0u, 4u})
        for (long rows_ : {10L, 1000L, 16384L, 65536L})
            for (long cols : {2000L, 40L, 4096L, 1024L}) {
                const EwSel s = select_ew(EW_CLAMP, rows_, cols, off, cols + 4, false, 0, 0, false, 0);
                if (!s.bad) emit(DNMF_DENSE_FAM_EW, 0, 0, s.longrow, 0, 0, s.vec ? 4 : 1, 0, s.stream, 0);
            }
    for (int b16 = 0; b16 < 2; ++b16)
        for (unsigned off : {0u, 4u}) emit(DNMF_DENSE_FAM_SQNORM, 0, select_sqnorm(100, 64, b16 ? 2 : 4, off, 68).fast, 0, 0, 0, 0, 0, 0, b16);
    return dnmf_dense_variants_kl_(rows, cap, nrows);                 // the KL products, the residual, the per-column error
}
