// dnmf_fit.hip -- whole fits on one rank: `itr` update steps, the final normalisation and the two squared norms of the
// relative error in ONE library call, for one problem or for a batch of same-shape problems (blockIdx.z = problem).
// Replaces the Python loop of PyNMF.fit (reference pyDNMF.py:138-182 with p_r = p_c = 1) and, batched, the sequential
// perturbation fits of an NMFk sweep (reference pyDNMFk.py:226-231).  No kernel of its own: every launch below is a launch
// of the per-step entry points, in the order the per-step callers issue them -- problem z of a batch runs the instructions
// a single fit runs, on the same operands (csrc/dnmf_common.h "batched launches").
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_small.h"
#include <atomic>

// csrc/dnmf.hip: offsets of the step workspace {G, S, x, partials, total}
__attribute__((visibility("hidden"))) void dnmf_ws_offsets_(long m, long n, int k, size_t out[5]);

namespace {

enum { FIT_MU_FRO = 0, FIT_MU_KL = 1, FIT_HALS_FRO = 2 };

inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

// The persistent small-problem fits (csrc/dnmf_small.h): which shapes take them, with what geometry and workspace.  k <= 32, n <= 4096;
// all of H + the slab's W (+ the slab of A when that fits) in the 160 KiB of LDS of a CU, 8-wave workgroups = 128-row slabs when that fits,
// else 4-wave = 64-row, at most 64 slabs per problem -- in practice n up to ~500 columns and m up to 8192 rows: the reference's example sizes.
enum { ROUTE_NONE = 0, ROUTE_BARRIER = 1, ROUTE_WFIXED = 2, ROUTE_HALS = 3 };
enum { FAM_KL = 0, FAM_FRO = 1, FAM_WFIXED = 2, FAM_HALS = 3 };             // the launch counters (dnmf_small_fit_launches)
constexpr size_t SMALL_LDS_MAX = 160 * 1024;
constexpr int HFIT_NW = 8;                                                  // waves of the W-fixed MU/KL kernel (small_kl_hfit_kernel)

// What a whole fit takes, from the shape alone: everything dnmf_small_fit_plan reports and everything small_launch needs.  All zero: route 0.
struct SmallPlan {
    int route, family, kp, nw, P, cw;
    bool alds, bf16_resident;
    long ns;
    size_t lds;                                  // dynamic LDS of the kernel chosen
    size_t part_floats, slot_words, bytes;       // workspace: partials | slots (HALS) | granules of H | arrival counter
};

// The geometry families: their {NW, A in LDS} tries in order of preference, their LDS function, and whether they have the slots and the
// column share cw = ceil(ns / P) of the HALS sweep.
//   MU on fp32 A (KL and FRO alike: FRO takes the KL geometry and the KL size): 128-row slabs with A in LDS when that fits; else 96-row
//     slabs with A in LDS (round 6: at 16 < k <= 32 the 1024 x 256 examples keep A on chip this way, and 20 problems x 11 slabs cover 220
//     of the 256 CUs where 8 slabs covered 160); else 128-row slabs with A streamed from the L2; else 64-row slabs with A in LDS, or
//     streamed (short, wide problems)
//   MU/FRO on bf16-stored A (params.precision = 'bfloat16'): the slab is half the size, it fits LDS where the fp32 one streams
//   HALS: A streamed, LDS holds H, the slab's W, the Gram matrix and the workgroup's share of W^T A; the geometry never depends on the
//     storage of A, only where A is read from (small_plan)
struct SmallTry { int nw; bool alds; };
struct SmallGeometry { SmallTry tries[5]; int ntries; size_t (*lds)(int kp, int nw, long n, bool alds, int cw); bool slots; };
enum { GEO_MU = 0, GEO_MU_BF16 = 1, GEO_HALS = 2 };
const SmallGeometry SMALL_GEOMETRIES[3] = {
    {{{8, true}, {6, true}, {8, false}, {4, true}, {4, false}}, 5, [](int kp, int nw, long n, bool alds, int) { return small_kl_lds(kp, nw, n, alds); }, false},
    {{{8, true}, {8, false}, {4, true}, {4, false}}, 4, [](int kp, int nw, long n, bool alds, int) { return small_fro_lds(kp, nw, n, alds, 2); }, false},
    {{{8, false}, {4, false}}, 2, [](int kp, int nw, long n, bool, int cw) { return small_hals_lds(kp, nw, n, cw, 0); }, true},
};

// geometry by shape alone (a batched fit must equal single fits bit for bit): the first try that fits the LDS in at most 64 slabs -- 8- and
// 6-wave workgroups only where that makes two slabs or more -- and the workspace layout that goes with it.  nw == 0: none
SmallPlan small_geometry(int geo, long m, long n, int k) {
    SmallPlan s{};
    if (m < 1 || n < 1 || k < 1 || k > 32 || n > 4096) return s;
    const SmallGeometry& g = SMALL_GEOMETRIES[geo];
    const int kp = k <= 16 ? 16 : 32;
    const long ns = round_up(n, 16);
    for (int i = 0; i < g.ntries; ++i) {
        const SmallTry t = g.tries[i];
        const long P = cdiv(m, 16L * t.nw);
        const int cw = g.slots ? (int)cdiv(ns, P) : 0;
        const size_t lds = g.lds(kp, t.nw, n, t.alds, cw);
        if (lds > SMALL_LDS_MAX || P > 64 || (t.nw != 4 && P < 2)) continue;
        s.kp = kp; s.nw = t.nw; s.P = (int)P; s.cw = cw; s.alds = t.alds; s.ns = ns; s.lds = lds;
        // W^T U / W^T A partials + (KL) column sums or (FRO, HALS) W^T W per slab; the slots and the granules {element, step} of H behind
        // them 16-byte aligned; the arrival counter in a 256-byte block of its own
        s.part_floats = ((size_t)P * kp * ns + (size_t)P * kp * kp + 3) & ~size_t(3);
        s.slot_words = g.slots ? ((size_t)2 * kp * P + 3) & ~size_t(3) : 0;
        s.bytes = al256((s.part_floats + s.slot_words + 2 * (size_t)kp * ns) * sizeof(float)) + 256;
        break;
    }
    return s;
}

// the small area of the fit workspace serves whichever family the fit call turns out to be
size_t small_area_bytes(long m, long n, int k) {
    return std::max(std::max(small_geometry(GEO_MU, m, n, k).bytes, small_geometry(GEO_HALS, m, n, k).bytes), small_geometry(GEO_MU_BF16, m, n, k).bytes);
}

// Which persistent kernel a whole fit takes: computed once per fit by fit_impl, and what dnmf_small_fit_plan reports.
SmallPlan small_plan(int method, bool bf, int w_update, long m, long n, int k) {
    if (method != FIT_MU_KL && method != FIT_MU_FRO && method != FIT_HALS_FRO) return SmallPlan{};
    // MU/KL reads fp32 A only; the Frobenius updates with W fixed: the hoisted H-only loop of fit_impl is the better path
    if (method == FIT_MU_KL ? bf : !w_update) return SmallPlan{};
    SmallPlan p = small_geometry(method == FIT_HALS_FRO ? GEO_HALS : bf ? GEO_MU_BF16 : GEO_MU, m, n, k);
    if (!p.nw) return SmallPlan{};
    if (method == FIT_HALS_FRO) {
        const size_t resident = small_hals_lds(p.kp, p.nw, n, p.cw, 2);         // with the bf16 slab of A in LDS
        p.route = ROUTE_HALS; p.family = FAM_HALS;
        p.alds = p.bf16_resident = bf && resident <= SMALL_LDS_MAX;
        if (p.bf16_resident) p.lds = resident;
    } else if (method == FIT_MU_KL && !w_update && small_kl_hfit_lds(p.kp, HFIT_NW, m) <= SMALL_LDS_MAX) {
        // the W-fixed MU/KL kernel keeps ALL of W in LDS: taken when that fits (else the barrier kernel runs with w_update = 0); a workgroup
        // per 16 columns, A streamed.  The workspace layout stays that of the barrier geometry: the kernel touches none of it
        p.route = ROUTE_WFIXED; p.family = FAM_WFIXED;
        p.nw = HFIT_NW; p.P = (int)(p.ns / 16); p.alds = false; p.lds = small_kl_hfit_lds(p.kp, HFIT_NW, m);
    } else {
        p.route = ROUTE_BARRIER; p.family = method == FIT_MU_FRO ? FAM_FRO : FAM_KL;
    }
    return p;
}

// kernel launches of the persistent small fits that were TAKEN, per family (host side; dnmf_small_fit_launches)
std::atomic<unsigned long long> g_small_launches[4];

// per-problem workspace: [ step workspace | s: KP floats (column sums of W) | ss2: KP doubles | sq: 2 doubles | small-fit partials ]
struct FitWs { size_t g_off, s_off, part_off, step_total, cs_off, ss2_off, sq_off, small_off, total; };

FitWs fit_layout(long m, long n, int k) {
    size_t o[5];
    dnmf_ws_offsets_(m, n, k, o);
    const int kp = dnmf_kp(k);
    FitWs f;
    f.g_off = o[0]; f.s_off = o[1]; f.part_off = o[3];
    // the partial area also serves the calls made on the factor alone (the persistent HALS W sweep and the column sums of W ask
    // for dnmf_ws_bytes(m, k, k))
    f.step_total = std::max(o[4], o[3] + al256(dnmf_ws_bytes(m, k, k)));
    f.cs_off = al256(f.step_total);
    f.ss2_off = f.cs_off + al256((size_t)kp * sizeof(float));
    f.sq_off = f.ss2_off + al256((size_t)kp * sizeof(double));
    f.small_off = f.sq_off + 256;
    f.total = f.small_off + small_area_bytes(m, n, k);
    return f;
}

inline bool wide_fit_k(int k) { return k > DNMF_TUNED_MAX_K; }

template <bool BF>
int hals_step(const void* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
              int clamp, int column_sweep, char* ws, const FitWs& f, void* stream) {
    float* G = (float*)(ws + f.g_off);
    float* Sb = (float*)(ws + f.s_off);
    void* part = ws + f.part_off;
    const size_t part_bytes = f.step_total - f.part_off;
    int rc;
    if (w_update) {                                                                   // FRO_HALS_update_W, dist_nmf.py:873-891
        if ((rc = dnmf_gram_hht(H, k, n, ldh, G, part, part_bytes, stream))) return rc;                  // :882
        if ((rc = BF ? dnmf_aht_bf16a(A, m, n, lda, H, k, ldh, Sb, k, stream)
                     : dnmf_aht((const float*)A, m, n, lda, H, k, ldh, Sb, k, stream))) return rc;       // :883
        if (column_sweep) rc = dnmf_hals_update_w(W, m, k, ldw, Sb, k, G, eps, (double*)(ws + f.ss2_off), stream);
        else rc = dnmf_hals_sweep_w(W, m, k, ldw, Sb, k, G, eps, part, part_bytes, stream);              // :884-891
        if (rc) return rc;
    }
    if ((rc = BF ? dnmf_wta_gram_bf16a(A, m, n, lda, W, k, ldw, Sb, n, G, part, part_bytes, stream)      // :902-903
                 : dnmf_wta_gram((const float*)A, m, n, lda, W, k, ldw, Sb, n, G, part, part_bytes, stream))) return rc;
    if ((rc = dnmf_hals_update_h(H, k, n, ldh, Sb, n, G, eps, stream))) return rc;                       // :905-909
    if (clamp) {                                                                                         // pyDNMF.py:170-172
        if ((rc = dnmf_clamp_min(H, k, n, ldh, eps, stream))) return rc;
        return dnmf_clamp_min(W, m, k, ldw, eps, stream);
    }
    return DNMF_OK;
}

unsigned long long g_small_patience = 200000000ull;

// a launch (or as few as keep every workgroup resident) of a persistent small-fit kernel
int resident_launch(void (*kern)(SmallKlArgs), int threads, size_t lds, int P, SmallKlArgs a, int batch, hipStream_t st, bool* taken, const char* what, int family) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        return fail(DNMF_EHIP, "small fit: cannot raise the dynamic LDS limit");
    int nb = 0, dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return fail(DNMF_EHIP, "small fit: device query failed");
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, lds) != hipSuccess || nb < 1) { clear_hip_error(); return DNMF_OK; }
    const long cap = (long)nb * cus;
    if (cap < P) return DNMF_OK;
    const int per_launch = (int)std::min<long>(batch, cap / P);
    const int each = (int)cdiv(batch, cdiv(batch, per_launch));
    unsigned long long launches = 0;
    for (int z0 = 0; z0 < batch; z0 += each) {
        a.z0 = z0;
        hipLaunchKernelGGL(kern, dim3((unsigned)P, 1, (unsigned)std::min(each, batch - z0)), dim3(threads), lds, st, a);
        const int rc = check_launch(what);
        if (rc) return rc;
        ++launches;
    }
    g_small_launches[family] += launches;
    *taken = true;
    return DNMF_OK;
}

// the kernel of a plan: the ONE place that names the 42 instantiations
struct SmallKernel { void (*fn)(SmallKlArgs); const char* name; };
template <int KP, int NW, bool ALDS>
SmallKernel small_kernel_at(int family, bool bf) {
    if (family == FAM_KL) return {small_kl_fit_kernel<KP, NW, ALDS>, "small_kl_fit_kernel"};
    if (family == FAM_FRO && !bf) return {small_fro_fit_kernel<KP, NW, ALDS, float>, "small_fro_fit_kernel"};
    if constexpr (NW != 6) {                               // (96-row slabs: MU on fp32 A only)
        if (family == FAM_FRO) return {small_fro_fit_kernel<KP, NW, ALDS, bf16_t>, "small_fro_fit_kernel(bf16)"};
        if constexpr (ALDS) {                              // HALS: ALDS == bf16_resident, fp32 A is always streamed
            if (family == FAM_HALS) return {small_hals_fit_kernel<KP, NW, bf16_t, true>, "small_hals_fit_kernel"};
        } else {
            if (family == FAM_HALS) return {bf ? small_hals_fit_kernel<KP, NW, bf16_t, false> : small_hals_fit_kernel<KP, NW, float, false>, "small_hals_fit_kernel"};
            if constexpr (NW == HFIT_NW)
                if (family == FAM_WFIXED) return {small_kl_hfit_kernel<KP, NW>, "small_kl_hfit_kernel"};
        }
    }
    return {nullptr, nullptr};
}
SmallKernel small_kernel(const SmallPlan& p, bool bf) {
#define SMALL_CASE(KP_, NW_, AL_) \
    if (p.kp == KP_ && p.nw == NW_ && p.alds == AL_) return small_kernel_at<KP_, NW_, AL_>(p.family, bf)
    SMALL_CASE(16, 8, true); SMALL_CASE(16, 6, true); SMALL_CASE(16, 8, false); SMALL_CASE(16, 4, true); SMALL_CASE(16, 4, false);
    SMALL_CASE(32, 8, true); SMALL_CASE(32, 6, true); SMALL_CASE(32, 8, false); SMALL_CASE(32, 4, true); SMALL_CASE(32, 4, false);
#undef SMALL_CASE
    return {nullptr, nullptr};
}

// all `itr` steps of `batch` small problems on the persistent kernel of the plan (csrc/dnmf_small.h): the barrier and HALS kernels as few
// launches as keep every workgroup of a launch resident at once
int small_launch(const SmallPlan& p, bool bf, const void* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
                 int itr, int batch, long a_stride, long w_stride, long h_stride, char* ws, const FitWs& f, void* stream, bool* taken) {
    *taken = false;
    const SmallKernel kern = small_kernel(p, bf);
    if (!p.route || !kern.fn || itr < 1) return DNMF_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    SmallKlArgs a{};
    a.A = (const float*)A; a.lda = lda; a.a_stride = a_stride; a.W = W; a.ldw = ldw; a.w_stride = w_stride; a.H = H; a.ldh = ldh; a.h_stride = h_stride;
    a.m = (int)m; a.n = (int)n; a.k = k; a.eps = eps; a.itr = itr; a.w_update = w_update; a.cw = p.cw;
    a.part = (float*)(ws + f.small_off); a.part_stride = (long)(f.total / sizeof(float));
    a.bar = (unsigned*)(ws + f.small_off + p.bytes - 256); a.bar_stride = (long)(f.total / sizeof(unsigned));
    a.hg = a.part + p.part_floats + p.slot_words; a.hg_stride = a.part_stride;      // [kp][ns] granules {H element, step}: zeroed below
    a.patience = g_small_patience;                                     // ticks of the 100 MHz wall clock (2 s unless dnmf_fit_set_timeout)
    if (batch == 1) { a.a_stride = a.w_stride = a.h_stride = 0; }
    if (p.route == ROUTE_WFIXED) {
        // W fixed: the columns of H are independent -- a workgroup per 16 columns, no barrier, nothing to keep resident and nothing to zero
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern.fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return fail(DNMF_EHIP, "small fit: cannot raise the dynamic LDS limit");
        hipLaunchKernelGGL(kern.fn, dim3((unsigned)p.P, 1, (unsigned)batch), dim3(64 * p.nw), p.lds, st, a);
        const int rc = check_launch(kern.name);
        if (!rc) { ++g_small_launches[p.family]; *taken = true; }
        return rc;
    }
    bool zeroed = hipMemset2DAsync(a.bar, f.total, 0, 2 * sizeof(unsigned), (size_t)batch, st) == hipSuccess &&
                  hipMemset2DAsync(a.hg, f.total, 0, 2 * (size_t)p.kp * p.ns * sizeof(float), (size_t)batch, st) == hipSuccess;
    if (p.route == ROUTE_HALS) {                                       // the column-norm slots of the W sweep, all SLOT_EMPTY
        a.slots = (unsigned*)a.part + p.part_floats; a.slots_stride = a.bar_stride;
        zeroed = zeroed && hipMemset2DAsync(a.slots, f.total, 0xff, p.slot_words * sizeof(unsigned), (size_t)batch, st) == hipSuccess;
    }
    if (!zeroed) return fail(DNMF_EHIP, "small fit: memset failed");
    return resident_launch(kern.fn, 64 * p.nw, p.lds, p.P, a, batch, st, taken, kern.name, p.family);
}

int fit_impl(int method, bool bf, const void* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps,
             int w_update, int itr, int column_sweep, int batch, long a_stride, long w_stride, long h_stride, double* sq_out,
             void* ws, size_t ws_bytes, void* stream) {
    REQUIRE_WS16(ws, "fit");
    const int kp = dnmf_kp(k);
    if (kp < 0 || !A || !W || !H || !sq_out || !ws || m < 1 || n < 1 || itr < 0 || batch < 1 || lda < n || ldw < k || ldh < n)
        return fail(DNMF_EINVAL, "fit: bad arguments (m=%ld n=%ld k=%d itr=%d batch=%d)", m, n, k, itr, batch);
    if (bf && method == FIT_MU_KL) return fail(DNMF_EINVAL, "fit: bfloat16 storage of A is for the Frobenius updates");
    const FitWs f = fit_layout(m, n, k);
    if (ws_bytes < (size_t)batch * f.total) return fail(DNMF_EWS, "fit: workspace %zu < %d x %zu", ws_bytes, batch, f.total);
    BatchCtx* ctx = dnmf_batch_();
    if (ctx->B != 1) return fail(DNMF_EINVAL, "fit: called inside a batched fit");
    BatchGuard guard(ctx);
    const size_t ea = bf ? 2 : 4;
    // (the family set-up and the guard: csrc/dnmf_host.h)
    if (int frc = batch_families(ctx, "fit", batch, A, ea, m, n, lda, a_stride, W, ldw, w_stride, H, ldh, h_stride, k, ws, f.total)) return frc;
    char* base = (char*)ws;
    int rc = DNMF_OK;
    bool small = false;
    const bool pers = dnmf_persistent_on_() != 0;
    if (!pers) column_sweep = 1;                                       // (the HALS steps below take the column launches)
    // (column_sweep != 0, also set just above: the HALS fit takes the launch chain; the MU entry points pass 0)
    const SmallPlan plan = pers && !column_sweep ? small_plan(method, bf, w_update, m, n, k) : SmallPlan{};
    if (plan.route) {
        // small problems: the whole loop as one persistent kernel per batch (csrc/dnmf_small.h); launched unbatched -- it indexes the problems itself
        const int B = ctx->B;
        ctx->B = 1;
        rc = small_launch(plan, bf, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, batch, a_stride, w_stride, h_stride, base, f, stream, &small);
        ctx->B = B;
        if (rc) return rc;
        // (the W-fixed KL kernel leaves W alone; the clamp of pyDNMF.py:155 after step 0 is this launch)
        if (small && method == FIT_MU_KL && !w_update && (rc = dnmf_clamp_min(W, m, k, ldw, eps, stream))) return rc;
    }
    // W fixed (the regression fit of an NMFk sweep, pyDNMFk.py:243-247): the Frobenius H updates read A only through W^T A, and W^T A and
    // W^T W are loop invariants once W has been clamped (the clamp after step 0 is the only thing that can still change W; it is idempotent
    // from then on).  Steps 0 and 1 run in full -- step 1 leaves W^T A and W^T W of the final W in the workspace --, every later step is
    // the H update alone on those: the same values the step would recompute, so the same bits, without the two passes over A.
    const bool h_only = !w_update && method != FIT_MU_KL && !wide_fit_k(k);
    const long ldatw = method == FIT_MU_FRO ? round_up(n, 4) : n;
    for (int i = 0; i < itr && !rc && !small; ++i) {                                  // pyDNMF.py:151-172
        const int clamp = (i % 10 == 0);
        if (h_only && i >= 2) {
            float* G = (float*)(base + f.g_off);
            float* Sb = (float*)(base + f.s_off);
            if (method == FIT_MU_FRO) rc = dnmf_mu_update_h(H, k, n, ldh, Sb, ldatw, G, eps, clamp, stream);          // dist_nmf.py:750-751
            else {
                rc = dnmf_hals_update_h(H, k, n, ldh, Sb, ldatw, G, eps, stream);                                     // :905-909
                if (!rc && clamp) rc = dnmf_clamp_min(H, k, n, ldh, eps, stream);
            }
            continue;
        }
        if (method == FIT_MU_FRO)
            rc = bf ? dnmf_mu_fro_step_bf16a(A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, clamp, ws, f.step_total, stream)
                    : dnmf_mu_fro_step((const float*)A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, clamp, ws, f.step_total, stream);
        else if (method == FIT_MU_KL)
            rc = dnmf_mu_kl_step((const float*)A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, clamp, ws, f.step_total, stream);
        else
            rc = bf ? hals_step<true>(A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, clamp, column_sweep, base, f, stream)
                    : hals_step<false>(A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, clamp, column_sweep, base, f, stream);
    }
    if (rc) return rc;
    // normalize_features (pyDNMF.py:185-194): s = column sums of W; W /= s + eps; H *= s^T
    float* s = (float*)(base + f.cs_off);
    void* part = base + f.part_off;
    const size_t part_bytes = f.step_total - f.part_off;
    if ((rc = dnmf_colsum(W, m, k, ldw, s, part, part_bytes, stream))) return rc;
    if ((rc = dnmf_scale_cols_div(W, m, k, ldw, s, eps, stream))) return rc;
    if ((rc = dnmf_scale_rows_mul(H, k, n, ldh, s, stream))) return rc;
    // relative_err (pyDNMF.py:205-218): sum (A - W H)^2 and sum A^2; the caller takes the square roots
    double* sq = (double*)(base + f.sq_off);
    if ((rc = bf ? dnmf_resid_sqnorm_ws_bf16a(A, m, n, lda, W, ldw, H, ldh, k, sq, ws, f.step_total, stream)
                 : dnmf_resid_sqnorm_ws((const float*)A, m, n, lda, W, ldw, H, ldh, k, sq, ws, f.step_total, stream))) return rc;
    if ((rc = bf ? dnmf_sqnorm_bf16a(A, m, n, lda, sq + 1, stream) : dnmf_sqnorm((const float*)A, m, n, lda, sq + 1, stream))) return rc;
    if (hipMemcpy2DAsync(sq_out, 2 * sizeof(double), sq, f.total, 2 * sizeof(double), (size_t)batch, hipMemcpyDeviceToDevice,
                         reinterpret_cast<hipStream_t>(stream)) != hipSuccess)
        return fail(DNMF_EHIP, "fit: copy of the squared norms failed");
    return DNMF_OK;
}

}  // namespace

// read-and-clear of the persistent small fit's sticky time-out word (csrc/dnmf_hals.hip: dnmf_hals_sweep_status reports it with the sweep's)
__attribute__((visibility("hidden"))) int dnmf_small_timeout_take_(unsigned* out) {
    unsigned v = 0;
    const unsigned zero = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_small_timeout), sizeof(v), 0, hipMemcpyDeviceToHost) != hipSuccess) return DNMF_EHIP;
    if (v && hipMemcpyToSymbol(HIP_SYMBOL(g_small_timeout), &zero, sizeof(zero), 0, hipMemcpyHostToDevice) != hipSuccess) return DNMF_EHIP;
    *out = v;
    return DNMF_OK;
}

__attribute__((visibility("hidden"))) void dnmf_team_set_patience_(unsigned long long ticks);   // csrc/dnmf_team.hip

extern "C" {

int dnmf_fit_set_timeout(double seconds) {
    if (!(seconds > 0.0) || seconds > 3600.0) return fail(DNMF_EINVAL, "fit_set_timeout: %g s", seconds);
    g_small_patience = (unsigned long long)(seconds * 1e8) + 1ull;
    dnmf_team_set_patience_(g_small_patience);
    return DNMF_OK;
}

int dnmf_hals_fit_persistent(long m, long n, int k) {
    return (dnmf_persistent_on_() && small_geometry(GEO_HALS, m, n, k).nw) ? 1 : 0;
}

int dnmf_mu_fit_persistent(long m, long n, int k) {
    return (dnmf_persistent_on_() && small_geometry(GEO_MU, m, n, k).nw) ? 1 : 0;
}

int dnmf_small_fit_plan(int method, int bf16, int w_update, long m, long n, int k, int out[8]) {
    if (method != FIT_MU_FRO && method != FIT_MU_KL && method != FIT_HALS_FRO) return fail(DNMF_EINVAL, "small_fit_plan: method %d (0 mu-fro, 1 mu-kl, 2 hals-fro)", method);
    if (bf16 && method == FIT_MU_KL) return fail(DNMF_EINVAL, "small_fit_plan: bfloat16 storage of A is for the Frobenius updates");
    if (!out || m < 1 || n < 1 || k < 1 || k > 32) return fail(DNMF_EINVAL, "small_fit_plan: null pointer or bad shape (m=%ld n=%ld k=%d; 1 <= k <= 32)", m, n, k);
    const SmallPlan r = small_plan(method, bf16 != 0, w_update, m, n, k);
    out[0] = r.route; out[1] = r.kp; out[2] = r.nw; out[3] = r.alds ? 1 : 0; out[4] = r.P; out[5] = (int)r.ns; out[6] = r.cw; out[7] = r.bf16_resident ? 1 : 0;
    return DNMF_OK;
}

int dnmf_small_fit_launches(unsigned long long out[4]) {
    if (!out) return fail(DNMF_EINVAL, "small_fit_launches: null pointer");
    for (int i = 0; i < 4; ++i) out[i] = g_small_launches[i].load();
    return DNMF_OK;
}

size_t dnmf_ws_bytes_fit(long m, long n, int k, int batch) {
    if (dnmf_kp(k) < 0 || m < 1 || n < 1 || batch < 1) return 0;
    return (size_t)batch * fit_layout(m, n, k).total;
}

int dnmf_mu_fro_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
                    int itr, int batch, long a_stride, long w_stride, long h_stride, double* sq_out, void* ws, size_t ws_bytes,
                    void* stream) {
    return fit_impl(FIT_MU_FRO, false, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, 0, batch, a_stride, w_stride, h_stride,
                    sq_out, ws, ws_bytes, stream);
}
int dnmf_mu_fro_fit_bf16a(const void* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps,
                          int w_update, int itr, int batch, long a_stride, long w_stride, long h_stride, double* sq_out, void* ws,
                          size_t ws_bytes, void* stream) {
    return fit_impl(FIT_MU_FRO, true, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, 0, batch, a_stride, w_stride, h_stride,
                    sq_out, ws, ws_bytes, stream);
}
int dnmf_mu_kl_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps, int w_update,
                   int itr, int batch, long a_stride, long w_stride, long h_stride, double* sq_out, void* ws, size_t ws_bytes,
                   void* stream) {
    return fit_impl(FIT_MU_KL, false, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, 0, batch, a_stride, w_stride, h_stride,
                    sq_out, ws, ws_bytes, stream);
}
int dnmf_hals_fro_fit(const float* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps,
                      int w_update, int itr, int column_sweep, int batch, long a_stride, long w_stride, long h_stride, double* sq_out,
                      void* ws, size_t ws_bytes, void* stream) {
    return fit_impl(FIT_HALS_FRO, false, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, column_sweep, batch, a_stride, w_stride,
                    h_stride, sq_out, ws, ws_bytes, stream);
}
int dnmf_hals_fro_fit_bf16a(const void* A, long m, long n, long lda, float* W, long ldw, float* H, long ldh, int k, float eps,
                            int w_update, int itr, int column_sweep, int batch, long a_stride, long w_stride, long h_stride,
                            double* sq_out, void* ws, size_t ws_bytes, void* stream) {
    return fit_impl(FIT_HALS_FRO, true, A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, column_sweep, batch, a_stride, w_stride,
                    h_stride, sq_out, ws, ws_bytes, stream);
}

}  // extern "C"
