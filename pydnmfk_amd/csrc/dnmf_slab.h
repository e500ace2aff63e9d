// dnmf_slab.h -- a step of ALL problems of a batch of Itakura-Saito / beta-divergence / weighted MU fits in TWO launches: fit_loop='slab'.
// Part of libdnmf_hip.so (kernels live in anonymous namespaces of the headers; the translation units csrc/*.hip include what they launch).
//
// The resident kernels (csrc/dnmf_resident.h) end where one workgroup's LDS ends: k <= 32 and (m + n) KP floats in 160 KiB.  Above that the
// launch chain (pair_mu_fit of csrc/dnmf_masked.h) runs one problem per call, five to six launches a step.  What the resident header
// says of a pair-rule step holds at any size: both sides are sums over a whole row (W side) or a whole column (H side) of the block.
// A workgroup that owns a SLAB of 64 rows therefore needs nothing from any other workgroup during the W phase, and one that owns 64
// columns nothing during the H phase: a step is pair_slab_w_kernel then pair_slab_h_kernel, grid x = slabs, z = problem of the batch.
// No split of the contraction, no partial-sum workspace, no reduction or ending launch, no atomics, no waiting between workgroups: the
// kernel boundary is the only synchronisation across workgroups, __syncthreads() the only one inside.  k <= 64 (KP = 16, 32, 64).
//
// Layout.  SL_NW = 4 waves, a wave owns one 16 x 16 tile row (W phase) or tile column (H phase) of the slab.  Tiles are those of
// v_mfma_f32_16x16x4_f32 with the lane roles of the resident kernel (lane l, i = l & 15, q = l >> 4;  A-operand: A[row i][kk = q],
// B-operand: B[kk = q][col i],  C/D: col = i, row = 4 q + reg).  The factor a phase does NOT own is streamed through LDS in PANELS that
// the four waves share: W phase H[0:KP][64 p .. 64 p + 63] at pitch 68, H phase W[64 p .. 64 p + 63][0:KP] at pitch KP + 4 (both 4 mod 8:
// 16-byte rows, the q groups of a scalar operand read in different banks).  Two panels, double-buffered: the loads of panel p + 1 are
// requested into registers before panel p is walked and stored behind it, ONE barrier per panel (the buffer written was last read
// before the previous barrier).  2 x 17 KiB at KP = 64, so several workgroups share a CU.
//
// W phase: the wave's rows of W are in registers (wreg[t][e] = W[r0 + i][16 t + 4 q + e]) and it walks ALL column tiles in increasing
// order.  S is formed TRANSPOSED (A-operand H[16 t + 4 q + e][c0 + i] from the panel, B-operand wreg[t][e]) so that lane (i, q) holds
// S[r0 + i][c0 + 4 q .. + 3], four consecutive elements of ONE row of A: one 16-byte load, requested a tile ahead (FAST; else element by
// element, the same bits).  masked_pair<MODE>, and under weights weigh(v, .), give (u_n, u_d); the second products num^T = H U_n^T,
// den^T = H U_d^T share their H operand (one float4 of the panel).  num and den accumulate in registers over all of n, pair_rule<RULE>
// ends in registers, the new rows go to global W predicated on the block.  H phase: the mirror image in the plain orientation (the
// wave's 16 columns of H in registers, hb[t][e] = H[16 t + 4 q + e][c0 + i]; lane (i, q) holds S[r0 + 4 q + reg][c0 + i], four scalar loads
// of A a tile ahead), ending with the clamp of H on the steps i % 10 == 0.  The clamp of W that follows it in pair_mu_fit's order
// belongs to the owner of the rows: it is PENDING in global W until the next W phase applies it on load (`wclamp`); an H phase that
// meets a pending clamp (W_update off) applies it to the panel it stages, and the finish applies what is still pending.  fmaxf(., eps)
// is idempotent, so the factors are those of pair_mu_fit's order of operations.
//
// Finish (once per fit, one workgroup per problem): column sums of W (512 / KP strided runs per column, added in run order),
// W /= s + eps, H *= s^T, then {sum (A - W H)^2, sum A^2} -- under weights {sum v (A - W H)^2, sum v A^2} over v > 0 -- on the tiles of the
// W phase, fp32 per tile and lane, float64 from there on (lanes by butterfly, waves in wave order).
//
// Padding is the argument of csrc/dnmf_is.h and csrc/dnmf_beta.h word for word: every load is predicated and gives 0 outside the block,
// so padded rows of W and padded rows / columns of H are zeros in registers and panels; u_d -- 2^23 for IS, eps^(beta - 1) for beta --
// meets an exact zero of the other factor where the padded index is contracted, and goes nowhere where it is an output index (every
// store is predicated).  Under weights a V load outside the block gives 0: a gap, (u_n, u_d) = (0, 0), and a zero weight hides what
// lies under it (NaN, inf, negative) by the select of weigh() before the second products.
//
// Reproducibility: every sum has ONE association that depends on (m, n, k) alone -- never on the batch, the pitches, the member distances
// or the alignment -- so problem b of a batch has the bits of the same problem fitted alone.  Against the launch chain and against
// fit_loop='resident' the agreement is to fp32 rounding, NOT bit for bit.
//
// Registers (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage): DESIGN.md section 7; no instantiation uses scratch.
#pragma once
#include "dnmf_is.h"
#include "dnmf_beta.h"
#include "dnmf_weighted.h"

#define SL_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

namespace {

constexpr int SL_NW = 4;                     // waves per workgroup of a step kernel
constexpr int SL_T = 64 * SL_NW;
constexpr int SL_SLAB = 64;                  // rows (W phase) or columns (H phase) a workgroup owns, and the width of a panel
constexpr int SL_PAD = 4;                    // pitch of a panel row beyond its width
constexpr int SL_MAX_K = 64;
constexpr long SL_MAX_DIM = 1L << 30;        // m, n: every tile index stays an int
constexpr int SL_FIN_NW = 8, SL_FIN_T = 64 * SL_FIN_NW;      // the finish: one workgroup per problem

struct SlabPlan { int eligible; int kp; long row_slabs, col_slabs, w_panels, h_panels; size_t lds_w, lds_h; };
inline SlabPlan plan_slab(long m, long n, int k) {
    SlabPlan r{};
    if (k < 1 || k > SL_MAX_K) return r;
    r.kp = k <= 16 ? 16 : (k <= 32 ? 32 : 64);
    r.row_slabs = cdiv(m, SL_SLAB);
    r.col_slabs = cdiv(n, SL_SLAB);
    r.w_panels = r.col_slabs;                // panels of H a workgroup of the W phase walks
    r.h_panels = r.row_slabs;                // panels of W a workgroup of the H phase walks
    r.lds_w = 2 * sizeof(float) * r.kp * (SL_SLAB + SL_PAD);
    r.lds_h = 2 * sizeof(float) * SL_SLAB * (r.kp + SL_PAD);
    r.eligible = m <= SL_MAX_DIM && n <= SL_MAX_DIM;
    return r;
}

struct SlabArgs {
    const float* A; long a_stride, lda;
    const float* V; long v_stride, ldv;      // read by the weighted instantiations alone
    float* W; long w_stride, ldw;
    float* H; long h_stride, ldh;
    int m, n, k;
    float eps, pexp, gamma;                  // pexp = beta - 2 and gamma(beta): read by PAIR_BETA alone
    double* sq;                              // [batch][2]
};

// ================================================================================================ W phase
// grid (row slabs, 1, problems).  wclamp: W = max(W, eps) is pending from the step before (applied on load, inside the block only)
template <int KT, bool FAST, int MODE, bool WT>
__global__ __launch_bounds__(SL_T) void pair_slab_w_kernel(SlabArgs p, int wclamp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KP = 16 * KT, LDH = SL_SLAB + SL_PAD, PANEL = KP * LDH, RULE = PairMode<MODE>::rule;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long prob = blockIdx.z;
    const float* __restrict__ A = p.A + prob * p.a_stride;
    const float* __restrict__ Hg = p.H + prob * p.h_stride;
    float* __restrict__ Wg = p.W + prob * p.w_stride;
    const int m = p.m, n = p.n, k = p.k;
    const float eps = p.eps;
    const int r0 = (int)blockIdx.x * SL_SLAB + wave * 16;
    const bool live = r0 < m;                                                  // (wave-uniform: a wave without rows only stages panels)
    const bool rok = r0 + i < m;
    const float* Ar = A + (long)(r0 + i) * p.lda;
    const float* Vr = WT ? p.V + prob * p.v_stride + (long)(r0 + i) * p.ldv : nullptr;
    float* wrow = Wg + (long)(r0 + i) * p.ldw;
    const int np = (n + SL_SLAB - 1) / SL_SLAB;

    f32x4 wreg[KT], on[KT], od[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        float w[4];
        load_vec<4, false>(w, wrow, 16 * t + 4 * q, k, rok);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (wclamp && rok && 16 * t + 4 * q + e < k) w[e] = fmaxf(w[e], eps);
            wreg[t][e] = w[e];
        }
        on[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        od[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // a panel: H[0:KP][64 pnl .. + 63], KT float4 per thread (thread -> row j = idx / 16, columns 4 (idx % 16) .. + 3)
    float stage[KT][4];
    auto fetch = [&](int pnl) {
#pragma unroll
        for (int u = 0; u < KT; ++u) {
            const int idx = tid + SL_T * u, j = idx >> 4, c4 = idx & 15;
            load_vec<4, FAST>(stage[u], Hg + (long)j * p.ldh, (long)pnl * SL_SLAB + 4 * c4, n, j < k);
        }
    };
    auto put = [&](float* buf) {
#pragma unroll
        for (int u = 0; u < KT; ++u) {
            const int idx = tid + SL_T * u, j = idx >> 4, c4 = idx & 15;
            *reinterpret_cast<f32x4*>(buf + j * LDH + 4 * c4) = f32x4{stage[u][0], stage[u][1], stage[u][2], stage[u][3]};
        }
    };
    fetch(0);
    put(smem);
    __syncthreads();

    float a_cur[4], a_nxt[4], v_cur[4] = {0.f, 0.f, 0.f, 0.f}, v_nxt[4] = {0.f, 0.f, 0.f, 0.f};
    load_vec<4, FAST>(a_cur, Ar, 4 * q, n, rok);
    if constexpr (WT) load_vec<4, FAST>(v_cur, Vr, 4 * q, n, rok);             // 0 outside the block: a gap
    for (int pnl = 0; pnl < np; ++pnl) {
        const float* Hs = smem + (pnl & 1) * PANEL;
        if (pnl + 1 < np) fetch(pnl + 1);
        if (live) {
            const int left = n - pnl * SL_SLAB, nt = left >= SL_SLAB ? 4 : (left + 15) >> 4;
            for (int ct = 0; ct < nt; ++ct) {
                const int cl = 16 * ct, c0 = pnl * SL_SLAB + cl;
                load_vec<4, FAST>(a_nxt, Ar, c0 + 16 + 4 * q, n, rok);         // (beyond n: zeros, nothing is read)
                if constexpr (WT) load_vec<4, FAST>(v_nxt, Vr, c0 + 16 + 4 * q, n, rok);
                f32x4 st = {0.f, 0.f, 0.f, 0.f};                               // S^T: lane (i, q) holds S[r0 + i][c0 + 4 q + reg]
#pragma unroll
                for (int t = 0; t < KT; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) st = SL_MFMA(Hs[(16 * t + 4 * q + e) * LDH + cl + i], wreg[t][e], st);
                f32x4 un, ud;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float x, y;
                    masked_pair<MODE>(a_cur[r], st[r], eps, p.pexp, x, y);
                    if constexpr (WT) weigh(v_cur[r], x, y);                   // the select: nothing of `a` passes where v > 0 fails
                    un[r] = x;
                    ud[r] = y;
                }
#pragma unroll
                for (int jt = 0; jt < KT; ++jt) {                              // num^T, den^T: rows j = 16 jt + 4 q + reg, column r0 + i
                    const f32x4 hh = *reinterpret_cast<const f32x4*>(Hs + (16 * jt + i) * LDH + cl + 4 * q);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        on[jt] = SL_MFMA(hh[r], un[r], on[jt]);
                        od[jt] = SL_MFMA(hh[r], ud[r], od[jt]);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    a_cur[r] = a_nxt[r];
                    if constexpr (WT) v_cur[r] = v_nxt[r];
                }
            }
        }
        if (pnl + 1 < np) put(smem + ((pnl + 1) & 1) * PANEL);
        __syncthreads();
    }
    if (rok) {
#pragma unroll
        for (int jt = 0; jt < KT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * jt + 4 * q + r;
                if (j < k) wrow[j] = pair_rule<RULE>(wreg[jt][r], on[jt][r], od[jt][r], eps, 0, p.gamma);
            }
    }
}

// ================================================================================================ H phase
// grid (column slabs, 1, problems).  clamp: H = max(H, eps) in the ending (the steps i % 10 == 0).  wclamp: a clamp of W is pending and
// no W phase runs (W_update off): the panels are staged clamped, global W is left to the finish
template <int KT, bool FAST, int MODE, bool WT>
__global__ __launch_bounds__(SL_T) void pair_slab_h_kernel(SlabArgs p, int clamp, int wclamp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KP = 16 * KT, LDW = KP + SL_PAD, PANEL = SL_SLAB * LDW, RULE = PairMode<MODE>::rule;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long prob = blockIdx.z;
    const float* __restrict__ A = p.A + prob * p.a_stride;
    const float* __restrict__ Wg = p.W + prob * p.w_stride;
    float* __restrict__ Hg = p.H + prob * p.h_stride;
    const int m = p.m, n = p.n, k = p.k;
    const float eps = p.eps;
    const int c0 = (int)blockIdx.x * SL_SLAB + wave * 16;
    const bool live = c0 < n;
    const bool cok = c0 + i < n;
    const float* Ac = A + c0 + i;
    const float* Vc = WT ? p.V + prob * p.v_stride + c0 + i : nullptr;
    const int np = (m + SL_SLAB - 1) / SL_SLAB;

    f32x4 hb[KT], outn[KT], outd[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 16 * t + 4 * q + e;
            hb[t][e] = (cok && j < k) ? Hg[(long)j * p.ldh + c0 + i] : 0.f;
        }
        outn[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        outd[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // a panel: W[64 pnl .. + 63][0:KP], KT float4 per thread (thread -> row idx / (KP / 4), columns 4 (idx % (KP / 4)) .. + 3)
    float stage[KT][4];
    auto fetch = [&](int pnl) {
#pragma unroll
        for (int u = 0; u < KT; ++u) {
            const int idx = tid + SL_T * u, r = idx / (KP / 4), c4 = idx % (KP / 4);
            const long row = (long)pnl * SL_SLAB + r;
            load_vec<4, FAST>(stage[u], Wg + row * p.ldw, 4 * c4, k, row < m);
            if (wclamp) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (row < m && 4 * c4 + e < k) stage[u][e] = fmaxf(stage[u][e], eps);
            }
        }
    };
    auto put = [&](float* buf) {
#pragma unroll
        for (int u = 0; u < KT; ++u) {
            const int idx = tid + SL_T * u, r = idx / (KP / 4), c4 = idx % (KP / 4);
            *reinterpret_cast<f32x4*>(buf + r * LDW + 4 * c4) = f32x4{stage[u][0], stage[u][1], stage[u][2], stage[u][3]};
        }
    };
    fetch(0);
    put(smem);
    __syncthreads();

    float a_cur[4], a_nxt[4], v_cur[4] = {0.f, 0.f, 0.f, 0.f}, v_nxt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool in = cok && 4 * q + r < m;
        a_cur[r] = in ? Ac[(long)(4 * q + r) * p.lda] : 0.f;
        if constexpr (WT) v_cur[r] = in ? Vc[(long)(4 * q + r) * p.ldv] : 0.f;
    }
    for (int pnl = 0; pnl < np; ++pnl) {
        const float* Ws = smem + (pnl & 1) * PANEL;
        if (pnl + 1 < np) fetch(pnl + 1);
        if (live) {
            const int left = m - pnl * SL_SLAB, nt = left >= SL_SLAB ? 4 : (left + 15) >> 4;
            for (int rt = 0; rt < nt; ++rt) {
                const int rl = 16 * rt, r0 = pnl * SL_SLAB + rl;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long row = (long)r0 + 16 + 4 * q + r;
                    const bool in = cok && row < m;
                    a_nxt[r] = in ? Ac[row * p.lda] : 0.f;
                    if constexpr (WT) v_nxt[r] = in ? Vc[row * p.ldv] : 0.f;
                }
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};                              // S: lane (i, q) holds S[r0 + 4 q + reg][c0 + i]
#pragma unroll
                for (int t = 0; t < KT; ++t) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(Ws + (rl + i) * LDW + 16 * t + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = SL_MFMA(w[e], hb[t][e], acc);
                }
                f32x4 un, ud;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float x, y;
                    masked_pair<MODE>(a_cur[r], acc[r], eps, p.pexp, x, y);
                    if constexpr (WT) weigh(v_cur[r], x, y);
                    un[r] = x;
                    ud[r] = y;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int jt = 0; jt < KT; ++jt) {                          // num, den: rows j = 16 jt + 4 q + reg, column c0 + i
                        const float w = Ws[(rl + 4 * q + r) * LDW + 16 * jt + i];
                        outn[jt] = SL_MFMA(w, un[r], outn[jt]);
                        outd[jt] = SL_MFMA(w, ud[r], outd[jt]);
                    }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    a_cur[r] = a_nxt[r];
                    if constexpr (WT) v_cur[r] = v_nxt[r];
                }
            }
        }
        if (pnl + 1 < np) put(smem + ((pnl + 1) & 1) * PANEL);
        __syncthreads();
    }
    if (cok) {
#pragma unroll
        for (int jt = 0; jt < KT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * jt + 4 * q + r;
                if (j < k) Hg[(long)j * p.ldh + c0 + i] = pair_rule<RULE>(hb[jt][r], outn[jt][r], outd[jt][r], eps, clamp, p.gamma);
            }
    }
}

// ================================================================================================ finish
// grid (problems).  normalize_features (pyDNMF.py:185-194) and relative_err (pyDNMF.py:205-218) of one problem in one workgroup; not
// hot (once per fit).  wclamp: the clamp of W of the last clamp step is still pending
template <int KT, bool FAST, bool WT>
__global__ __launch_bounds__(SL_FIN_T) void pair_slab_finish_kernel(SlabArgs p, int wclamp) {
    __shared__ float red[SL_FIN_T];
    __shared__ float cs[SL_MAX_K];
    __shared__ double wsum[2 * SL_FIN_NW];
    constexpr int KP = 16 * KT, NPART = SL_FIN_T / KP;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long prob = blockIdx.x;
    const float* __restrict__ A = p.A + prob * p.a_stride;
    float* Wg = p.W + prob * p.w_stride;
    float* Hg = p.H + prob * p.h_stride;
    const int m = p.m, n = p.n, k = p.k;
    const float eps = p.eps;
    {
        const int j = tid % KP, part = tid / KP;
        float s = 0.f;
        if (j < k)
            for (int r = part; r < m; r += NPART) {
                const float w = Wg[(long)r * p.ldw + j];
                s += wclamp ? fmaxf(w, eps) : w;
            }
        red[part * KP + j] = s;
        __syncthreads();
        if (tid < KP) {
            float t = 0.f;
            for (int pp = 0; pp < NPART; ++pp) t += red[pp * KP + tid];
            cs[tid] = t;
        }
        __syncthreads();
    }
    for (long idx = tid; idx < (long)m * k; idx += SL_FIN_T) {
        const long r = idx / k;
        const int j = (int)(idx - r * k);
        const float w = Wg[r * p.ldw + j];
        Wg[r * p.ldw + j] = (wclamp ? fmaxf(w, eps) : w) / (cs[j] + eps);
    }
    for (long idx = tid; idx < (long)k * n; idx += SL_FIN_T) {
        const int j = (int)(idx / n);
        const long c = idx - (long)j * n;
        Hg[(long)j * p.ldh + c] *= cs[j];
    }
    __syncthreads();                                                           // (this workgroup's own stores: visible to it behind the barrier)

    const int nrt = (m + 15) >> 4, nct = (n + 15) >> 4;
    double dres = 0.0, dnorm = 0.0;
    for (int rt = wave; rt < nrt; rt += SL_FIN_NW) {
        const int r0 = rt * 16;
        const bool rok = r0 + i < m;
        const float* Ar = A + (long)(r0 + i) * p.lda;
        const float* Vr = WT ? p.V + prob * p.v_stride + (long)(r0 + i) * p.ldv : nullptr;
        f32x4 wreg[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            float w[4];
            load_vec<4, false>(w, Wg + (long)(r0 + i) * p.ldw, 16 * t + 4 * q, k, rok);
            wreg[t] = f32x4{w[0], w[1], w[2], w[3]};
        }
        for (int ct = 0; ct < nct; ++ct) {
            const int c0 = ct * 16;
            float a[4], v[4];
            load_vec<4, FAST>(a, Ar, c0 + 4 * q, n, rok);
            if constexpr (WT) load_vec<4, FAST>(v, Vr, c0 + 4 * q, n, rok);
            f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 16 * t + 4 * q + e;
                    const float h = (j < k && c0 + i < n) ? Hg[(long)j * p.ldh + c0 + i] : 0.f;
                    st = SL_MFMA(h, wreg[t][e], st);
                }
            float part = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (WT) {                                            // both terms selected: what lies under a zero weight, or outside
                    const bool obs = v[r] > 0.f;                               // the block (V loaded as 0), enters neither sum
                    const float d = obs ? a[r] - st[r] : 0.f;
                    part = fmaf(obs ? v[r] * d : 0.f, d, part);
                    dnorm += obs ? ((double)v[r] * (double)a[r]) * (double)a[r] : 0.0;
                } else {                                                       // outside the block a = 0 and S = 0 exactly
                    const float d = a[r] - st[r];
                    part = fmaf(d, d, part);
                    dnorm += (double)a[r] * (double)a[r];
                }
            }
            dres += (double)part;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        dres += __shfl_xor(dres, off);
        dnorm += __shfl_xor(dnorm, off);
    }
    if (lane == 0) { wsum[2 * wave] = dres; wsum[2 * wave + 1] = dnorm; }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < SL_FIN_NW; ++w) { a += wsum[2 * w]; b += wsum[2 * w + 1]; }
        p.sq[2 * prob] = a;
        p.sq[2 * prob + 1] = b;
    }
}

}  // namespace
