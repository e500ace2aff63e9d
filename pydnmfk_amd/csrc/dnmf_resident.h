// dnmf_resident.h -- the whole Itakura-Saito / beta-divergence MU fit of a SMALL dense float32 problem in ONE workgroup.
// Part of libdnmf_hip.so (kernels live in anonymous namespaces of the headers; the translation units csrc/*.hip include what they launch).
//
// At the sizes of an NMFk sweep (120 x 90, k <= 16) a step of the launch-chain fit (pair_mu_fit of csrc/dnmf_masked.h: two pair kernels,
// two endings, the clamps) is launch latency, not arithmetic.  Both sides of a pair-rule step are sums over a whole row (W side) or a
// whole column (H side) of the block, so a workgroup that holds ALL of W and H needs nothing from any other workgroup: one workgroup per
// problem, blockIdx.x = the problem of a batch, W and H in LDS from the first step to the last.  What csrc/dnmf_small.h needs for its
// whole fits -- an arrival counter, a patience word, co-residency, a fall-back path -- does not exist here: __syncthreads() between the
// phases is the only synchronisation; no atomics, no device-scope loads or stores, no spinning, no waiting on another workgroup.
//
// Layout.  RS_NW = 8 waves (512 threads, two waves per SIMD: the second hides the first one's L2 latency).  Everything is cut into
// 16 x 16 tiles of v_mfma_f32_16x16x4_f32 (lane l, i = l & 15, q = l >> 4;  A-operand: A[row i][kk = q],  B-operand: B[kk = q][col i],
// C/D: col = i, row = 4 q + reg), for KP = 16 (k <= 16, KT = 1) and KP = 32 (k <= 32, KT = 2) alike: the 32 x 32 x 2 instruction would
// leave half of its rows to padding at the shapes this kernel is for.  LDS (floats): a header of RS_HDR (the partial column sums, the
// column sums, two doubles per wave), then Ws[MP][KP + 4] and Hs[KP][NP + 4], MP / NP = m / n rounded up to 16, zero outside m x k and
// k x n.  The row pitches are 4 (mod 8): 16-byte aligned rows, and the four q groups of a scalar operand read (rows 4 q apart) fall
// into different banks.  A is read from global memory every step (at these sizes it stays in L2) and never written.
//
// W phase: a wave owns the 16-row tiles rt = wave, wave + 8, ... and walks ALL column tiles of each.  Its W rows are in registers
// (wreg[t][e] = W[r0 + i][16 t + 4 q + e], KT float4 LDS reads per tile).  The S tile is formed TRANSPOSED, S^T = H^T W^T (A-operand
// H[16 t + 4 q + e][c0 + i], B-operand wreg[t][e]: the contraction index is walked as 16 t + 4 q + e, any order serves), so that lane
// (i, q) holds S[r0 + i][c0 + 4 q .. + 3] -- the four consecutive elements of ONE row of A (one 16-byte load, requested a tile ahead).
// masked_pair<MODE> of csrc/dnmf_masked.h turns them into (u_n, u_d); both are B-operands of the two second products num^T = H U_n^T,
// den^T = H U_d^T, which SHARE their A-operand, one float4 of Hs per (jt, lane).  num and den of the wave's rows accumulate in
// registers over all of n (2 KT float4); the ending is pair_rule<RULE> (sqrt for IS, exponent gamma for beta) on the W registers, the
// new rows go to Ws.  No cross-wave sum.  H phase: the mirror image -- a wave owns column tiles, keeps its 16 columns of H in
// registers (hb[t][e] = H[16 t + 4 q + e][c0 + i]), forms S = W H in the plain orientation (lane (i, q): S[r0 + 4 q + reg][c0 + i]), and
// the second products num = W^T U_n, den = W^T U_d share the scalar W operand Ws[r0 + 4 q + reg][16 jt + i].  H is clamped inside its
// ending on the steps i % 10 == 0 and the W clamp follows behind a barrier, the order of pair_mu_fit.  After the loop: column sums of W
// (32 or 16 parts per column, each a strided run of rows, added in part order), W /= s + eps, H *= s^T, then {||A - W H||^2, ||A||^2}
// (fp32 per tile and lane, float64 from there on: lanes by butterfly, waves in wave order), and W, H and the two doubles are stored once.
//
// Padding is the argument of csrc/dnmf_is.h and csrc/dnmf_beta.h word for word: rows >= m of Ws and rows >= k / columns >= n of Hs are
// zeros and STAY zeros (every store into Ws and Hs is predicated on the block), an A load outside the block gives 0, so u_n = 0 there
// and u_d -- 2^23 for IS, eps^(beta - 1) for beta, finite on [-2, 4] -- meets an exact zero of the other factor where the padded index is
// contracted, and goes nowhere where it is an output index.  Any lda / ldw / ldh and any per-problem stride; the vector load of A needs
// 16-byte rows (FAST), else it is taken element by element.
//
// Reproducibility: every sum has one association that depends on (m, n, k) alone -- never on the batch, the strides or the alignment --
// so problem b of a batch has the bits of the same problem fitted alone.  Against the launch-chain kernels the agreement is to fp32
// rounding, NOT bit for bit (other tile shapes, other orders of the sums): the status csrc/dnmf_small.h has against its step kernels.
//
// Per-entry weights (params.weights, the four modes of csrc/dnmf_weighted.h): pair_resident_weighted_kernel at the end of this file, a
// sibling with V as a second m x n operand read the way A is read.
//
// Registers (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage): see the tables in DESIGN.md section 7; no instantiation uses scratch.
#pragma once
#include "dnmf_is.h"
#include "dnmf_beta.h"
#include "dnmf_weighted.h"

#define RS_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

namespace {

constexpr int RS_NW = 8;                     // waves per workgroup
constexpr int RS_T = 64 * RS_NW;
constexpr int RS_HDR = 640;                  // floats: red[RS_T], cs[32], then 2 doubles per wave
constexpr int RS_PADW = 4, RS_PADH = 4;      // row pitches of Ws / Hs beyond KP / NP
constexpr size_t RS_LDS_MAX = 160 * 1024;    // what a workgroup of gfx950 may hold
constexpr int RS_MAX_K = 32;

struct ResidentPlan { int eligible; int kp; long rowtiles, coltiles; size_t lds; };
inline ResidentPlan plan_resident(long m, long n, int k) {
    ResidentPlan r{};
    if (k < 1 || k > RS_MAX_K) return r;
    r.kp = k <= 16 ? 16 : 32;
    r.rowtiles = cdiv(m, 16);
    r.coltiles = cdiv(n, 16);
    // (beyond 2^20 rows or columns nothing can fit; the cut keeps the product below in range)
    if (m > (1 << 20) || n > (1 << 20)) { r.lds = ~size_t(0); return r; }
    r.lds = sizeof(float) * ((size_t)RS_HDR + (size_t)r.rowtiles * 16 * (r.kp + RS_PADW) + (size_t)r.kp * (r.coltiles * 16 + RS_PADH));
    r.eligible = r.lds <= RS_LDS_MAX;
    return r;
}

struct ResidentArgs {
    const float* A; long a_stride, lda;
    float* W; long w_stride, ldw;
    float* H; long h_stride, ldh;
    int m, n, k;
    float eps, pexp, gamma;                  // pexp = beta - 2 and gamma(beta): read by PAIR_BETA alone
    int w_update, itr;
    double* sq;                              // [batch][2]
};

template <int KT, bool FAST, int MODE>
__global__ __launch_bounds__(RS_T) void pair_resident_kernel(ResidentArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KP = 16 * KT, LDW = KP + RS_PADW, RULE = PairMode<MODE>::rule;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long prob = blockIdx.x;
    const float* __restrict__ A = p.A + prob * p.a_stride;
    float* __restrict__ Wg = p.W + prob * p.w_stride;
    float* __restrict__ Hg = p.H + prob * p.h_stride;
    const int m = p.m, n = p.n, k = p.k;
    const int nrt = (m + 15) >> 4, nct = (n + 15) >> 4, MP = nrt * 16, LDH = nct * 16 + RS_PADH;
    const float eps = p.eps;
    float* red = smem;
    float* cs = smem + RS_T;
    double* wsum = reinterpret_cast<double*>(smem + RS_T + 32);
    float* Ws = smem + RS_HDR;
    float* Hs = Ws + MP * LDW;

    for (int idx = tid; idx < MP * LDW; idx += RS_T) {
        const int r = idx / LDW, j = idx - r * LDW;
        Ws[idx] = (r < m && j < k) ? Wg[(long)r * p.ldw + j] : 0.f;
    }
    for (int idx = tid; idx < KP * LDH; idx += RS_T) {
        const int j = idx / LDH, c = idx - j * LDH;
        Hs[idx] = (j < k && c < n) ? Hg[(long)j * p.ldh + c] : 0.f;
    }
    __syncthreads();

    for (int it = 0; it < p.itr; ++it) {
        const int clamp = (it % 10 == 0);
        if (p.w_update) {
            for (int rt = wave; rt < nrt; rt += RS_NW) {                      // ---- W phase
                const int r0 = rt * 16;
                const bool rok = r0 + i < m;
                const float* Ar = A + (long)(r0 + i) * p.lda;
                float* wrow = Ws + (r0 + i) * LDW;
                f32x4 wreg[KT], on[KT], od[KT];
#pragma unroll
                for (int t = 0; t < KT; ++t) {
                    wreg[t] = *reinterpret_cast<const f32x4*>(wrow + 16 * t + 4 * q);
                    on[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                    od[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                float a_cur[4], a_nxt[4] = {0.f, 0.f, 0.f, 0.f};
                load_vec<4, FAST>(a_cur, Ar, 4 * q, n, rok);
                for (int ct = 0; ct < nct; ++ct) {
                    const int c0 = ct * 16;
                    if (ct + 1 < nct) load_vec<4, FAST>(a_nxt, Ar, c0 + 16 + 4 * q, n, rok);
                    f32x4 st = {0.f, 0.f, 0.f, 0.f};                           // S^T: lane (i, q) holds S[r0 + i][c0 + 4 q + reg]
#pragma unroll
                    for (int t = 0; t < KT; ++t)
#pragma unroll
                        for (int e = 0; e < 4; ++e) st = RS_MFMA(Hs[(16 * t + 4 * q + e) * LDH + c0 + i], wreg[t][e], st);
                    f32x4 un, ud;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float x, y;
                        masked_pair<MODE>(a_cur[r], st[r], eps, p.pexp, x, y);
                        un[r] = x;
                        ud[r] = y;
                    }
#pragma unroll
                    for (int jt = 0; jt < KT; ++jt) {                          // num^T, den^T: rows j = 16 jt + 4 q + reg, column r0 + i
                        const f32x4 hh = *reinterpret_cast<const f32x4*>(Hs + (16 * jt + i) * LDH + c0 + 4 * q);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            on[jt] = RS_MFMA(hh[r], un[r], on[jt]);
                            od[jt] = RS_MFMA(hh[r], ud[r], od[jt]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) a_cur[r] = a_nxt[r];
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
            __syncthreads();
        }
        for (int ct = wave; ct < nct; ct += RS_NW) {                          // ---- H phase (with the new W)
            const int c0 = ct * 16;
            const bool cok = c0 + i < n;
            const float* Ac = A + c0 + i;
            f32x4 hb[KT], outn[KT], outd[KT];
#pragma unroll
            for (int t = 0; t < KT; ++t) {
#pragma unroll
                for (int e = 0; e < 4; ++e) hb[t][e] = Hs[(16 * t + 4 * q + e) * LDH + c0 + i];
                outn[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                outd[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            float a_cur[4], a_nxt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) a_cur[r] = (cok && 4 * q + r < m) ? Ac[(long)(4 * q + r) * p.lda] : 0.f;
            for (int rt = 0; rt < nrt; ++rt) {
                const int r0 = rt * 16;
                if (rt + 1 < nrt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = r0 + 16 + 4 * q + r;
                        a_nxt[r] = (cok && row < m) ? Ac[(long)row * p.lda] : 0.f;
                    }
                }
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};                              // S: lane (i, q) holds S[r0 + 4 q + reg][c0 + i]
#pragma unroll
                for (int t = 0; t < KT; ++t) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(Ws + (r0 + i) * LDW + 16 * t + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = RS_MFMA(w[e], hb[t][e], acc);
                }
                f32x4 un, ud;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float x, y;
                    masked_pair<MODE>(a_cur[r], acc[r], eps, p.pexp, x, y);
                    un[r] = x;
                    ud[r] = y;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int jt = 0; jt < KT; ++jt) {                          // num, den: rows j = 16 jt + 4 q + reg, column c0 + i
                        const float w = Ws[(r0 + 4 * q + r) * LDW + 16 * jt + i];
                        outn[jt] = RS_MFMA(w, un[r], outn[jt]);
                        outd[jt] = RS_MFMA(w, ud[r], outd[jt]);
                    }
#pragma unroll
                for (int r = 0; r < 4; ++r) a_cur[r] = a_nxt[r];
            }
            if (cok) {
#pragma unroll
                for (int jt = 0; jt < KT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = 16 * jt + 4 * q + r;
                        if (j < k) Hs[j * LDH + c0 + i] = pair_rule<RULE>(hb[jt][r], outn[jt][r], outd[jt][r], eps, clamp, p.gamma);
                    }
            }
        }
        __syncthreads();
        if (clamp) {                                                           // W = max(W, eps) after H's (pyDNMF.py:170-172)
            for (int idx = tid; idx < m * k; idx += RS_T) {
                float* w = Ws + (idx / k) * LDW + idx % k;
                *w = fmaxf(*w, eps);
            }
            __syncthreads();
        }
    }

    // ---- normalize_features (pyDNMF.py:185-194): s = column sums of W in a fixed order; W /= s + eps; H *= s^T
    {
        constexpr int NPART = RS_T / KP;
        const int j = tid % KP, part = tid / KP;
        float s = 0.f;
        for (int r = part; r < m; r += NPART) s += Ws[r * LDW + j];
        red[part * KP + j] = s;
        __syncthreads();
        if (tid < KP) {
            float t = 0.f;
            for (int pp = 0; pp < NPART; ++pp) t += red[pp * KP + tid];
            cs[tid] = t;
        }
        __syncthreads();
    }
    for (int idx = tid; idx < m * k; idx += RS_T) {
        const int r = idx / k, j = idx - r * k;
        const float v = Ws[r * LDW + j] / (cs[j] + eps);
        Ws[r * LDW + j] = v;
        Wg[(long)r * p.ldw + j] = v;
    }
    for (int idx = tid; idx < k * n; idx += RS_T) {
        const int j = idx / n, c = idx - j * n;
        const float v = Hs[j * LDH + c] * cs[j];
        Hs[j * LDH + c] = v;
        Hg[(long)j * p.ldh + c] = v;
    }
    __syncthreads();

    // ---- relative_err (pyDNMF.py:205-218): {sum (A - W H)^2, sum A^2}; the tiles of the W phase
    double dres = 0.0, dnorm = 0.0;
    for (int rt = wave; rt < nrt; rt += RS_NW) {
        const int r0 = rt * 16;
        const bool rok = r0 + i < m;
        const float* Ar = A + (long)(r0 + i) * p.lda;
        f32x4 wreg[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) wreg[t] = *reinterpret_cast<const f32x4*>(Ws + (r0 + i) * LDW + 16 * t + 4 * q);
        for (int ct = 0; ct < nct; ++ct) {
            const int c0 = ct * 16;
            float a[4];
            load_vec<4, FAST>(a, Ar, c0 + 4 * q, n, rok);
            f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) st = RS_MFMA(Hs[(16 * t + 4 * q + e) * LDH + c0 + i], wreg[t][e], st);
            float part = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {                                      // outside the block a = 0 and S = 0 exactly
                const float d = a[r] - st[r];
                part = fmaf(d, d, part);
                dnorm += (double)a[r] * (double)a[r];
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
        for (int w = 0; w < RS_NW; ++w) { a += wsum[2 * w]; b += wsum[2 * w + 1]; }
        p.sq[2 * prob] = a;
        p.sq[2 * prob + 1] = b;
    }
}

// ================================================================================================ the same fit under per-entry weights
// pair_resident_weighted_kernel: objective sum_ij v_ij d(a_ij | (W H)_ij) for the four modes of csrc/dnmf_weighted.h (PAIR_FRO, PAIR_KL,
// PAIR_IS, PAIR_BETA).  A SIBLING of the kernel above, not a flag of it: with the two fits in one body (tried: a __forceinline__ body
// with `if constexpr (WT)`) hipcc schedules and allocates the unweighted instantiations differently, and their code is to stay as it is,
// instruction for instruction.  Geometry, LDS layout, barriers and the order in which every accumulator chain receives its products are
// the kernel's above, line by line; what is new is V, a second m x n operand that goes the way A goes:
//   W phase   the lane's four consecutive elements of its row of V (one 16-byte load when FAST, which now must hold for V's rows too),
//             requested one tile ahead, beside a_nxt;
//   H phase   four strided scalar loads beside A's four, requested one row tile ahead;
//   step      masked_pair<MODE>, then weigh(v, un, ud): the select on v > 0 stands before the second products, so where it fails `a` is
//             never looked at (NaN, inf, 0, negative) and no NaN reaches an MFMA operand;
//   padding   a V load outside the block returns 0: a padded position is a gap, (u_n, u_d) = (0, 0), under all four modes -- the
//             argument of csrc/dnmf_weighted.h.  (The unweighted u_d = 2^23 or eps^(beta - 1) met an exact zero there; 0 meets it now.)
//   error     {sum v (a - s)^2, sum v a^2} over v > 0, BOTH terms selected, the float64 one included.
// V is read from L2 every step and takes no LDS: plan_resident is the plan.  ResidentWeights is a second kernel argument; v_stride = 0
// gives every problem of the batch the same V.  With V = 1 under PAIR_IS / PAIR_BETA every product by v is exact (x * 1) and the chains
// receive what they receive above in the same order: the factors and the pair are the unweighted kernel's bit for bit.
struct ResidentWeights { const float* V; long v_stride, ldv; };

template <int KT, bool FAST, int MODE>
__global__ __launch_bounds__(RS_T) void pair_resident_weighted_kernel(ResidentArgs p, ResidentWeights pv) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KP = 16 * KT, LDW = KP + RS_PADW, RULE = PairMode<MODE>::rule;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long prob = blockIdx.x;
    const float* __restrict__ A = p.A + prob * p.a_stride;
    const float* __restrict__ V = pv.V + prob * pv.v_stride;
    float* __restrict__ Wg = p.W + prob * p.w_stride;
    float* __restrict__ Hg = p.H + prob * p.h_stride;
    const int m = p.m, n = p.n, k = p.k;
    const int nrt = (m + 15) >> 4, nct = (n + 15) >> 4, MP = nrt * 16, LDH = nct * 16 + RS_PADH;
    const float eps = p.eps;
    float* red = smem;
    float* cs = smem + RS_T;
    double* wsum = reinterpret_cast<double*>(smem + RS_T + 32);
    float* Ws = smem + RS_HDR;
    float* Hs = Ws + MP * LDW;

    for (int idx = tid; idx < MP * LDW; idx += RS_T) {
        const int r = idx / LDW, j = idx - r * LDW;
        Ws[idx] = (r < m && j < k) ? Wg[(long)r * p.ldw + j] : 0.f;
    }
    for (int idx = tid; idx < KP * LDH; idx += RS_T) {
        const int j = idx / LDH, c = idx - j * LDH;
        Hs[idx] = (j < k && c < n) ? Hg[(long)j * p.ldh + c] : 0.f;
    }
    __syncthreads();

    for (int it = 0; it < p.itr; ++it) {
        const int clamp = (it % 10 == 0);
        if (p.w_update) {
            for (int rt = wave; rt < nrt; rt += RS_NW) {                      // ---- W phase
                const int r0 = rt * 16;
                const bool rok = r0 + i < m;
                const float* Ar = A + (long)(r0 + i) * p.lda;
                const float* Vr = V + (long)(r0 + i) * pv.ldv;
                float* wrow = Ws + (r0 + i) * LDW;
                f32x4 wreg[KT], on[KT], od[KT];
#pragma unroll
                for (int t = 0; t < KT; ++t) {
                    wreg[t] = *reinterpret_cast<const f32x4*>(wrow + 16 * t + 4 * q);
                    on[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                    od[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                float a_cur[4], a_nxt[4] = {0.f, 0.f, 0.f, 0.f};
                float v_cur[4], v_nxt[4] = {0.f, 0.f, 0.f, 0.f};
                load_vec<4, FAST>(a_cur, Ar, 4 * q, n, rok);
                load_vec<4, FAST>(v_cur, Vr, 4 * q, n, rok);                   // 0 outside the block: a gap
                for (int ct = 0; ct < nct; ++ct) {
                    const int c0 = ct * 16;
                    if (ct + 1 < nct) {
                        load_vec<4, FAST>(a_nxt, Ar, c0 + 16 + 4 * q, n, rok);
                        load_vec<4, FAST>(v_nxt, Vr, c0 + 16 + 4 * q, n, rok);
                    }
                    f32x4 st = {0.f, 0.f, 0.f, 0.f};                           // S^T: lane (i, q) holds S[r0 + i][c0 + 4 q + reg]
#pragma unroll
                    for (int t = 0; t < KT; ++t)
#pragma unroll
                        for (int e = 0; e < 4; ++e) st = RS_MFMA(Hs[(16 * t + 4 * q + e) * LDH + c0 + i], wreg[t][e], st);
                    f32x4 un, ud;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float x, y;
                        masked_pair<MODE>(a_cur[r], st[r], eps, p.pexp, x, y);
                        weigh(v_cur[r], x, y);                                 // the select: nothing of `a` passes where v > 0 fails
                        un[r] = x;
                        ud[r] = y;
                    }
#pragma unroll
                    for (int jt = 0; jt < KT; ++jt) {                          // num^T, den^T: rows j = 16 jt + 4 q + reg, column r0 + i
                        const f32x4 hh = *reinterpret_cast<const f32x4*>(Hs + (16 * jt + i) * LDH + c0 + 4 * q);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            on[jt] = RS_MFMA(hh[r], un[r], on[jt]);
                            od[jt] = RS_MFMA(hh[r], ud[r], od[jt]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        a_cur[r] = a_nxt[r];
                        v_cur[r] = v_nxt[r];
                    }
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
            __syncthreads();
        }
        for (int ct = wave; ct < nct; ct += RS_NW) {                          // ---- H phase (with the new W)
            const int c0 = ct * 16;
            const bool cok = c0 + i < n;
            const float* Ac = A + c0 + i;
            const float* Vc = V + c0 + i;
            f32x4 hb[KT], outn[KT], outd[KT];
#pragma unroll
            for (int t = 0; t < KT; ++t) {
#pragma unroll
                for (int e = 0; e < 4; ++e) hb[t][e] = Hs[(16 * t + 4 * q + e) * LDH + c0 + i];
                outn[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                outd[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            float a_cur[4], a_nxt[4] = {0.f, 0.f, 0.f, 0.f};
            float v_cur[4], v_nxt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = cok && 4 * q + r < m;
                a_cur[r] = in ? Ac[(long)(4 * q + r) * p.lda] : 0.f;
                v_cur[r] = in ? Vc[(long)(4 * q + r) * pv.ldv] : 0.f;
            }
            for (int rt = 0; rt < nrt; ++rt) {
                const int r0 = rt * 16;
                if (rt + 1 < nrt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = r0 + 16 + 4 * q + r;
                        const bool in = cok && row < m;
                        a_nxt[r] = in ? Ac[(long)row * p.lda] : 0.f;
                        v_nxt[r] = in ? Vc[(long)row * pv.ldv] : 0.f;
                    }
                }
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};                              // S: lane (i, q) holds S[r0 + 4 q + reg][c0 + i]
#pragma unroll
                for (int t = 0; t < KT; ++t) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(Ws + (r0 + i) * LDW + 16 * t + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = RS_MFMA(w[e], hb[t][e], acc);
                }
                f32x4 un, ud;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float x, y;
                    masked_pair<MODE>(a_cur[r], acc[r], eps, p.pexp, x, y);
                    weigh(v_cur[r], x, y);
                    un[r] = x;
                    ud[r] = y;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int jt = 0; jt < KT; ++jt) {                          // num, den: rows j = 16 jt + 4 q + reg, column c0 + i
                        const float w = Ws[(r0 + 4 * q + r) * LDW + 16 * jt + i];
                        outn[jt] = RS_MFMA(w, un[r], outn[jt]);
                        outd[jt] = RS_MFMA(w, ud[r], outd[jt]);
                    }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    a_cur[r] = a_nxt[r];
                    v_cur[r] = v_nxt[r];
                }
            }
            if (cok) {
#pragma unroll
                for (int jt = 0; jt < KT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = 16 * jt + 4 * q + r;
                        if (j < k) Hs[j * LDH + c0 + i] = pair_rule<RULE>(hb[jt][r], outn[jt][r], outd[jt][r], eps, clamp, p.gamma);
                    }
            }
        }
        __syncthreads();
        if (clamp) {                                                           // W = max(W, eps) after H's
            for (int idx = tid; idx < m * k; idx += RS_T) {
                float* w = Ws + (idx / k) * LDW + idx % k;
                *w = fmaxf(*w, eps);
            }
            __syncthreads();
        }
    }

    // ---- normalize_features: s = column sums of W in a fixed order; W /= s + eps; H *= s^T
    {
        constexpr int NPART = RS_T / KP;
        const int j = tid % KP, part = tid / KP;
        float s = 0.f;
        for (int r = part; r < m; r += NPART) s += Ws[r * LDW + j];
        red[part * KP + j] = s;
        __syncthreads();
        if (tid < KP) {
            float t = 0.f;
            for (int pp = 0; pp < NPART; ++pp) t += red[pp * KP + tid];
            cs[tid] = t;
        }
        __syncthreads();
    }
    for (int idx = tid; idx < m * k; idx += RS_T) {
        const int r = idx / k, j = idx - r * k;
        const float v = Ws[r * LDW + j] / (cs[j] + eps);
        Ws[r * LDW + j] = v;
        Wg[(long)r * p.ldw + j] = v;
    }
    for (int idx = tid; idx < k * n; idx += RS_T) {
        const int j = idx / n, c = idx - j * n;
        const float v = Hs[j * LDH + c] * cs[j];
        Hs[j * LDH + c] = v;
        Hg[(long)j * p.ldh + c] = v;
    }
    __syncthreads();

    // ---- the weighted error pair {sum v (A - W H)^2, sum v A^2} over v > 0 (dnmf_weighted_resid_sqnorm's); the tiles of the W phase
    double dres = 0.0, dnorm = 0.0;
    for (int rt = wave; rt < nrt; rt += RS_NW) {
        const int r0 = rt * 16;
        const bool rok = r0 + i < m;
        const float* Ar = A + (long)(r0 + i) * p.lda;
        const float* Vr = V + (long)(r0 + i) * pv.ldv;
        f32x4 wreg[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) wreg[t] = *reinterpret_cast<const f32x4*>(Ws + (r0 + i) * LDW + 16 * t + 4 * q);
        for (int ct = 0; ct < nct; ++ct) {
            const int c0 = ct * 16;
            float a[4], v[4];
            load_vec<4, FAST>(a, Ar, c0 + 4 * q, n, rok);
            load_vec<4, FAST>(v, Vr, c0 + 4 * q, n, rok);
            f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) st = RS_MFMA(Hs[(16 * t + 4 * q + e) * LDH + c0 + i], wreg[t][e], st);
            float part = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // both terms selected: what lies under a zero weight, or outside the block (V loaded as 0), enters neither sum.  At
                // v = 1 the products by v are exact and the terms are the unweighted kernel's, bit for bit
                const bool obs = v[r] > 0.f;
                const float d = obs ? a[r] - st[r] : 0.f;
                part = fmaf(obs ? v[r] * d : 0.f, d, part);
                dnorm += obs ? ((double)v[r] * (double)a[r]) * (double)a[r] : 0.0;
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
        for (int w = 0; w < RS_NW; ++w) { a += wsum[2 * w]; b += wsum[2 * w + 1]; }
        p.sq[2 * prob] = a;
        p.sq[2 * prob + 1] = b;
    }
}

}  // namespace
