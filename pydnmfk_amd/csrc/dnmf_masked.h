// dnmf_masked.h -- dense data with missing entries (NaN = not observed): the masked MU rules on the matrix cores.
// Part of libdnmf_hip.so (kernels live in anonymous namespaces of the headers; the translation units csrc/*.hip include what they launch).
//
// With Omega the observed positions (a == a), S = W H and eps the float32 machine epsilon, both sides of a step are a pair
//     fro:  num = P(A) F,          den = P(S) F                      (dist_nmf.py:729-732 for W, :748-751 for H, sums over Omega)
//     kl:   num = P(A / (S + eps)) F,  den = P(1) F                  (dist_nmf.py:806-810, :827-849)
// with F = H^T on the W side and W on the H side.  These are the two products of the dense KL kernels (csrc/dnmf_nn.h: a tile of S in
// MFMA accumulators, an element-wise step against A, a second MFMA product) with another element-wise step -- one compare and two
// selects per element -- and TWO second products that share their F fragments.  The data stay as handed over: there is no mask array,
// the compare is the mask.
//
// No NaN reaches an MFMA operand: the selects come BEFORE the second product (0 * NaN is NaN), and the first product never sees A.
// An A load outside the block returns 0, which reads as an OBSERVED zero: u_n = 0 either way, and u_d (S for fro, 1 for kl) meets a
// zero of F there by construction -- a column c >= n is a zero column of the staged H tile (so is S), a row r >= m is a zero W row (the
// predicated W loads) -- so it adds exactly nothing.  The padded contraction indices j >= k are zero rows of the staged H and zero
// columns of the loaded W.  A row or column without an observation has u_n = u_d = 0 throughout: exact zeros in both halves.
//
// Every kernel here is generic: bounds by predication, any shape, any leading dimension (FAST = 16-byte rows, vector loads).  Sums
// over column splits (W side) and row chunks (H side) are left as partials and added in split / chunk order by masked_reduce_kernel --
// no float atomics, so a fit's factors are bit-reproducible.  Plain launch chains: no workgroup waits for another one.
//
// The pair kernels serve a third rule, Itakura-Saito (MODE = PAIR_IS, csrc/dnmf_is.h), and a fourth, the beta-divergence for a runtime
// beta (MODE = PAIR_BETA, csrc/dnmf_beta.h).  Everything around them exists once, in the
// host part at the end of this file: plans, the launcher of each side, the ending, the plan report and the chain of a whole fit.
#pragma once
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_nt.h"
#include "dnmf_stream.h"
#include "dnmf_nn.h"
#include "dnmf_sums.h"

namespace {

// the element-wise step: (u_n, u_d) of one element from its datum `a` and its model value s = <W[r], H[:, c]>.  MODE: the two masked
// rules above, or the Itakura-Saito pair of csrc/dnmf_is.h, which has no mask (its padding argument is written there), or the pair of
// a general beta-divergence (csrc/dnmf_beta.h: no mask either; `e` = beta - 2 is NnArgs::pexp, which the other modes never read)
enum { PAIR_FRO = 0, PAIR_KL = 1, PAIR_IS = 2, PAIR_BETA = 3 };
template <int MODE>
__device__ __forceinline__ void masked_pair(float a, float s, float eps, float e, float& un, float& ud) {
    if constexpr (MODE == PAIR_BETA) {
        const float sp = s + eps;                  // S' = S + eps >= 2^-23
        const float p = __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(sp));   // P = S'^e: v_log_f32, v_mul_f32, v_exp_f32
        un = a * p;                                // A . P
        ud = sp * p;                               // S' . P
    } else if constexpr (MODE == PAIR_IS) {
        ud = __builtin_amdgcn_rcpf(s + eps);       // r = 1 / (S + eps): v_rcp_f32, the form of kl_quot
        un = a * ud * ud;                          // a r^2
    } else {
        const bool obs = a == a;
        if constexpr (MODE == PAIR_KL) {
            un = obs ? kl_quot(a, s + eps) : 0.f;
            ud = obs ? 1.f : 0.f;
        } else {
            un = obs ? a : 0.f;
            ud = obs ? s : 0.f;
        }
    }
}

// ---- W side: P[split][half][m][KP], half 0 = num, 1 = den, over the columns of this split (row tiling of kl_uht_kernel: a workgroup
// owns 128 rows, a lane the W row of its A row; S is formed transposed so that the contraction index of the second products is in
// registers).  Two output accumulator sets do not fit next to the W row at KP = 128, so a workgroup owns JT of the KT 32-wide tiles of
// output columns (blockIdx.z picks them; JT = KT up to KP = 64, JT = 2 at KP = 128 where S is formed twice).  (Both sets DO fit at
// KP = 128 once the accumulators may live in AGPRs -- 254 + 156 registers, no scratch --: the Itakura-Saito mode launches JT = 4 there, csrc/dnmf_is.h.)
template <int KT, int JT, bool FAST, int MODE>
__global__ __launch_bounds__(256, KT == 4 ? 1 : 2) void masked_uht_kernel(NnArgs p, float* __restrict__ P, long split_stride,
                                                                          long half_stride, long cols_per_split) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KP = 32 * KT, T = 256, STAGE = KP * BK, NY = KP / (T / 8);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
    const long arow = (long)blockIdx.x * 128 + wave * 32 + li;
    const bool rok = arow < p.m;
    const long cbeg = (long)blockIdx.y * cols_per_split;
    long cend = cbeg + cols_per_split;
    if (cend > p.n) cend = p.n;
    const long nt = (cend - cbeg + BK - 1) / BK;
    const int jt0 = (int)blockIdx.z * JT;

    f32x16 on[JT], od[JT];  // (num)^T and (den)^T tiles: rows j, lanes i
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { on[jt][r] = 0.f; od[jt][r] = 0.f; }
    float wreg[4 * KT][4];   // W[arow][8s + 4h + e]; zero for j >= k and for rows >= m
#pragma unroll
    for (int s = 0; s < 4 * KT; ++s) load_vec<4, FAST>(wreg[s], p.W + arow * p.ldw, 8 * s + 4 * h, p.k, rok);

    f32x4 hst[NY];
    float a_cur[4][4];
    if (nt > 0) {
        stage_load<KP, T, FAST, false>(hst, p.H, p.ldh, p.k, cend, 0, cbeg, tid);     // zero outside k x [.., cend)
        stage_store<KP, T>(smem, hst, tid);
#pragma unroll
        for (int g = 0; g < 4; ++g) load_vec<4, FAST>(a_cur[g], p.A + arow * p.lda, cbeg + 8 * g + 4 * h, cend, rok);
    }
    __syncthreads();
    for (long t = 0; t < nt; ++t) {
        const int cur = t & 1;
        const bool more = t + 1 < nt;
        const long c1 = cbeg + (t + 1) * BK;
        const float* Hs = smem + cur * STAGE;
        f32x16 st;  // S^T tile: rows c, lanes i.  Starts from zero (an inline constant: HAZARD 2 of dnmf_common.h does not arise)
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 4 * KT; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) st = MFMA32(Hs[lds_idx(8 * s + 4 * h + e, li >> 2) + (li & 3)], wreg[s][e], st);
        f32x16 un, ud;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float x, y;
                masked_pair<MODE>(a_cur[g][e], st[4 * g + e], p.eps, p.pexp, x, y);
                un[4 * g + e] = x;
                ud[4 * g + e] = y;
            }
        if (more) {   // the A registers are free now: the next tile's pieces (and the next H tile) under the second products
            stage_load<KP, T, FAST, false>(hst, p.H, p.ldh, p.k, cend, 0, c1, tid);
#pragma unroll
            for (int g = 0; g < 4; ++g) load_vec<4, FAST>(a_cur[g], p.A + arow * p.lda, c1 + 8 * g + 4 * h, cend, rok);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                const f32x4 hh = *reinterpret_cast<const f32x4*>(&Hs[lds_idx((jt0 + jt) * 32 + li, 2 * g + h)]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    on[jt] = MFMA32(hh[e], un[4 * g + e], on[jt]);
                    od[jt] = MFMA32(hh[e], ud[4 * g + e], od[jt]);
                }
            }
        if (more) stage_store<KP, T>(smem + (cur ^ 1) * STAGE, hst, tid);
        __syncthreads();
    }
    // on[jt] (reg, lane): j = (jt0 + jt) * 32 + crow(reg, h), i = arow; registers 4g..4g+3 are 4 consecutive j.  The slab rows are
    // KP floats at a 256-byte aligned base: every store is a whole aligned vector inside the slab
    if (rok) {
        float* dn = P + (long)blockIdx.y * split_stride + arow * KP;
        float* dd = dn + half_stride;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int j = (jt0 + jt) * 32 + 8 * g + 4 * h;
                *reinterpret_cast<f32x4*>(dn + j) = f32x4{on[jt][4 * g], on[jt][4 * g + 1], on[jt][4 * g + 2], on[jt][4 * g + 3]};
                *reinterpret_cast<f32x4*>(dd + j) = f32x4{od[jt][4 * g], od[jt][4 * g + 1], od[jt][4 * g + 2], od[jt][4 * g + 3]};
            }
    }
}

// ---- H side: P[chunk][half][KP][ldp] over the rows of this chunk (the scheme of kl_wtu_kernel: a workgroup = 4 waves that share one
// block of CW = 32 NT columns, whose KP x CW block of H is staged once; a wave walks a chunk of 32-row blocks, forms S, turns it into
// (u_n, u_d) in place and feeds both as B operands of W^T u with the same W fragments).  ldp = ncolblk * CW: every store is in the slab.
template <int KT, int NT, bool FAST, int MODE>
__global__ __launch_bounds__(256, 1) void masked_wtu_kernel(NnArgs p, long half_stride, long rowblks_per_chunk) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KP = 32 * KT, CW = 32 * NT;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, h = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const long nchunks = cdiv(p.nrowblk, rowblks_per_chunk);
    const long colblk = blockIdx.x % p.ncolblk;
    const long chunk = (blockIdx.x / p.ncolblk) * 4 + wid;
    const long col0 = colblk * CW;
    for (int idx = tid; idx < KP * (CW / 4); idx += 256) {     // stage H[0:KP][col0:col0+CW] (zero outside k x n)
        const int jj = idx / (CW / 4), c4 = (idx % (CW / 4)) * 4;
        float d[4];
        load_vec<4, FAST>(d, p.H + (long)jj * p.ldh, col0 + c4, p.n, jj < p.k);
        *reinterpret_cast<f32x4*>(&smem[jj * CW + c4]) = f32x4{d[0], d[1], d[2], d[3]};
    }
    __syncthreads();
    if (chunk >= nchunks) return;

    f32x16 outn[KT][NT], outd[KT][NT];
#pragma unroll
    for (int ke = 0; ke < KT; ++ke)
#pragma unroll
        for (int ne = 0; ne < NT; ++ne)
#pragma unroll
            for (int r = 0; r < 16; ++r) { outn[ke][ne][r] = 0.f; outd[ke][ne][r] = 0.f; }
    long rb1 = (chunk + 1) * rowblks_per_chunk;
    if (rb1 > p.nrowblk) rb1 = p.nrowblk;
    for (long rb = chunk * rowblks_per_chunk; rb < rb1; ++rb) {
        const long row0 = rb * 32;
        float areg[16][NT];   // A[row0 + crow(r,h)][col0 + NT*li + ne], requested first; becomes u_n
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long row = row0 + crow(r, h);
            load_vec<NT, FAST>(areg[r], p.A + row * p.lda, col0 + NT * li, p.n, row < p.m);
        }
        f32x16 acc[NT];       // S, then u_d
#pragma unroll
        for (int ne = 0; ne < NT; ++ne)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ne][r] = 0.f;
        const long wrow = row0 + li;
#pragma unroll
        for (int s = 0; s < 4 * KT; ++s) {  // S = W H: contraction jj = 8s + 4h + e
            float a[4];
            load_vec<4, FAST>(a, p.W + wrow * p.ldw, 8 * s + 4 * h, p.k, wrow < p.m);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int jj = 8 * s + 4 * h + e;
                float b[NT];
                load_vec_raw<NT>(b, &smem[jj * CW + NT * li]);
#pragma unroll
                for (int ne = 0; ne < NT; ++ne) acc[ne] = MFMA32(a[e], b[ne], acc[ne]);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int ne = 0; ne < NT; ++ne) {
                float x, y;
                masked_pair<MODE>(areg[r][ne], acc[ne][r], p.eps, p.pexp, x, y);
                areg[r][ne] = x;
                acc[ne][r] = y;
            }
        // out[ke][ne] += sum_i W[i][KT*li + ke] * u[i][c]: A-operand lane (li, h) holds W[row0 + crow(r,h)][KT*li + ke]
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long row = row0 + crow(r, h);
            float w[KT];
            load_vec<KT, FAST>(w, p.W + row * p.ldw, (long)KT * li, p.k, row < p.m);
#pragma unroll
            for (int ke = 0; ke < KT; ++ke)
#pragma unroll
                for (int ne = 0; ne < NT; ++ne) {
                    outn[ke][ne] = MFMA32(w[ke], areg[r][ne], outn[ke][ne]);
                    outd[ke][ne] = MFMA32(w[ke], acc[ne][r], outd[ke][ne]);
                }
        }
    }
    float* Pn = p.P + chunk * p.chunk_stride;
    float* Pd = Pn + half_stride;
#pragma unroll
    for (int ke = 0; ke < KT; ++ke)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = KT * crow(r, h) + ke;
            float dn[NT], dd[NT];
#pragma unroll
            for (int ne = 0; ne < NT; ++ne) { dn[ne] = outn[ke][ne][r]; dd[ne] = outd[ke][ne][r]; }
            store_vec<NT, true>(dn, Pn + (long)j * p.ldp, col0 + (long)NT * li, p.ldp, true);
            store_vec<NT, true>(dd, Pd + (long)j * p.ldp, col0 + (long)NT * li, p.ldp, true);
        }
}

// ---- the endings: the partials added in part order, then either the pair stored (num, den with leading dimension ldo: the two halves
// of one contiguous buffer where the sums cross ranks) or the rule applied in place, max(., eps) with clamp.  The rule: the ratio,
// X <- X * (num / (den + eps)) (the masked rules; the expression of dnmf_csr_ratio_update, which follows an allreduce of the stored
// pair), or with RULE_SQRT its square root, X <- X * sqrt(num / (den + eps)) (the Itakura-Saito rule, csrc/dnmf_is.h), or with
// RULE_POW its power with a runtime exponent, X <- X * (num / (den + eps))^gamma (the beta-divergence rule, csrc/dnmf_beta.h: gamma = 1
// takes the plain ratio; powf(0, gamma) is 0 for gamma > 0, so a quotient of 0 gives 0, not NaN).  `gamma` is read by RULE_POW alone
enum { RULE_RATIO = 0, RULE_SQRT = 1, RULE_POW = 2 };
template <int RULE>
__device__ __forceinline__ float pair_rule(float x, float a, float b, float eps, int clamp, float gamma = 1.f) {
    const float q = a / (b + eps);
    float f;
    if constexpr (RULE == RULE_POW) f = gamma == 1.f ? q : powf(q, gamma);
    else f = RULE == RULE_SQRT ? sqrtf(q) : q;
    const float y = x * f;
    return clamp ? fmaxf(y, eps) : y;
}

template <int RULE>
__global__ __launch_bounds__(256) void masked_reduce_kernel(const float* __restrict__ P, long part_stride, long half_stride, long ldp,
                                                          int nparts, long rows, long cols, float* __restrict__ num,
                                                          float* __restrict__ den, long ldo, float* __restrict__ X, long ldx, float eps,
                                                          int clamp, float gamma) {
    const long total = rows * cols;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / cols, c = idx % cols;
        const float* q = P + r * ldp + c;
        float a = q[0], b = q[half_stride];
        for (int s = 1; s < nparts; ++s) {
            a += q[s * part_stride];
            b += q[s * part_stride + half_stride];
        }
        if (X) {
            X[r * ldx + c] = pair_rule<RULE>(X[r * ldx + c], a, b, eps, clamp, gamma);
        } else {
            num[r * ldo + c] = a;
            den[r * ldo + c] = b;
        }
    }
}

// ---- the rule on a stored pair (after its allreduce on a 1D grid): pair_rule as in the ending above
template <int RULE>
__global__ __launch_bounds__(256) void pair_ratio_kernel(float* __restrict__ X, long rows, long cols, long ldx, const float* __restrict__ num,
                                                         const float* __restrict__ den, long ldo, float eps, int clamp, float gamma) {
    const long total = rows * cols;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / cols, c = idx % cols;
        X[r * ldx + c] = pair_rule<RULE>(X[r * ldx + c], num[r * ldo + c], den[r * ldo + c], eps, clamp, gamma);
    }
}

// ---- sum over Omega of (a - d)^2 (pyDNMF.py:205-218 over the observed positions): resid_kernel's tiles with the select; fp32 per tile
// and lane (64 terms), float64 from there on, ending the way the dense residual does
template <int KT, bool FAST>
__global__ __launch_bounds__(256) void masked_resid_kernel(NnArgs p) {
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long gw = (long)blockIdx.x * 4 + wid;
    double total = 0.0;
    if (gw < p.nrowblk * p.ncolblk) {
        const long row0 = (gw / p.ncolblk) * 32, col0 = (gw % p.ncolblk) * 128;
        f32x16 acc[4];
        nn_tile<KT, 4, FAST, false>(acc, p.W, p.ldw, p.m, p.k, p.H, p.ldh, p.n, row0, col0, li, h);
        float part = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long row = row0 + crow(r, h);
            float a[4];
            load_vec<4, FAST>(a, p.A + row * p.lda, col0 + 4 * li, p.n, row < p.m);
#pragma unroll
            for (int ne = 0; ne < 4; ++ne) {
                // outside the block a = 0 and acc = 0 (zero-filled operands): an observed zero that is reproduced exactly
                const float d = (a[ne] == a[ne]) ? a[ne] - acc[ne][r] : 0.f;
                part = fmaf(d, d, part);
            }
        }
        total = (double)part;
    }
    block_atomic_sum(total, p.out);
}

// ---- per-column error over Omega (PyNMF.column_err, pyDNMF.py:221-239 with both sums over the observed positions): colerr_kernel of
// csrc/dnmf_nn.h with the select above and without atomics -- col_sums_kernel<KT, FAST, MaskedErrTerm> of csrc/dnmf_sums.h, launched by
// col_sums below.

// out[0] = sum over Omega of a^2, out[1] = |Omega| (both float64; the count is exact below 2^53)
__global__ __launch_bounds__(256) void masked_sqnorm_kernel(const float* __restrict__ A, long m, long n, long lda, double* __restrict__ out) {
    double s = 0.0, cnt = 0.0;
    const long total = m * n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const float a = A[(idx / n) * lda + idx % n];
        if (a == a) { s += (double)a * (double)a; cnt += 1.0; }
    }
    block_atomic_sum(s, out);
    __syncthreads();                       // (block_atomic_sum's shared slots are read by thread 0 after its barrier)
    block_atomic_sum(cnt, out + 1);
}

// ================================================================================================ host side
// The ONE launch path of the pair kernels above: plans, launchers of both sides, the ending, the plan report and the chain of a whole
// fit, templated on MODE so that a translation unit instantiates only the kernels of the modes it launches (csrc/dnmf_masked.hip:
// PAIR_FRO and PAIR_KL; csrc/dnmf_is.hip: PAIR_IS; csrc/dnmf_beta.hip: PAIR_BETA).

// What a mode chooses: its two plan parameters (below), the form of its rule, and how the messages name its kernels.  The masked
// modes take these; csrc/dnmf_is.h states the Itakura-Saito ones, csrc/dnmf_beta.h those of a general beta.
template <int MODE>
struct PairMode {
    static constexpr int zdim128 = 2;           // parts of the output columns at KP = 128: JT = KT / zdim128 tiles per workgroup
    static constexpr long min_chunks = 1;       // the fewest row chunks the H side asks for
    static constexpr int rule = RULE_RATIO;     // pair_rule's RULE
    static constexpr const char* serves = "masked dense data";
};

// W side: 128-row tiles x column splits (x zdim128 = KT / JT parts of the output columns at KP = 128: 2 with JT = 2); splits are whole
// 32-column tiles
struct MaskedUhtPlan { long rowtiles; int zdim; long cols_per_split; int nsplit; size_t bytes; };
MaskedUhtPlan plan_masked_uht(long m, long n, int kt, int zdim128) {
    MaskedUhtPlan u{};
    u.rowtiles = cdiv(m, 128);
    u.zdim = kt == 4 ? zdim128 : 1;
    const long tiles = cdiv(n, BK);
    long ns = std::max<long>(1, 512 / (u.rowtiles * u.zdim));       // about two workgroups per CU
    ns = std::min<long>(std::min<long>(ns, tiles), 32);
    u.cols_per_split = cdiv(tiles, ns) * BK;
    u.nsplit = (int)cdiv(n, u.cols_per_split);
    u.bytes = (size_t)u.nsplit * 2 * m * (32 * kt) * sizeof(float);
    return u;
}

// H side: column blocks of CW = 32 NT columns x row chunks (a wave per chunk).  min_chunks: the fewest chunks to ask for (a workgroup
// is four chunks: with fewer, waves of every workgroup idle)
struct MaskedWtuPlan { int nt; int ncolblk; long ldp; long nrowblk; long rowblks_per_chunk; long nchunks; size_t bytes; };
MaskedWtuPlan plan_masked_wtu(long m, long n, int kt, long min_chunks) {
    MaskedWtuPlan w{};
    w.nt = kt == 1 ? 4 : (kt == 2 ? 2 : 1);
    w.ncolblk = (int)cdiv(n, 32 * w.nt);
    w.ldp = (long)w.ncolblk * 32 * w.nt;
    w.nrowblk = cdiv(m, 32);
    const long want = std::min<long>(std::max<long>(min_chunks, 1024 / w.ncolblk), 64);   // about a wave per SIMD
    w.rowblks_per_chunk = std::max<long>(1, cdiv(w.nrowblk, want));
    w.nchunks = cdiv(w.nrowblk, w.rowblks_per_chunk);
    w.bytes = (size_t)w.nchunks * 2 * (32 * kt) * w.ldp * sizeof(float);
    return w;
}

// per-column error: 128-column blocks x row chunks (a wave per chunk and column block).  About two waves per SIMD, and at most 256
// chunks: the ending adds a column's chunk sums one after another.  `per_col`: float64 sums a chunk leaves per column (the masked
// error's pair: 2; the Itakura-Saito per-column divergence of csrc/dnmf_is.h: 1)
struct MaskedColerrPlan { long ncolblk; long ldc; long nrowblk; long rowblks_per_chunk; long nchunks; size_t bytes; };
MaskedColerrPlan plan_masked_colerr(long m, long n, int per_col = 2) {
    MaskedColerrPlan c{};
    c.ncolblk = cdiv(n, 128);
    c.ldc = c.ncolblk * 128;
    c.nrowblk = cdiv(m, 32);
    const long want = std::min<long>(std::max<long>(1, 2048 / c.ncolblk), 256);
    c.rowblks_per_chunk = std::max<long>(1, cdiv(c.nrowblk, want));
    c.nchunks = cdiv(c.nrowblk, c.rowblks_per_chunk);
    c.bytes = (size_t)c.nchunks * per_col * c.ldc * sizeof(double);
    return c;
}

template <int MODE> MaskedUhtPlan pair_uht_plan(long m, long n, int kt) { return plan_masked_uht(m, n, kt, PairMode<MODE>::zdim128); }
template <int MODE> MaskedWtuPlan pair_wtu_plan(long m, long n, int kt) { return plan_masked_wtu(m, n, kt, PairMode<MODE>::min_chunks); }

// the slabs of one step: the larger side's
template <int MODE>
size_t pair_step_bytes(long m, long n, int kt) {
    return align256(std::max(pair_uht_plan<MODE>(m, n, kt).bytes, pair_wtu_plan<MODE>(m, n, kt).bytes));
}

// the two runtime scalars of a mode whose step and rule take one each (PAIR_BETA: e = beta - 2 and gamma(beta)); every other mode
// leaves them at what changes nothing
struct PairExp { float e = 0.f; float gamma = 1.f; };

NnArgs masked_args(const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k, float eps) {
    NnArgs a{};                                 // (pexp = 0: the caller of a PAIR_BETA launch sets it)
    a.A = A; a.lda = lda; a.m = m; a.n = n; a.W = W; a.ldw = ldw; a.H = H; a.ldh = ldh; a.k = k; a.eps = eps; a.kreal = k;
    a.nrowblk = cdiv(m, 32); a.ncolblk = (int)cdiv(n, 128);
    return a;
}

bool masked_fast(const float* A, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k) {
    return aligned16(A) && aligned16(W) && aligned16(H) && lda % 4 == 0 && n % 4 == 0 && ldw % 4 == 0 && k % 4 == 0 && ldh % 4 == 0;
}

// workgroups of masked_reduce_kernel (256 output elements each per grid-stride trip) for rows x cols outputs
long masked_reduce_grid(long rows, long cols) { return std::min<long>(cdiv(rows * cols, 256), 8192); }

template <int MODE>
int pair_reduce(const float* P, long part_stride, long half_stride, long ldp, int nparts, long rows, long cols, float* num, float* den,
                long ldo, float* X, long ldx, float eps, int clamp, hipStream_t st, const char* who, float gamma = 1.f) {
    const unsigned grid = (unsigned)masked_reduce_grid(rows, cols);
    hipLaunchKernelGGL(masked_reduce_kernel<PairMode<MODE>::rule>, dim3(grid), dim3(256), 0, st, P, part_stride, half_stride, ldp, nparts,
                       rows, cols, num, den, ldo, X, ldx, eps, clamp, gamma);
    return check_launch(who);
}

// the rule of MODE on a stored pair
template <int MODE>
int pair_ratio_update(const char* who, float* X, long rows, long cols, long ldx, const float* num, const float* den, long ldo, float eps,
                      int clamp, void* stream, float gamma = 1.f) {
    REQUIRE(X && num && den && rows >= 1 && cols >= 1 && ldx >= cols && ldo >= cols, "%s: null pointer or bad shape", who);
    const unsigned grid = (unsigned)masked_reduce_grid(rows, cols);
    hipLaunchKernelGGL(pair_ratio_kernel<PairMode<MODE>::rule>, dim3(grid), dim3(256), 0, S(stream), X, rows, cols, ldx, num, den, ldo, eps,
                       clamp != 0, gamma);
    return check_launch(who);
}

// ---- the sums of csrc/dnmf_sums.h.  `serves` names the kernels in the rank message, as PairMode<MODE>::serves does for the pairs.
#define SUMS_CHECKS(who, serves, outs_ok)                                                                                  \
    const int kt = kt_of(k);                                                                                               \
    REQUIRE(kt > 0, "%s: rank k=%d unsupported (1 <= k <= %d for %s)", who, k, DNMF_TUNED_MAX_K, serves);                  \
    REQUIRE(A && W && H && (outs_ok) && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n, "%s: null pointer or bad shape", who)
// f(KtFast<KT, FAST>{}) for the rank's KT and the operands' alignment
template <int KT_, bool FAST_> struct KtFast { static constexpr int KT = KT_; static constexpr bool FAST = FAST_; };
template <class F>
void with_kt_fast(int kt, bool fast, F f) {
    if (kt == 1) { if (fast) f(KtFast<1, true>{}); else f(KtFast<1, false>{}); }
    else if (kt == 2) { if (fast) f(KtFast<2, true>{}); else f(KtFast<2, false>{}); }
    else { if (fast) f(KtFast<4, true>{}); else f(KtFast<4, false>{}); }
}

// per column: out0[c] (and out1[c] where the Term has two sums) over the block's rows
template <class Term>
int col_sums(const char* who, const char* serves, const float* A, long m, long n, long lda, const float* W, long ldw, const float* H,
             long ldh, int k, float eps, Term term, double* out0, double* out1, void* ws, size_t ws_bytes, void* stream) {
    SUMS_CHECKS(who, serves, out0 && (Term::NSUM == 1 || out1));
    const MaskedColerrPlan c = plan_masked_colerr(m, n, Term::NSUM);
    if (!ws || ws_bytes < c.bytes || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, c.bytes);
    hipStream_t st = S(stream);
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    double* P = (double*)ws;
    const dim3 grid((unsigned)cdiv(c.nchunks * c.ncolblk, 4)), block(256);
    with_kt_fast(kt, fast, [&](auto v) { col_sums_launch<v.KT, v.FAST>(grid, block, st, a, P, c.ldc, c.rowblks_per_chunk, term); });
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(col_sums_reduce_kernel<Term::NSUM>, dim3((unsigned)std::min<long>(cdiv(n, 256), 4096)), dim3(256), 0, st,
                       (const double*)P, c.ldc, c.nchunks, n, out0, out1);
    return check_launch(who);
}

size_t col_sums_ws_bytes(long m, long n, int k, int per_col) {
    if (kt_of(k) < 0 || m < 1 || n < 1) return 0;
    return align256(plan_masked_colerr(m, n, per_col).bytes);
}

// the launch plan of col_sums as numbers (host arithmetic, no GPU)
int col_sums_plan_report(const char* who, const char* serves, long m, long n, int k, int per_col, long* out) {
    REQUIRE(kt_of(k) > 0, "%s: rank k=%d unsupported (1 <= k <= %d for %s)", who, k, DNMF_TUNED_MAX_K, serves);
    REQUIRE(out && m >= 1 && n >= 1, "%s: null pointer or bad shape", who);
    const MaskedColerrPlan c = plan_masked_colerr(m, n, per_col);
    out[0] = c.rowblks_per_chunk;       // 32-row blocks a wave walks (the last chunk may hold fewer)
    out[1] = c.nchunks;
    out[2] = c.ncolblk;                 // 128-column blocks (the last may be ragged)
    return DNMF_OK;
}

// one scalar: the divergence leaves one double per 32 x 128 tile
size_t div_bytes(long m, long n) { return (size_t)cdiv(m, 32) * cdiv(n, 128) * sizeof(double); }

template <class Term>
int tile_sum(const char* who, const char* serves, const float* A, long m, long n, long lda, const float* W, long ldw, const float* H,
             long ldh, int k, float eps, Term term, double* out, void* ws, size_t ws_bytes, void* stream) {
    SUMS_CHECKS(who, serves, out);
    const size_t need = div_bytes(m, n);
    if (!ws || ws_bytes < need || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    hipStream_t st = S(stream);
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    const long tiles = a.nrowblk * a.ncolblk;
    double* P = (double*)ws;
    const dim3 grid((unsigned)cdiv(tiles, 4)), block(256);
    with_kt_fast(kt, fast, [&](auto v) { hipLaunchKernelGGL((tile_sum_kernel<v.KT, v.FAST, Term>), grid, block, 0, st, a, P, term); });
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(slot_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)P, tiles, out);
    return check_launch(who);
}
#undef SUMS_CHECKS

// ---- what the modes with a divergence (PAIR_IS, PAIR_BETA) share beyond the pairs: one workspace serves a step and the divergence
template <int MODE>
size_t div_step_bytes(long m, long n, int kt) { return align256(std::max(pair_step_bytes<MODE>(m, n, kt), div_bytes(m, n))); }

// the W side into partial slabs, then the ending: (num, den) stored, or X = W updated in place
template <int MODE>
int pair_w_side(const char* who, const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                float eps, float* num, float* den, long ldo, float* X, void* ws, size_t ws_bytes, void* stream, PairExp px = {}) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "%s: rank k=%d unsupported (1 <= k <= %d for %s)", who, k, DNMF_TUNED_MAX_K, PairMode<MODE>::serves);
    REQUIRE(A && W && H && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && (X || (num && den && ldo >= k)),
            "%s: null pointer or bad shape", who);
    const MaskedUhtPlan u = pair_uht_plan<MODE>(m, n, kt);
    if (!ws || ws_bytes < u.bytes || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, u.bytes);
    const int kp = 32 * kt;
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    a.pexp = px.e;
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    const long half = m * kp, split = 2 * half;
    const dim3 grid((unsigned)u.rowtiles, (unsigned)u.nsplit, (unsigned)u.zdim), block(256);
    const size_t lds = 2ul * kp * BK * sizeof(float);
    hipStream_t st = S(stream);
    float* P = (float*)ws;
#define PW_CASE(KT_, JT_)                                                                                                              \
    if (kt == KT_) {                                                                                                                   \
        if (fast) hipLaunchKernelGGL((masked_uht_kernel<KT_, JT_, true, MODE>), grid, block, lds, st, a, P, split, half, u.cols_per_split);  \
        else hipLaunchKernelGGL((masked_uht_kernel<KT_, JT_, false, MODE>), grid, block, lds, st, a, P, split, half, u.cols_per_split);      \
    }
    PW_CASE(1, 1) PW_CASE(2, 2) PW_CASE(4, 4 / PairMode<MODE>::zdim128)
#undef PW_CASE
    if (int rc = check_launch(who)) return rc;
    return pair_reduce<MODE>(P, split, half, kp, u.nsplit, m, k, num, den, ldo, X, ldw, eps, 0, st, who, px.gamma);
}

template <int MODE>
int pair_h_side(const char* who, const float* A, long m, long n, long lda, const float* W, long ldw, const float* H, long ldh, int k,
                float eps, float* num, float* den, long ldo, float* X, int clamp, void* ws, size_t ws_bytes, void* stream,
                PairExp px = {}) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "%s: rank k=%d unsupported (1 <= k <= %d for %s)", who, k, DNMF_TUNED_MAX_K, PairMode<MODE>::serves);
    REQUIRE(A && W && H && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && (X || (num && den && ldo >= n)),
            "%s: null pointer or bad shape", who);
    const MaskedWtuPlan w = pair_wtu_plan<MODE>(m, n, kt);
    if (!ws || ws_bytes < w.bytes || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, w.bytes);
    const int kp = 32 * kt;
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    a.ncolblk = w.ncolblk;
    a.pexp = px.e;
    const long half = (long)kp * w.ldp;
    a.P = (float*)ws; a.ldp = w.ldp; a.chunk_stride = 2 * half;
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k);
    const dim3 grid((unsigned)(cdiv(w.nchunks, 4) * w.ncolblk)), block(256);     // 4 row chunks (waves) per workgroup
    const size_t lds = (size_t)kp * 32 * w.nt * sizeof(float);
    hipStream_t st = S(stream);
#define PH_CASE(KT_, NT_)                                                                                                         \
    if (kt == KT_) {                                                                                                              \
        if (fast) hipLaunchKernelGGL((masked_wtu_kernel<KT_, NT_, true, MODE>), grid, block, lds, st, a, half, w.rowblks_per_chunk);    \
        else hipLaunchKernelGGL((masked_wtu_kernel<KT_, NT_, false, MODE>), grid, block, lds, st, a, half, w.rowblks_per_chunk);        \
    }
    PH_CASE(1, 4) PH_CASE(2, 2) PH_CASE(4, 1)
#undef PH_CASE
    if (int rc = check_launch(who)) return rc;
    return pair_reduce<MODE>(a.P, a.chunk_stride, half, w.ldp, (int)w.nchunks, k, n, num, den, ldo, X, ldh, eps, clamp, st, who, px.gamma);
}

// the launch plans of both sides as numbers (host arithmetic, no GPU): what the launches above use, for callers and tests that must
// know which loops of the kernels a shape enters
template <int MODE>
int pair_plan_report(const char* who, long m, long n, int k, long* out) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "%s: rank k=%d unsupported (1 <= k <= %d for %s)", who, k, DNMF_TUNED_MAX_K, PairMode<MODE>::serves);
    REQUIRE(out && m >= 1 && n >= 1, "%s: null pointer or bad shape", who);
    const MaskedUhtPlan u = pair_uht_plan<MODE>(m, n, kt);
    const MaskedWtuPlan w = pair_wtu_plan<MODE>(m, n, kt);
    out[0] = u.cols_per_split / BK;     // 32-column tiles a workgroup of the W side walks (the last split may hold fewer)
    out[1] = u.nsplit;
    out[2] = u.zdim;
    out[3] = w.rowblks_per_chunk;       // 32-row blocks a wave of the H side walks (the last chunk may hold fewer)
    out[4] = w.nchunks;
    out[5] = w.nrowblk;
    return DNMF_OK;
}

// workspace of a whole fit: the step's slabs, the partials of the column sums of W (dnmf_colsum: at most 1024 slabs of KP floats), the
// sums themselves, and 256 bytes for the doubles of the error ({resid, ||A||^2}; masked: {resid, ||P(A)||^2, |Omega|})
struct PairFitWs { size_t step; size_t part_off; size_t part_bytes; size_t cs_off; size_t sq_off; size_t total; };
PairFitWs pair_fit_layout(size_t step, int k) {
    PairFitWs f{};
    const size_t kp = 32 * (size_t)kt_of(k);
    f.step = step;
    f.part_off = f.step;
    f.part_bytes = align256(1024 * kp * sizeof(float));
    f.cs_off = f.part_off + f.part_bytes;
    f.sq_off = f.cs_off + align256(kp * sizeof(float));
    f.total = f.sq_off + 256;
    return f;
}

// workspace of a step, or of a whole fit, of a mode with a divergence; 0 for a rank or a shape its kernels do not serve
template <int MODE>
size_t div_ws_bytes(long m, long n, int k, bool fit) {
    const int kt = kt_of(k);
    if (kt < 0 || m < 1 || n < 1) return 0;
    const size_t step = div_step_bytes<MODE>(m, n, kt);
    return fit ? pair_fit_layout(step, k).total : step;
}

// the launch plans of both sides and of their endings as numbers (host arithmetic, no GPU)
template <int MODE>
int div_plan_report(const char* who, long m, long n, int k, long* out) {
    if (int rc = pair_plan_report<MODE>(who, m, n, k, out)) return rc;
    out[6] = masked_reduce_grid(m, k);  // workgroups (256 outputs each per grid-stride trip) of the W side's ending
    out[7] = masked_reduce_grid(k, n);  // and of the H side's
    return DNMF_OK;
}

// pyDNMF.py:138-182 under a pair rule on one rank: the launches the step loop makes, in its order, with nothing in between.  The rule
// is its two step calls (step_w(bytes), step_h(clamp, bytes), on the first `bytes` = step_bytes(m, n, kt) of the workspace) and the two
// squared norms of its error (resid(sq), sqnorm(sq + 1))
template <int MODE, class StepW, class StepH, class Resid, class Sqnorm>
int pair_mu_fit(const char* who, size_t (*step_bytes)(long, long, int), const float* A, long m, long n, long lda, float* W, long ldw,
                float* H, long ldh, int k, float eps, int w_update, int itr, double* sq_out, void* ws, size_t ws_bytes, void* stream,
                StepW step_w, StepH step_h, Resid resid, Sqnorm sqnorm) {
    const int kt = kt_of(k);
    REQUIRE(kt > 0, "%s: rank k=%d unsupported (1 <= k <= %d for %s)", who, k, DNMF_TUNED_MAX_K, PairMode<MODE>::serves);
    REQUIRE(A && W && H && sq_out && m >= 1 && n >= 1 && lda >= n && ldw >= k && ldh >= n && itr >= 0,
            "%s: null pointer or bad shape (m=%ld n=%ld k=%d itr=%d)", who, m, n, k, itr);
    const PairFitWs f = pair_fit_layout(step_bytes(m, n, kt), k);
    if (!ws || ws_bytes < f.total || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, f.total);
    char* base = (char*)ws;
    int rc = DNMF_OK;
    for (int i = 0; i < itr; ++i) {                                                                   // pyDNMF.py:151-172
        const int clamp = (i % 10 == 0);
        if (w_update && (rc = step_w(f.step))) return rc;
        if ((rc = step_h(clamp, f.step))) return rc;
        if (clamp && (rc = dnmf_clamp_min(W, m, k, ldw, eps, stream))) return rc;
    }
    // normalize_features (pyDNMF.py:185-194): s = column sums of W; W /= s + eps; H *= s^T
    float* s = (float*)(base + f.cs_off);
    if ((rc = dnmf_colsum(W, m, k, ldw, s, base + f.part_off, f.part_bytes, stream))) return rc;
    if ((rc = dnmf_scale_cols_div(W, m, k, ldw, s, eps, stream))) return rc;
    if ((rc = dnmf_scale_rows_mul(H, k, n, ldh, s, stream))) return rc;
    // relative_err (pyDNMF.py:205-218); the caller takes the square roots
    double* sq = (double*)(base + f.sq_off);
    if ((rc = resid(sq))) return rc;
    if ((rc = sqnorm(sq + 1))) return rc;
    if (hipMemcpyAsync(sq_out, sq, 2 * sizeof(double), hipMemcpyDeviceToDevice, S(stream)) != hipSuccess)
        return fail(DNMF_EHIP, "%s: copy of the squared norms failed", who);
    return DNMF_OK;
}

}  // namespace
