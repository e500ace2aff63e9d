// dnmf_weighted.h -- per-entry weights for the MU pair rules (fro, kl, is, beta): objective sum_ij v_ij d(a_ij | (W H)_ij), V >= 0 of A's shape.
// Part of libdnmf_hip.so (kernels live in anonymous namespaces of the headers; the translation units csrc/*.hip include what they launch).
//
// Padding and gaps, all four modes: the kernels' test is v > 0, and where it fails u_n = u_d = 0 by a SELECT placed before the second
// product, whatever `a` and S hold there (NaN, inf, 0, negative) -- and a V load outside the block returns 0, so a padded position is a gap.
//
// With S' = W H + eps, F = H^T on the W side and F = W on the H side, and (u_n, u_d) the mode's own pair (masked_pair<MODE> of
// csrc/dnmf_masked.h), a side is
//     num = (V . u_n) F,   den = (V . u_d) F,   X <- X . rule(num / (den + eps))
// with the mode's own rule (pair_rule: ratio, sqrt, pow gamma(beta)) and clamp schedule.  Every term of the mode's majoriser is scaled
// by v_ij >= 0, so this is the majorisation-minimisation rule of the weighted objective, which never increases.  v = 0 is "not
// observed": weights = ~isnan(A) is the masked rule of any mode, with no mask semantics of its own.
//
// The kernels are new ones, not a fifth mode of the pair kernels: V is a second m x n operand of the element-wise step, which those
// have no way to bring there.  What they keep is the mode's launch geometry number for number (pair_uht_plan<MODE>, pair_wtu_plan<MODE>:
// splits, chunks, zdim) and the order in which every accumulator chain receives its products, so that the partial sums are the
// unweighted kernels' where V is 0/1 (x * 1 is exact) -- bit for bit -- and the endings (masked_reduce_kernel<RULE>) are reused unchanged.
//
// W side, weighted_uht_kernel.  A workgroup owns 128 rows, a lane its row of A and of V; the H tile is double-buffered in LDS.  The
// unweighted kernel turns a whole 32-column S^T tile into (u_n, u_d) -- 32 registers -- and then runs the second products over it.  Here
// the element-wise step is QUARTERED: for each quarter g of the tile's columns (the four columns one lane holds of a_cur[g], v_cur[g] and
// st[4g..4g+3]) the pair of four elements is formed -- 8 live registers, not 32 -- and consumed at once by that quarter's second products
// into every output tile; a_cur[g] and v_cur[g] are dead from there and are refilled for the next tile right under those MFMAs.  The 24
// registers this saves pay for the 16 of v_cur: every instantiation stays within its unweighted twin's register file, none uses
// scratch (table below).  An accumulator chain on[jt] / od[jt] still receives g = 0..3, e = 0..3 in that order per tile.
//
// H side, weighted_wtu_kernel.  A wave walks 32-row blocks of one 32 NT-column block; areg[16][NT] and vreg[16][NT] are requested
// together before S is formed, the element-wise step runs in place (areg <- u_n, acc <- u_d) and vreg is dead before the second product.
// At KT = 1, NT = 4 the unweighted kernel already fills the register file (256 VGPRs + 228 AGPRs) and 64 more registers of V do not
// fit: there the lane's four column sets are walked in two GROUPS of two -- one group's A, V, S and pair are live at a time, the outputs
// of both stay resident, and a scheduling barrier keeps group 1's loads behind group 0 (hoisted above it they are live next to group 0's
// pair, and the FAST form spills).  Each output chain outn[ke][ne] / outd[ke][ne] belongs to one group and receives r = 0..15 in the
// unweighted order.  The price: group 1's loads are not issued under group 0's first product (DESIGN.md section 7 has the times).
//
// Sums, weighted_tile_sum_kernel: the tile walk of csrc/dnmf_sums.h (a wave per 32 x 128 tile, fp32 per lane and tile, one double per
// wave and sum, the slots added in fixed order by slot_sum_kernel) with V loaded beside A and a term of (a, s, v) selected to 0 where
// v is not positive.  Terms: v (a - s)^2 with v a^2 (the weighted error pair) and v d_beta(a | s') with the arithmetic of BetaDivTerm.
//
// Registers (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage remarks): DESIGN.md section 7, "Per-entry weights".
#pragma once
#include "dnmf_masked.h"
#include "dnmf_is.h"
#include "dnmf_beta.h"

namespace {

// the select and the two multiplies: after masked_pair<MODE>
__device__ __forceinline__ void weigh(float v, float& un, float& ud) {
    const bool on = v > 0.f;
    un = on ? un * v : 0.f;
    ud = on ? ud * v : 0.f;
}

template <int KT, int MODE> struct WeightedJt { static constexpr int value = KT == 4 ? 4 / PairMode<MODE>::zdim128 : KT; };

// ---- W side: P[split][half][m][KP] as masked_uht_kernel leaves it (same grid, same slab)
template <int KT, bool FAST, int MODE>
__global__ __launch_bounds__(256, KT == 4 ? 1 : 2) void weighted_uht_kernel(NnArgs p, const float* __restrict__ V, long ldv,
                                                                            float* __restrict__ P, long split_stride, long half_stride,
                                                                            long cols_per_split) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int JT = WeightedJt<KT, MODE>::value;
    constexpr int KP = 32 * KT, T = 256, STAGE = KP * BK, NY = KP / (T / 8);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
    const long arow = (long)blockIdx.x * 128 + wave * 32 + li;
    const bool rok = arow < p.m;
    const long cbeg = (long)blockIdx.y * cols_per_split;
    long cend = cbeg + cols_per_split;
    if (cend > p.n) cend = p.n;
    const long nt = (cend - cbeg + BK - 1) / BK;
    const int jt0 = (int)blockIdx.z * JT;
    const float* Arow = p.A + arow * p.lda;
    const float* Vrow = V + arow * ldv;

    f32x16 on[JT], od[JT];  // (num)^T and (den)^T tiles: rows j, lanes i
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { on[jt][r] = 0.f; od[jt][r] = 0.f; }
    float wreg[4 * KT][4];   // W[arow][8s + 4h + e]; zero for j >= k and for rows >= m
#pragma unroll
    for (int s = 0; s < 4 * KT; ++s) load_vec<4, FAST>(wreg[s], p.W + arow * p.ldw, 8 * s + 4 * h, p.k, rok);

    f32x4 hst[NY];
    float a_cur[4][4], v_cur[4][4];     // the lane's 16 columns of A and of V in this tile: quarter g = columns 8g + 4h .. + 3
    if (nt > 0) {
        stage_load<KP, T, FAST, false>(hst, p.H, p.ldh, p.k, cend, 0, cbeg, tid);     // zero outside k x [.., cend)
        stage_store<KP, T>(smem, hst, tid);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            load_vec<4, FAST>(a_cur[g], Arow, cbeg + 8 * g + 4 * h, cend, rok);
            load_vec<4, FAST>(v_cur[g], Vrow, cbeg + 8 * g + 4 * h, cend, rok);       // 0 outside the block: a gap
        }
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
        if (more) stage_load<KP, T, FAST, false>(hst, p.H, p.ldh, p.k, cend, 0, c1, tid);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float un[4], ud[4];         // the quarter's pair: live over this quarter's second products only
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                masked_pair<MODE>(a_cur[g][e], st[4 * g + e], p.eps, p.pexp, un[e], ud[e]);
                weigh(v_cur[g][e], un[e], ud[e]);
            }
            if (more) {                 // the quarter's A and V registers are free: the next tile's, under this quarter's MFMAs
                load_vec<4, FAST>(a_cur[g], Arow, c1 + 8 * g + 4 * h, cend, rok);
                load_vec<4, FAST>(v_cur[g], Vrow, c1 + 8 * g + 4 * h, cend, rok);
            }
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                const f32x4 hh = *reinterpret_cast<const f32x4*>(&Hs[lds_idx((jt0 + jt) * 32 + li, 2 * g + h)]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    on[jt] = MFMA32(hh[e], un[e], on[jt]);
                    od[jt] = MFMA32(hh[e], ud[e], od[jt]);
                }
            }
        }
        if (more) stage_store<KP, T>(smem + (cur ^ 1) * STAGE, hst, tid);
        __syncthreads();
    }
    // the epilogue of masked_uht_kernel: whole aligned vectors inside the slab
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

// ---- H side: P[chunk][half][KP][ldp] as masked_wtu_kernel leaves it (same grid, same slab).  The NT column sets of a lane are walked
// in HALVES groups of NH = NT / HALVES: one group's A, V, S and pair are live at a time; the outputs of all groups stay.
template <int KT, int NT, bool FAST, int MODE>
__global__ __launch_bounds__(256, 1) void weighted_wtu_kernel(NnArgs p, const float* __restrict__ V, long ldv, long half_stride,
                                                              long rowblks_per_chunk) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KP = 32 * KT, CW = 32 * NT;
    constexpr int HALVES = NT == 4 ? 2 : 1, NH = NT / HALVES;
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
        const long wrow = row0 + li;
        static_for<0, HALVES>([&](auto hv) {
            constexpr int N0 = hv.value * NH;                   // this group's first column set of the lane's NT
            const long cl = col0 + NT * li + N0;                // and the lane's first column in it
            // (a group's loads stay behind the group before it: hoisted above its second products they would be live next to its pair,
            // which is what the groups are there to avoid -- the FAST form at NT = 4 then spills)
            if constexpr (hv.value > 0) __builtin_amdgcn_sched_barrier(0);
            float areg[16][NH], vreg[16][NH];                   // requested together, first; areg becomes u_n, vreg dies with the step
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long row = row0 + crow(r, h);
                load_vec<NH, FAST>(areg[r], p.A + row * p.lda, cl, p.n, row < p.m);
                load_vec<NH, FAST>(vreg[r], V + row * ldv, cl, p.n, row < p.m);      // 0 outside the block: a gap
            }
            f32x16 acc[NH];       // S, then u_d
#pragma unroll
            for (int ne = 0; ne < NH; ++ne)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ne][r] = 0.f;
#pragma unroll
            for (int s = 0; s < 4 * KT; ++s) {  // S = W H: contraction jj = 8s + 4h + e
                float a[4];
                load_vec<4, FAST>(a, p.W + wrow * p.ldw, 8 * s + 4 * h, p.k, wrow < p.m);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int jj = 8 * s + 4 * h + e;
                    float b[NH];
                    load_vec_raw<NH>(b, &smem[jj * CW + NT * li + N0]);
#pragma unroll
                    for (int ne = 0; ne < NH; ++ne) acc[ne] = MFMA32(a[e], b[ne], acc[ne]);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int ne = 0; ne < NH; ++ne) {
                    float x, y;
                    masked_pair<MODE>(areg[r][ne], acc[ne][r], p.eps, p.pexp, x, y);
                    weigh(vreg[r][ne], x, y);
                    areg[r][ne] = x;
                    acc[ne][r] = y;
                }
            // out[ke][N0 + ne] += sum_i W[i][KT*li + ke] * u[i][c]: A-operand lane (li, h) holds W[row0 + crow(r,h)][KT*li + ke]
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long row = row0 + crow(r, h);
                float w[KT];
                load_vec<KT, FAST>(w, p.W + row * p.ldw, (long)KT * li, p.k, row < p.m);
#pragma unroll
                for (int ke = 0; ke < KT; ++ke)
#pragma unroll
                    for (int ne = 0; ne < NH; ++ne) {
                        outn[ke][N0 + ne] = MFMA32(w[ke], areg[r][ne], outn[ke][N0 + ne]);
                        outd[ke][N0 + ne] = MFMA32(w[ke], acc[ne][r], outd[ke][N0 + ne]);
                    }
            }
        });
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

// ---- the terms of the sums: add(t, a, s, v, eps).  v > 0 selects; a load outside the block gave v = 0
// v (a - s)^2 * scale and, with N = 2, v a^2: the weighted error pair (scale 1), or the Frobenius objective (N = 1, scale 1/2)
template <int N>
struct WeightedErrTerm {
    static constexpr int NSUM = N;
    float scale = 1.f;
    __device__ __forceinline__ void add(float (&t)[N], float a, float s, float v, float) const {
        const bool on = v > 0.f;
        const float d = a - s;
        t[0] += on ? v * (d * d) * scale : 0.f;
        if constexpr (N == 2) t[1] += on ? v * (a * a) : 0.f;
    }
};

// v d_beta(a | s + eps): the arithmetic of BetaDivTerm<FORM, 1> (csrc/dnmf_sums.h), scaled and selected
template <int FORM>
struct WeightedDivTerm {
    static constexpr int NSUM = 1;
    float beta = 0.f, c = 1.f;
    __device__ __forceinline__ void add(float (&t)[1], float a, float s, float v, float eps) const {
        float pw;
        const float d = beta_div_term_pw<FORM>(a, s + eps, beta, c, pw);
        t[0] += v > 0.f ? v * d : 0.f;
    }
};

// ---- tile_sum_kernel of csrc/dnmf_sums.h with V beside A: a wave leaves Term::NSUM doubles, sum j in slot P[j * tiles + tile]
template <int KT, bool FAST, class Term>
__global__ __launch_bounds__(256) void weighted_tile_sum_kernel(NnArgs p, const float* __restrict__ V, long ldv, double* __restrict__ P,
                                                                Term term) {
    constexpr int NS = Term::NSUM;
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long gw = (long)blockIdx.x * 4 + wid, tiles = p.nrowblk * p.ncolblk;
    if (gw >= tiles) return;
    const long row0 = (gw / p.ncolblk) * 32, col0 = (gw % p.ncolblk) * 128;
    f32x16 acc[4];
    nn_tile<KT, 4, FAST, false>(acc, p.W, p.ldw, p.m, p.k, p.H, p.ldh, p.n, row0, col0, li, h);
    float part[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) part[j] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long row = row0 + crow(r, h);
        float a[4], v[4];
        load_vec<4, FAST>(a, p.A + row * p.lda, col0 + 4 * li, p.n, row < p.m);
        load_vec<4, FAST>(v, V + row * ldv, col0 + 4 * li, p.n, row < p.m);
#pragma unroll
        for (int ne = 0; ne < 4; ++ne) term.add(part, a[ne], acc[ne][r], v[ne], p.eps);
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double total = (double)part[j];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) total += __shfl_xor(total, off, 64);
        if (lane == 0) P[j * tiles + gw] = total;
    }
}

// ---- the per-column pair of an NMFk sweep under weights: num[c] and den[c] over the block's rows, v > 0 only (DESIGN.md section 7,
// "NMFk under weights").  add(t, a, s, v, eps) with t[0] the column's numerator and t[1] its scale.
// v (a - s)^2 and v a^2 with the contraction STATED (fmaf): at v in {0, 1} the operations of MaskedErrTerm on A with NaN where v = 0
struct WeightedColErrTerm {
    __device__ __forceinline__ void add(float (&t)[2], float a, float s, float v, float) const {
        const bool on = v > 0.f;
        const float d = on ? a - s : 0.f;
        const float ao = on ? a : 0.f;
        t[0] = fmaf(on ? v * d : 0.f, d, t[0]);
        t[1] = fmaf(on ? v * ao : 0.f, ao, t[1]);
    }
};

// v d_beta(a | s + eps) and v a^beta (v a under kl, v under is: the column's weight sum)
template <int FORM>
struct WeightedColDivTerm {
    float beta = 0.f, c = 1.f;
    __device__ __forceinline__ void add(float (&t)[2], float a, float s, float v, float eps) const {
        float pw;
        const float d = beta_div_term_pw<FORM>(a, s + eps, beta, c, pw);
        const bool on = v > 0.f;
        t[0] += on ? v * d : 0.f;
        t[1] += on ? v * pw : 0.f;
    }
};

// The geometry, the plan (plan_masked_colerr(m, n, 2)), the slab and the ending (col_sums_reduce_kernel<2>) of col_sums_kernel
// (csrc/dnmf_sums.h); its own is the second m x n operand.  KT <= 2 (HOLD): the lane's 16 x 4 weights of a row block live in vreg, one
// buffer.  The chunk's first block requests them before its nn_tile products; from there on row r of the NEXT block is requested into
// vreg[r] where row r of this block has just been consumed, next to the request for row r of A and ahead of the row's terms, so a
// block's V is in flight under the previous block's terms and its own products.  Only a block whose 32 x 128 tile lies inside the
// matrix (a wave-uniform test) is requested ahead, with plain vector loads; a ragged block is loaded predicated at its own top, where
// a V load outside the block returns 0: a gap, with no bounds select.  KT = 4: the carried buffer spills (the products fill the
// register file), so a row's V is requested with its A through predicated loads.  Forms tried and registers: DESIGN.md section 7.
template <int KT, bool FAST, class Term>
__global__ __launch_bounds__(256) void weighted_col_sums_kernel(NnArgs p, const float* __restrict__ V, long ldv, double* __restrict__ P,
                                                                long ldc, long rowblks_per_chunk, Term term) {
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long gw = (long)blockIdx.x * 4 + wid;
    const long nchunks = cdiv(p.nrowblk, rowblks_per_chunk);
    if (gw >= nchunks * p.ncolblk) return;
    const long chunk = gw / p.ncolblk, colblk = gw % p.ncolblk;
    const long col0 = colblk * 128, col = col0 + 4 * li;
    constexpr bool HOLD = KT < 4;                               // vreg is carried over the products (see above)
    const bool cols_in = FAST && col0 + 128 <= p.n;             // wave-uniform: with rows_in(rb), the block's tile is interior
    auto rows_in = [&](long rb) { return rb * 32 + 32 <= p.m; };
    double dv[4][2];
#pragma unroll
    for (int ne = 0; ne < 4; ++ne) dv[ne][0] = dv[ne][1] = 0.0;
    float vreg[16][4];
    bool have = false;                                          // vreg holds this block's weights already (requested a block ago)
    long rb1 = (chunk + 1) * rowblks_per_chunk;
    if (rb1 > p.nrowblk) rb1 = p.nrowblk;
    for (long rb = chunk * rowblks_per_chunk; rb < rb1; ++rb) {
        const long row0 = rb * 32;
        const bool in = cols_in && rows_in(rb);
        const bool pre = HOLD && in && rb + 1 < rb1 && rows_in(rb + 1);  // the next block is interior: its V rows are requested in the walk
        if (HOLD && !have) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long row = row0 + crow(r, h);
                if (in) load_tile_vec<4, FAST, true>(vreg[r], V + row * ldv, col, p.n, true);
                else load_vec<4, FAST>(vreg[r], V + row * ldv, col, p.n, row < p.m);    // 0 outside the block: a gap
            }
        }
        f32x16 acc[4];
        nn_tile<KT, 4, FAST, false>(acc, p.W, p.ldw, p.m, p.k, p.H, p.ldh, p.n, row0, col0, li, h);
        // (the rows of A stay behind the products: hoisted above them, an interior block's 64 registers of A are live next to the
        // products' W and H operands and to vreg, and KT = 4 spills; behind them they take the registers those operands leave)
        __builtin_amdgcn_sched_barrier(0);
        float pv[4][2];
#pragma unroll
        for (int ne = 0; ne < 4; ++ne) pv[ne][0] = pv[ne][1] = 0.f;
        auto walk = [&](auto interior) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long row = row0 + crow(r, h);
                float a[4], v[4];
                load_tile_vec<4, FAST, interior.value>(a, p.A + row * p.lda, col, p.n, row < p.m);
                if constexpr (HOLD) {
#pragma unroll
                    for (int ne = 0; ne < 4; ++ne) v[ne] = vreg[r][ne];
                } else {
                    load_tile_vec<4, FAST, interior.value>(v, V + row * ldv, col, p.n, row < p.m);
                }
                if constexpr (HOLD && interior.value)
                    if (pre) load_tile_vec<4, FAST, true>(vreg[r], V + (row + 32) * ldv, col, p.n, true);
#pragma unroll
                for (int ne = 0; ne < 4; ++ne) term.add(pv[ne], a[ne], acc[ne][r], v[ne], p.eps);
            }
        };
        if constexpr (HOLD) {
            if (in) walk(std::true_type{});
            else walk(std::false_type{});
        } else {
            walk(std::false_type{});
        }
        have = pre;
#pragma unroll
        for (int ne = 0; ne < 4; ++ne) { dv[ne][0] += (double)pv[ne][0]; dv[ne][1] += (double)pv[ne][1]; }
    }
    double* Pc = P + chunk * 2 * ldc + col;
#pragma unroll
    for (int ne = 0; ne < 4; ++ne)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            dv[ne][j] += __shfl_xor(dv[ne][j], 32, 64);
            if (h == 0) Pc[j * ldc + ne] = dv[ne][j];
        }
}

// ================================================================================================ host side
// norm of the C ABI -> MODE: f(std::integral_constant<int, MODE>{})
template <class F>
int with_weighted_mode(int norm, F f) {
    if (norm == 0) return f(std::integral_constant<int, PAIR_FRO>{});
    if (norm == 1) return f(std::integral_constant<int, PAIR_KL>{});
    if (norm == 2) return f(std::integral_constant<int, PAIR_IS>{});
    return f(std::integral_constant<int, PAIR_BETA>{});
}

inline bool weighted_fast(const float* V, long ldv) { return aligned16(V) && ldv % 4 == 0; }

// one workspace serves a step of any mode, the error pair (two slots per tile) and the divergence
size_t weighted_step_bytes(long m, long n, int kt) {
    size_t b = 2 * div_bytes(m, n);
    b = std::max(b, pair_step_bytes<PAIR_FRO>(m, n, kt));
    b = std::max(b, pair_step_bytes<PAIR_KL>(m, n, kt));
    b = std::max(b, pair_step_bytes<PAIR_IS>(m, n, kt));
    b = std::max(b, pair_step_bytes<PAIR_BETA>(m, n, kt));
    return align256(b);
}

#define WEIGHTED_CHECKS(who, extra)                                                                                                  \
    const int kt = kt_of(k);                                                                                                         \
    REQUIRE(kt > 0, "%s: rank k=%d unsupported (1 <= k <= %d for the weighted kernels)", who, k, DNMF_TUNED_MAX_K);                  \
    REQUIRE(A && V && W && H && m >= 1 && n >= 1 && lda >= n && ldv >= n && ldw >= k && ldh >= n && (extra),                         \
            "%s: null pointer or bad shape", who)

// the W side into partial slabs with the mode's own plan, then the mode's ending: (num, den) stored, or X = W updated in place
template <int MODE>
int weighted_w_side(const char* who, const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw,
                    const float* H, long ldh, int k, float eps, float* num, float* den, long ldo, float* X, void* ws, size_t ws_bytes,
                    void* stream, PairExp px) {
    WEIGHTED_CHECKS(who, X || (num && den && ldo >= k));
    const MaskedUhtPlan u = pair_uht_plan<MODE>(m, n, kt);
    if (!ws || ws_bytes < u.bytes || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, u.bytes);
    const int kp = 32 * kt;
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    a.pexp = px.e;
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k) && weighted_fast(V, ldv);
    const long half = m * kp, split = 2 * half;
    const dim3 grid((unsigned)u.rowtiles, (unsigned)u.nsplit, (unsigned)u.zdim), block(256);
    const size_t lds = 2ul * kp * BK * sizeof(float);
    hipStream_t st = S(stream);
    float* P = (float*)ws;
    with_kt_fast(kt, fast, [&](auto v) {
        hipLaunchKernelGGL((weighted_uht_kernel<v.KT, v.FAST, MODE>), grid, block, lds, st, a, V, ldv, P, split, half, u.cols_per_split);
    });
    if (int rc = check_launch(who)) return rc;
    return pair_reduce<MODE>(P, split, half, kp, u.nsplit, m, k, num, den, ldo, X, ldw, eps, 0, st, who, px.gamma);
}

template <int MODE>
int weighted_h_side(const char* who, const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw,
                    const float* H, long ldh, int k, float eps, float* num, float* den, long ldo, float* X, int clamp, void* ws,
                    size_t ws_bytes, void* stream, PairExp px) {
    WEIGHTED_CHECKS(who, X || (num && den && ldo >= n));
    const MaskedWtuPlan w = pair_wtu_plan<MODE>(m, n, kt);
    if (!ws || ws_bytes < w.bytes || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, w.bytes);
    const int kp = 32 * kt;
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    a.ncolblk = w.ncolblk;
    a.pexp = px.e;
    const long half = (long)kp * w.ldp;
    a.P = (float*)ws; a.ldp = w.ldp; a.chunk_stride = 2 * half;
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k) && weighted_fast(V, ldv);
    const dim3 grid((unsigned)(cdiv(w.nchunks, 4) * w.ncolblk)), block(256);     // 4 row chunks (waves) per workgroup
    const size_t lds = (size_t)kp * 32 * w.nt * sizeof(float);
    hipStream_t st = S(stream);
    with_kt_fast(kt, fast, [&](auto v) {
        constexpr int NT = v.KT == 1 ? 4 : (v.KT == 2 ? 2 : 1);
        hipLaunchKernelGGL((weighted_wtu_kernel<v.KT, NT, v.FAST, MODE>), grid, block, lds, st, a, V, ldv, half, w.rowblks_per_chunk);
    });
    if (int rc = check_launch(who)) return rc;
    return pair_reduce<MODE>(a.P, a.chunk_stride, half, w.ldp, (int)w.nchunks, k, n, num, den, ldo, X, ldh, eps, clamp, st, who, px.gamma);
}

// Term::NSUM doubles into out[0..NSUM): the walk, then slot_sum_kernel once per sum
template <class Term>
int weighted_tile_sum(const char* who, const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw,
                      const float* H, long ldh, int k, float eps, Term term, double* out, void* ws, size_t ws_bytes, void* stream) {
    WEIGHTED_CHECKS(who, out);
    const size_t need = Term::NSUM * div_bytes(m, n);
    if (!ws || ws_bytes < need || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    hipStream_t st = S(stream);
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k) && weighted_fast(V, ldv);
    const long tiles = a.nrowblk * a.ncolblk;
    double* P = (double*)ws;
    const dim3 grid((unsigned)cdiv(tiles, 4)), block(256);
    with_kt_fast(kt, fast, [&](auto v) {
        hipLaunchKernelGGL((weighted_tile_sum_kernel<v.KT, v.FAST, Term>), grid, block, 0, st, a, V, ldv, P, term);
    });
    if (int rc = check_launch(who)) return rc;
    for (int j = 0; j < Term::NSUM; ++j) {
        hipLaunchKernelGGL(slot_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)(P + j * tiles), tiles, out + j);
        if (int rc = check_launch(who)) return rc;
    }
    return DNMF_OK;
}

// num[0..n) and den[0..n): the walk into the chunks' slab rows, then col_sums_reduce_kernel<2>
template <class Term>
int weighted_col_sums(const char* who, const float* A, long m, long n, long lda, const float* V, long ldv, const float* W, long ldw,
                      const float* H, long ldh, int k, float eps, Term term, double* num, double* den, void* ws, size_t ws_bytes,
                      void* stream) {
    WEIGHTED_CHECKS(who, num && den);
    const MaskedColerrPlan c = plan_masked_colerr(m, n, 2);
    if (!ws || ws_bytes < c.bytes || !aligned16(ws)) return fail(DNMF_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, c.bytes);
    hipStream_t st = S(stream);
    NnArgs a = masked_args(A, m, n, lda, W, ldw, H, ldh, k, eps);
    const bool fast = masked_fast(A, n, lda, W, ldw, H, ldh, k) && weighted_fast(V, ldv);
    double* P = (double*)ws;
    const dim3 grid((unsigned)cdiv(c.nchunks * c.ncolblk, 4)), block(256);
    with_kt_fast(kt, fast, [&](auto v) {
        hipLaunchKernelGGL((weighted_col_sums_kernel<v.KT, v.FAST, Term>), grid, block, 0, st, a, V, ldv, P, c.ldc, c.rowblks_per_chunk,
                           term);
    });
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(col_sums_reduce_kernel<2>, dim3((unsigned)std::min<long>(cdiv(n, 256), 4096)), dim3(256), 0, st, (const double*)P,
                       c.ldc, c.nchunks, n, num, den);
    return check_launch(who);
}
#undef WEIGHTED_CHECKS

}  // namespace
