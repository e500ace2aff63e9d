// dnmf_f64_div.h -- Itakura-Saito and the beta-divergence, -2 <= beta <= 4, in float64 on the fp64 matrix cores (included by
// csrc/dnmf_f64_div.hip).  The rule is the one of csrc/dnmf_is.h / csrc/dnmf_beta.h (Fevotte & Idier 2011, scikit-learn's), in the
// dtype of the data as the reference computes (pyDNMF.py:68).  With eps the float64 machine epsilon, F = H^T (W side) or W (H side):
//   IS:    R = 1 / (W H + eps)                u_n = A . R . R    u_d = R          X <- X . sqrt(num / (den + eps))
//   beta:  S' = W H + eps, P = S'^(beta - 2)  u_n = A . P        u_d = S' . P     X <- X . (num / (den + eps))^gamma(beta)
//   num = u_n F,  den = u_d F;  gamma = 1 / (2 - beta) for beta < 1, 1 for 1 <= beta <= 2, 1 / (beta - 1) for beta > 2;  beta = 0 takes the IS pair.
//
// Structure (that of csrc/dnmf_f64_kl.h, with a pair where KL has one quotient).  A wave forms a 16 x 16 tile of W H with
// v_mfma_f64_16x16x4_f64 in the orientation whose C/D layout (col = i, row = q + 4 reg) is an operand layout of the next MFMA, turns
// its four elements per lane into (u_n, u_d) in registers and feeds BOTH into two second products that share every F operand:
//   W side (f64_div_uht_kernel): first product transposed, lane (i, q) holds element [row i][col q + 4 reg] = an A-operand of step
//     `reg`; the wave keeps its RT x 16 rows of W in registers and walks the columns of its split;
//   H side (f64_div_wtu_kernel): first product as written, lane (i, q) holds [row q + 4 reg][col i] = a B-operand; the wave keeps
//     its k x 16 CT piece of H in registers and walks the rows of its chunk.
// Nothing moves between lanes, no m x n image is written, no LDS: operands go from memory to registers through buffer descriptors
// (csrc/dnmf_f64_ops.h), 16-byte accesses where rows allow (VEC), A several tiles ahead in a register ring, the small operand one tile.
//
// Two accumulator sets.  num and den double the accumulators of the KL kernels, so their RT / CT do not carry over:
//   W side  RT = 2 row tiles at every NT: 2 x RT x NT accumulators of 4 doubles (k = 64: 64 doubles = 128 registers), RT x 4 NT doubles of
//           W, the ring of A three tiles deep (two at NT = 4, where a third sends the element-wise loads of the generic kernel to
//           scratch), the H operands one tile ahead;
//   H side  CT = 4 / 4 / 2 column tiles at NT = 1 / 2 / 4: 2 x NT x CT accumulators (k = 64: 64 doubles), 4 NT x CT doubles of H.
// A workgroup is four waves at one wave per SIMD (launch bounds 256: 512 registers a lane, accumulators in AGPRs where hipcc puts
// them).  Registers from hipcc's kernel-resource-usage remarks: DESIGN.md section 7; no instantiation uses scratch.
//
// The element-wise step.  fp64 vector instructions do not overlap with fp64 MFMAs on gfx950 (tools/f64clock.hip), so the step is the
// cost centre and the exponent class is a launch-time mode (template PM), never a per-element branch:
//   PM_IS    r = rcp(s') refined by two Newton steps (div_pos64 without its quotient): u_d = r, u_n = (a r) r.  No division fix-up, no
//            range scaling: s' >= eps and r^2 <= 2^104.
//   PM_HALF  2 (beta - 2) is an integer h in [-8, 4] (beta = -2, -1.5, ..., 4): P = b^(|h| / 2) [. s'^(+-1/2) if h is odd] with
//            b = s' (h > 0) or the refined reciprocal (h < 0), |h| / 2 <= 4 multiplies in a wave-uniform loop, and the odd half from
//            v_rsq_f64 with two Newton steps (sqrt s' = s' rsq s').  h = 0 (beta = 2): P = 1 exactly.
//   PM_GEN   any other beta: P = pow(s', beta - 2), the double-precision library function (below 1 ulp).
// Each refined value is within about 2 ulp (two Newton steps from the 2^-23 of v_rcp_f64 / v_rsq_f64 leave the rounding of the last
// fma), a P of PM_HALF within 2 + |h| / 2 ulp.
//
// Padding adds exactly nothing, without inf or 0 * inf (the argument of csrc/dnmf_masked.h and csrc/dnmf_beta.h in float64).  An A
// load outside the block, outside the wave's column split (W side) or row chunk (H side) returns 0, and so do the loads of H for such
// a column and of W for such a row: S = 0 there, s' = eps = 2^-52 exactly, P = 2^(-52 (beta - 2)).  Within -2 <= beta <= 4 that is
// between 2^-104 (beta = 4) and 2^208 ~ 4e62 (beta = -2) -- finite and normal in float64, as are u_d = s' P in [2^-156, 2^156] and the
// IS pair r = 2^52, r^2 = 2^104 -- so u_n = 0 * P = 0 exactly, and u_d meets an exact zero of F in the second product wherever that
// product contracts over the padded index (W side: over the columns, H[:, c] = 0; H side: over the rows, W[r, :] = 0).  Hence no mask
// on u at all, and the SAME range of beta as in float32.  Where the padded index is an output index (a row >= m of the W side, a
// column >= n of the H side, a factor column j >= k) the sums are finite and are not stored.  A contraction index j >= k is a zero
// column of W and a zero row of H.  Inside the block S >= 0, so s' >= eps and the bounds hold likewise.
//
// Partials and endings.  Every column split (W side) / row chunk (H side) leaves its pair in its own slab of the workspace,
// ws[split][half][rows][pitch]; f64_pair_end_kernel adds the slabs in slab order and either stores (num, den) or applies the rule
// to X -- one function, pair_rule64, for the fused endings and for the rule on a stored pair, so both give the same bits.  No float
// atomics: bit-reproducible.  The rule uses the IEEE division, sqrt and pow: m k + k n elements a step, not m n.
//
// The objective (f64_div_sum_kernel): the walk of f64_nn_rows_kernel -- a wave keeps 16 rows of W, forms 16 x 16 tiles of S along
// its column range -- with the element's divergence added per lane in tile order, a fixed-order tree per workgroup, one slot of the
// workspace per workgroup and the slots added in a fixed order: two calls are bit-identical.  (The 32 x 128 tiles of
// csrc/dnmf_sums.h are those of the fp32 32x32x2 MFMA and its LDS-staged H; they do not fit the 16-wide fp64 tiles.)
#pragma once
#include "dnmf_f64_ops.h"

namespace {

enum { PM_IS = 0, PM_HALF = 1, PM_GEN = 2 };
struct PowArgs { double e; int ipow, inv, odd; };      // P = s'^e; PM_HALF: b^ipow [. s'^(+-1/2) if odd], b = 1 / s' if inv

// 1 / d for 0 < d < inf away from the ends of the exponent range: div_pos64 (csrc/dnmf_f64_kl.h) without its quotient
__device__ __forceinline__ double rcp_pos64(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
    return __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
}
// 1 / sqrt(d) alike: y <- y + (y / 2) (1 - d y^2), twice
__device__ __forceinline__ double rsq_pos64(double d) {
    double y = __builtin_amdgcn_rsq(d);
    y = __builtin_fma(0.5 * y, __builtin_fma(-(d * y), y, 1.0), y);
    return __builtin_fma(0.5 * y, __builtin_fma(-(d * y), y, 1.0), y);
}

// (u_n, u_d) of N elements of a tile: a = data, s = W H (eps not yet added)
template <int PM, int N>
__device__ __forceinline__ void div_pair64(const double (&a)[N], const double (&s)[N], double eps, const PowArgs& pa, double (&un)[N], double (&ud)[N]) {
    if constexpr (PM == PM_IS) {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const double r = rcp_pos64(s[e] + eps);
            ud[e] = r;
            un[e] = (a[e] * r) * r;
        }
    } else {
        double sp[N], p[N];
#pragma unroll
        for (int e = 0; e < N; ++e) sp[e] = s[e] + eps;
        if constexpr (PM == PM_GEN) {
#pragma unroll
            for (int e = 0; e < N; ++e) p[e] = pow(sp[e], pa.e);
        } else {
            double b[N];
#pragma unroll
            for (int e = 0; e < N; ++e) { b[e] = pa.inv ? rcp_pos64(sp[e]) : sp[e]; p[e] = 1.0; }
            for (int j = 0; j < pa.ipow; ++j)                       // (wave-uniform trip count: a kernel argument)
#pragma unroll
                for (int e = 0; e < N; ++e) p[e] *= b[e];
            if (pa.odd) {
#pragma unroll
                for (int e = 0; e < N; ++e) { const double y = rsq_pos64(sp[e]); p[e] *= pa.inv ? y : sp[e] * y; }
            }
        }
#pragma unroll
        for (int e = 0; e < N; ++e) { un[e] = a[e] * p[e]; ud[e] = sp[e] * p[e]; }
    }
}

// ------------------------------------------------------------------------------------------------ W side: row strips
// one wave = RT 16-row tiles of A (its rows of W stay in registers), all columns of its split, 16 at a time.  Tile column of MFMA row
// rho = q + 4 reg is c0 + 4 q + reg (a lane's four elements of A are consecutive); contraction index of step s in lane group q is
// j = q KS + s.  No row mask and no column mask (the padding argument above): a lane beyond the split is switched off in the loads.
// out[split][half][m][ldo]: half_stride between num and den.  VEC: n % 4 == 0.
template <int NT, int RT, bool VEC, int PM, int D = 1>
__global__ __launch_bounds__(256) void f64_div_uht_kernel(const double* __restrict__ A, long lda, long m, long n, const double* __restrict__ W, long ldw,
                                                          const double* __restrict__ H, long ldh, int kc, double eps, PowArgs pa, double* __restrict__ out,
                                                          long ldo, long split_stride, long half_stride, long cols_per_split) {
    constexpr int KS = 4 * NT;
    const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
    const long r0 = ((long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * (16 * RT);
    if (r0 >= m) return;
    const long cb = (long)blockIdx.y * cols_per_split;
    const long ce = cb + cols_per_split < n ? cb + cols_per_split : n;
    const long rows = m - r0 < 16 * RT ? m - r0 : 16 * RT;
    const i32x4 ad = rsrc64(A + r0 * lda, ((rows - 1) * lda + n) * 8), wd = rsrc64(W + r0 * ldw, ((rows - 1) * ldw + kc) * 8);
    const i32x4 hd = rsrc64(H, ((long)(kc - 1) * ldh + n) * 8);
    int avo[RT];
    double wreg[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        avo[rt] = (int)(((16 * rt + i) * lda + 4 * q) * 8);
#pragma unroll
        for (int v = 0; v < NT; ++v) {
            double t4[4];
            ldq<4, false>(t4, wd, (int)(((16 * rt + i) * ldw + q * KS + 4 * v) * 8), 0, clampi(kc - (q * KS + 4 * v), 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) wreg[rt][4 * v + e] = t4[e];
        }
    }
    const int c1 = 4 * (i & 3) + (i >> 2);
    int h1vo[KS], h2vo[NT];                          // first product: H[j = q KS + s][column of MFMA row i]; second: H[16 t + i][c0 + 4 q ..]
#pragma unroll
    for (int s = 0; s < KS; ++s) h1vo[s] = q * KS + s < kc ? (int)(((q * KS + s) * ldh + c1) * 8) : BUF_OOB;
#pragma unroll
    for (int t = 0; t < NT; ++t) h2vo[t] = 16 * t + i < kc ? (int)(((16 * t + i) * ldh + 4 * q) * 8) : BUF_OOB;
    f64x4 accn[RT][NT], accd[RT][NT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NT; ++t) accn[rt][t] = accd[rt][t] = f64x4{0.0, 0.0, 0.0, 0.0};
    auto load_a = [&](double (&a)[RT][4], long c0) __attribute__((always_inline)) {
        const int so = sgpr(c0 * 8);
        const int nv = clampi(ce - (c0 + 4 * q), 4);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) ldq<4, VEC>(a[rt], ad, avo[rt], so, nv);
    };
    auto load_h = [&](double (&h1)[KS], double (&h2)[NT][4], long c0) __attribute__((always_inline)) {
        const int so = sgpr(c0 * 8);
        const int nv = clampi(ce - (c0 + 4 * q), 4), n1 = c0 + c1 < ce ? 1 : 0;
#pragma unroll
        for (int s = 0; s < KS; ++s) { double t1[1]; ldq<1, true>(t1, hd, h1vo[s], so, n1); h1[s] = t1[0]; }
#pragma unroll
        for (int t = 0; t < NT; ++t) ldq<4, VEC>(h2[t], hd, h2vo[t], so, nv);
    };
    auto tile = [&](const double (&a)[RT][4], const double (&h1)[KS], const double (&h2)[NT][4]) __attribute__((always_inline)) {
        f64x4 s4[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {                              // the RT first products are independent chains
            s4[rt] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < KS; ++s) s4[rt] = MFMA64(h1[s], wreg[rt][s], s4[rt]);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const double s[4] = {s4[rt][0], s4[rt][1], s4[rt][2], s4[rt][3]};
            double un[4], ud[4];
            div_pair64<PM, 4>(a[rt], s, eps, pa, un, ud);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < NT; ++t) {                        // both second products share h2[t][e]
                    accn[rt][t] = MFMA64(un[e], h2[t][e], accn[rt][t]);
                    accd[rt][t] = MFMA64(ud[e], h2[t][e], accd[rt][t]);
                }
        }
    };
    // Two rings (f64_kl_uht_kernel): the pieces of A come from HBM and are small -- DA tiles ahead; the operands from H come from the
    // L2 and are large -- one tile ahead.  Nothing is conditional around a load: the trip count is rounded up to the ring, a tile
    // beyond the split has every lane switched off, reads zeros and adds nothing (the padding argument).
    constexpr int DA = D + 2, U = DA % 2 == 0 ? DA : 2 * DA;
    const long ntiles = cdiv(ce - cb, 16);
    auto tcol = [&](long t) __attribute__((always_inline)) { return cb + 16 * t; };
    double a[DA][RT][4], h1[2][KS], h2[2][NT][4];
    static_for<0, DA - 1>([&](auto d) __attribute__((always_inline)) { load_a(a[d], tcol(d)); });
    load_h(h1[0], h2[0], cb);
    for (long it = 0; it < ntiles; it += U)
        static_for<0, U>([&](auto d) __attribute__((always_inline)) {
            load_a(a[(d + DA - 1) % DA], tcol(it + d + (DA - 1)));
            load_h(h1[(d + 1) % 2], h2[(d + 1) % 2], tcol(it + d + 1));
            __builtin_amdgcn_sched_barrier(0);                    // (loads first, see f64_nt_kernel)
            tile(a[d % DA], h1[d % 2], h2[d % 2]);
        });
    double* on = out + (long)blockIdx.y * split_stride;
    double* od = on + half_stride;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = r0 + 16 * rt + q + 4 * r;
                const int col = 16 * t + i;
                if (row < m && col < kc) { on[row * ldo + col] = accn[rt][t][r]; od[row * ldo + col] = accd[rt][t][r]; }
            }
}

// ------------------------------------------------------------------------------------------------ H side: column strips
// one wave = 16 CT columns (tile cb holds the columns c0 + CT i + cb: CT consecutive doubles of a row per lane) -- its k x 16 CT piece
// of H stays in registers -- and a chunk of rows, 16 at a time.  Output row tile t holds the factor columns (t / VJ) 16 VJ + VJ i + t % VJ
// (f64_tn_kernel's permutation).  Per-tile descriptors for A and W: rows beyond the chunk lie outside the byte count and read zeros.
// P[chunk][half][kp][ldp].  VEC: n % CT == 0 and kc % 4 == 0.
template <int NT, int CT, bool VEC, int PM, int D = 1>
__global__ __launch_bounds__(256) void f64_div_wtu_kernel(const double* __restrict__ A, long lda, long m, long n, const double* __restrict__ W, long ldw,
                                                          const double* __restrict__ H, long ldh, int kc, double eps, PowArgs pa, long rows_per_chunk,
                                                          int ncolblk, long nwaves, double* __restrict__ P, long chunk_stride, long half_stride, long ldp) {
    constexpr int KS = 4 * NT, VJ = NT < 4 ? NT : 4, NV = NT / VJ;
    const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
    const long gw = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (gw >= nwaves) return;
    const long chunk = gw / ncolblk, c0 = (gw % ncolblk) * (16 * CT);
    const long rb = chunk * rows_per_chunk;
    const long re = rb + rows_per_chunk < m ? rb + rows_per_chunk : m;
    const int nva = clampi(n - (c0 + CT * i), CT);
    double hb[KS][CT];
    {
        const i32x4 hd = rsrc64(H, ((long)(kc - 1) * ldh + n) * 8);
#pragma unroll
        for (int s = 0; s < KS; ++s) ldq<CT, VEC>(hb[s], hd, q * KS + s < kc ? (int)(((q * KS + s) * ldh + c0 + CT * i) * 8) : BUF_OOB, 0, nva);
    }
    f64x4 accn[NT][CT], accd[NT][CT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int cb = 0; cb < CT; ++cb) accn[t][cb] = accd[t][cb] = f64x4{0.0, 0.0, 0.0, 0.0};
    int avo[4], w2vo[4], nv1[NT], nv2[NV];
    const int w1vo = (int)((i * ldw + q * KS) * 8);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        avo[r] = (int)(((q + 4 * r) * lda + c0 + CT * i) * 8);
        w2vo[r] = (int)(((q + 4 * r) * ldw + VJ * i) * 8);
    }
#pragma unroll
    for (int v = 0; v < NT; ++v) nv1[v] = clampi(kc - (q * KS + 4 * v), 4);
#pragma unroll
    for (int v = 0; v < NV; ++v) nv2[v] = clampi(kc - (16 * VJ * v + VJ * i), VJ);
    auto load_a = [&](double (&av)[4][CT], long r0) __attribute__((always_inline)) {
        const i32x4 ad = rsrc64(A + r0 * lda, ((re - r0 - 1) * lda + n) * 8);
#pragma unroll
        for (int r = 0; r < 4; ++r) ldq<CT, VEC>(av[r], ad, avo[r], 0, nva);
    };
    auto load_w = [&](double (&w1)[KS], double (&w2)[4][NV][VJ], long r0) __attribute__((always_inline)) {
        const i32x4 wd = rsrc64(W + r0 * ldw, ((re - r0 - 1) * ldw + kc) * 8);
#pragma unroll
        for (int v = 0; v < NT; ++v) {
            double t4[4];
            ldq<4, VEC>(t4, wd, w1vo + 32 * v, 0, nv1[v]);
#pragma unroll
            for (int e = 0; e < 4; ++e) w1[4 * v + e] = t4[e];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int v = 0; v < NV; ++v) ldq<VJ, VEC>(w2[r][v], wd, w2vo[r] + 16 * VJ * 8 * v, 0, nv2[v]);
    };
    auto tile = [&](const double (&w1)[KS], const double (&w2)[4][NV][VJ], const double (&av)[4][CT]) __attribute__((always_inline)) {
        f64x4 s4[CT];
#pragma unroll
        for (int cb = 0; cb < CT; ++cb) s4[cb] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int cb = 0; cb < CT; ++cb) s4[cb] = MFMA64(w1[s], hb[s][cb], s4[cb]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double s[CT], un[CT], ud[CT];
#pragma unroll
            for (int cb = 0; cb < CT; ++cb) s[cb] = s4[cb][r];
            div_pair64<PM, CT>(av[r], s, eps, pa, un, ud);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int cb = 0; cb < CT; ++cb) {                     // both second products share w2[r][..]
                    accn[t][cb] = MFMA64(w2[r][t / VJ][t % VJ], un[cb], accn[t][cb]);
                    accd[t][cb] = MFMA64(w2[r][t / VJ][t % VJ], ud[cb], accd[t][cb]);
                }
        }
    };
    // rings (f64_kl_wtu_kernel): A DA tiles ahead, the rows of W one tile ahead; the trip count is rounded up, a tile beyond the chunk
    // has descriptors of zero bytes, reads zeros and adds nothing (the padding argument)
    constexpr int DA = D + 2, U = DA % 2 == 0 ? DA : 2 * DA;
    double w1[2][KS], w2[2][4][NV][VJ], av[DA][4][CT];
    static_for<0, DA - 1>([&](auto d) __attribute__((always_inline)) { load_a(av[d], rb + 16 * d); });
    load_w(w1[0], w2[0], rb);
    for (long r = rb; r < re; r += 16 * U)
        static_for<0, U>([&](auto d) __attribute__((always_inline)) {
            load_a(av[(d + DA - 1) % DA], r + 16 * (d + DA - 1));
            load_w(w1[(d + 1) % 2], w2[(d + 1) % 2], r + 16 * (d + 1));
            __builtin_amdgcn_sched_barrier(0);                    // (loads first, see f64_nt_kernel)
            tile(w1[d % 2], w2[d % 2], av[d % DA]);
        });
    double* on = P + chunk * chunk_stride;
    double* od = on + half_stride;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ip = q + 4 * r;
            const int j = (t / VJ) * 16 * VJ + VJ * ip + t % VJ;
            if (j >= kc) continue;
#pragma unroll
            for (int cb = 0; cb < CT; ++cb) {
                const long col = c0 + CT * i + cb;
                if (col < n) { on[(long)j * ldp + col] = accn[t][cb][r]; od[(long)j * ldp + col] = accd[t][cb][r]; }
            }
        }
}

// ------------------------------------------------------------------------------------------------ endings
enum { RULE64_QUOT = 0, RULE64_SQRT = 1, RULE64_POW = 2 };
// x (num / (den + eps))^gamma: gamma = 1 is the plain quotient, gamma = 1/2 the square root; a quotient of 0 gives 0
__device__ __forceinline__ double pair_rule64(double x, double num, double den, double eps, int rule, double gamma, int clamp) {
    const double qt = num / (den + eps);
    const double f = rule == RULE64_QUOT ? qt : (rule == RULE64_SQRT ? sqrt(qt) : pow(qt, gamma));
    const double v = x * f;
    return clamp ? (v > eps ? v : eps) : v;
}
// the pair of element (r, c) = the sum of its `nslab` partials Pn / Pd[slab][r][c] in slab order; APPLY: X <- rule, else stored to
// (num, den).  A stored pair is the case nslab = 1.
template <bool APPLY>
__global__ __launch_bounds__(256) void f64_pair_end_kernel(const double* __restrict__ Pn, const double* __restrict__ Pd, long slab_stride, long ldp, int nslab,
                                                           long rows, long cols, double* __restrict__ X, long ldx, double* __restrict__ num,
                                                           double* __restrict__ den, long ldo, double eps, int rule, double gamma, int clamp) {
    const long total = rows * cols;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / cols, c = idx % cols;
        const long o = r * ldp + c;
        double sn = Pn[o], sd = Pd[o];
        for (int s = 1; s < nslab; ++s) { sn += Pn[o + s * slab_stride]; sd += Pd[o + s * slab_stride]; }
        if constexpr (APPLY) X[r * ldx + c] = pair_rule64(X[r * ldx + c], sn, sd, eps, rule, gamma, clamp);
        else { num[r * ldo + c] = sn; den[r * ldo + c] = sd; }
    }
}

// ------------------------------------------------------------------------------------------------ the objective
enum { DIV64_KL = 0, DIV64_IS = 1, DIV64_GEN = 2 };
// d_beta(a | s') of one element; c = 1 / (beta (beta - 1)) (DIV64_GEN); a^beta is 0 at a = 0
template <int FORM>
__device__ __forceinline__ double div_term64(double a, double sp, double beta, double c) {
    if constexpr (FORM == DIV64_IS) { const double qt = a / sp; return qt - log(qt) - 1.0; }
    else if constexpr (FORM == DIV64_KL) return a > 0.0 ? a * log(a / sp) - a + sp : sp;
    else {
        const double ab = a > 0.0 ? pow(a, beta) : 0.0, sb1 = pow(sp, beta - 1.0);
        return c * (ab + (beta - 1.0) * (sb1 * sp) - beta * (a * sb1));
    }
}
// part[workgroup] = sum of d(a | s + eps) over the workgroup's 64 rows (16 per wave, their W in registers) and its column range
template <int KS, int FORM>
__global__ __launch_bounds__(256) void f64_div_sum_kernel(const double* __restrict__ A, long lda, long m, long n, const double* __restrict__ W, long ldw,
                                                          const double* __restrict__ H, long ldh, int kc, double eps, double beta, double c,
                                                          long cols_per_wg, double* __restrict__ part) {
    __shared__ double red[256];
    const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
    const long r0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const long cb = (long)blockIdx.y * cols_per_wg;
    const long ce = cb + cols_per_wg < n ? cb + cols_per_wg : n;
    double sum = 0.0;
    if (r0 < m) {                                                       // (no early return: every wave meets the barriers of block_sum)
        double xa[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) xa[s] = (r0 + i < m && 4 * s + q < kc) ? W[(r0 + i) * ldw + 4 * s + q] : 0.0;
        for (long c0 = cb; c0 < ce; c0 += 16) {
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
            const bool cok = c0 + i < ce;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const double b = (cok && 4 * s + q < kc) ? H[(long)(4 * s + q) * ldh + c0 + i] : 0.0;
                acc = MFMA64(xa[s], b, acc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = r0 + q + 4 * r;
                if (row < m && cok) sum += div_term64<FORM>(A[row * lda + c0 + i], acc[r] + eps, beta, c);
            }
        }
    }
    const double s = block_sum(sum, red);
    if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------------ plans
constexpr int DIV64_MAX_K = 64;
constexpr int DIV64_RT = 2;                                           // W side: 16-row tiles per wave
constexpr int div64_ct(int nt) { return nt <= 2 ? 4 : 2; }            // H side: 16-column tiles per wave
constexpr int div64_uht_d(int nt) { return nt <= 2 ? 1 : 0; }         // W side: the ring of A is D + 2 tiles deep (k = 64: two, or the element-wise loads spill)
inline int div64_nt(int k) { const int nt = tiles16(k); return nt <= 1 ? 1 : nt <= 2 ? 2 : 4; }

struct DivUhtPlan { long nsplit, cps; unsigned gx; bool vec; int nt, kp; };
inline DivUhtPlan plan_div_uht(long m, long n, int k) {
    DivUhtPlan p;
    const long wr = cdiv(m, 16 * DIV64_RT);
    const long ns = std::max<long>(1, std::min<long>(2048 / wr, n / 512));
    p.cps = round_up(cdiv(n, ns), 16);
    p.nsplit = cdiv(n, p.cps);
    p.gx = (unsigned)cdiv(wr, 4);
    p.vec = n % 4 == 0;
    p.nt = div64_nt(k);
    p.kp = 16 * tiles16(k);
    return p;
}
struct DivWtuPlan { int ct, ncolblk, nt, kp; long nchunks, rows_per_chunk, nwaves, ldp; unsigned gx; bool vec; };
inline DivWtuPlan plan_div_wtu(long m, long n, int k) {
    DivWtuPlan p;
    p.nt = div64_nt(k);
    p.kp = 16 * tiles16(k);
    p.ct = div64_ct(p.nt);
    p.ncolblk = (int)cdiv(n, 16 * p.ct);
    long nch = std::max<long>(1, 2048 / p.ncolblk);
    nch = std::min<long>(nch, std::max<long>(1, cdiv(m, 64)));
    p.rows_per_chunk = round_up(cdiv(m, nch), 16);
    p.nchunks = cdiv(m, p.rows_per_chunk);
    p.nwaves = p.nchunks * p.ncolblk;
    p.gx = (unsigned)cdiv(p.nwaves, 4);
    p.ldp = round_up(n, 16);
    p.vec = n % p.ct == 0 && k % 4 == 0;
    return p;
}
struct DivSumPlan { int ks; unsigned gx, gy; long cpw; };
inline DivSumPlan plan_div_sum(long m, long n, int k) {
    DivSumPlan p;
    p.ks = k <= 16 ? 4 : k <= 32 ? 8 : 16;
    p.gx = (unsigned)cdiv(cdiv(m, 16), 4);
    const long ns = std::max<long>(1, std::min<long>(cdiv(n, 16), 2048 / p.gx));
    p.cpw = round_up(cdiv(n, ns), 16);
    p.gy = (unsigned)cdiv(n, p.cpw);
    return p;
}
// the three regions never live together: the W side's slabs, the H side's slabs, the objective's slots
inline size_t div64_ws_bytes(long m, long n, int k) {
    if (k < 1 || k > DIV64_MAX_K || m < 1 || n < 1) return 0;
    const size_t D = sizeof(double);
    const DivUhtPlan u = plan_div_uht(m, n, k);
    const DivWtuPlan w = plan_div_wtu(m, n, k);
    const DivSumPlan s = plan_div_sum(m, n, k);
    size_t b = (size_t)u.nsplit * 2 * m * u.kp * D;
    b = std::max(b, (size_t)w.nchunks * 2 * w.kp * w.ldp * D);
    b = std::max(b, (size_t)s.gx * s.gy * D);
    return al256(b) + 256;
}

}  // namespace
