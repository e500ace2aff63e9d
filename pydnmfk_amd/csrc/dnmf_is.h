// dnmf_is.h -- the Itakura-Saito objective (beta = 0): the MU rule in its majorisation-minimisation form on the matrix cores.
// Part of libdnmf_hip.so (kernels live in anonymous namespaces of the headers; the translation units csrc/*.hip include what they launch).
//
// With S = W H, R = 1 / (S + eps) element-wise (eps the float32 machine epsilon) and F = H^T on the W side, F = W on the H side:
//     num = (A . R . R) F,   den = R F,   X <- X . sqrt(num / (den + eps))            (Fevotte & Idier 2011; the exponent 1/2 keeps
//     D_IS(A | S + eps) = sum (q - log q - 1), q = A . R, from increasing; scikit-learn's rule for beta_loss='itakura-saito')
// This is the structure of the masked pairs (csrc/dnmf_masked.h: a tile of S in MFMA accumulators, one element-wise step against A, TWO
// second products that share their F fragments) with another step -- one v_rcp_f32 and two multiplies per element, no compare: there
// is no mask.  The pair kernels ARE masked_uht_kernel / masked_wtu_kernel in their third mode (PAIR_IS), launched with the masked
// launch plans but for two choices at wide shapes and KP = 128 (plan_is_uht / plan_is_wtu in csrc/dnmf_is.hip); this file adds the
// endings (the square-root form of the ratio), the divergence and the divergence per column (what an NMFk sweep compares across k).
//
// Padding adds exactly nothing, without inf or 0 * inf.  An A load outside the block returns 0, so u_n = a r r = 0 * r * r there.  A
// padded column c >= n is a zero column of the staged H tile and a padded row r >= m a zero row of W (the predicated loads), so S = 0,
// r = 1 / eps = 2^23 and r^2 = 2^46 ~ 7e13 there: both finite in fp32, hence u_n = 0 * 2^46 = 0 exactly, and u_d = 2^23 meets an exact
// zero of F in the second product where that product contracts over the padded index (W side: over the columns c, and H[:, c] = 0;
// H side: over the rows r, and W[r, :] = 0).  Where the padded index is an OUTPUT index (a row >= m of the W side, a column >= n of
// the H side) the sums are finite and go nowhere: the W side does not store such a row, the H side stores such a column into the
// slab's own padding (ldp), which the ending never reads.  Inside the block S >= 0 (non-negative factors), so S + eps >= eps and
// r <= 2^23 likewise; a padded contraction index j >= k is a zero row of H and a zero column of W.  eps added to the finished
// accumulator (here) or taken as its initial value (the dense KL kernels) differ by rounding only: the sum is >= eps > 0 either way.
//
// Data must be strictly positive (PyNMF checks once per fit): a zero of A is legal for the pair (u_n = 0) but sends the divergence to
// infinity, a NaN would reach an MFMA operand.
#pragma once
#include "dnmf_masked.h"

namespace {

// ---- what the Itakura-Saito mode chooses on the launch path of csrc/dnmf_masked.h
template <>
struct PairMode<PAIR_IS> {
    // The W side's plan: the masked one with ONE part of the output columns at KP = 128 (JT = KT = 4).  masked_uht_kernel<4, 2> forms
    // every S tile twice, once per half of the output columns: 8 m n k flop for an IS side's 6 m n k.  With all four output tiles of
    // both halves in one workgroup (128 accumulator registers, which the compiler keeps in AGPRs: 254 VGPRs + 156 AGPRs, no scratch,
    // one wave per SIMD as before) S is formed once.  Up to KP = 64 nothing changes.
    static constexpr int zdim128 = 1;
    // The H side's plan: the masked one, but never fewer than four row chunks.  masked_wtu_kernel's workgroup is four waves = four
    // chunks; the masked plan asks for 1024 / ncolblk of them, which is TWO at n = 16384, KP = 128 (512 column blocks of 32): half the
    // waves of every workgroup returned at once and the pass ran on half the SIMDs (measured, 32768 x 16384, k = 128: 10.8 ms).
    // Shapes with at most 256 column blocks -- every shape of the masked suite -- get the masked plan unchanged.
    static constexpr long min_chunks = 4;
    static constexpr int rule = RULE_SQRT;      // X <- X * sqrt(num / (den + eps))
    static constexpr const char* serves = "the Itakura-Saito kernels";
};

// ---- the rule on a stored pair (after its allreduce on a 1D grid): pair_rule's square-root form, as in the ending
__global__ __launch_bounds__(256) void is_ratio_kernel(float* __restrict__ X, long rows, long cols, long ldx, const float* __restrict__ num,
                                                       const float* __restrict__ den, long ldo, float eps, int clamp) {
    const long total = rows * cols;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / cols, c = idx % cols;
        X[r * ldx + c] = pair_rule<RULE_SQRT>(X[r * ldx + c], num[r * ldo + c], den[r * ldo + c], eps, clamp);
    }
}

// ---- D_IS(A | W H + eps) = sum (q - log q - 1), q = a / (s + eps): masked_resid_kernel's tiles (a wave per 32 x 128 tile of S in
// accumulators) with another term.  fp32 per tile and lane (64 terms), float64 from there on; a wave leaves ONE double in its own slot
// of P (lanes added by a fixed shuffle tree) and is_div_sum_kernel adds the slots in a fixed order: no atomics, bit-reproducible.
// Outside the block a = 0 and s = 0 give q = 0 and log q = -inf: the term is SELECTED away, never multiplied.
template <int KT, bool FAST>
__global__ __launch_bounds__(256) void is_div_kernel(NnArgs p, double* __restrict__ P) {
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long gw = (long)blockIdx.x * 4 + wid;
    if (gw >= p.nrowblk * p.ncolblk) return;
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
            const float q = kl_quot(a[ne], acc[ne][r] + p.eps);
            const float t = (q - 1.f) - logf(q);
            part += (row < p.m && col0 + 4 * li + ne < p.n) ? t : 0.f;
        }
    }
    double total = (double)part;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) total += __shfl_xor(total, off, 64);
    if (lane == 0) P[gw] = total;
}

// one workgroup: thread t adds the slots t, t + 256, ... in that order, then a fixed tree over the 256 sums
__global__ __launch_bounds__(256) void is_div_sum_kernel(const double* __restrict__ P, long nparts, double* __restrict__ out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (long i = threadIdx.x; i < nparts; i += 256) s += P[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

// ---- per-column divergence, div[c] = sum_i (q - log q - 1) over this block's rows (PyNMF.is_column_divergence: the per-column statistic
// of an NMFk sweep under norm='is'): masked_colerr_kernel's structure (csrc/dnmf_masked.h) with is_div_kernel's term.  A wave owns a
// 128-column block and a chunk of 32-row blocks; fp32 over the 16 rows a lane holds of one row block, float64 from there on, one shuffle
// joins the lane halves.  The chunk's sums go to its own slab row, P[chunk][ldc] with ldc = ncolblk * 128 (every store is inside the
// slab); is_coldiv_reduce_kernel adds the rows in chunk order and STORES div[c]: no atomics, nothing accumulated into the output.
// Outside the block the term is SELECTED away (q = 0, log q = -inf there), never multiplied.
template <int KT, bool FAST>
__global__ __launch_bounds__(256) void is_coldiv_kernel(NnArgs p, double* __restrict__ P, long ldc, long rowblks_per_chunk) {
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long gw = (long)blockIdx.x * 4 + wid;
    const long nchunks = cdiv(p.nrowblk, rowblks_per_chunk);
    if (gw >= nchunks * p.ncolblk) return;
    const long chunk = gw / p.ncolblk, colblk = gw % p.ncolblk;
    const long col0 = colblk * 128;
    double dv[4] = {0.0, 0.0, 0.0, 0.0};
    long rb1 = (chunk + 1) * rowblks_per_chunk;
    if (rb1 > p.nrowblk) rb1 = p.nrowblk;
    for (long rb = chunk * rowblks_per_chunk; rb < rb1; ++rb) {
        const long row0 = rb * 32;
        f32x16 acc[4];
        nn_tile<KT, 4, FAST, false>(acc, p.W, p.ldw, p.m, p.k, p.H, p.ldh, p.n, row0, col0, li, h);
        float pv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long row = row0 + crow(r, h);
            float a[4];
            load_vec<4, FAST>(a, p.A + row * p.lda, col0 + 4 * li, p.n, row < p.m);
#pragma unroll
            for (int ne = 0; ne < 4; ++ne) {
                const float q = kl_quot(a[ne], acc[ne][r] + p.eps);
                const float t = (q - 1.f) - logf(q);
                pv[ne] += (row < p.m && col0 + 4 * li + ne < p.n) ? t : 0.f;
            }
        }
#pragma unroll
        for (int ne = 0; ne < 4; ++ne) dv[ne] += (double)pv[ne];
    }
    double* Pc = P + chunk * ldc + col0 + 4 * li;
#pragma unroll
    for (int ne = 0; ne < 4; ++ne) {
        dv[ne] += __shfl_xor(dv[ne], 32, 64);
        if (h == 0) Pc[ne] = dv[ne];
    }
}

__global__ __launch_bounds__(256) void is_coldiv_reduce_kernel(const double* __restrict__ P, long ldc, long nchunks, long n,
                                                               double* __restrict__ div) {
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long)gridDim.x * 256) {
        double a = P[c];
        for (long s = 1; s < nchunks; ++s) a += P[s * ldc + c];
        div[c] = a;
    }
}

}  // namespace
