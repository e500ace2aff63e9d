// dnmf_sums.h -- the ONE tile walk behind every error and divergence sum of the pair rules: sums over the elements of a block, of terms
// that depend on a datum `a` and its model value s = <W[r], H[:, c]>, per column (col_sums_kernel) or as one scalar (tile_sum_kernel).
// Part of libdnmf_hip.so (kernels live in anonymous namespaces of the headers; the translation units csrc/*.hip include what they launch).
//
// A Term says what is summed: `NSUM` float32 sums per element and add(t, a, s, eps, in), which adds the element's terms to t[0..NSUM).
// `in` is false outside the block, where the loads return a = 0 and the zero-filled operands give s = 0.  The terms:
//   MaskedErrTerm        the masked error pair of csrc/dnmf_masked.h: (a - s)^2 and a^2 over the observed positions
//   BetaDivTerm<FORM, N> the beta-divergence of csrc/dnmf_beta.h in its three forms (BETA_DIV_IS is the Itakura-Saito divergence of
//                        csrc/dnmf_is.h), and with N = 2 the element's a^beta next to it
// Both walks keep float32 over the 16 rows a lane holds of one 32-row block and float64 from there on, and end without atomics: a
// wave stores its sums into its own slots of a slab, and a second launch adds the slots in a fixed order.  Bit-reproducible.
// The host launchers of these kernels are in csrc/dnmf_masked.h, next to the argument block and the plan they share with the pairs.
#pragma once
#include "dnmf_common.h"
#include "dnmf_nn.h"

namespace {

// ---- the masked error pair: outside the block a = 0 and s = 0 (zero-filled operands), which reads as an observed zero that is
// reproduced exactly -- both terms are 0 there, so there is no bounds select
struct MaskedErrTerm {
    static constexpr int NSUM = 2;
    __device__ __forceinline__ void add(float (&t)[2], float a, float s, float, bool) const {
        const bool obs = a == a;
        const float d = obs ? a - s : 0.f;
        const float ao = obs ? a : 0.f;
        t[0] = fmaf(d, d, t[0]);
        t[1] = fmaf(ao, ao, t[1]);
    }
};

// ---- d_beta(a | s'), s' = s + eps.  FORM picks the expression:
//   BETA_DIV_GEN  (a^beta + (beta - 1) s'^beta - beta a s'^(beta - 1)) / (beta (beta - 1)), as s'^(beta - 1) ((beta - 1) s' - beta a) + a^beta
//                 times c = 1 / (beta (beta - 1)) from the host; a^beta at a = 0 is SELECTED to 0 (beta > 0; log2 0 = -inf never meets it)
//   BETA_DIV_KL   beta = 1, where that form is singular: a log(a / s') - a + s', and s' where a = 0
//   BETA_DIV_IS   beta = 0, singular as well: q - log q - 1, q = a / s' (the Itakura-Saito divergence)
// The library log2f / exp2f / logf here (not the one-instruction forms of the pair): these kernels run once per report, not per step.
enum { BETA_DIV_GEN = 0, BETA_DIV_KL = 1, BETA_DIV_IS = 2 };
// the term and, in `pw`, a^beta of the same element (the general form computes it anyway; a at beta = 1, 1 at beta = 0): what the
// per-column statistic of an NMFk sweep divides by
template <int FORM>
__device__ __forceinline__ float beta_div_term_pw(float a, float sp, float beta, float c, float& pw) {
    if constexpr (FORM == BETA_DIV_KL) {
        pw = a;
        return a > 0.f ? a * logf(a / sp) - a + sp : sp;
    } else if constexpr (FORM == BETA_DIV_IS) {
        pw = 1.f;
        const float q = kl_quot(a, sp);
        return (q - 1.f) - logf(q);
    } else {
        const float sb1 = exp2f((beta - 1.f) * log2f(sp));          // s'^(beta - 1)
        const float ab = a > 0.f ? exp2f(beta * log2f(a)) : 0.f;    // a^beta, 0 at a = 0
        pw = ab;
        return (ab + sb1 * ((beta - 1.f) * sp - beta * a)) * c;
    }
}

// Outside the block every term is SELECTED away, never multiplied: a = 0 and s = 0 give q = 0 and log q = -inf, and for beta <= 0
// log2 0 = -inf and a^beta = inf.  N = 1: the divergence alone; N = 2: a^beta in the second sum
template <int FORM, int N>
struct BetaDivTerm {
    static constexpr int NSUM = N;
    float beta = 0.f, c = 1.f;      // read by BETA_DIV_GEN alone
    __device__ __forceinline__ void add(float (&t)[N], float a, float s, float eps, bool in) const {
        float w;
        const float d = beta_div_term_pw<FORM>(a, s + eps, beta, c, w);
        t[0] += in ? d : 0.f;
        if constexpr (N == 2) t[1] += in ? w : 0.f;
    }
};

// ---- per column: out[j][c] = sum over this block's rows of the Term's sum j.  A wave owns a 128-column block and a chunk of 32-row
// blocks; fp32 over the 16 rows a lane holds of one row block, float64 from there on, one shuffle joins the lane halves.  The chunk's
// sums go to its own slab rows, P[chunk][NSUM][ldc] with ldc = ncolblk * 128 (every store is inside the slab); col_sums_reduce_kernel
// adds the rows in chunk order and STORES the results: no atomics, nothing accumulated into the outputs.
template <int KT, bool FAST, class Term>
__global__ __launch_bounds__(256) void col_sums_kernel(NnArgs p, double* __restrict__ P, long ldc, long rowblks_per_chunk, Term term) {
    constexpr int NS = Term::NSUM;
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long gw = (long)blockIdx.x * 4 + wid;
    const long nchunks = cdiv(p.nrowblk, rowblks_per_chunk);
    if (gw >= nchunks * p.ncolblk) return;
    const long chunk = gw / p.ncolblk, colblk = gw % p.ncolblk;
    const long col0 = colblk * 128;
    double dv[4][NS];
#pragma unroll
    for (int ne = 0; ne < 4; ++ne)
#pragma unroll
        for (int j = 0; j < NS; ++j) dv[ne][j] = 0.0;
    long rb1 = (chunk + 1) * rowblks_per_chunk;
    if (rb1 > p.nrowblk) rb1 = p.nrowblk;
    for (long rb = chunk * rowblks_per_chunk; rb < rb1; ++rb) {
        const long row0 = rb * 32;
        f32x16 acc[4];
        nn_tile<KT, 4, FAST, false>(acc, p.W, p.ldw, p.m, p.k, p.H, p.ldh, p.n, row0, col0, li, h);
        float pv[4][NS];
#pragma unroll
        for (int ne = 0; ne < 4; ++ne)
#pragma unroll
            for (int j = 0; j < NS; ++j) pv[ne][j] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long row = row0 + crow(r, h);
            float a[4];
            load_vec<4, FAST>(a, p.A + row * p.lda, col0 + 4 * li, p.n, row < p.m);
#pragma unroll
            for (int ne = 0; ne < 4; ++ne) term.add(pv[ne], a[ne], acc[ne][r], p.eps, row < p.m && col0 + 4 * li + ne < p.n);
        }
#pragma unroll
        for (int ne = 0; ne < 4; ++ne)
#pragma unroll
            for (int j = 0; j < NS; ++j) dv[ne][j] += (double)pv[ne][j];
    }
    double* Pc = P + chunk * NS * ldc + col0 + 4 * li;
#pragma unroll
    for (int ne = 0; ne < 4; ++ne)
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            dv[ne][j] += __shfl_xor(dv[ne][j], 32, 64);
            if (h == 0) Pc[j * ldc + ne] = dv[ne][j];
        }
}

// ---- NOT merged into the walk above: the general form with two sums (dnmf_beta_column_div at beta other than 0 and 1).  The term
// leaves the contraction of (beta - 1) s' - beta a to the compiler, and in THIS kernel the compiler forms the two products of the last
// row's four elements with one packed multiply and subtracts them, where every other element -- and every element of
// col_sums_kernel<KT, FAST, BetaDivTerm<BETA_DIV_GEN, 2>> -- gets one multiply and one FMA: 4 of a lane's 64 terms per row block
// differ in their last bit (found by comparing the raw outputs of both kernels on random operands; at beta = 0.5, 1.5 and 2, where
// one product is exact, they agree).  So that dnmf_beta_column_div keeps its bits the kernel stays as it was written, and
// col_sums_launch below launches it for its term.  A change that may move result bits should state the contraction in the term
// (fmaf) and retire this kernel.
template <int KT, bool FAST, int FORM>
__global__ __launch_bounds__(256) void beta_coldiv_kernel(NnArgs p, double* __restrict__ P, long ldc, long rowblks_per_chunk, float beta,
                                                          float c) {
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long gw = (long)blockIdx.x * 4 + wid;
    const long nchunks = cdiv(p.nrowblk, rowblks_per_chunk);
    if (gw >= nchunks * p.ncolblk) return;
    const long chunk = gw / p.ncolblk, colblk = gw % p.ncolblk;
    const long col0 = colblk * 128;
    double dv[4] = {0.0, 0.0, 0.0, 0.0}, dp[4] = {0.0, 0.0, 0.0, 0.0};
    long rb1 = (chunk + 1) * rowblks_per_chunk;
    if (rb1 > p.nrowblk) rb1 = p.nrowblk;
    for (long rb = chunk * rowblks_per_chunk; rb < rb1; ++rb) {
        const long row0 = rb * 32;
        f32x16 acc[4];
        nn_tile<KT, 4, FAST, false>(acc, p.W, p.ldw, p.m, p.k, p.H, p.ldh, p.n, row0, col0, li, h);
        float pv[4] = {0.f, 0.f, 0.f, 0.f}, pp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long row = row0 + crow(r, h);
            float a[4];
            load_vec<4, FAST>(a, p.A + row * p.lda, col0 + 4 * li, p.n, row < p.m);
#pragma unroll
            for (int ne = 0; ne < 4; ++ne) {
                float w;
                const float t = beta_div_term_pw<FORM>(a[ne], acc[ne][r] + p.eps, beta, c, w);
                const bool in = row < p.m && col0 + 4 * li + ne < p.n;
                pv[ne] += in ? t : 0.f;
                pp[ne] += in ? w : 0.f;
            }
        }
#pragma unroll
        for (int ne = 0; ne < 4; ++ne) { dv[ne] += (double)pv[ne]; dp[ne] += (double)pp[ne]; }
    }
    double* Pv = P + chunk * 2 * ldc + col0 + 4 * li;
    double* Pp = Pv + ldc;
#pragma unroll
    for (int ne = 0; ne < 4; ++ne) {
        dv[ne] += __shfl_xor(dv[ne], 32, 64);
        dp[ne] += __shfl_xor(dp[ne], 32, 64);
        if (h == 0) { Pv[ne] = dv[ne]; Pp[ne] = dp[ne]; }
    }
}

// the per-column launch of a Term
template <int KT, bool FAST, class Term>
void col_sums_launch(dim3 grid, dim3 block, hipStream_t st, const NnArgs& a, double* P, long ldc, long rowblks_per_chunk, Term term) {
    if constexpr (std::is_same_v<Term, BetaDivTerm<BETA_DIV_GEN, 2>>)
        hipLaunchKernelGGL((beta_coldiv_kernel<KT, FAST, BETA_DIV_GEN>), grid, block, 0, st, a, P, ldc, rowblks_per_chunk, term.beta, term.c);
    else
        hipLaunchKernelGGL((col_sums_kernel<KT, FAST, Term>), grid, block, 0, st, a, P, ldc, rowblks_per_chunk, term);
}

// out1 is read by NSUM = 2 alone
template <int NSUM>
__global__ __launch_bounds__(256) void col_sums_reduce_kernel(const double* __restrict__ P, long ldc, long nchunks, long n,
                                                              double* __restrict__ out0, double* __restrict__ out1) {
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long)gridDim.x * 256) {
        double a[NSUM];
#pragma unroll
        for (int j = 0; j < NSUM; ++j) a[j] = P[j * ldc + c];
        for (long s = 1; s < nchunks; ++s)
#pragma unroll
            for (int j = 0; j < NSUM; ++j) a[j] += P[(s * NSUM + j) * ldc + c];
        out0[c] = a[0];
        if constexpr (NSUM == 2) out1[c] = a[1];
    }
}

// ---- one scalar: the Term's sum 0 over the block.  A wave per 32 x 128 tile of S in accumulators (masked_resid_kernel's tiles);
// fp32 per tile and lane (64 terms), float64 from there on; a wave leaves ONE double in its own slot of P (lanes added by a fixed
// shuffle tree) and slot_sum_kernel adds the slots in a fixed order: no atomics, bit-reproducible.
template <int KT, bool FAST, class Term>
__global__ __launch_bounds__(256) void tile_sum_kernel(NnArgs p, double* __restrict__ P, Term term) {
    static_assert(Term::NSUM == 1, "tile_sum_kernel leaves one sum per wave");
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long gw = (long)blockIdx.x * 4 + wid;
    if (gw >= p.nrowblk * p.ncolblk) return;
    const long row0 = (gw / p.ncolblk) * 32, col0 = (gw % p.ncolblk) * 128;
    f32x16 acc[4];
    nn_tile<KT, 4, FAST, false>(acc, p.W, p.ldw, p.m, p.k, p.H, p.ldh, p.n, row0, col0, li, h);
    float part[1] = {0.f};
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long row = row0 + crow(r, h);
        float a[4];
        load_vec<4, FAST>(a, p.A + row * p.lda, col0 + 4 * li, p.n, row < p.m);
#pragma unroll
        for (int ne = 0; ne < 4; ++ne) term.add(part, a[ne], acc[ne][r], p.eps, row < p.m && col0 + 4 * li + ne < p.n);
    }
    double total = (double)part[0];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) total += __shfl_xor(total, off, 64);
    if (lane == 0) P[gw] = total;
}

// one workgroup: thread t adds the slots t, t + 256, ... in that order, then a fixed tree over the 256 sums
__global__ __launch_bounds__(256) void slot_sum_kernel(const double* __restrict__ P, long nparts, double* __restrict__ out) {
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

}  // namespace
