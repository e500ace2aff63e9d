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

// ---- the rule on a stored pair is pair_ratio_kernel<RULE_SQRT> (csrc/dnmf_masked.h).  The divergence
//     D_IS(A | W H + eps) = sum (q - log q - 1), q = a / (s + eps)
// and its per-column form, div[c] = the same sum over this block's rows (PyNMF.is_column_divergence: the per-column statistic of an
// NMFk sweep under norm='is'), are the two walks of csrc/dnmf_sums.h with the term BetaDivTerm<BETA_DIV_IS, 1>: tile_sum_kernel leaves
// one double per 32 x 128 tile, col_sums_kernel one double per column and chunk of row blocks.
using IsDivTerm = BetaDivTerm<BETA_DIV_IS, 1>;

}  // namespace
