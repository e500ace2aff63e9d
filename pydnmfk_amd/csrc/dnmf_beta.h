// dnmf_beta.h -- the beta-divergence for any beta in [-2, 4]: the MU rule in its majorisation-minimisation form on the matrix cores.
// Part of libdnmf_hip.so (kernels live in anonymous namespaces of the headers; the translation units csrc/*.hip include what they launch).
//
//     d_beta(a | s) = (a^beta + (beta - 1) s^beta - beta a s^(beta - 1)) / (beta (beta - 1))
// (beta = 2: half the squared error; beta -> 1: Kullback-Leibler; beta -> 0: Itakura-Saito).  With S' = W H + eps (eps the float32 machine
// epsilon, placed as in csrc/dnmf_is.h), P = S'^(beta - 2) element-wise and F = H^T on the W side, F = W on the H side (with the new W):
//     u_n = A . P,   u_d = S' . P,   num = u_n F,   den = u_d F,   X <- X . (num / (den + eps))^gamma(beta)
//     gamma = 1 / (2 - beta) for beta < 1,   1 for 1 <= beta <= 2,   1 / (beta - 1) for beta > 2
// (Fevotte & Idier 2011, the majorisation-minimisation rule: D_beta(A | W H + eps) never increases).  This is the structure of the masked
// pairs (csrc/dnmf_masked.h) with a fourth element-wise step, MODE = PAIR_BETA, and ONE runtime scalar e = beta - 2 that the host
// computes once (NnArgs::pexp).  The pair kernels ARE masked_uht_kernel / masked_wtu_kernel; this file adds the mode's choices, the
// rule on a stored pair (pair_rule's RULE_POW form, the same function as in the reduce ending), the divergence and the divergence per
// column with the column's sum of a^beta (what an NMFk sweep compares across k).
//
// The element-wise step.  p = exp2(e * log2(s + eps)) with the ONE-INSTRUCTION forms v_log_f32 and v_exp_f32 (__builtin_amdgcn_logf /
// __builtin_amdgcn_exp2f), not the library log2f / exp2f: the library forms add a range scaling for denormal arguments and results
// (three to four more vector instructions each), and neither can occur -- s + eps >= 2^-23 and, inside the accepted range of beta,
// p of a padded position is within [2^-46, 2^92]; a p that underflows inside the block (a model value of 1e10 under beta = -2) is a zero
// weight, which is what the limit is.  Both instructions are accurate to 1 ulp of their result, so the absolute error of e * log2 s is
// about (1 + |e|) ulp(log2 s) + ulp(e log2 s) / 2 and the relative error of p is ln 2 times that: for S in [0.05, 200] and |e| <= 4
// below 2e-6 per element, before the averaging of the second products.  Per element: v_add_f32 (s + eps), v_log_f32, v_mul_f32 (e .),
// v_exp_f32, v_mul_f32 (a p), v_mul_f32 (s' p) -- SIX vector instructions where the Itakura-Saito step has four (v_add, v_rcp, two
// v_mul).  On gfx950 a vector instruction beside the MFMAs costs about 3.3 matrix-pipe cycles (README, round 3): two more per element
// is what this mode pays over IS, about 6.6 cycles per element on each side, next to the 6 KP / 8 cycles per element of a side's three
// 32x32x2 products (24 / 48 / 96 at KP = 32 / 64 / 128).  Measured (tools/betabench.py, profiles/beta_step_times.md, one MI355X,
// 32768 x 16384): a beta step takes 1.04 / 1.01 / 1.00 times the Itakura-Saito step at k = 32 / 64 / 128 -- the pair kernels are plain
// loops that wait for their loads, and the two additional instructions issue under those waits.
// Measured accuracy against float64 (tests/test_gpu_beta.py, bound 1e-5): pairs 6.5e-7 (largest at beta = -2), updates 1.6e-7;
// v_exp_f32 of an exact zero is exactly 1, so at beta = 2 the pairs of exact operands are exact.
//
// Padding adds exactly nothing, without inf or 0 * inf.  An A load outside the block returns 0.  A padded column c >= n is a zero
// column of the staged H tile and a padded row r >= m a zero row of W (the predicated loads), so S = 0 there and s + eps = 2^-23
// exactly: log2 is -23, p = 2^(-23 (beta - 2)).  That must be FINITE so that u_n = 0 * p = 0 exactly and u_d = 2^-23 p meets an exact zero
// of F in the second product where that product contracts over the padded index (W side: over the columns c, and H[:, c] = 0; H side:
// over the rows r, and W[r, :] = 0).  Finite in fp32 means 23 |beta - 2| < 128, |beta - 2| < 5.5; the accepted range is -2 <= beta <= 4,
// |beta - 2| <= 4 < 5.5: p <= 2^92 (beta = -2), u_d <= 2^69, and p >= 2^-46 (beta = 4), u_d >= 2^-69, a normal number.  Outside that range
// the entry points return DNMF_EINVAL (beta_ok below) and Python raises ValueError naming the range.  Where the padded index is an
// OUTPUT index (a row >= m of the W side, a column >= n of the H side) the sums are finite and go nowhere: the W side does not store
// such a row, the H side stores such a column into the slab's own padding (ldp), which the ending never reads.  Inside the block
// S >= 0 (non-negative factors), so s + eps >= 2^-23 and the bounds on p hold likewise; a padded contraction index j >= k is a zero row of
// H and a zero column of W.
//
// Data: strictly positive for beta <= 0 (a zero sends the divergence to infinity), non-negative for beta > 0 (a zero gives u_n = 0 and
// a^beta = 0).  PyNMF checks once per fit.  A NaN would reach an MFMA operand.
//
// Registers (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage remarks; every PAIR_BETA instantiation, none uses scratch):
//   masked_uht_kernel<KT, JT, FAST, PAIR_BETA>   VGPR  AGPR  scratch  waves/SIMD     masked_wtu_kernel<KT, NT, FAST, PAIR_BETA>   VGPR  AGPR  scratch  waves/SIMD
//   <1, 1, true>                                  158     0     0        3           <1, 4, true>                                  256   160     0        1
//   <1, 1, false>                                 156     0     0        3           <1, 4, false>                                 256   228     0        1
//   <2, 2, true>                                  236     0     0        2           <2, 2, true>                                  238   132     0        1
//   <2, 2, false>                                 236     0     0        2           <2, 2, false>                                 240   132     0        1
//   <4, 4, true>                                  254   156     0        1           <4, 1, true>                                  193   128     0        1
//   <4, 4, false>                                 256   157     0        1           <4, 1, false>                                 197   128     0        1
// (the waves per SIMD are those of the launch bounds, as for the other modes).  JT = 4 at KP = 128 does not spill, so the W side takes
// the Itakura-Saito plan there (one pass over S), not the masked plan's JT = 2.  masked_reduce_kernel<RULE_POW>: 33 VGPRs;
// pair_ratio_kernel<RULE_POW>: 29; tile_sum_kernel<KT, FAST, BetaDivTerm<FORM, 1>> (csrc/dnmf_sums.h): 91 to 166 VGPRs + 64 AGPRs (KL
// 94 / 91 at three waves per SIMD, IS 136 / 134 and GEN 138 / 166 at two, FAST / generic, the same at every KT); none uses scratch.
// The per-column walk with two sums (csrc/dnmf_sums.h; one wave per SIMD):
//   <KT, FAST>    GEN, beta_coldiv_kernel: VGPR  AGPR  scratch    KL, col_sums_kernel: VGPR  AGPR  scratch    IS, col_sums_kernel: VGPR  AGPR  scratch
//   <1, true>                               229    64     0                             226    64     0                             222    64     0
//   <1, false>                              230    64     0                             228    64     0                             224    64     0
//   <2, true>                               256    70     0                             256    67     0                             255    64     0
//   <2, false>                              256    72     0                             256    70     0                             256    67     0
//   <4, true>                               256   136     0                             256   132     0                             256   128     0
//   <4, false>                              256   140     0                             256   136     0                             256   134     0
// (the launch bounds of 256 allow 512 registers per lane; no instantiation spills; KL and IS are col_sums_kernel<KT, FAST,
// BetaDivTerm<FORM, 2>>, the general form keeps its own kernel for the reason written there).  col_sums_reduce_kernel<2>, the ending:
// 18 VGPRs.
#pragma once
#include "dnmf_masked.h"

namespace {

// -2 <= beta <= 4 (the padding argument above); a NaN compares false
inline bool beta_ok(float beta) { return beta >= -2.f && beta <= 4.f; }

// the exponent of the rule
inline float beta_gamma(float beta) { return beta < 1.f ? 1.f / (2.f - beta) : (beta <= 2.f ? 1.f : 1.f / (beta - 1.f)); }

inline PairExp beta_exp(float beta) { return PairExp{beta - 2.f, beta_gamma(beta)}; }

// ---- what the mode chooses on the launch path of csrc/dnmf_masked.h: the Itakura-Saito plans (csrc/dnmf_is.h: one part of the output
// columns at KP = 128 -- JT = 4 holds next to the two transcendentals without scratch, see the table above -- and at least four row
// chunks on the H side), the rule with a runtime exponent
template <>
struct PairMode<PAIR_BETA> {
    static constexpr int zdim128 = 1;
    static constexpr long min_chunks = 4;
    static constexpr int rule = RULE_POW;       // X <- X * (num / (den + eps))^gamma
    static constexpr const char* serves = "the beta-divergence kernels";
};

// ---- the rule on a stored pair is pair_ratio_kernel<RULE_POW> (csrc/dnmf_masked.h).  The divergence D_beta(A | W H + eps) is
// tile_sum_kernel of csrc/dnmf_sums.h with the term BetaDivTerm<FORM, 1>, FORM and the constant c from beta_form below.
//
// The divergence column by column, with the column's sum of a^beta next to it: div[c] = sum_i d_beta(a_ic | s'_ic) and
// pw[c] = sum_i a_ic^beta over this block's rows (PyNMF.beta_column_divergence divides the one by the other after the sums have crossed
// the ranks: both scale as lambda^beta with a column's scale, so the ratio is the scale-invariant per-column statistic of an NMFk sweep
// under norm='beta'; at beta = 0 pw is the row count and the ratio the Itakura-Saito mean per entry).  It is col_sums_kernel with the
// term BetaDivTerm<FORM, 2> (the general form: beta_coldiv_kernel, the same walk kept as first written, see csrc/dnmf_sums.h): the chunk's
// pair goes to its own slab rows in the masked per-column error's layout, P[chunk][half][ldc].

// which expression serves this beta, and its constant: the general form is singular at beta = 1 and beta = 0
struct BetaForm { int form; float c; };
inline BetaForm beta_form(float beta) {
    const int form = beta == 1.f ? BETA_DIV_KL : (beta == 0.f ? BETA_DIV_IS : BETA_DIV_GEN);
    return BetaForm{form, form == BETA_DIV_GEN ? (float)(1.0 / ((double)beta * ((double)beta - 1.0))) : 1.f};
}

// f(term) with the BetaDivTerm<FORM, NSUM> of this beta
template <int NSUM, class F>
int with_beta_term(float beta, F f) {
    const BetaForm bf = beta_form(beta);
    if (bf.form == BETA_DIV_KL) return f(BetaDivTerm<BETA_DIV_KL, NSUM>{beta, bf.c});
    if (bf.form == BETA_DIV_IS) return f(BetaDivTerm<BETA_DIV_IS, NSUM>{beta, bf.c});
    return f(BetaDivTerm<BETA_DIV_GEN, NSUM>{beta, bf.c});
}

}  // namespace
