// dnmf_huber.h -- the Huber loss for a runtime threshold delta > 0: robust NMF by reweighted MU on the matrix cores.
// Part of libdnmf_hip.so (kernels live in anonymous namespaces of the headers; the translation units csrc/*.hip include what they launch).
//
//     rho_delta(r) = r^2 / 2 for |r| <= delta,   delta |r| - delta^2 / 2 otherwise;      objective  sum rho_delta(a - s'),  s' = W H + eps
// (eps the float32 machine epsilon, placed as in csrc/dnmf_is.h).  Quadratic in a small residual and linear in a large one: a gross
// outlier pulls the factors with a force that stops growing at delta, where every smooth objective of this family lets it pull as hard
// as it is large.  With P = min(1, delta / |A - S'|) element-wise (1 where |r| <= delta, and at r = 0) and F = H^T on the W side, F = W on
// the H side (with the new W):
//     u_n = A . P,   u_d = S' . P,   num = u_n F,   den = u_d F,   X <- X . num / (den + eps)
// At fixed P this is the MU step of the weighted Frobenius objective sum p (a - s')^2 / 2, which decreases it; that quadratic touches
// rho_delta at the current residual and lies above it everywhere else (half-quadratic majorisation: rho_delta(r) <= rho_delta(r0) +
// p(r0) (r^2 - r0^2) / 2, since rho_delta(sqrt(t)) is concave in t), so the Huber objective never rises.  delta = inf is P = 1: the
// Frobenius objective under this family's rule, the beta = 2 step of csrc/dnmf_beta.h.  This is the structure of the masked pairs
// (csrc/dnmf_masked.h) with a fifth element-wise step, MODE = PAIR_HUBER, and ONE runtime scalar, delta, which travels where the
// beta mode's exponent travels (NnArgs::pexp).  The pair kernels ARE masked_uht_kernel / masked_wtu_kernel; this file adds the mode's
// choices and the objective.
//
// The element-wise step.  p = min(1, delta * rcp(|a - s'|)) with the ONE-INSTRUCTION form v_rcp_f32 (__builtin_amdgcn_rcpf; its source
// modifier takes the absolute value), never delta / max(delta, |r|): a division is a dozen instructions, and at delta = inf it is inf / inf.
// Per element, after the v_add_f32 that forms s' = s + eps in every mode of this family: v_sub_f32 (a - s'), v_rcp_f32 (|.|), v_mul_f32
// (delta .), v_min_f32 (1, .), v_mul_f32 (a p), v_mul_f32 (s' p) -- SIX, seven with the add, where the beta step has six with its add (v_add,
// v_log, v_mul, v_exp, two v_mul) and the Itakura-Saito step four.  The cases at the ends:
//   r = 0           rcp(0) = inf, delta * inf = inf for every delta > 0, min(1, inf) = 1: p = 1, the quadratic branch, no 0 * inf
//   delta = inf     rcp(|r|) > 0 for |r| < 2^126, inf * that = inf, p = 1 EXACTLY at every element: u_n = a and u_d = s', the beta = 2 pair
//                   bit for bit.  At |r| > 2^126 the reciprocal is a denormal, which v_rcp_f32 may return as 0, and inf * 0 is a NaN;
//                   v_min_f32 returns its other operand then (IEEE minNum): p = 1 as well
//   delta finite    delta * rcp is finite or inf, p in [0, 1]; a p that underflows to 0 (a residual of 1e38 under delta = 1) is a zero weight,
//                   which is what the limit is
// v_rcp_f32 is accurate to 1 ulp, the products are correctly rounded: p is within 1.5 ulp where |r| > delta and exact where |r| <= delta,
// but for the elements whose |r| is within 2 ulp of delta, where p = 1 - O(1e-7) may stand for 1 or the reverse: P is continuous there.
//
// Padding adds exactly nothing, for every finite delta > 0 and for delta = inf, without inf or 0 * inf in a product.  An A load outside
// the block returns 0.  A padded column c >= n is a zero column of the staged H tile and a padded row r >= m a zero row of W (the
// predicated loads), so S = 0 there and s' = 2^-23 exactly: r = -2^-23, rcp(|r|) = 2^23 exactly, delta * 2^23 is a positive number or inf,
// and p = min(1, .) lies in (0, 1]: FINITE whatever delta is (the smallest float32 delta, 2^-149, gives p = 2^-126).  Hence u_n = 0 * p = 0
// exactly, and u_d = 2^-23 p <= 2^-23 meets an exact zero of F in the second product where that product contracts over the padded index
// (W side: over the columns c, and H[:, c] = 0; H side: over the rows r, and W[r, :] = 0).  Where the padded index is an OUTPUT index (a
// row >= m of the W side, a column >= n of the H side) the sums are finite and go nowhere: the W side does not store such a row, the H
// side stores such a column into the slab's own padding (ldp), which the ending never reads.  A padded contraction index j >= k is a
// zero row of H and a zero column of W.  Inside the block p is in [0, 1] for finite data, so u_n and u_d are no larger than a and s'.
//
// Data: dense float32, finite and non-negative (PyNMF checks once per fit).  A NaN would reach an MFMA operand; a negative entry is
// legal for the pair but can turn a numerator, and with it a factor, negative.
//
// Registers (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage remarks; every PAIR_HUBER instantiation, none uses scratch):
//   masked_uht_kernel<KT, JT, FAST, PAIR_HUBER>  VGPR  AGPR  scratch  waves/SIMD     masked_wtu_kernel<KT, NT, FAST, PAIR_HUBER>  VGPR  AGPR  scratch  waves/SIMD
//   <1, 1, true>                                  158     0     0        3           <1, 4, true>                                  256   160     0        1
//   <1, 1, false>                                 156     0     0        3           <1, 4, false>                                 256   228     0        1
//   <2, 2, true>                                  236     0     0        2           <2, 2, true>                                  238   132     0        1
//   <2, 2, false>                                 236     0     0        2           <2, 2, false>                                 240   132     0        1
//   <4, 4, true>                                  254   156     0        1           <4, 1, true>                                  193   128     0        1
//   <4, 4, false>                                 256   157     0        1           <4, 1, false>                                 197   128     0        1
// (the waves per SIMD are those of the launch bounds, as for the other modes; the figures are those of PAIR_BETA in csrc/dnmf_beta.h,
// register for register).  JT = 4 at KP = 128 does not spill, so the W side takes the Itakura-Saito and beta plan there (one pass over
// S): the launch geometry, and with it the order of every sum, is that of PAIR_BETA at every shape, which is what makes delta = inf
// the beta = 2 step bit for bit.  masked_reduce_kernel<RULE_RATIO>: 20 VGPRs; tile_sum_kernel<KT, FAST, HuberTerm>: 136 VGPRs (FAST) /
// 134 (generic) + 64 AGPRs at two waves per SIMD, the same at every KT; slot_sum_kernel: 12 VGPRs; none uses scratch.
#pragma once
#include "dnmf_masked.h"

namespace {

// delta > 0, inf included; a NaN compares false
inline bool huber_delta_ok(float delta) { return delta > 0.f; }

// delta in the place of the beta mode's exponent; the rule's exponent stays 1
inline PairExp huber_exp(float delta) { return PairExp{delta, 1.f}; }

// ---- what the mode chooses on the launch path of csrc/dnmf_masked.h: the Itakura-Saito and beta plans ON PURPOSE (one part of the
// output columns at KP = 128, at least four row chunks on the H side: the table above shows JT = 4 without scratch), the plain ratio
template <>
struct PairMode<PAIR_HUBER> {
    static constexpr int zdim128 = 1;
    static constexpr long min_chunks = 4;
    static constexpr int rule = RULE_RATIO;     // X <- X * num / (den + eps)
    static constexpr const char* serves = "the Huber kernels";
};

// ---- the objective sum rho_delta(a - s') is tile_sum_kernel of csrc/dnmf_sums.h with this term: the walk as it is, fp32 over the 64
// elements a lane holds of one 32 x 128 tile, float64 from there on, every tile's sum in its own slot and the slots added in a fixed
// order -- no atomics, two calls are bit-identical.  Both branches are evaluated and one is selected (at delta = inf the linear one is
// inf or NaN and never taken: |r| <= inf).  Outside the block r = -eps, a term of 7e-15 that is SELECTED away, like every term of this walk
struct HuberTerm {
    static constexpr int NSUM = 1;
    float delta = 1.f;
    __device__ __forceinline__ void add(float (&t)[1], float a, float s, float eps, bool in) const {
        const float r = fabsf(a - (s + eps));
        const float d = r <= delta ? 0.5f * r * r : delta * (r - 0.5f * delta);
        t[0] += in ? d : 0.f;
    }
};

}  // namespace
