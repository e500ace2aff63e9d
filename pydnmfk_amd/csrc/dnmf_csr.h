// dnmf_csr.h -- kernels for a data block held as CSR (int32 row pointers and column indices, float32 values, columns sorted
// within a row) next to the CSR of its transpose.  Every update rule touches A only through products in which a zero of A
// contributes exactly zero, so a step needs three kinds of pass over the stored entries:
//     mm      Out[r] = sum_p val[p] F[col[p]]                                   (A H^T on the block, (W^T A)^T on the transpose)
//     kl_mm   Out[r] = sum_p val[p] / (<L[r], F[col[p]]> + eps) F[col[p]]       (the KL products, quotient fused)
//     resid   sum_p val[p] (val[p] - 2 <L[r], F[col[p]]>) in float64           (||A - W H||^2 minus the Gram term)
// A block whose UNSTORED entries are missing (not observed) restricts the objective to the stored positions: its passes have the
// same shape but leave TWO k-vectors per row, the numerator and the denominator of the multiplicative rule,
//     m_fro   num[r] = sum_p val[p] F[col[p]],                      den[r] = sum_p <L[r], F[col[p]]> F[col[p]]
//     m_kl    num[r] = sum_p val[p] / (<L[r], F[col[p]]> + eps) F[col[p]],   den[r] = sum_p F[col[p]]
//     m_resid sum_p (val[p] - <L[r], F[col[p]]>)^2 in float64        (no Gram term: nothing outside the stored positions counts)
// An NMFk sweep adds two passes outside the fits (end of this file): the perturbed copy of a CSR image keyed by dense position, and
//     col_err num[c], den[c] in float64 per column from the transpose's image (the residual of modes 2 / 5, kept per row)
// The masked passes end either by storing the pair (the sides whose sums cross ranks) or, the wave holding L[r] in registers, by writing
// X[r] = L[r] * num / (den + eps) straight into the factor (it reads the packed copy, so nothing is updated under a reader).
// F and L are PACKED factor images [rows x KPAD] (csr_pack_kernel / csr_pack_t_kernel): KPAD = 16 / 32 / 64 / 128 / 256 floats,
// zero padded, so that a gathered row is 64 B (inside one 128-byte line) or whole 128-byte lines and is read as one float4 per
// lane, whatever k is.
//
// Work split (template parameter G = KPAD / 4 lanes per stored entry): a wave owns a row; it reads 64 (col, val) pairs coalesced,
// hands entry j to lane group j % (64 / G) by cross-lane reads, every group accumulates its entries in order, and the groups are
// folded once per row by an xor butterfly.  Nothing in this file is accumulated with atomics: the order of every sum is
// fixed by the matrix and G alone, so these kernels are bit-reproducible.
// Long rows (more than CSR_SEG entries; listed at construction of the block): cut into segments of CSR_SEG entries, one wave per
// segment writing a partial row, and one small launch that adds a row's partials in segment order.
#pragma once
#include "dnmf_common.h"
#include "dnmf_stream.h"

namespace {

constexpr int CSR_SEG = 1024;            // entries of one segment of a long row; rows up to this length are one wave's work
constexpr int CSR_RESID_WAVES = 8192;    // waves of the residual pass over the rows (each leaves one float64 partial)

template <int G, typename T>
__device__ inline T csr_sum_in_group(T v) {
#pragma unroll
    for (int off = 1; off < G; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int G, typename T>
__device__ inline T csr_sum_over_groups(T v) {
#pragma unroll
    for (int off = G; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int G>
__device__ inline f32x4 csr_fold(f32x4 a) {
    a.x = csr_sum_over_groups<G>(a.x);
    a.y = csr_sum_over_groups<G>(a.y);
    a.z = csr_sum_over_groups<G>(a.z);
    a.w = csr_sum_over_groups<G>(a.w);
    return a;
}

enum { CSR_MM = 0, CSR_KL_MM = 1, CSR_RESID = 2, CSR_M_FRO = 3, CSR_M_KL = 4, CSR_M_RESID = 5 };
enum { CSR_END_STORE = 0, CSR_END_UPDATE = 1 };     // masked passes: store [num | den], or write L[r] * num / (den + eps)

// MODE 0: mm, 1: kl_mm, 2: resid, 3: m_fro, 4: m_kl, 5: m_resid.  The stored entries [p0, p1) of one row; `lrow` = this lane's
// float4 of the packed row L[r]; `acc2` = the denominator's k-vector of the masked passes (untouched by the others).
template <int G, int MODE>
__device__ inline void csr_span(const int* __restrict__ col, const float* __restrict__ val, int p0, int p1,
                                const float* __restrict__ F, const f32x4 lrow, float eps, f32x4& acc, f32x4& acc2, double& dacc) {
    constexpr int NG = 64 / G, KPAD = 4 * G;
    const int lane = threadIdx.x & 63, grp = lane / G, l = lane % G;
    for (int base = p0; base < p1; base += 64) {
        const int p = base + lane;
        const bool in = p < p1;
        const int c = in ? col[p] : 0;
        const float v = in ? val[p] : 0.f;
        const int cnt = min(64, p1 - base);
#pragma unroll 2
        for (int j0 = 0; j0 < cnt; j0 += NG) {
            const int j = j0 + grp;                               // (< 64: j0 <= 64 - NG)
            const int cj = __shfl(c, j, 64);
            const float vj = __shfl(v, j, 64);
            const bool ok = j < cnt;                              // uniform inside a lane group
            f32x4 f = {0.f, 0.f, 0.f, 0.f};
            if (ok) f = *reinterpret_cast<const f32x4*>(F + (size_t)cj * KPAD + 4 * l);
            if (MODE == 0) {
                if (ok) {
                    acc.x = fmaf(vj, f.x, acc.x); acc.y = fmaf(vj, f.y, acc.y);
                    acc.z = fmaf(vj, f.z, acc.z); acc.w = fmaf(vj, f.w, acc.w);
                }
            } else if (MODE == 1) {
                float t = lrow.x * f.x;
                t = fmaf(lrow.y, f.y, t); t = fmaf(lrow.z, f.z, t); t = fmaf(lrow.w, f.w, t);
                const float d = csr_sum_in_group<G>(t);
                if (ok) {
                    const float q = vj / (d + eps);
                    acc.x = fmaf(q, f.x, acc.x); acc.y = fmaf(q, f.y, acc.y);
                    acc.z = fmaf(q, f.z, acc.z); acc.w = fmaf(q, f.w, acc.w);
                }
            } else if (MODE == 3 || MODE == 4) {
                float t = lrow.x * f.x;
                t = fmaf(lrow.y, f.y, t); t = fmaf(lrow.z, f.z, t); t = fmaf(lrow.w, f.w, t);
                const float d = csr_sum_in_group<G>(t);
                if (ok) {
                    if (MODE == 3) {
                        acc.x = fmaf(vj, f.x, acc.x); acc.y = fmaf(vj, f.y, acc.y);
                        acc.z = fmaf(vj, f.z, acc.z); acc.w = fmaf(vj, f.w, acc.w);
                        acc2.x = fmaf(d, f.x, acc2.x); acc2.y = fmaf(d, f.y, acc2.y);
                        acc2.z = fmaf(d, f.z, acc2.z); acc2.w = fmaf(d, f.w, acc2.w);
                    } else {
                        const float q = vj / (d + eps);             // (a stored zero: q = 0, and it counts in the denominator)
                        acc.x = fmaf(q, f.x, acc.x); acc.y = fmaf(q, f.y, acc.y);
                        acc.z = fmaf(q, f.z, acc.z); acc.w = fmaf(q, f.w, acc.w);
                        acc2.x += f.x; acc2.y += f.y; acc2.z += f.z; acc2.w += f.w;
                    }
                }
            } else {
                double t = (double)lrow.x * (double)f.x;
                t = fma((double)lrow.y, (double)f.y, t); t = fma((double)lrow.z, (double)f.z, t); t = fma((double)lrow.w, (double)f.w, t);
                const double d = csr_sum_in_group<G>(t);
                if (MODE == 2) {
                    if (ok && l == 0) dacc += (double)vj * ((double)vj - 2.0 * d);
                } else if (ok && l == 0) {
                    const double e = (double)vj - d;
                    dacc = fma(e, e, dacc);
                }
            }
        }
    }
}

__device__ inline void csr_store(float* __restrict__ out, long ldo, int out_trans, long r, int c0, const f32x4 a, int k) {
    const float e[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (c0 + i < k) {
            if (out_trans) out[(size_t)(c0 + i) * ldo + r] = e[i];
            else out[(size_t)r * ldo + c0 + i] = e[i];
        }
}

// the masked passes' pair: num -> out, den -> out2 at the same offsets.  (One loop for both: two csr_store calls in a row crash
// hipcc 7.2's optimizer at G = 64, where every lane stores.)
__device__ inline void csr_store_pair(float* __restrict__ out, float* __restrict__ out2, long ldo, int out_trans, long r, int c0,
                                      const f32x4 a, const f32x4 b, int k) {
    const float e[4] = {a.x, a.y, a.z, a.w}, g[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (c0 + i < k) {
            const size_t o = out_trans ? (size_t)(c0 + i) * ldo + r : (size_t)r * ldo + c0 + i;
            out[o] = e[i];
            out2[o] = g[i];
        }
}

// the multiplicative rule on this lane's float4: x * num / (den + eps), optionally clamped from below (0 / (0 + eps) = 0 stays finite)
__device__ inline float csr_ratio1(float x, float num, float den, float eps, int clamp) {
    const float y = x * (num / (den + eps));
    return clamp ? fmaxf(y, eps) : y;
}

__device__ inline f32x4 csr_ratio(const f32x4 x, const f32x4 num, const f32x4 den, float eps, int clamp) {
    return f32x4{csr_ratio1(x.x, num.x, den.x, eps, clamp), csr_ratio1(x.y, num.y, den.y, eps, clamp),
                 csr_ratio1(x.z, num.z, den.z, eps, clamp), csr_ratio1(x.w, num.w, den.w, eps, clamp)};
}

// one wave per row, four rows per workgroup; rows longer than CSR_SEG are left to the segment kernels.  Masked passes (MODE 3, 4):
// END = CSR_END_STORE writes num -> out, den -> out2 (same ld and orientation); CSR_END_UPDATE writes L[r] * num / (den + eps) -> out
template <int G, int MODE, int END = CSR_END_STORE>
__global__ __launch_bounds__(256) void csr_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                       const float* __restrict__ val, long rows, const float* __restrict__ L,
                                                       const float* __restrict__ F, int k, float eps, float* __restrict__ out,
                                                       long ldo, int out_trans, float* __restrict__ out2, int clamp) {
    constexpr int KPAD = 4 * G;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63, l = lane % G;
    const int p0 = rowptr[r], p1 = rowptr[r + 1];
    if (p1 - p0 > CSR_SEG) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f}, lrow = {0.f, 0.f, 0.f, 0.f};
    double dacc = 0.0;
    if (MODE != 0 && p1 > p0) lrow = *reinterpret_cast<const f32x4*>(L + (size_t)r * KPAD + 4 * l);
    csr_span<G, MODE>(col, val, p0, p1, F, lrow, eps, acc, acc2, dacc);
    acc = csr_fold<G>(acc);
    if (MODE == 3 || MODE == 4) {
        acc2 = csr_fold<G>(acc2);
        if (lane < G) {
            if (END == CSR_END_STORE) {
                csr_store_pair(out, out2, ldo, out_trans, r, 4 * l, acc, acc2, k);
            } else {                                              // (a row without a stored entry: num = 0, the row becomes 0)
                csr_store(out, ldo, out_trans, r, 4 * l, csr_ratio(lrow, acc, acc2, eps, clamp), k);
            }
        }
    } else if (lane < G) {
        csr_store(out, ldo, out_trans, r, 4 * l, acc, k);
    }
}

// the residual's pass over the rows: a fixed number of waves, wave w takes rows w, w + nw, ... and leaves ONE float64 partial
template <int G, int MODE = 2>
__global__ __launch_bounds__(256) void csr_resid_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const float* __restrict__ val, long rows, const float* __restrict__ L,
                                                             const float* __restrict__ F, double* __restrict__ dpart) {
    constexpr int KPAD = 4 * G;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
    const int lane = threadIdx.x & 63, l = lane % G;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
    double dacc = 0.0;
    for (long r = w; r < rows; r += nw) {
        const int p0 = rowptr[r], p1 = rowptr[r + 1];
        if (p1 == p0 || p1 - p0 > CSR_SEG) continue;
        const f32x4 lrow = *reinterpret_cast<const f32x4*>(L + (size_t)r * KPAD + 4 * l);
        csr_span<G, MODE>(col, val, p0, p1, F, lrow, 0.f, acc, acc2, dacc);
    }
    dacc = csr_sum_over_groups<G>(dacc);
    if (lane == 0) dpart[w] = dacc;
}

// one wave per segment of a long row: partial rows [nseg][KPAD] (MODE 0, 1), partial pairs [nseg][num | den][KPAD] (MODE 3, 4) or one
// float64 per segment (MODE 2, 5)
template <int G, int MODE>
__global__ __launch_bounds__(256) void csr_long_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                       const float* __restrict__ val, const float* __restrict__ L,
                                                       const float* __restrict__ F, float eps, const int* __restrict__ long_rows,
                                                       const int* __restrict__ long_segptr, int n_long, float* __restrict__ part,
                                                       double* __restrict__ dpart) {
    constexpr int KPAD = 4 * G;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= long_segptr[n_long]) return;
    int lo = 0, hi = n_long;                                       // the long row whose segments include s
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (long_segptr[mid] <= s) lo = mid; else hi = mid;
    }
    const long r = long_rows[lo];
    const int lane = threadIdx.x & 63, l = lane % G;
    const int p0 = rowptr[r] + (s - long_segptr[lo]) * CSR_SEG, p1 = min(p0 + CSR_SEG, rowptr[r + 1]);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f}, lrow = {0.f, 0.f, 0.f, 0.f};
    double dacc = 0.0;
    if (MODE != 0) lrow = *reinterpret_cast<const f32x4*>(L + (size_t)r * KPAD + 4 * l);
    csr_span<G, MODE>(col, val, p0, p1, F, lrow, eps, acc, acc2, dacc);
    if (MODE == 2 || MODE == 5) {
        dacc = csr_sum_over_groups<G>(dacc);
        if (lane == 0) dpart[s] = dacc;
    } else if (MODE == 3 || MODE == 4) {
        acc = csr_fold<G>(acc);
        acc2 = csr_fold<G>(acc2);
        if (lane < G) {
            *reinterpret_cast<f32x4*>(part + ((size_t)s * 2) * KPAD + 4 * l) = acc;
            *reinterpret_cast<f32x4*>(part + ((size_t)s * 2 + 1) * KPAD + 4 * l) = acc2;
        }
    } else {
        acc = csr_fold<G>(acc);
        if (lane < G) *reinterpret_cast<f32x4*>(part + (size_t)s * KPAD + 4 * l) = acc;
    }
}

// a long row's partial rows added in segment order: one workgroup of `kpad` threads per long row
__global__ void csr_long_reduce_kernel(const float* __restrict__ part, int kpad, const int* __restrict__ long_rows,
                                       const int* __restrict__ long_segptr, int k, float* __restrict__ out, long ldo, int out_trans) {
    const int i = blockIdx.x, c = threadIdx.x;
    const long r = long_rows[i];
    float a = 0.f;
    for (int s = long_segptr[i]; s < long_segptr[i + 1]; ++s) a += part[(size_t)s * kpad + c];
    if (c < k) {
        if (out_trans) out[(size_t)c * ldo + r] = a;
        else out[(size_t)r * ldo + c] = a;
    }
}

// a long row's partial pairs [num | den] added in segment order, then stored as a pair (END = CSR_END_STORE: num -> out, den ->
// out2) or applied (CSR_END_UPDATE: L[r] * num / (den + eps) -> out): one workgroup of `kpad` threads per long row
template <int END>
__global__ void csr_long_reduce_pair_kernel(const float* __restrict__ part, int kpad, const int* __restrict__ long_rows,
                                            const int* __restrict__ long_segptr, const float* __restrict__ L, int k, float eps, int clamp,
                                            float* __restrict__ out, float* __restrict__ out2, long ldo, int out_trans) {
    const int i = blockIdx.x, c = threadIdx.x;
    const long r = long_rows[i];
    float a = 0.f, b = 0.f;
    for (int s = long_segptr[i]; s < long_segptr[i + 1]; ++s) {
        a += part[((size_t)s * 2) * kpad + c];
        b += part[((size_t)s * 2 + 1) * kpad + c];
    }
    if (c < k) {
        const size_t o = out_trans ? (size_t)c * ldo + r : (size_t)r * ldo + c;
        if (END == CSR_END_STORE) {
            out[o] = a;
            out2[o] = b;
        } else {
            out[o] = csr_ratio1(L[(size_t)r * kpad + c], a, b, eps, clamp);
        }
    }
}

// X = X * num / (den + eps), optionally clamped from below: the multiplicative rule after the pair has been summed over the ranks.
// X [rows x cols] with leading dimension ldx; num and den [rows x cols] with leading dimension ldp.  V = 4: 16-byte accesses.
template <int V>
__global__ __launch_bounds__(256) void csr_ratio_kernel(float* __restrict__ X, long rows, long cols, long ldx, const float* __restrict__ num,
                                                        const float* __restrict__ den, long ldp, float eps, int clamp) {
    const long cv = cols / V, total = rows * cv;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / cv, c = (idx % cv) * V;
        if (V == 4) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(X + r * ldx + c);
            const f32x4 a = *reinterpret_cast<const f32x4*>(num + r * ldp + c);
            const f32x4 b = *reinterpret_cast<const f32x4*>(den + r * ldp + c);
            *reinterpret_cast<f32x4*>(X + r * ldx + c) = csr_ratio(x, a, b, eps, clamp);
        } else {
            X[r * ldx + c] = csr_ratio1(X[r * ldx + c], num[r * ldp + c], den[r * ldp + c], eps, clamp);
        }
    }
}

// ---- packed factor images
// P[rows x kpad] = X[rows x k], zero padded (W)
__global__ __launch_bounds__(256) void csr_pack_kernel(const float* __restrict__ X, long rows, int k, long ldx, float* __restrict__ P,
                                                       int kpad) {
    const int q = kpad / 4;
    const long total = rows * q;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / q;
        const int c = (int)(idx % q) * 4;
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = c + e < k ? X[r * ldx + c + e] : 0.f;
        *reinterpret_cast<f32x4*>(P + r * kpad + c) = f32x4{d[0], d[1], d[2], d[3]};
    }
}

// P[n x kpad] = X[k x n]^T, zero padded (H): 32 x 32 tiles through LDS, reads and writes both along rows
__global__ __launch_bounds__(256) void csr_pack_t_kernel(const float* __restrict__ X, int k, long n, long ldx, float* __restrict__ P,
                                                         int kpad) {
    __shared__ float tile[32][33];
    const long n0 = (long)blockIdx.x * 32;
    const int k0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int kk = k0 + ty + 8 * i;
        tile[ty + 8 * i][tx] = (kk < k && n0 + tx < n) ? X[(size_t)kk * ldx + n0 + tx] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cc = ty + 8 * i;
        if (n0 + cc < n && k0 + tx < kpad) P[(size_t)(n0 + cc) * kpad + k0 + tx] = tile[tx][cc];
    }
}

// ---- float64 Gram partials of a packed image: part[chunk][k x k] = sum over the chunk's rows of X[r][i] X[r][j]
__global__ __launch_bounds__(256) void csr_gram_f64_kernel(const float* __restrict__ X, long rows, int kpad, int k, long rows_per_chunk,
                                                           double* __restrict__ part) {
    __shared__ float sa[64][17], sb[64][17];
    const int nt = (k + 15) / 16;
    const int ti = blockIdx.y / nt, tj = blockIdx.y % nt, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long r0 = (long)blockIdx.x * rows_per_chunk, r1 = min(rows, r0 + rows_per_chunk);
    double acc = 0.0;
    for (long rb = r0; rb < r1; rb += 64) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = threadIdx.x + 256 * e, rr = idx >> 4, cc = idx & 15;
            const long row = rb + rr;
            sa[rr][cc] = row < r1 ? X[(size_t)row * kpad + ti * 16 + cc] : 0.f;
            sb[rr][cc] = row < r1 ? X[(size_t)row * kpad + tj * 16 + cc] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int rr = 0; rr < 64; ++rr) acc = fma((double)sa[rr][ty], (double)sb[rr][tx], acc);
        __syncthreads();
    }
    const int i = ti * 16 + ty, j = tj * 16 + tx;
    if (i < k && j < k) part[(size_t)blockIdx.x * k * k + i * k + j] = acc;
}

// sq[0] = max(0, sum_e (sum_c gw[c][e]) (sum_c gh[c][e]) + sum dpart): one workgroup, every sum in a fixed order
__global__ __launch_bounds__(256) void csr_resid_final_kernel(const double* __restrict__ gw, int ncw, const double* __restrict__ gh,
                                                              int nch, int k, const double* __restrict__ dpart, long ndpart,
                                                              double* __restrict__ sq) {
    __shared__ double sh[256];
    const int kk = k * k;
    double t = 0.0;
    for (int e = threadIdx.x; e < kk; e += 256) {
        double a = 0.0, b = 0.0;
        for (int c = 0; c < ncw; ++c) a += gw[(size_t)c * kk + e];
        for (int c = 0; c < nch; ++c) b += gh[(size_t)c * kk + e];
        t = fma(a, b, t);
    }
    double u = 0.0;
    for (long e = threadIdx.x; e < ndpart; e += 256) u += dpart[e];
    sh[threadIdx.x] = t + u;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) sq[0] = sh[0] > 0.0 ? sh[0] : 0.0;
}

// ---- NMFk on a sparse block: the perturbed copy and the per-column error
// val_out[p] = val[p] * (1 + nv + 2 nv u), u the uniform the dense kernels of csrc/dnmf_stream.h give the element's position in the
// DENSE block (perturb_factor: one definition of the stream), so the perturbed block is the dense kernels' output at the stored
// positions, bit for bit.  One kernel for both images: on the block's own image a stored entry (ir, ic) sits at dense position
// (ir, ic), on the transpose's image (`transposed`) at (ic, ir); `ncols` = the dense block's column count.  A wave takes rows
// w, w + nw, ... and walks each 64 entries at a time, however long the row is; a value depends on (seed, position) only.
__global__ __launch_bounds__(256) void csr_perturb_uniform_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                  const float* __restrict__ val, long rows, long ncols, int transposed,
                                                                  float nv, unsigned long long seed, float* __restrict__ val_out) {
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
    const int lane = threadIdx.x & 63;
    const unsigned long long key = perturb_key(seed);
    for (long ir = w; ir < rows; ir += nw) {
        const int p1 = rowptr[ir + 1];
        for (int p = rowptr[ir] + lane; p < p1; p += 64) {
            const unsigned long long ic = (unsigned long long)col[p];
            const unsigned long long L = transposed ? ic * (unsigned long long)ncols + (unsigned long long)ir
                                                    : (unsigned long long)ir * (unsigned long long)ncols + ic;
            val_out[p] = val[p] * perturb_factor(key, L, nv);
        }
    }
}

// The stored entries [p0, p1) of one row of the TRANSPOSE's image (a column c of the block), `lrow` = this lane's float4 of the
// packed H^T[c], F = packed W: per entry d = <H^T[c], W[r]> in float64 as in csr_span modes 2 and 5, then
//     zero meaning:  num += a (a - 2 d)      missing='unstored':  num += (a - d)^2      both:  den += a^2
// accumulated by lane 0 of every lane group (the caller folds the groups).
template <int G, bool MASKED>
__device__ inline void csr_span_err(const int* __restrict__ col, const float* __restrict__ val, int p0, int p1, const float* __restrict__ F,
                                    const f32x4 lrow, double& num, double& den) {
    constexpr int NG = 64 / G, KPAD = 4 * G;
    const int lane = threadIdx.x & 63, grp = lane / G, l = lane % G;
    for (int base = p0; base < p1; base += 64) {
        const int p = base + lane;
        const bool in = p < p1;
        const int c = in ? col[p] : 0;
        const float v = in ? val[p] : 0.f;
        const int cnt = min(64, p1 - base);
#pragma unroll 2
        for (int j0 = 0; j0 < cnt; j0 += NG) {
            const int j = j0 + grp;
            const int cj = __shfl(c, j, 64);
            const double vj = (double)__shfl(v, j, 64);
            const bool ok = j < cnt;                              // uniform inside a lane group
            f32x4 f = {0.f, 0.f, 0.f, 0.f};
            if (ok) f = *reinterpret_cast<const f32x4*>(F + (size_t)cj * KPAD + 4 * l);
            double t = (double)lrow.x * (double)f.x;
            t = fma((double)lrow.y, (double)f.y, t); t = fma((double)lrow.z, (double)f.z, t); t = fma((double)lrow.w, (double)f.w, t);
            const double d = csr_sum_in_group<G>(t);
            if (ok && l == 0) {
                if (MASKED) {
                    const double e = vj - d;
                    num = fma(e, e, num);
                } else {
                    num += vj * (vj - 2.0 * d);
                }
                den = fma(vj, vj, den);
            }
        }
    }
}

// h^T Gm h in float64 for one packed row h and the symmetric k x k matrix Gm = W^T W (row-major; read through L2: 512 KB at k = 256
// do not fit LDS).  Lane i takes rows i, i + 64, ... (column i of Gm read along the lanes: Gm is symmetric), the lanes' sums are
// folded by an xor butterfly: every lane of the wave returns the total, in an order fixed by k alone.
__device__ inline double csr_gram_quad(const double* __restrict__ Gm, const float* __restrict__ h, int k) {
    double t = 0.0;
    for (int i = threadIdx.x & 63; i < k; i += 64) {
        double s = 0.0;
        for (int j = 0; j < k; ++j) s = fma(Gm[(size_t)j * k + i], (double)h[j], s);
        t = fma((double)h[i], s, t);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) t += __shfl_xor(t, off, 64);
    return t;
}

// one wave per row of the transpose's image (a column of the block), four per workgroup: num[c], den[c].  Gm = nullptr under
// missing='unstored' (no Gram term).  A row without a stored entry: den = 0, num = the Gram term or 0.  Rows longer than CSR_SEG
// are left to the two kernels below.
template <int G, bool MASKED>
__global__ __launch_bounds__(256) void csr_colerr_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              const float* __restrict__ val, long rows, const float* __restrict__ L,
                                                              const float* __restrict__ F, int k, const double* __restrict__ Gm,
                                                              double* __restrict__ num, double* __restrict__ den) {
    constexpr int KPAD = 4 * G;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63, l = lane % G;
    const int p0 = rowptr[r], p1 = rowptr[r + 1];
    if (p1 - p0 > CSR_SEG) return;
    double a = 0.0, b = 0.0;
    if (p1 > p0) {
        const f32x4 lrow = *reinterpret_cast<const f32x4*>(L + (size_t)r * KPAD + 4 * l);
        csr_span_err<G, MASKED>(col, val, p0, p1, F, lrow, a, b);
        a = csr_sum_over_groups<G>(a);
        b = csr_sum_over_groups<G>(b);
    }
    if (!MASKED) a += csr_gram_quad(Gm, L + (size_t)r * KPAD, k);
    if (lane == 0) {
        num[r] = a;
        den[r] = b;
    }
}

// one wave per segment of a long row: the pair of float64 partials dpart[2 s], dpart[2 s + 1]
template <int G, bool MASKED>
__global__ __launch_bounds__(256) void csr_colerr_long_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              const float* __restrict__ val, const float* __restrict__ L,
                                                              const float* __restrict__ F, const int* __restrict__ long_rows,
                                                              const int* __restrict__ long_segptr, int n_long, double* __restrict__ dpart) {
    constexpr int KPAD = 4 * G;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= long_segptr[n_long]) return;
    int lo = 0, hi = n_long;                                       // the long row whose segments include s
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (long_segptr[mid] <= s) lo = mid; else hi = mid;
    }
    const long r = long_rows[lo];
    const int lane = threadIdx.x & 63, l = lane % G;
    const int p0 = rowptr[r] + (s - long_segptr[lo]) * CSR_SEG, p1 = min(p0 + CSR_SEG, rowptr[r + 1]);
    const f32x4 lrow = *reinterpret_cast<const f32x4*>(L + (size_t)r * KPAD + 4 * l);
    double a = 0.0, b = 0.0;
    csr_span_err<G, MASKED>(col, val, p0, p1, F, lrow, a, b);
    a = csr_sum_over_groups<G>(a);
    b = csr_sum_over_groups<G>(b);
    if (lane == 0) {
        dpart[2 * (size_t)s] = a;
        dpart[2 * (size_t)s + 1] = b;
    }
}

// a long row's partial pairs added in segment order, then the Gram term (Gm != nullptr): one wave per long row
__global__ __launch_bounds__(64) void csr_colerr_long_reduce_kernel(const double* __restrict__ dpart, const int* __restrict__ long_rows,
                                                                    const int* __restrict__ long_segptr, const float* __restrict__ L,
                                                                    int kpad, int k, const double* __restrict__ Gm,
                                                                    double* __restrict__ num, double* __restrict__ den) {
    const int i = blockIdx.x;
    const long r = long_rows[i];
    double a = 0.0, b = 0.0;
    for (int s = long_segptr[i]; s < long_segptr[i + 1]; ++s) {
        a += dpart[2 * (size_t)s];
        b += dpart[2 * (size_t)s + 1];
    }
    if (Gm) a += csr_gram_quad(Gm, L + (size_t)r * kpad, k);
    if (threadIdx.x == 0) {
        num[r] = a;
        den[r] = b;
    }
}

// Gm[e] = sum over the chunks of csr_gram_f64_kernel's partials, in chunk order
__global__ __launch_bounds__(256) void csr_gram_sum_kernel(const double* __restrict__ part, int nchunks, int kk, double* __restrict__ Gm) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= kk) return;
    double a = 0.0;
    for (int c = 0; c < nchunks; ++c) a += part[(size_t)c * kk + e];
    Gm[e] = a;
}

}  // namespace
