// dnmf_csr_batch.h -- the passes of csrc/dnmf_csr.h for a BATCH of problems that share one CSR pattern (row pointers, column indices,
// the transpose's pattern, the long-row lists) and differ in their value arrays and factors: the perturbation fits of an NMFk sweep
// over a sparse block (SparseBlock.with_values).  The index stream is the same for all of them, so it is read once per tile of BT
// problems, and the factor rows that one stored entry gathers for the BT problems lie next to each other in memory.
//
// Problem-interleaved packed images.  csrb_pack_kernel / csrb_pack_t_kernel write W and H^T of tile t (problems t BT .. t BT + BT - 1)
// as [tile][row][BT][KPAD] floats.  What one stored entry (r, c) gathers for the whole tile is then ONE contiguous run of BT KPAD 4
// bytes: at KPAD = 16 the single kernels fetch a 64-byte row out of a 128-byte line per problem, here every fetched line is used whole.
//
// Work split.  A wave owns a row (or a CSR_SEG segment of a long row), reads 64 column indices once, reads the 64 values of each problem
// of its tile coalesced from the stacked value array [batch][nnz] (`vstride` elements apart) and keeps BT accumulator sets in registers;
// gridDim.z = tiles, the last tile may hold fewer than BT problems (`nb`, wave-uniform).  BT per KPAD (csrb_bt): the registers of a lane
// do not depend on KPAD (G = KPAD / 4 lanes share an entry, each holds one float4 per k-vector), the line argument only needs
// BT KPAD >= 32, and from KPAD = 32 on a gathered row is whole lines already -- there BT only spares index reads, so it shrinks as the
// bytes gathered per index grow.  A single problem (batch == 1) runs the same kernels at BT = 1: its images are the plain packed images
// (rows interleaved with absent problems would only spread the gather over BT times the memory, and the accumulator sets of absent
// problems cost occupancy: measured on 2^20 x 2^16 with 5 10^7 entries, a single fit at BT = 8 took 1.28 x the step loop's time).
//
// Bits.  For every problem the association of every sum is csr_span's: the same G lanes per entry, entry j of a 64-entry group in lane
// group j % (64 / G), in-order accumulation (csrb_entry is the body of csr_span's inner loop, statement for statement), the same xor
// butterflies, long rows cut at CSR_SEG with partials added in segment order, the float64 partial layout of the residual and its final
// sum order.  Problem b of a batch therefore has the bits of the same problem run through the single kernels.  No atomics.
#pragma once
#include "dnmf_csr.h"

namespace {

constexpr int csrb_bt(int kpad) { return kpad <= 16 ? 8 : (kpad <= 64 ? 4 : 2); }

// a pointer `bytes` further on (the per-problem workspace slices and factor stacks are addressed by byte distances)
template <typename T>
__device__ __forceinline__ T* csrb_at(T* p, long bytes) { return (T*)((char*)p + bytes); }

// one stored entry of one problem: the body of csr_span's inner loop (MODE as there; `ok` and `l` as there)
template <int G, int MODE>
__device__ __forceinline__ void csrb_entry(const float vj, const f32x4 f, const bool ok, const int l, const f32x4 lrow, const float eps,
                                           f32x4& acc, f32x4& acc2, double& dacc) {
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
                const float q = vj / (d + eps);
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

// The stored entries [p0, p1) of one row for the `nb` problems of a tile.  `val`: the tile's first value array; `F`: the tile's
// interleaved image [frows][BT][KPAD]; lrow / acc / acc2 / dacc: one per problem (compile-time indexed: registers).
template <int G, int MODE, int BT>
__device__ inline void csrb_span(const int* __restrict__ col, const float* __restrict__ val, long vstride, int nb, int p0, int p1,
                                 const float* __restrict__ F, const f32x4 (&lrow)[BT], float eps, f32x4 (&acc)[BT], f32x4 (&acc2)[BT],
                                 double (&dacc)[BT]) {
    constexpr int NG = 64 / G, KPAD = 4 * G;
    const int lane = threadIdx.x & 63, grp = lane / G, l = lane % G;
    for (int base = p0; base < p1; base += 64) {
        const int p = base + lane;
        const bool in = p < p1;
        const int c = in ? col[p] : 0;                            // ONE index read for the tile
        float v[BT];
        static_for<0, BT>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            v[b] = (in && b < nb) ? val[(size_t)b * vstride + p] : 0.f;
        });
        const int cnt = min(64, p1 - base);
        for (int j0 = 0; j0 < cnt; j0 += NG) {
            const int j = j0 + grp;                               // (< 64: j0 <= 64 - NG)
            const int cj = __shfl(c, j, 64);
            const bool ok = j < cnt;                              // uniform inside a lane group
            const float* frow = F + (size_t)cj * (BT * KPAD) + 4 * l;      // the run of BT KPAD floats this entry gathers
            static_for<0, BT>([&](auto bc) {
                constexpr int b = decltype(bc)::value;
                if (b < nb) {                                     // (wave-uniform)
                    const float vj = __shfl(v[b], j, 64);
                    f32x4 f = {0.f, 0.f, 0.f, 0.f};
                    if (ok) f = *reinterpret_cast<const f32x4*>(frow + b * KPAD);
                    csrb_entry<G, MODE>(vj, f, ok, l, lrow[b], eps, acc[b], acc2[b], dacc[b]);
                }
            });
        }
    }
}

template <int BT>
__device__ __forceinline__ void csrb_zero(f32x4 (&a)[BT], f32x4 (&b)[BT], f32x4 (&c)[BT], double (&d)[BT]) {
    static_for<0, BT>([&](auto bc) {
        constexpr int i = decltype(bc)::value;
        a[i] = f32x4{0.f, 0.f, 0.f, 0.f}; b[i] = a[i]; c[i] = a[i]; d[i] = 0.0;
    });
}

// the packed rows L[r] of the tile's problems (this lane's float4 each)
template <int G, int BT>
__device__ __forceinline__ void csrb_lrows(const float* __restrict__ Lt, long r, int nb, f32x4 (&lrow)[BT]) {
    constexpr int KPAD = 4 * G;
    const int l = (threadIdx.x & 63) % G;
    static_for<0, BT>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if (b < nb) lrow[b] = *reinterpret_cast<const f32x4*>(Lt + ((size_t)r * BT + b) * KPAD + 4 * l);
    });
}

// one wave per row, four rows per workgroup, gridDim.z = tiles; rows longer than CSR_SEG are left to the segment kernels.  Problem b
// writes at `out` + b `ostride` BYTES (a workspace slice, or the factor stack itself under CSR_END_UPDATE); endings as csr_rows_kernel
template <int G, int MODE, int END, int BT>
__global__ __launch_bounds__(256) void csrb_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const float* __restrict__ val, long vstride, long rows, int batch,
                                                        const float* __restrict__ Limg, const float* __restrict__ Fimg, long frows, int k,
                                                        float eps, float* __restrict__ out, float* __restrict__ out2, long ostride, long ldo,
                                                        int out_trans, int clamp) {
    constexpr int KPAD = 4 * G;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int tile = blockIdx.z, nb = min(BT, batch - tile * BT);
    const int lane = threadIdx.x & 63, l = lane % G;
    const int p0 = rowptr[r], p1 = rowptr[r + 1];
    if (p1 - p0 > CSR_SEG) return;
    f32x4 acc[BT], acc2[BT], lrow[BT];
    double dacc[BT];
    csrb_zero<BT>(acc, acc2, lrow, dacc);
    if (MODE != 0 && p1 > p0) csrb_lrows<G, BT>(Limg + (size_t)tile * rows * BT * KPAD, r, nb, lrow);
    csrb_span<G, MODE, BT>(col, val + (size_t)tile * BT * vstride, vstride, nb, p0, p1, Fimg + (size_t)tile * frows * BT * KPAD, lrow, eps,
                           acc, acc2, dacc);
    static_for<0, BT>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if (b < nb) {
            const long ob = (long)(tile * BT + b) * ostride;
            const f32x4 a = csr_fold<G>(acc[b]);
            if (MODE == 3 || MODE == 4) {
                const f32x4 a2 = csr_fold<G>(acc2[b]);
                if (lane < G) {
                    if (END == CSR_END_STORE) csr_store_pair(csrb_at(out, ob), csrb_at(out2, ob), ldo, out_trans, r, 4 * l, a, a2, k);
                    else csr_store(csrb_at(out, ob), ldo, out_trans, r, 4 * l, csr_ratio(lrow[b], a, a2, eps, clamp), k);
                }
            } else if (lane < G) {
                csr_store(csrb_at(out, ob), ldo, out_trans, r, 4 * l, a, k);
            }
        }
    });
}

// the residual's pass over the rows (csr_resid_rows_kernel): wave w of a tile takes rows w, w + nw, ... and leaves ONE float64 partial
// per problem, dpart[w] of that problem's slice (`dstride` bytes apart)
template <int G, int MODE, int BT>
__global__ __launch_bounds__(256) void csrb_resid_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              const float* __restrict__ val, long vstride, long rows, int batch,
                                                              const float* __restrict__ Limg, const float* __restrict__ Fimg, long frows,
                                                              double* __restrict__ dpart, long dstride) {
    constexpr int KPAD = 4 * G;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
    const int tile = blockIdx.z, nb = min(BT, batch - tile * BT);
    const int lane = threadIdx.x & 63;
    f32x4 acc[BT], acc2[BT], lrow[BT];
    double dacc[BT];
    csrb_zero<BT>(acc, acc2, lrow, dacc);
    const float* Lt = Limg + (size_t)tile * rows * BT * KPAD;
    const float* Ft = Fimg + (size_t)tile * frows * BT * KPAD;
    val += (size_t)tile * BT * vstride;
    for (long r = w; r < rows; r += nw) {
        const int p0 = rowptr[r], p1 = rowptr[r + 1];
        if (p1 == p0 || p1 - p0 > CSR_SEG) continue;
        csrb_lrows<G, BT>(Lt, r, nb, lrow);
        csrb_span<G, MODE, BT>(col, val, vstride, nb, p0, p1, Ft, lrow, 0.f, acc, acc2, dacc);
    }
    static_for<0, BT>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if (b < nb) {
            const double d = csr_sum_over_groups<G>(dacc[b]);
            if (lane == 0) csrb_at(dpart, (long)(tile * BT + b) * dstride)[w] = d;
        }
    });
}

// one wave per segment of a long row (csr_long_kernel): per problem partial rows [nseg][KPAD] (MODE 0, 1), partial pairs
// [nseg][num | den][KPAD] (MODE 3, 4) or one float64 per segment (MODE 2, 5), in that problem's slice (`pstride` bytes apart)
template <int G, int MODE, int BT>
__global__ __launch_bounds__(256) void csrb_long_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const float* __restrict__ val, long vstride, long rows, int batch,
                                                        const float* __restrict__ Limg, const float* __restrict__ Fimg, long frows, float eps,
                                                        const int* __restrict__ long_rows, const int* __restrict__ long_segptr, int n_long,
                                                        float* __restrict__ part, double* __restrict__ dpart, long pstride) {
    constexpr int KPAD = 4 * G;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= long_segptr[n_long]) return;
    int lo = 0, hi = n_long;                                       // the long row whose segments include s
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (long_segptr[mid] <= s) lo = mid; else hi = mid;
    }
    const long r = long_rows[lo];
    const int tile = blockIdx.z, nb = min(BT, batch - tile * BT);
    const int lane = threadIdx.x & 63, l = lane % G;
    const int p0 = rowptr[r] + (s - long_segptr[lo]) * CSR_SEG, p1 = min(p0 + CSR_SEG, rowptr[r + 1]);
    f32x4 acc[BT], acc2[BT], lrow[BT];
    double dacc[BT];
    csrb_zero<BT>(acc, acc2, lrow, dacc);
    if (MODE != 0) csrb_lrows<G, BT>(Limg + (size_t)tile * rows * BT * KPAD, r, nb, lrow);
    csrb_span<G, MODE, BT>(col, val + (size_t)tile * BT * vstride, vstride, nb, p0, p1, Fimg + (size_t)tile * frows * BT * KPAD, lrow, eps,
                           acc, acc2, dacc);
    static_for<0, BT>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if (b < nb) {
            const long ob = (long)(tile * BT + b) * pstride;
            if (MODE == 2 || MODE == 5) {
                const double d = csr_sum_over_groups<G>(dacc[b]);
                if (lane == 0) csrb_at(dpart, ob)[s] = d;
            } else if (MODE == 3 || MODE == 4) {
                const f32x4 a = csr_fold<G>(acc[b]), a2 = csr_fold<G>(acc2[b]);
                if (lane < G) {
                    *reinterpret_cast<f32x4*>(csrb_at(part, ob) + ((size_t)s * 2) * KPAD + 4 * l) = a;
                    *reinterpret_cast<f32x4*>(csrb_at(part, ob) + ((size_t)s * 2 + 1) * KPAD + 4 * l) = a2;
                }
            } else {
                const f32x4 a = csr_fold<G>(acc[b]);
                if (lane < G) *reinterpret_cast<f32x4*>(csrb_at(part, ob) + (size_t)s * KPAD + 4 * l) = a;
            }
        }
    });
}

// a long row's partial rows added in segment order (csr_long_reduce_kernel): a workgroup of `kpad` threads per long row and problem
__global__ void csrb_long_reduce_kernel(const float* __restrict__ part, long pstride, int kpad, const int* __restrict__ long_rows,
                                        const int* __restrict__ long_segptr, int k, float* __restrict__ out, long ostride, long ldo,
                                        int out_trans) {
    const int i = blockIdx.x, c = threadIdx.x, b = blockIdx.y;
    const long r = long_rows[i];
    part = csrb_at(part, (long)b * pstride);
    out = csrb_at(out, (long)b * ostride);
    float a = 0.f;
    for (int s = long_segptr[i]; s < long_segptr[i + 1]; ++s) a += part[(size_t)s * kpad + c];
    if (c < k) {
        if (out_trans) out[(size_t)c * ldo + r] = a;
        else out[(size_t)r * ldo + c] = a;
    }
}

// a long row's partial pairs added in segment order, then stored or applied (csr_long_reduce_pair_kernel); L[r] of problem b is read from
// the interleaved image [tile][rows][bt][kpad]
template <int END>
__global__ void csrb_long_reduce_pair_kernel(const float* __restrict__ part, long pstride, int kpad, const int* __restrict__ long_rows,
                                             const int* __restrict__ long_segptr, const float* __restrict__ Limg, long rows, int bt, int k,
                                             float eps, int clamp, float* __restrict__ out, float* __restrict__ out2, long ostride, long ldo,
                                             int out_trans) {
    const int i = blockIdx.x, c = threadIdx.x, pb = blockIdx.y;
    const long r = long_rows[i];
    part = csrb_at(part, (long)pb * pstride);
    float a = 0.f, b = 0.f;
    for (int s = long_segptr[i]; s < long_segptr[i + 1]; ++s) {
        a += part[((size_t)s * 2) * kpad + c];
        b += part[((size_t)s * 2 + 1) * kpad + c];
    }
    if (c < k) {
        const size_t o = out_trans ? (size_t)c * ldo + r : (size_t)r * ldo + c;
        if (END == CSR_END_STORE) {
            csrb_at(out, (long)pb * ostride)[o] = a;
            csrb_at(out2, (long)pb * ostride)[o] = b;
        } else {
            const float x = Limg[(((size_t)(pb / bt) * rows + r) * bt + pb % bt) * kpad + c];
            csrb_at(out, (long)pb * ostride)[o] = csr_ratio1(x, a, b, eps, clamp);
        }
    }
}

// ---- problem-interleaved packed images
// P[b / bt][r][b % bt][kpad] = X_b[rows x k], zero padded (the W stack; X_b = X + b xstride elements); blockIdx.y = problem
__global__ __launch_bounds__(256) void csrb_pack_kernel(const float* __restrict__ X, long xstride, long rows, int k, long ldx,
                                                        float* __restrict__ P, int kpad, int bt) {
    const int q = kpad / 4, b = blockIdx.y;
    const long total = rows * q;
    X += (size_t)b * xstride;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / q;
        const int c = (int)(idx % q) * 4;
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = c + e < k ? X[r * ldx + c + e] : 0.f;
        *reinterpret_cast<f32x4*>(P + (((size_t)(b / bt) * rows + r) * bt + b % bt) * kpad + c) = f32x4{d[0], d[1], d[2], d[3]};
    }
}

// P[b / bt][c][b % bt][kpad] = X_b[k x n]^T, zero padded (the H stack): 32 x 32 tiles through LDS; blockIdx.z = problem
__global__ __launch_bounds__(256) void csrb_pack_t_kernel(const float* __restrict__ X, long xstride, int k, long n, long ldx,
                                                          float* __restrict__ P, int kpad, int bt) {
    __shared__ float tile[32][33];
    const long n0 = (long)blockIdx.x * 32;
    const int k0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5, b = blockIdx.z;
    X += (size_t)b * xstride;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int kk = k0 + ty + 8 * i;
        tile[ty + 8 * i][tx] = (kk < k && n0 + tx < n) ? X[(size_t)kk * ldx + n0 + tx] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cc = ty + 8 * i;
        if (n0 + cc < n && k0 + tx < kpad) P[(((size_t)(b / bt) * n + n0 + cc) * bt + b % bt) * kpad + k0 + tx] = tile[tx][cc];
    }
}

// ---- the residual's Gram term from the interleaved images (csr_gram_f64_kernel, csr_resid_final_kernel): blockIdx.z / blockIdx.x = problem
__global__ __launch_bounds__(256) void csrb_gram_f64_kernel(const float* __restrict__ X, long rows, int kpad, int bt, int k,
                                                            long rows_per_chunk, double* __restrict__ part, long pstride) {
    __shared__ float sa[64][17], sb[64][17];
    const int b = blockIdx.z;
    const int nt = (k + 15) / 16;
    const int ti = blockIdx.y / nt, tj = blockIdx.y % nt, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long r0 = (long)blockIdx.x * rows_per_chunk, r1 = min(rows, r0 + rows_per_chunk);
    X += ((size_t)(b / bt) * rows * bt + b % bt) * kpad;          // row r of problem b: X + r bt kpad
    const size_t ldx = (size_t)bt * kpad;
    double acc = 0.0;
    for (long rb = r0; rb < r1; rb += 64) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = threadIdx.x + 256 * e, rr = idx >> 4, cc = idx & 15;
            const long row = rb + rr;
            sa[rr][cc] = row < r1 ? X[(size_t)row * ldx + ti * 16 + cc] : 0.f;
            sb[rr][cc] = row < r1 ? X[(size_t)row * ldx + tj * 16 + cc] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int rr = 0; rr < 64; ++rr) acc = fma((double)sa[rr][ty], (double)sb[rr][tx], acc);
        __syncthreads();
    }
    const int i = ti * 16 + ty, j = tj * 16 + tx;
    if (i < k && j < k) csrb_at(part, (long)b * pstride)[(size_t)blockIdx.x * k * k + i * k + j] = acc;
}

__global__ __launch_bounds__(256) void csrb_resid_final_kernel(const double* __restrict__ gw, int ncw, const double* __restrict__ gh, int nch,
                                                               int k, const double* __restrict__ dpart, long ndpart, double* __restrict__ sq,
                                                               long stride) {
    __shared__ double sh[256];
    const long off = (long)blockIdx.x * stride;
    gw = csrb_at(gw, off); gh = csrb_at(gh, off); dpart = csrb_at(dpart, off); sq = csrb_at(sq, off);
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
    for (int off2 = 128; off2 > 0; off2 >>= 1) {
        if ((int)threadIdx.x < off2) sh[threadIdx.x] += sh[threadIdx.x + off2];
        __syncthreads();
    }
    if (threadIdx.x == 0) sq[0] = sh[0] > 0.0 ? sh[0] : 0.0;
}

}  // namespace
