// dnmf_f64_ops.h -- what the float64 translation units share (csrc/dnmf_f64.hip, csrc/dnmf_f64_div.hip): the fp64 MFMA, the MUBUF
// operand loads through buffer descriptors, the fixed-order block sum and the small host helpers.  Part of libdnmf_hip.so.
//
// v_mfma_f64_16x16x4_f64 operand maps (lane l, i = l & 15, q = l >> 4):
//   A-operand: A[row i][kk = q]   B-operand: B[kk = q][col i]   C/D: col = i, row = q + 4 * reg (reg in [0, 4))
#pragma once
#include "dnmf_common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
#define MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

namespace {

#define REQ(cond, ...) do { if (!(cond)) return fail(DNMF_EINVAL, __VA_ARGS__); } while (0)
inline hipStream_t ST(void* s) { clear_hip_error(); return reinterpret_cast<hipStream_t>(s); }
inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }
inline int tiles16(int k) { return (k + 15) / 16; }

// ---- MUBUF operand loads (dnmf_common.h "buffer addressing").  Round 6: the flat loads of the first version sat behind runtime
// branches (vector or element-wise, in or out of range), and hipcc answers a load under a branch with s_waitcnt vmcnt(0) at the next
// use -- the "two register sets" of the NT / TN kernels never overlapped anything (3 waits in f64_nt_kernel<4,4>, all vmcnt(0), behind
// 335 branches).  A buffer load needs no branch: a lane is switched off through its offset, rows beyond the operand fall outside the
// descriptor's byte count (the hardware returns 0), a 16-byte access only needs 4-byte alignment.
// descriptor over `bytes` bytes from `base` (both wave-uniform; at most 2 GiB: offsets are 31-bit, BUF_OOB is the off switch)
__device__ __forceinline__ i32x4 rsrc64(const double* base, long bytes) {
    i32x4 r = buf_rsrc(base);
    const long b = bytes < 0 ? 0 : (bytes > 0x7fffffffL ? 0x7fffffffL : bytes);
    r[2] = __builtin_amdgcn_readfirstlane((int)b);
    return r;
}
// N consecutive doubles (N = 1, 2, 4) at byte offset vo + soff; `nvalid` of them are in range (the rest: zero).  VEC: nvalid is 0 or N
// by construction of the caller (column counts divisible by N), so the lane moves as a whole
template <int N, bool VEC>
__device__ __forceinline__ void ldq(double (&d)[N], i32x4 rs, int vo, int soff, int nvalid) {
    if constexpr (VEC) {
        const int o = nvalid > 0 ? vo : BUF_OOB;
        if constexpr (N == 4) {
            const f32x4 a = buf_ld_f32x4(rs, o, soff, 0), b = buf_ld_f32x4(rs, o + 16, soff, 0);
            const f64x2 x = __builtin_bit_cast(f64x2, a), y = __builtin_bit_cast(f64x2, b);
            d[0] = x[0]; d[1] = x[1]; d[2] = y[0]; d[3] = y[1];
        } else if constexpr (N == 2) {
            const f64x2 x = __builtin_bit_cast(f64x2, buf_ld_f32x4(rs, o, soff, 0));
            d[0] = x[0]; d[1] = x[1];
        } else d[0] = __builtin_bit_cast(double, buf_ld_f32x2(rs, o, soff, 0));
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) d[e] = __builtin_bit_cast(double, buf_ld_f32x2(rs, e < nvalid ? vo + 8 * e : BUF_OOB, soff, 0));
    }
}
__device__ __forceinline__ int sgpr(long x) { return __builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ int clampi(long x, int hi) { return x < 0 ? 0 : (x > hi ? hi : (int)x); }

__device__ __forceinline__ double block_sum(double v, double* red) {       // fixed-order tree: deterministic
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}
__global__ __launch_bounds__(256) void f64_sum_final_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int p = threadIdx.x; p < nparts; p += 256) acc += part[p];
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) *out = s;
}

// `rows` rows of pitch ld (plus one more row of slack for the lane offsets inside a row) stay inside a descriptor's 31-bit offsets
inline bool buf_ok(long ld, long rows) { return (rows + 1) * ld * 8 < 0x7fffffffL; }

}  // namespace
