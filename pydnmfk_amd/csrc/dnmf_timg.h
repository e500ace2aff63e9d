// dnmf_timg.h -- the MU/Frobenius W phase from a TRANSPOSED IMAGE of A: At[c][i] = A[i][c] (n x m, built once per fit).
// Part of libdnmf_hip.so (csrc/dnmf_timg.hip plans and launches these kernels; DESIGN.md section 2 "the image").
//
// Why: A H^T in the NT form (dnmf_nt.h) has to carry every byte of A through VGPR -> LDS -> VGPR, because the MFMA wants the
// rows of A across lanes; the TN form (dnmf_tn.h) feeds its streamed operand from global memory straight into the MFMA and
// holds a higher clock.  With the contraction index c down the ROWS of the image, A H^T is a TN product: C[j][i] = sum_c
// Ht[c][j] At[c][i].  aht_t_kernel is tn_mainloop's software pipeline on (Ht, At) -- no LDS, both operands through MUBUF
// descriptors, two register batches, nothing conditional around a load -- followed by nt_kernel<.., NT_FUSED_W>'s epilogue.
//
// BIT-EQUAL to nt_kernel by construction (tests/test_gpu_wimage.py compares with torch.equal): every output element (i, j)
// runs the SAME chain of v_mfma_f32_32x32x2_f32 steps as in nt_kernel -- the k-tiles t = (tt + kshift) mod nk in the rotated
// order of the 128-row block the row belongs to (kshift = (block * 37) mod nk, block = i / 128 = the blockIdx.x nt_kernel
// gives that row), inside a tile the fragment groups s = 0..3 and elements e = 0..3, one MFMA adding the pair c = 32 t + 8 s + e
// (lane half 0) and c + 4 (lane half 1), accumulators from zero.  The MFMA is an fmaf chain per output element (DESIGN.md
// section 3) and a product does not depend on the order of its factors, so it does not matter that A now sits on the B side.
// The second product den = W G and the update follow nt_kernel's epilogue the same way: tiles 0, 1 unrotated, pairs (l, l + 4),
// zero beyond k, then w * (ah / (den + eps)) as written there.
//
// A wave owns the 128 rows of one NT row block and all 64 columns j (four waves to a workgroup, or one when there are at most
// 1024 blocks: csrc/dnmf_timg.hip): acc[ke][ne][reg] = AH[i = row0 + 4 li + ne][j = 2 crow(reg, h)
// + ke].  Descriptor windows: a row of At is m floats, so one 2 GiB MUBUF window covers only a few thousand (or a few dozen)
// of its n rows; the descriptor of At is rebased -- wave-uniform, scalar arithmetic only -- on windows of R = 2^rshift rows
// with (R + 8) * ldat * 4 < 2^31 (the host computes rshift; every 8-row batch lies inside one window).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): see the table in the header comment of
// csrc/dnmf_timg.hip.
#pragma once
#include "dnmf_common.h"

namespace {

// ----------------------------------------------------------------------------------------------- transpose through LDS
// out[c][i] = in[i][c] for i < rows, c < cols.  64 x 64 tiles, 256 threads: 16-byte loads along c (256 B per row visit),
// scalar LDS writes and reads on a 65-float pitch (both conflict free), 16-byte stores along i.  rows % 4 == 0, cols % 4 == 0,
// ldi % 4 == 0, ldo % 4 == 0, both bases 16-byte aligned (host checked).  Serves the image (A -> At, once per fit) and
// Ht = H^T (k x n -> n x k, once per step).
__global__ __launch_bounds__(256) void transpose_image_kernel(const float* __restrict__ in, long rows, long cols, long ldi,
                                                              float* __restrict__ out, long ldo, long tiles_c) {
    __shared__ float tile[64][65];
    const long tr = (long)blockIdx.x / tiles_c, tc = (long)blockIdx.x % tiles_c;
    const long i0 = tr * 64, c0 = tc * 64;
    const int t = threadIdx.x, q = t & 15, r = t >> 4;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const long i = i0 + r + 16 * it, c = c0 + 4 * q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (i < rows && c < cols) v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(in + i * ldi + c));
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[r + 16 * it][4 * q + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int cl = r + 16 * it;
        const long c = c0 + cl, i = i0 + 4 * q;
        if (c < cols && i < rows) {
            const f32x4 v = {tile[4 * q][cl], tile[4 * q + 1][cl], tile[4 * q + 2][cl], tile[4 * q + 3][cl]};
            *reinterpret_cast<f32x4*>(out + c * ldo + i) = v;
        }
    }
}

// ----------------------------------------------------------------------------------------------- A H^T + W update, TN form
struct TimgArgs {
    const float* At; long ldat;          // image [n x m]
    const float* Ht; int ldht;           // H^T   [n x k]
    long m; int nk; int k;               // nk = n / 32 k-tiles
    int rshift;                          // descriptor window of At: 2^rshift rows
    float* W; long ldw; const float* G;  // G: [64 x 64], ld 64 (read as nt_kernel reads it: G[j][l], zero beyond k)
    float eps;
};

template <int KT>
__global__ __launch_bounds__(256, 2) void aht_t_kernel(TimgArgs p) {
    static_assert(KT == 2, "instantiated for 32 < k <= 64");
    constexpr int NT = 4, U = 4;         // columns of At per lane; MFMA steps (row pairs e) per register batch = one fragment group s
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long gw = (long)blockIdx.x * (blockDim.x >> 6) + wid;   // = the blockIdx.x of nt_kernel for these 128 rows
    const long row0 = gw * 128;
    if (row0 >= p.m) return;
    const int nk = p.nk, nb = 4 * nk;                    // batches of 8 image rows: (tile tt, group s) -> b = 4 tt + s
    const int bshift = 4 * (int)(((unsigned)gw * 37u) % (unsigned)nk);

    f32x16 acc[KT][NT];
#pragma unroll
    for (int ke = 0; ke < KT; ++ke)
#pragma unroll
        for (int ne = 0; ne < NT; ++ne)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ke][ne][r] = 0.f;

    // lanes beyond k / beyond m read a clamped valid column (tn_mainloop): they feed outputs that are never stored
    int xc = KT * li;
    xc = xc < p.k ? xc : p.k - KT;
    long yc = row0 + NT * li;
    yc = yc < p.m ? yc : p.m - NT;
    const int ldat4 = (int)(p.ldat * 4), ldht4 = p.ldht * 4;
    int xb[U], yb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {        // step e = u of a group: lane half h reads image row 8 s + e + 4 h of the tile
        xb[u] = (u + 4 * h) * ldht4 + xc * 4;
        yb[u] = (u + 4 * h) * ldat4 + (int)(yc * 4);
    }
    const i32x4 rsx = buf_rsrc(p.Ht);
    const long win_bytes = ((long)ldat4) << p.rshift;
    const int rmask = (1 << p.rshift) - 1;
    float a0[U][KT], a1[U][KT], q0[U][NT], q1[U][NT];
    // batch b of this wave's order -> its first image row; the descriptor of At at that row's window and the offset inside
    auto rot = [&](int b) {
        int x = b + bshift;
        x = x >= nb ? x - nb : x;
        return x * 8;
    };
    auto ldb = [&](float (&a)[U][KT], float (&q)[U][NT], int u, i32x4 rsy, int sx, int sy) {
        buf_load<KT, 0>(a[u], rsx, xb[u], sx);
        buf_load<NT, 2>(q[u], rsy, yb[u], sy);
    };
    auto window = [&](int row, int& sy) {
        sy = (row & rmask) * ldat4;
        return buf_rsrc(reinterpret_cast<const char*>(p.At) + (long)(row >> p.rshift) * win_bytes);
    };
    {
        const int r0 = rot(0);
        int sy;
        const i32x4 rsy = window(r0, sy);
#pragma unroll
        for (int u = 0; u < U; ++u) ldb(a0, q0, u, rsy, r0 * ldht4, sy);
    }
    for (int b = 0; b < nb; b += 2) {                    // nb is even; the prefetch past the end re-reads the last batch (unused)
        const int r1 = rot(b + 1);
        const int r2 = rot(b + 2 < nb ? b + 2 : nb - 1);
        int sy1, sy2;
        const i32x4 rs1 = window(r1, sy1), rs2 = window(r2, sy2);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ldb(a1, q1, u, rs1, r1 * ldht4, sy1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ke = 0; ke < KT; ++ke)
#pragma unroll
                for (int ne = 0; ne < NT; ++ne) acc[ke][ne] = MFMA32(a0[u][ke], q0[u][ne], acc[ke][ne]);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ldb(a0, q0, u, rs2, r2 * ldht4, sy2);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ke = 0; ke < KT; ++ke)
#pragma unroll
                for (int ne = 0; ne < NT; ++ne) acc[ke][ne] = MFMA32(a1[u][ke], q1[u][ne], acc[ke][ne]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // epilogue = nt_kernel<.., NT_FUSED_W>: den = W[rows] . G over l (tiles 0, 1, groups s, elements e, pairs (l, l + 4); zero
    // beyond k), then W = w * (ah / (den + eps)).  Two halves of the wave's rows (ne in {0, 1}, then {2, 3}) bound the registers.
    const i32x4 rsw = buf_rsrc(p.W + row0 * p.ldw), rsg = buf_rsrc(p.G);
    const int ldw4 = (int)(p.ldw * 4);
    const int wrow = (int)(yc - row0);                   // this lane's first row inside the wave's block (clamped)
    const bool live = row0 + NT * li < p.m;
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
        f32x16 den[KT][2];
#pragma unroll
        for (int ke = 0; ke < KT; ++ke)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) den[ke][q][r] = 0.f;
#pragma unroll
        for (int g8 = 0; g8 < 8; ++g8) {                 // g8 = 4 t + s: l0 = 32 t + 8 s + 4 h
            const int l0 = 8 * g8 + 4 * h;
            const int lo = l0 < p.k ? l0 * 4 : BUF_OOB;  // beyond k: the load returns 0 (k % 4 == 0: a group is in or out)
            f32x4 g[KT], w[2];
#pragma unroll
            for (int ke = 0; ke < KT; ++ke) g[ke] = buf_ld_f32x4(rsg, lo == BUF_OOB ? BUF_OOB : (KT * li + ke) * 256 + lo, 0, 0);
#pragma unroll
            for (int q = 0; q < 2; ++q) w[q] = buf_ld_f32x4(rsw, lo == BUF_OOB ? BUF_OOB : (wrow + 2 * nh + q) * ldw4 + lo, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int ke = 0; ke < KT; ++ke)
#pragma unroll
                    for (int q = 0; q < 2; ++q) den[ke][q] = MFMA32(g[ke][e], w[q][e], den[ke][q]);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ne = 2 * nh + q;
            const int wo = (wrow + ne) * ldw4;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = KT * crow(r, h);
                if (live && j < p.k) {                   // k is even: the pair (j, j + 1) is in or out
                    const f32x2 w2 = buf_ld_f32x2(rsw, wo + j * 4, 0, 0);
                    f32x2 o;
                    {
                        const float ah = acc[0][ne][r];
                        const float qq = ah / (den[0][q][r] + p.eps);   // dist_nmf.py:731-732
                        o[0] = w2[0] * qq;
                    }
                    {
                        const float ah = acc[1][ne][r];
                        const float qq = ah / (den[1][q][r] + p.eps);
                        o[1] = w2[1] * qq;
                    }
                    buf_st_f32x2(o, rsw, wo + j * 4, 0, 0);
                }
            }
        }
    }
}

}  // namespace
