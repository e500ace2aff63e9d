// dnmf_bcd.h -- kernels of the accelerated block coordinate descent for Frobenius NMF (method = 'bcd'; reference
// dist_nmf.py:474-579 (2D), :940-1047 (1D), called from pyDNMF.py:151-152).  C ABI in csrc/dnmf_bcd.hip.
//
// One BCD iteration = the two projected-gradient steps (W, then H), the residual, then a Nesterov extrapolation or a restart.
// The big products (A H^T, W^T A, the Gram matrices, sum (A - W H)^2) are the existing entry points; the kernels here are what
// is new: the two gradient steps on the k x k Gram, the column scale of W, the decision and the extrapolate / restore pass.
// Every scalar of the method lives in a float64 STATE BLOCK in device memory (BcdSlot): the decision kernel writes it, every
// later pass reads it, so an iteration never goes back to the host and a fit of `itr` iterations is launches only.
#pragma once
#include "dnmf_common.h"

// slots of the float64 state block (the reference's Python scalars, FRO_BCD_update)
enum BcdSlot {
    BCD_XN = 0,        // Xnorm = sum A^2 (global)
    BCD_SW = 1,        // sum W0^2, sum H0^2 (global over the ranks that hold disjoint pieces): the initial scaling
    BCD_SH = 2,
    BCD_OBJ_OLD = 3,   // obj_old, t_old
    BCD_T_OLD = 4,
    BCD_LW = 5,        // HHTnorm (Lipschitz bound of the W step) and its previous value
    BCD_LW_OLD = 6,
    BCD_LH = 7,        // WTWnorm and its previous value
    BCD_LH_OLD = 8,
    BCD_ACC = 9,       // 1: the last iteration lowered the objective (extrapolate), 0: restart
    BCD_WW = 10,       // extrapolation weights of W and H
    BCD_WH = 11,
    BCD_OBJ = 12,      // the last iteration's objective and t (diagnostics)
    BCD_T = 13,
    BCD_NSLOTS = 16
};

constexpr int BCD_ROWS = 64;      // rows (W step) / columns (H step) of a workgroup: one per lane
constexpr int BCD_CG = 16;        // output columns of one wave
constexpr int BCD_LT = 32;        // contraction slab staged in LDS

// Batched launches (csrc/dnmf_common.h): every kernel below takes the BatchTab and moves its pointers into its problem first thing.
// The move is guarded by `bt.n` (0 outside a batched fit, where it would add zero anyway): the family search is some 25 scalar
// instructions per pointer on the CU's one scalar unit, and the element-wise kernels here run workgroups of a few hundred cycles --
// unguarded, bcd_extrapolate_kernel of a single 65536 x 16 fit went from 9.4 to 15.6 us (rocprofv3 --kernel-trace --stats).

// ---- the projected-gradient step (dist_nmf.py:999-1003 / :1011-1015, 2D :531-535 / :543-547):
//   W side (HS = false): W = max(0, Wm - (Wm G - P) / L),  Wm, P, W [R x k], G = H H^T,  L = ||G||_F
//   H side (HS = true):  H = max(0, Hm - (G Hm - P) / L),  Hm, P, H [k x R], G = W^T W
// "element (i, c)" is row i, column c of the m x k factor on the W side and column i, row c of the k x n factor on the H side, so
// both are out(i, c) = max(0, X(i, c) - (sum_l X(i, l) G'(l, c) - P(i, c)) / L) with G' = G (W side) or G^T (H side; the Gram is
// read as stored, no symmetry is assumed).  A workgroup = 64 lanes (i) x 4 waves, a wave = 16 consecutive c; the X(i, l) slab
// [64 x 32] is staged in LDS, G is read through the scalar cache (its address is wave-uniform).  The k x k product is done on
// the vector ALU: it moves k FMAs per element against the 3 floats per element (Wm, P, W) the step reads and writes, so the pass
// stays bound by those bytes at the ranks served here (profiles/bcd_*).  The division is IEEE (the reference divides).
// Column sums of the new W (W side, `part` != null): per workgroup, [gridDim.x][k] partials (summed by bcd_colsum_kernel).
template <bool HS>
__global__ __launch_bounds__(256) void bcd_pg_kernel(const float* __restrict__ Xm, long ldx, const float* __restrict__ P, long ldp,
                                                     const float* __restrict__ G, int ldg, long R, int k,
                                                     const double* __restrict__ st, int lslot, float* __restrict__ X, long ldo,
                                                     float* __restrict__ part, BatchTab bt) {
#pragma clang fp contract(off)
    if (bt.n) { REBASE(Xm); REBASE(P); REBASE(G); REBASE(st); REBASE(X); REBASE(part); }      // (part == null falls in no family: stays null)
    __shared__ float sx[BCD_ROWS][BCD_LT + 1];
    const int lane = threadIdx.x & 63;
    const int cg = __builtin_amdgcn_readfirstlane((int)blockIdx.y * 4 + (int)(threadIdx.x >> 6));
    const int c0 = cg * BCD_CG;
    const bool active = c0 < k;                                   // (wave-uniform)
    const long i0 = (long)blockIdx.x * BCD_ROWS;
    float acc[BCD_CG];
#pragma unroll
    for (int j = 0; j < BCD_CG; ++j) acc[j] = 0.f;
    for (int l0 = 0; l0 < k; l0 += BCD_LT) {
        for (int e = threadIdx.x; e < BCD_ROWS * BCD_LT; e += 256) {
            // W side: a row's 32 slab elements are contiguous; H side: 64 consecutive columns of one factor row
            const int i = HS ? (e & 63) : (e >> 5), l = HS ? (e >> 6) : (e & 31);
            const long gi = i0 + i;
            const int gl = l0 + l;
            float v = 0.f;
            if (gi < R && gl < k) v = HS ? Xm[(long)gl * ldx + gi] : Xm[gi * ldx + gl];
            sx[i][l] = v;
        }
        __syncthreads();
        if (active) {
            const int lend = min(BCD_LT, k - l0);
            for (int l = 0; l < lend; ++l) {
                const float a = sx[lane][l];
                // G' rows l0 + l < k <= KP and columns c0 + j < round_up(k, 16) <= KP: inside the KP x KP buffer
                if (HS) {
                    const float* g = G + (long)c0 * ldg + (l0 + l);
#pragma unroll
                    for (int j = 0; j < BCD_CG; ++j) acc[j] = __builtin_fmaf(a, g[(long)j * ldg], acc[j]);
                } else {
                    const float* g = G + (long)(l0 + l) * ldg + c0;
#pragma unroll
                    for (int j = 0; j < BCD_CG; ++j) acc[j] = __builtin_fmaf(a, g[j], acc[j]);
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    const long i = i0 + lane;
    const float L = (float)st[lslot];
    float cs[BCD_CG];
#pragma unroll
    for (int j = 0; j < BCD_CG; ++j) {
        const int c = c0 + j;
        float y = 0.f;
        if (i < R && c < k) {
            const float xm = HS ? Xm[(long)c * ldx + i] : Xm[i * ldx + c];
            const float p = HS ? P[(long)c * ldp + i] : P[i * ldp + c];
            const float gr = acc[j] - p;                          // GW = WmHHT - AHT
            y = xm - gr / L;                                      // Wm - GW / HHTnorm
            y = y < 0.f ? 0.f : y;                                // np.maximum(0, .): a NaN stays NaN
            if (HS) X[(long)c * ldo + i] = y;
            else X[i * ldo + c] = y;
        }
        cs[j] = y;
    }
    if (HS || part == nullptr) return;
    // column sums of this workgroup's rows (lanes past R contributed 0): a butterfly over the wave, lane 0 writes
#pragma unroll
    for (int j = 0; j < BCD_CG; ++j) {
        float v = cs[j];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        cs[j] = v;
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < BCD_CG; ++j)
            if (c0 + j < k) part[(long)blockIdx.x * k + c0 + j] = cs[j];
    }
}

// s[c] = sum over the nb workgroup partials of column c, in float64 and a fixed order (one workgroup per column)
__global__ __launch_bounds__(256) void bcd_colsum_kernel(const float* __restrict__ part, long nb, int k, float* __restrict__ s, BatchTab bt) {
    if (bt.n) { REBASE(part); REBASE(s); }
    __shared__ double red[256];
    const int c = blockIdx.x;
    double v = 0.0;
    for (long b = threadIdx.x; b < nb; b += 256) v += (double)part[b * k + c];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) s[c] = (float)red[0];
}

// W[i][c] /= s[c] (dist_nmf.py:1005-1009, 2D :537-540): no eps -- a zero column sum gives inf / NaN, as in the reference
__global__ __launch_bounds__(256) void bcd_scale_cols_kernel(float* __restrict__ W, long m, int k, long ldw, const float* __restrict__ s,
                                                             BatchTab bt) {
    if (bt.n) { REBASE(W); REBASE(s); }
    const long total = m * (long)k;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long i = e / k;
        const int c = (int)(e - i * k);
        W[i * ldw + c] = W[i * ldw + c] / s[c];
    }
}

// L_old = L; L = ||G[:k, :k]||_F (np.linalg.norm of the float32 Gram: the value is kept rounded to float32).  One workgroup.
__global__ __launch_bounds__(256) void bcd_lipschitz_kernel(const float* __restrict__ G, int ldg, int k, double* __restrict__ st, int slot,
                                                            BatchTab bt) {
    if (bt.n) { REBASE(G); REBASE(st); }
    __shared__ double red[256];
    double v = 0.0;
    for (int e = threadIdx.x; e < k * k; e += 256) {
        const double g = (double)G[(long)(e / k) * ldg + (e % k)];
        v += g * g;
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        st[slot + 1] = st[slot];
        st[slot] = (double)(float)sqrt(red[0]);
    }
}

// state init (initWandH, dist_nmf.py:947-965 / 2D :485-499): from sq = {sum A^2, sum W0^2, sum H0^2}
__global__ void bcd_state_init_kernel(double* __restrict__ st, const double* __restrict__ sq, BatchTab bt) {
    if (bt.n) { REBASE(st); REBASE(sq); }
    if (threadIdx.x != 0) return;
    for (int i = 0; i < BCD_NSLOTS; ++i) st[i] = 0.0;
    st[BCD_XN] = sq[0];
    st[BCD_SW] = sq[1];
    st[BCD_SH] = sq[2];
    st[BCD_OBJ_OLD] = 0.5 * sq[0];
    st[BCD_T_OLD] = 1.0;
    st[BCD_LW] = 1.0;
    st[BCD_LH] = 1.0;
}

// X_old = X_m = X0 / sqrt(sum X0^2) * sqrt(sqrt(Xnorm)), in float32 as numpy evaluates it (two roundings)
__global__ __launch_bounds__(256) void bcd_init_factor_kernel(const float* __restrict__ X0, long rows, long cols, long ld0, float* __restrict__ Xo,
                                                              long ldo, float* __restrict__ Xm, long ldm, const double* __restrict__ st, int slot, BatchTab bt) {
#pragma clang fp contract(off)
    if (bt.n) { REBASE(X0); REBASE(Xo); REBASE(Xm); REBASE(st); }
    const float a = (float)sqrt(st[slot]);
    const float b = (float)sqrt(sqrt(st[BCD_XN]));
    const long total = rows * cols;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / cols, c = e - r * cols;
        const float v = X0[r * ld0 + c] / a * b;
        Xo[r * ldo + c] = v;
        Xm[r * ldm + c] = v;
    }
}

// the decision (dist_nmf.py:1024-1047 / 2D :556-579): obj = sq / 2; t = (1 + sqrt(1 + 4 t_old^2)) / 2; obj >= obj_old: restart;
// else w = (t_old - 1) / t, ww = min(w, sqrt(Lw_old / Lw)), wh = min(w, sqrt(Lh_old / Lh)), t_old = t, obj_old = obj.  One lane.
__global__ void bcd_decide_kernel(double* __restrict__ st, const double* __restrict__ sq, BatchTab bt) {
#pragma clang fp contract(off)
    if (bt.n) { REBASE(st); REBASE(sq); }
    if (threadIdx.x != 0) return;
    const double obj = 0.5 * sq[0];
    const double t_old = st[BCD_T_OLD];
    const double t = (1.0 + sqrt(1.0 + 4.0 * t_old * t_old)) / 2.0;
    st[BCD_OBJ] = obj;
    st[BCD_T] = t;
    if (obj >= st[BCD_OBJ_OLD]) {
        st[BCD_ACC] = 0.0;
        return;
    }
    const double w = (t_old - 1.0) / t;
    // (the ratio of the float32 norms is a float32 in the reference; sqrt of it in float32)
    const float rw = sqrtf((float)st[BCD_LW_OLD] / (float)st[BCD_LW]);
    const float rh = sqrtf((float)st[BCD_LH_OLD] / (float)st[BCD_LH]);
    st[BCD_ACC] = 1.0;
    st[BCD_WW] = fmin(w, (double)rw);
    st[BCD_WH] = fmin(w, (double)rh);
    st[BCD_T_OLD] = t;
    st[BCD_OBJ_OLD] = obj;
}

// ---- the extrapolate / restore pass: up to four jobs in one launch (blockIdx.y = job), each reading the decision:
//   kind 0 (a factor; x = the iterate, o = the last accepted iterate, p = the extrapolation):
//       accept: p = x + w (x - o), o = x        restart: p = o
//   kind 1 (a product of H that a restart needs back; x = current, o = the copy kept for H_old):
//       accept: o = x                           restart: x = o
struct BcdJob { float* x; float* o; float* p; long rows, cols, ldx, ldo, ldp; int kind, wslot; };
struct BcdJobs { BcdJob j[4]; int n; };

// Batched: blockIdx.y stays the job, blockIdx.z is the problem; each job's pointers are moved into the problem here (they
// arrive inside the struct), as rebase_args does for NtArgs in dnmf_nt.h.
__global__ __launch_bounds__(256) void bcd_extrapolate_kernel(BcdJobs jobs, const double* __restrict__ st, BatchTab bt) {
#pragma clang fp contract(off)
    if ((int)blockIdx.y >= jobs.n) return;
    if (bt.n) { REBASE(st); }
    BcdJob J = jobs.j[blockIdx.y];
    if (bt.n) { rebase(J.x, bt); rebase(J.o, bt); rebase(J.p, bt); }             // (p == null in the kind-1 jobs: no family, stays null)
    const bool acc = st[BCD_ACC] != 0.0;
    const float w = J.kind == 0 ? (float)st[J.wslot] : 0.f;
    const long total = J.rows * J.cols;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / J.cols, c = e - r * J.cols;
        float* xp = J.x + r * J.ldx + c;
        float* op = J.o + r * J.ldo + c;
        if (J.kind == 0) {
            float* pp = J.p + r * J.ldp + c;
            if (acc) {
                const float x = *xp;
                const float d = x - *op;
                *pp = x + w * d;
                *op = x;
            } else {
                *pp = *op;
            }
        } else {
            if (acc) *op = *xp;
            else *xp = *op;
        }
    }
}
