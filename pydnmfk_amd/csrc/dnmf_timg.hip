// dnmf_timg.hip -- the transposed image of A and the W phase that streams it (kernels: csrc/dnmf_timg.h).
//
// dnmf_wimage_build writes At[c][i] = A[i][c] once per fit; dnmf_wimage_bind names it to the calling thread; from then on
// aht_update_w_impl<float> (csrc/dnmf.hip -- the one place that asks) runs aht_t_kernel instead of nt_kernel whenever
// wimage_plan() says so.  Results are bit-equal either way (csrc/dnmf_timg.h), so which path ran never shows in the numbers.
//
// The image buffer is [At: n x ldat floats | 256-byte aligned: Ht = H^T, n x 64 floats]; Ht is rewritten before every W phase
// (2 MB at n = 8192) by the same transpose kernel.  dnmf_wimage_bytes covers both.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; python -m pydnmfk_amd.build --report):
//   aht_t_kernel<2>            vgpr 238  agpr 0  spill 0  scratch 0  waves/SIMD 2  lds 0
//   transpose_image_kernel     vgpr  15  agpr 0  spill 0  scratch 0  waves/SIMD 8  lds 16640
// The main loop of aht_t_kernel holds no vector ALU instruction: 8 buffer loads and 32 MFMAs per batch, every address
// computed on the scalar unit (checked in the ISA: s_mul / s_and / s_ashr between the MFMA groups, counted vmcnt waits).
#include "dnmf_common.h"
#include "dnmf_host.h"
#include "dnmf_timg.h"

namespace {

struct WimgBind { const float* A; long m, n, lda; float* At; long ldat; };
WimgBind* wimage_bound() {
    static thread_local WimgBind b = {nullptr, 0, 0, 0, nullptr, 0};
    return &b;
}
int g_wimage_mode = 1;                     // 0 off, 1 auto, 2 forced (dnmf_set_wimage)
int* wimage_launches() {                   // W phases this thread has run from an image (dnmf_wimage_plan reports it: tests)
    static thread_local int count = 0;
    return &count;
}

inline size_t wimage_at_bytes(long n, long ldat) { return align256((size_t)n * ldat * sizeof(float)); }

// In auto mode the image is taken where a sweep measured a gain (profiles/r07_wimage_sweep.md: whole steps, image off against
// forced, k = 64, 24 shapes from 2^27 to 2^31 elements): a wave owns a whole 128-row block over ALL of n, so the launch cannot be cut
// finer than blocks, and it keeps the chip evenly busy only when the blocks come in whole half-rounds of 1024 waves (one per
// SIMD).  Every shape with m a multiple of 131072 gained 1.8-3.2 % per step (8 % at 131072 x 1024); every other one LOST --
// 6 % at 768 blocks, 12 % at 1536, 16 % at 2049, 23-51 % below 1024 -- where nt_kernel's 128-row workgroups still spread evenly.
// Nothing below 2^27 elements was measured.
inline bool image_pays(long m, long n) { return m % (128L * 1024) == 0 && (double)m * (double)n >= (double)(1L << 27); }

enum {
    WIMG_TAKEN = 0,
    WIMG_OFF = 1,            // dnmf_set_wimage(0)
    WIMG_SHAPE = 2,          // n % 32 != 0 or m % 4 != 0
    WIMG_A_ALIGN = 3,        // A, At or H not 16-byte aligned / lda, ldh not multiples of 4
    WIMG_W_ALIGN = 4,        // W not 16-byte aligned / ldw % 4 != 0 / k % 4 != 0 / 128 rows of W beyond one 2 GiB window
    WIMG_RANK = 5,           // rank outside 32 < k <= 64
    WIMG_SMALL = 6,          // auto mode: image_pays says no (row count not a multiple of 131072, or below 2^27 elements)
    WIMG_WINDOW = 7,         // a row of the image too long for a 16-row window, or Ht beyond one window
};

inline int wimage_waves_per_wg(long m) { return cdiv(m, 128) > 1024 ? 4 : 1; }

struct WimgPlan { int taken, reason, R, grid, kt, rshift; };

// THE conditions: the plan query and the launch both come here.
WimgPlan wimage_plan(long m, long n, int k, long lda, bool a_aligned, bool w_aligned, int mode) {
    WimgPlan p = {0, WIMG_TAKEN, 0, 0, 0, 0};
    const long ldat = round_up(m, 4);
    auto no = [&](int why) { p.reason = why; return p; };
    if (mode == 0) return no(WIMG_OFF);
    if (m < 4 || n < 32 || n % 32 != 0 || m % 4 != 0) return no(WIMG_SHAPE);
    if (!a_aligned || lda % 4 != 0) return no(WIMG_A_ALIGN);
    if (!(k > 32 && k <= 64)) return no(WIMG_RANK);
    if (!w_aligned || k % 4 != 0) return no(WIMG_W_ALIGN);
    // windows of R = 2^rshift image rows with (R + 8) * ldat * 4 < 2^31, R >= 8; Ht (n x k) inside one window
    int rs = 3;
    while (rs < 20 && ((1L << (rs + 1)) + 8) * ldat * 4 < 0x7fffffffL) ++rs;
    if (((1L << rs) + 8) * ldat * 4 >= 0x7fffffffL || (n + 8) * (long)k * 4 >= 0x7fffffffL) return no(WIMG_WINDOW);
    if (mode == 1 && !image_pays(m, n)) return no(WIMG_SMALL);
    p.taken = 1;
    p.rshift = rs;
    p.R = 1 << rs;
    p.kt = 2;
    // one wave per 128-row block.  From 1025 waves on they go four to a workgroup (2048 waves = two workgroups on every CU: one
    // resident round); up to 1024 waves a workgroup is ONE wave, so that the dispatcher spreads them over all the CUs instead
    // of filling a quarter of the chip four waves deep.
    p.grid = (int)cdiv(cdiv(m, 128), wimage_waves_per_wg(m));
    return p;
}

int launch_transpose(const float* in, long rows, long cols, long ldi, float* out, long ldo, hipStream_t st) {
    const long tiles_c = cdiv(cols, 64), tiles = cdiv(rows, 64) * tiles_c;
    if (tiles >= (1L << 31)) return fail(DNMF_EINVAL, "wimage: %ld x %ld has too many tiles", rows, cols);
    hipLaunchKernelGGL(transpose_image_kernel, dim3((unsigned)tiles), dim3(256), 0, st, in, rows, cols, ldi, out, ldo, tiles_c);
    return check_launch("transpose_image");
}

}  // namespace

// csrc/dnmf.hip (aht_update_w_impl<float>): 1 = not applicable, run the NT kernel; otherwise the launch status
__attribute__((visibility("hidden"))) int dnmf_wimage_try_(const float* A, long m, long n, long lda, const float* H, int k, long ldh,
                                                           const float* G, float* W, long ldw, float eps, void* stream);
int dnmf_wimage_try_(const float* A, long m, long n, long lda, const float* H, int k, long ldh, const float* G, float* W, long ldw,
                     float eps, void* stream) {
    const WimgBind* b = wimage_bound();
    if (!b->At || b->A != A || b->m != m || b->n != n || b->lda != lda || dnmf_batch_()->B != 1) return 1;
    const bool a_ok = aligned16(A) && aligned16(b->At) && aligned16(H) && ldh % 4 == 0 && b->ldat % 4 == 0 && b->ldat >= m &&
                      b->ldat == round_up(m, 4);
    const bool w_ok = aligned16(W) && ldw % 4 == 0 && aligned16(G) && (128 * ldw + 64) * 4 < 0x7fffffffL;
    const WimgPlan p = wimage_plan(m, n, k, lda, a_ok, w_ok, g_wimage_mode);
    if (!p.taken) return 1;
    hipStream_t st = S(stream);
    float* Ht = (float*)((char*)b->At + wimage_at_bytes(n, b->ldat));
    if (int rc = launch_transpose(H, k, n, ldh, Ht, k, st)) return rc;
    TimgArgs a{};
    a.At = b->At; a.ldat = b->ldat; a.Ht = Ht; a.ldht = k;
    a.m = m; a.nk = (int)(n / 32); a.k = k; a.rshift = p.rshift;
    a.W = W; a.ldw = ldw; a.G = G; a.eps = eps;
    hipLaunchKernelGGL(aht_t_kernel<2>, dim3((unsigned)p.grid), dim3(64 * wimage_waves_per_wg(m)), 0, st, a);
    ++*wimage_launches();
    return check_launch("aht_t_kernel");
}

extern "C" {

size_t dnmf_wimage_bytes(long m, long n) {
    if (m < 1 || n < 1) return 0;
    return wimage_at_bytes(n, round_up(m, 4)) + align256((size_t)n * 64 * sizeof(float));
}

int dnmf_wimage_build(const float* A, long m, long n, long lda, float* At, long ldat, void* stream) {
    REQUIRE(A && At && m >= 1 && n >= 1 && lda >= n && ldat >= m, "wimage_build: bad arguments");
    REQUIRE(m % 4 == 0 && n % 4 == 0 && lda % 4 == 0 && ldat % 4 == 0 && aligned16(A) && aligned16(At),
            "wimage_build: needs m, n, lda, ldat multiples of 4 and 16-byte aligned A and At (m=%ld n=%ld lda=%ld ldat=%ld)", m, n, lda, ldat);
    return launch_transpose(A, m, n, lda, At, ldat, S(stream));
}

int dnmf_wimage_bind(const float* A, long m, long n, long lda, float* At, long ldat) {
    REQUIRE(A && At && m >= 1 && n >= 1 && lda >= n && ldat == round_up(m, 4), "wimage_bind: bad arguments (ldat must be m rounded up to 4)");
    *wimage_bound() = WimgBind{A, m, n, lda, At, ldat};
    return DNMF_OK;
}

void dnmf_wimage_unbind(void) { *wimage_bound() = WimgBind{nullptr, 0, 0, 0, nullptr, 0}; }

int dnmf_set_wimage(int mode) {
    const int was = g_wimage_mode;
    if (mode >= 0 && mode <= 2) g_wimage_mode = mode;
    return was;
}

int dnmf_wimage_plan(long m, long n, int k, long lda, int a_aligned, int w_aligned, int out[6]) {
    REQUIRE(out, "wimage_plan: null output");
    const WimgPlan p = wimage_plan(m, n, k, lda, a_aligned != 0, w_aligned != 0, g_wimage_mode);
    out[0] = p.taken; out[1] = p.reason; out[2] = p.R; out[3] = p.grid; out[4] = p.kt; out[5] = *wimage_launches();
    return DNMF_OK;
}

}  // extern "C"
