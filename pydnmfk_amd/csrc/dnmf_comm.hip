// dnmf_comm.hip -- the grid exchanges INSIDE the library: RCCL communicators for the p_r x p_c grid (dist_comm.py:16-56), the direct
// two-shot allreduce over IPC peer buffers, the collectives over the groups of the grid and the cross-rank HALS W sweep -- what the
// library-sequenced steps of csrc/dnmf_grid.hip enqueue between their kernels (csrc/dnmf_comm.h) -- and the dnmf_comm_* entry points.
//
// RCCL is bound at run time (dlopen): the library loads and every compute entry point works on a host without RCCL; the
// first dnmf_comm_* call looks for an RCCL that is ALREADY in the process (PyTorch's own copy: two RCCL / HIP runtime
// instances in one process do not share device state) and only then loads librccl.so.1 by name.
#include <dlfcn.h>

#include "dnmf_comm.h"

// csrc/dnmf_hals.hip: the persistent W sweep with the column norms summed over the ranks of `pe` (nullptr: applicability check only)
__attribute__((visibility("hidden"))) int dnmf_hals_sweep_w_peers_(float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G,
                                                                   float eps, void* ws, size_t ws_bytes, const HalsPeers* pe, int* nwg,
                                                                   void* stream);

namespace {

struct Rccl {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommSplit)(ncclComm_t, int, int, ncclComm_t*, ncclConfig_t*) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetVersion)(int*) = nullptr;                  // optional
    const char* origin = "";
};

Rccl* rccl() {
    // bound once (function-local static: initialisation is serialised by the language, callers on any thread see the result)
    static Rccl* const inst = []() -> Rccl* {
        static Rccl r;
        const char* resident[] = {"librccl.so", "librccl.so.1"};
        for (const char* n : resident)
            if (!r.handle && (r.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) r.origin = "already in the process";
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names)
            if (!r.handle && (r.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) r.origin = n;
        if (!r.handle) return nullptr;
#define BIND(field, sym) \
        r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.handle, sym)); \
        if (!r.field) return nullptr;
        BIND(GetUniqueId, "ncclGetUniqueId") BIND(CommInitRank, "ncclCommInitRank") BIND(CommDestroy, "ncclCommDestroy")
        BIND(AllReduce, "ncclAllReduce") BIND(AllGather, "ncclAllGather")
        BIND(ReduceScatter, "ncclReduceScatter") BIND(GroupStart, "ncclGroupStart") BIND(GroupEnd, "ncclGroupEnd")
        BIND(GetErrorString, "ncclGetErrorString")
#undef BIND
        // optional symbols (round 4): ncclCommSplit is needed by 2D grids only -- a 1D grid must not lose the in-library exchange
        // to an RCCL without it; ncclGetVersion feeds dnmf_comm_rccl_version
        r.CommSplit = reinterpret_cast<decltype(r.CommSplit)>(dlsym(r.handle, "ncclCommSplit"));
        r.GetVersion = reinterpret_cast<decltype(r.GetVersion)>(dlsym(r.handle, "ncclGetVersion"));
        return &r;
    }();
    return inst;
}

int nccl_fail(const char* what, ncclResult_t e) {
    Rccl* r = rccl();
    return fail(DNMF_ECOMM, "%s: RCCL error %d (%s)", what, (int)e, r ? r->GetErrorString(e) : "?");
}
#define NCCL_OK(call, what) do { ncclResult_t e_ = (call); if (e_ != ncclSuccess) return nccl_fail(what, e_); } while (0)

// The three collectives of the path over a GROUP of the grid (G_WORLD / G_ROW / G_COL, csrc/dnmf_comm.h).  A group of one member is
// the identity (unless `always` asks a one-rank communicator to issue its calls anyway); a hosted communicator hands every call to
// the host's function.
enum { OP_ALLREDUCE = DNMF_ALLREDUCE, OP_ALLGATHER = DNMF_ALLGATHER, OP_REDUCE_SCATTER = DNMF_REDUCE_SCATTER };

int group_size(const dnmf_comm* cm, int g) { return g == G_WORLD ? cm->nranks : g == G_ROW ? cm->p_r : cm->p_c; }
ncclComm_t group_comm(const dnmf_comm* cm, int g) {
    if (g == G_WORLD) return cm->world;
    if (g == G_ROW) return cm->row ? cm->row : (cm->p_c == 1 ? cm->world : nullptr);   // 1D grids: the long axis IS the world
    return cm->col ? cm->col : (cm->p_r == 1 ? cm->world : nullptr);
}
// 0: run the collective on *out; 1: identity (nothing to exchange); < 0: error
int resolve(dnmf_comm* cm, int g, ncclComm_t* out, const char* what) {
    if (cm->null_exchange) return 1;
    if (group_size(cm, g) == 1 && (!cm->always || cm->hook)) return 1;   // (a hosted communicator never sees a group of one)
    if (cm->hook) { *out = nullptr; return 0; }
    if (cm->emulated) { *out = cm->world; return 0; }            // every group's call is issued for real, on the one-rank communicator
    ncclComm_t c = group_comm(cm, g);
    if (!c && group_size(cm, g) == 1) c = cm->world;              // `always` on a one-rank communicator
    if (!c) return fail(DNMF_EINVAL, "%s: sub-communicator %d missing", what, g);
    *out = c;
    return 0;
}

// ---------------------------------------------------------------------------------------------- direct two-shot allreduce
// SURVEY section 5 / VERDICT r03: the packed [W^T A | W^T W] message of config 3 is 2 MiB -- latency-bound for a ring over
// point-to-point xGMI links.  The direct form reads PEER memory instead: every rank owns a region of uncached device memory
// exported with hipIpcGetMemHandle and mapped by all the others;
//   region = [flag1[P] | flag2[P] | status]  [send, parity 0 | send, parity 1]  [reduced, parity 0 | reduced, parity 1]  [HALS slot slab x 2]
// and one allreduce is, on the caller's stream:  copy the message into send[parity]  ->  signal + wait (everybody has written)  ->
// REDUCE: rank r sums chunk r of all P send buffers in rank order (one owner per element: every rank ends with the same bits,
// whatever the timing) into reduced[parity]  ->  signal + wait  ->  GATHER every chunk from its owner.  Four small launches; the
// stream order between them is the grid-wide barrier, so nothing needs to be co-resident, and each wait is ONE workgroup
// spinning on flags the peers store with system scope.  Alternating parity makes a trailing barrier unnecessary: a rank reaches
// call s + 2 only after every peer has signalled in call s + 1, i.e. has finished reading the buffers of call s.
// Remote data are read with system-scope loads (no stale lines from the previous step: the same addresses carry new data every
// call).  A wait that sees no progress for the configured time (30 s by default) sets the region's status word (dnmf_comm_direct_status) and gives up.
// NOT measured on more than one GPU (this pool has none): bench.py treats it as a third arm of its warm-up A/B and only after
// its result has matched RCCL's on the warm-up step.
constexpr unsigned long long DIRECT_MAGIC = 0x444e4d4644495231ull;      // "DNMFDIR1"
constexpr size_t DIRECT_HDR = 8192;       // flag1 @0, flag2 @1024, status @2048, small-message flags @3072, small-message slots @4096
// behind the four message buffers: the two slot slabs (by sweep parity) of the cross-rank persistent HALS W sweep, 1 MiB each
constexpr size_t HALS_SLAB_BYTES = (size_t)DNMF_TUNED_MAX_K * HALS_MAX_WG * sizeof(unsigned long long);
inline size_t direct_hals_off(size_t cap) { return (DIRECT_HDR + 4 * cap * sizeof(float) + 255) & ~size_t(255); }
struct DirectArgs {
    char* peer[DNMF_DIRECT_MAX_RANKS];
    int P, rank, par;
    size_t cap;                      // floats per send / reduced buffer
    size_t count, chunk;             // message length, floats per owner
    unsigned long long seq;
    unsigned long long patience;     // ticks of the 100 MHz wall clock a wait may see no progress (dnmf_comm_set_direct_timeout)
};
__device__ __forceinline__ unsigned long long* d_flags(char* region, int which) { return reinterpret_cast<unsigned long long*>(region + 1024 * which); }
__device__ __forceinline__ float* d_send(char* region, size_t cap, int par) { return reinterpret_cast<float*>(region + DIRECT_HDR) + (size_t)par * cap; }
__device__ __forceinline__ float* d_red(char* region, size_t cap, int par) { return reinterpret_cast<float*>(region + DIRECT_HDR) + (size_t)(2 + par) * cap; }

__global__ __launch_bounds__(64) void direct_signal_wait_kernel(DirectArgs a, int which) {
    const int q = threadIdx.x;
    __threadfence_system();                                        // (everything this stream wrote before is visible first)
    if (q < a.P) __hip_atomic_store(d_flags(a.peer[q], which) + a.rank, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (q < a.P) {
        const unsigned long long* mine = d_flags(a.peer[a.rank], which) + q;
        const unsigned long long t0 = wall_clock64();             // (100 MHz, independent of the shader clock)
        while (__hip_atomic_load(mine, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < a.seq) {
            __builtin_amdgcn_s_sleep(8);
            if (wall_clock64() - t0 > a.patience) {                // a peer is gone -- say so instead of hanging the GPU
                __hip_atomic_store(d_flags(a.peer[a.rank], 2), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
        }
    }
    __threadfence_system();
}

__device__ __forceinline__ f32x2 load_sys2(const float* p) {
    const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return f32x2{__uint_as_float((unsigned)(v & 0xffffffffu)), __uint_as_float((unsigned)(v >> 32))};
}

// this rank's chunk of the sum, in rank order, into its reduced buffer (pairs of floats: count and chunk are even)
__global__ __launch_bounds__(256) void direct_reduce_kernel(DirectArgs a) {
    const size_t beg = (size_t)a.rank * a.chunk, end = std::min(beg + a.chunk, a.count);
    float* red = d_red(a.peer[a.rank], a.cap, a.par);
    for (size_t i = beg + 2 * ((size_t)blockIdx.x * 256 + threadIdx.x); i < end; i += 2 * (size_t)gridDim.x * 256) {
        f32x2 s = {0.f, 0.f};
        for (int q = 0; q < a.P; ++q) {
            const f32x2 v = load_sys2(d_send(a.peer[q], a.cap, a.par) + i);
            s[0] += v[0]; s[1] += v[1];
        }
        *reinterpret_cast<f32x2*>(red + i) = s;
    }
}

__global__ __launch_bounds__(256) void direct_gather_kernel(DirectArgs a, float* __restrict__ out) {
    for (size_t i = 2 * ((size_t)blockIdx.x * 256 + threadIdx.x); i < a.count; i += 2 * (size_t)gridDim.x * 256) {
        const int owner = (int)(i / a.chunk);
        const f32x2 v = load_sys2(d_red(a.peer[owner], a.cap, a.par) + i);
        *reinterpret_cast<f32x2*>(out + i) = v;
    }
}

int direct_allreduce(dnmf_comm* cm, float* buf, size_t count, hipStream_t st) {
    REQUIRE(cm->direct_peer[cm->rank] && count <= cm->direct_cap, "allreduce(direct): not set up for %zu floats", count);
    REQUIRE(count % 2 == 0 && ((uintptr_t)buf & 7) == 0, "allreduce(direct): the message must be an even number of floats, 8-byte aligned");
    DirectArgs a{};
    for (int q = 0; q < cm->nranks; ++q) a.peer[q] = cm->direct_peer[q];
    a.P = cm->nranks; a.rank = cm->rank; a.cap = cm->direct_cap; a.count = count;
    a.chunk = (cdiv((long)count, cm->nranks) + 1) / 2 * 2;
    a.seq = ++cm->direct_seq;
    a.par = (int)(a.seq & 1);
    a.patience = cm->direct_patience;
    float* send = reinterpret_cast<float*>(cm->direct_peer[cm->rank] + DIRECT_HDR) + (size_t)a.par * a.cap;
    HIP_OK(hipMemcpyAsync(send, buf, count * sizeof(float), hipMemcpyDeviceToDevice, st), "allreduce(direct): copy");
    const unsigned g1 = (unsigned)std::max<long>(1, std::min<long>(64, cdiv((long)a.chunk, 512)));
    const unsigned g2 = (unsigned)std::max<long>(1, std::min<long>(256, cdiv((long)count, 512)));
    hipLaunchKernelGGL(direct_signal_wait_kernel, dim3(1), dim3(64), 0, st, a, 0);
    hipLaunchKernelGGL(direct_reduce_kernel, dim3(g1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(direct_signal_wait_kernel, dim3(1), dim3(64), 0, st, a, 1);
    hipLaunchKernelGGL(direct_gather_kernel, dim3(g2), dim3(256), 0, st, a, buf);
    return check_launch("allreduce(direct)");
}

// ONE-shot form for a few doubles (the column norms of the HALS W sweep, utils.py:388-391: k DEPENDENT 8-byte allreduces per
// iteration when W's rows are spread over ranks -- pure latency): a single launch of one wave.  Thread q pushes this rank's
// values into slot [parity][rank] of peer q's region and then raises its flag there; when all P flags of the own region have
// arrived the values are summed in rank order -- identical bits everywhere.  Same parity argument as above.
constexpr int DIRECT_SMALL_MAX = 8;
__global__ __launch_bounds__(64) void direct_small_f64_kernel(DirectArgs a, double* __restrict__ buf, int count) {
    const int q = threadIdx.x;
    double mine[DIRECT_SMALL_MAX];
#pragma unroll
    for (int i = 0; i < DIRECT_SMALL_MAX; ++i) mine[i] = i < count ? buf[i] : 0.0;
    __threadfence_system();
    if (q < a.P) {
        double* slot = reinterpret_cast<double*>(a.peer[q] + 4096) + ((size_t)a.par * DNMF_DIRECT_MAX_RANKS + a.rank) * DIRECT_SMALL_MAX;
        for (int i = 0; i < count; ++i)
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(slot) + i, (unsigned long long)__double_as_longlong(mine[i]), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        __threadfence_system();
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(a.peer[q] + 3072) + a.rank, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        const unsigned long long* flag = reinterpret_cast<const unsigned long long*>(a.peer[a.rank] + 3072) + q;
        const unsigned long long t0 = wall_clock64();
        while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < a.seq) {
            __builtin_amdgcn_s_sleep(2);
            if (wall_clock64() - t0 > a.patience) {
                __hip_atomic_store(d_flags(a.peer[a.rank], 2), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
        }
    }
    __syncthreads();
    if (q < count) {
        const unsigned long long* slots = reinterpret_cast<const unsigned long long*>(a.peer[a.rank] + 4096) + (size_t)a.par * DNMF_DIRECT_MAX_RANKS * DIRECT_SMALL_MAX;
        double s = 0.0;
        for (int r = 0; r < a.P; ++r)
            s += __longlong_as_double((long long)__hip_atomic_load(slots + (size_t)r * DIRECT_SMALL_MAX + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
        buf[q] = s;
    }
}

int direct_allreduce_small_f64(dnmf_comm* cm, double* buf, size_t count, hipStream_t st) {
    DirectArgs a{};
    for (int q = 0; q < cm->nranks; ++q) a.peer[q] = cm->direct_peer[q];
    a.P = cm->nranks; a.rank = cm->rank; a.cap = cm->direct_cap; a.count = count;
    a.seq = ++cm->direct_small_seq;
    a.par = (int)(a.seq & 1);
    a.patience = cm->direct_patience;
    hipLaunchKernelGGL(direct_small_f64_kernel, dim3(1), dim3(64), 0, st, a, buf, (int)count);
    return check_launch("allreduce(direct, small)");
}

}  // namespace

// ---------------------------------------------------------------------------------------------- what csrc/dnmf_grid.hip calls (dnmf_comm.h)
int dnmf_allreduce_f32_(dnmf_comm* cm, int g, float* buf, size_t count, hipStream_t st) {
    if (cm->direct_on && g == G_WORLD && cm->nranks > 1 && !cm->null_exchange && count <= cm->direct_cap && count % 2 == 0 &&
        ((uintptr_t)buf & 7) == 0)
        return direct_allreduce(cm, buf, count, st);
    ncclComm_t c;
    const int r = resolve(cm, g, &c, "allreduce");
    if (r) return r < 0 ? r : DNMF_OK;
    if (cm->hook) return cm->hook(cm->hook_user, OP_ALLREDUCE, g, buf, buf, count, st) ? fail(DNMF_ECOMM, "allreduce: the host collective failed") : DNMF_OK;
    NCCL_OK(rccl()->AllReduce(buf, buf, count, ncclFloat32, ncclSum, c, st), "allreduce");
    return DNMF_OK;
}

int dnmf_allreduce_f64_(dnmf_comm* cm, int g, double* buf, size_t count, hipStream_t st) {
    if (cm->direct_on && g == G_WORLD && cm->nranks > 1 && !cm->null_exchange && count >= 1 && count <= DIRECT_SMALL_MAX)
        return direct_allreduce_small_f64(cm, buf, count, st);
    ncclComm_t c;
    const int r = resolve(cm, g, &c, "allreduce");
    if (r) return r < 0 ? r : DNMF_OK;
    if (cm->hook)
        return cm->hook(cm->hook_user, DNMF_ALLREDUCE_F64, g, buf, buf, count, st)
                   ? fail(DNMF_ECOMM, "allreduce: the host collective failed") : DNMF_OK;
    NCCL_OK(rccl()->AllReduce(buf, buf, count, ncclFloat64, ncclSum, c, st), "allreduce");
    return DNMF_OK;
}

// The W sweep of HALS with cross-rank column norms (dist_nmf.py:884-891 with utils.norm :388-391): column kernel, 8-byte
// allreduce, next column (which first applies the pending normalisation), final scale.  ss2 = k device doubles.
// Do ALL ranks take the one-launch cross-rank sweep for this shape?  Decided once per (rows, rank k) by the ranks together: every rank
// contributes its workgroup count (0: the persistent sweep does not apply here -- too many rows to keep resident, workspace too
// small) through a world allreduce; the sweep is on when every rank can and the slots fit a column of the slab.  The counts also
// give each rank its first slot.  (Host-synchronous, once per shape.)
static int hals_xsweep_agree(dnmf_comm* cm, float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G, float eps, void* ws,
                             size_t ws_bytes, hipStream_t st) {
    cm->xs_m = m; cm->xs_k = k; cm->xs_ok = 0; cm->xs_seen_epoch = cm->xs_epoch; cm->xs_pers = dnmf_persistent_on_();
    int nwg = 0;
    const bool mine = ws && ws_bytes >= 64 * sizeof(float) &&
                      dnmf_hals_sweep_w_peers_(W, m, k, ldw, AH, ldah, G, eps, ws, ws_bytes, nullptr, &nwg, (void*)st) == 0;
    float host[DNMF_DIRECT_MAX_RANKS] = {};
    host[cm->rank] = mine ? (float)nwg : -1.0e6f;                  // (a rank that cannot poisons the sum of its own slot)
    // the comm's own buffer: a rank that cannot take the sweep (no workspace, too small a one) still joins the allreduce
    if (!cm->agree_buf) HIP_OK(hipMalloc((void**)&cm->agree_buf, sizeof(host)), "hals sweep: agreement buffer");
    float* dev = cm->agree_buf;
    HIP_OK(hipMemcpyAsync(dev, host, sizeof(host), hipMemcpyHostToDevice, st), "hals sweep: agreement");
    HIP_OK(hipStreamSynchronize(st), "hals sweep: agreement");
    if (int rc = dnmf_allreduce_f32_(cm, G_WORLD, dev, DNMF_DIRECT_MAX_RANKS, st)) return rc;
    HIP_OK(hipMemcpyAsync(host, dev, sizeof(host), hipMemcpyDeviceToHost, st), "hals sweep: agreement");
    HIP_OK(hipStreamSynchronize(st), "hals sweep: agreement");
    int total = 0, first = 0;
    bool all = true;
    for (int q = 0; q < cm->nranks; ++q) {
        if (!(host[q] >= 1.0f)) all = false;
        if (q < cm->rank) first += (int)host[q];
        total += (int)host[q];
    }
    cm->xs_ok = all && total <= HALS_MAX_WG;
    cm->xs_first = first; cm->xs_total = total;
    return DNMF_OK;
}

int dnmf_hals_sweep_exchanged_(dnmf_comm* cm, float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G, float eps,
                               double* ss2, void* ws, size_t ws_bytes, void* stream, int column_sweep) {
    hipStream_t st = S(stream);
    // ONE persistent launch when the direct peer regions are up (dnmf_comm_set_direct) and every rank can keep its rows resident:
    // the column partials cross the ranks through the slot slabs in the exported regions (csrc/dnmf_hals.h, HalsPeers)
    // (`column_sweep`: the caller asked for the column launches -- every rank passes the same value, params.hals_sweep = 'columns')
    if (!column_sweep && cm->direct_on && !cm->null_exchange && k <= DNMF_TUNED_MAX_K && cm->nranks <= DNMF_DIRECT_MAX_RANKS) {
        if (cm->xs_seen_epoch != cm->xs_epoch || cm->xs_k != k || cm->xs_pers != dnmf_persistent_on_()) {
            if (int rc = hals_xsweep_agree(cm, W, m, k, ldw, AH, ldah, G, eps, ws, ws_bytes, st)) return rc;
        } else if (cm->xs_m != m)                                   // a rank cannot re-open the agreement on its own
            return fail(DNMF_EINVAL, "hals sweep: the row count of rank %d changed (%ld -> %ld) inside one fit: call dnmf_comm_fit_begin on every rank "
                                     "before the first step on new data", cm->rank, cm->xs_m, m);
        if (cm->xs_ok) {
            HalsPeers pe{};
            pe.P = cm->nranks; pe.rank = cm->rank; pe.first = cm->xs_first; pe.total = cm->xs_total; pe.patience = cm->direct_patience;
            const size_t off = direct_hals_off(cm->direct_cap) + (size_t)(cm->hals_seq & 1) * HALS_SLAB_BYTES;
            for (int q = 0; q < cm->nranks; ++q) pe.slab[q] = reinterpret_cast<unsigned long long*>(cm->direct_peer[q] + off);
            ++cm->hals_seq;
            const int rc = dnmf_hals_sweep_w_peers_(W, m, k, ldw, AH, ldah, G, eps, ws, ws_bytes, &pe, nullptr, stream);
            if (rc != 1) return rc;
            return fail(DNMF_EINVAL, "hals sweep: the persistent sweep the ranks agreed on does not apply on rank %d", cm->rank);
        }
    }
    HIP_OK(hipMemsetAsync(ss2, 0, (size_t)k * sizeof(double), st), "hals sweep: memset");
    int rc;
    for (int kk = 0; kk < k; ++kk) {
        if ((rc = dnmf_hals_w_col(W, m, k, ldw, AH, ldah, G, kk, kk > 0 ? ss2 + kk - 1 : nullptr, eps, ss2 + kk, stream))) return rc;
        if ((rc = dnmf_allreduce_f64_(cm, G_WORLD, ss2 + kk, 1, st))) return rc;
    }
    return dnmf_hals_w_scale(W, m, ldw, k - 1, ss2 + k - 1, stream);
}
// ... and with local norms: the persistent sweep (or its column form on request)
int dnmf_hals_sweep_local_(float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G, float eps, int column_sweep,
                           double* ss2, void* ws, size_t kws, void* stream) {
    if (column_sweep) {
        HIP_OK(hipMemsetAsync(ss2, 0, (size_t)k * sizeof(double), S(stream)), "hals sweep: memset");
        return dnmf_hals_update_w(W, m, k, ldw, AH, ldah, G, eps, ss2, stream);
    }
    return dnmf_hals_sweep_w(W, m, k, ldw, AH, ldah, G, eps, ws, kws, stream);
}

int dnmf_allgather_f32_(dnmf_comm* cm, int g, const float* send, float* recv, size_t count, hipStream_t st) {
    ncclComm_t c;
    const int r = resolve(cm, g, &c, "allgather");
    if (r < 0) return r;
    if (r) {                                                       // one member (or a stubbed exchange): its own block
        HIP_OK(hipMemcpyAsync(recv, send, count * sizeof(float), hipMemcpyDeviceToDevice, st), "allgather: copy");
        return DNMF_OK;
    }
    if (cm->hook) return cm->hook(cm->hook_user, OP_ALLGATHER, g, send, recv, count, st) ? fail(DNMF_ECOMM, "allgather: the host collective failed") : DNMF_OK;
    NCCL_OK(rccl()->AllGather(send, recv, count, ncclFloat32, c, st), "allgather");
    if (cm->emulated)      // (the other members' blocks: copies of this one, so that the step runs on finite numbers)
        for (int q = 1; q < group_size(cm, g); ++q)
            HIP_OK(hipMemcpyAsync(recv + (size_t)q * count, recv, count * sizeof(float), hipMemcpyDeviceToDevice, st), "allgather: copy");
    return DNMF_OK;
}

int dnmf_reduce_scatter_f32_(dnmf_comm* cm, int g, const float* send, float* recv, size_t count, int member, hipStream_t st) {
    ncclComm_t c;
    const int r = resolve(cm, g, &c, "reduce_scatter");
    if (r < 0) return r;
    if (r) {
        const size_t at = group_size(cm, g) == 1 ? 0 : (size_t)member * count;
        HIP_OK(hipMemcpyAsync(recv, send + at, count * sizeof(float), hipMemcpyDeviceToDevice, st), "reduce_scatter: copy");
        return DNMF_OK;
    }
    if (cm->hook) return cm->hook(cm->hook_user, OP_REDUCE_SCATTER, g, send, recv, count, st) ? fail(DNMF_ECOMM, "reduce_scatter: the host collective failed") : DNMF_OK;
    NCCL_OK(rccl()->ReduceScatter(cm->emulated ? send + (size_t)member * count : send, recv, count, ncclFloat32, ncclSum, c, st), "reduce_scatter");
    return DNMF_OK;
}

extern "C" {

int dnmf_comm_unique_id(void* id_out) {
    REQUIRE(id_out, "comm_unique_id: null pointer");
    Rccl* r = rccl();
    if (!r) return fail(DNMF_ECOMM, "comm_unique_id: no RCCL library found (librccl.so.1)");
    ncclUniqueId id;
    NCCL_OK(r->GetUniqueId(&id), "ncclGetUniqueId");
    memcpy(id_out, &id, DNMF_UNIQUE_ID_BYTES);
    return DNMF_OK;
}

int dnmf_comm_create(const void* unique_id, int nranks, int rank, int p_r, int p_c, dnmf_comm_t** out) {
    REQUIRE(unique_id && out && nranks >= 1 && rank >= 0 && rank < nranks && p_r >= 1 && p_c >= 1 && p_r * p_c == nranks,
            "comm_create: bad arguments (nranks %d, rank %d, grid %d x %d)", nranks, rank, p_r, p_c);
    static_assert(DNMF_UNIQUE_ID_BYTES == sizeof(ncclUniqueId), "unique id size");
    Rccl* r = rccl();
    if (!r) return fail(DNMF_ECOMM, "comm_create: no RCCL library found (librccl.so.1)");
    dnmf_comm* c = new dnmf_comm();
    c->nranks = nranks; c->rank = rank; c->p_r = p_r; c->p_c = p_c;
    if (p_r > 1 && p_c > 1 && !r->CommSplit) {
        delete c;
        return fail(DNMF_ECOMM, "comm_create: this RCCL (%s) has no ncclCommSplit: a %d x %d grid needs it (1D grids do not)", r->origin, p_r, p_c);
    }
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    ncclResult_t e = r->CommInitRank(&c->world, nranks, id, rank);
    if (e != ncclSuccess) { delete c; return nccl_fail("ncclCommInitRank", e); }
    if (p_r > 1 && p_c > 1) {            // rank = i * p_c + j (dist_comm.py:22, reorder = False)
        const int i = rank / p_c, j = rank % p_c;
        e = r->CommSplit(c->world, j, i, &c->row, nullptr);                    // same grid column j, ordered by i (dist_comm.py:25-37)
        if (e == ncclSuccess) e = r->CommSplit(c->world, i, j, &c->col, nullptr);   // same grid row i, ordered by j (dist_comm.py:39-51)
        if (e != ncclSuccess) { dnmf_comm_destroy(c); return nccl_fail("ncclCommSplit", e); }
    }
    if (hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking) != hipSuccess) { dnmf_comm_destroy(c); return fail(DNMF_EHIP, "comm_create: stream"); }
    for (int q = 0; q < MAX_CHUNKS; ++q)
        if (hipEventCreateWithFlags(&c->ready[q], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->done[q], hipEventDisableTiming) != hipSuccess) { dnmf_comm_destroy(c); return fail(DNMF_EHIP, "comm_create: events"); }
    *out = c;
    return DNMF_OK;
}

// MEASUREMENT ONLY (bench.py --emulate-ranks on a one-GPU box): member `rank` of a p_r x p_c grid whose collectives -- world, row
// and column groups alike -- are issued for real on a ONE-rank RCCL communicator: launch and stream-ordering costs are real, there
// is no wire, and the buffers have the sizes of the real grid (the other members' allgather blocks are copies of this member's).
// The step entry points then run exactly as on the grid; their results are not a factorisation of anything.
int dnmf_comm_create_emulated(int p_r, int p_c, int rank, dnmf_comm_t** out) {
    REQUIRE(out && p_r >= 1 && p_c >= 1 && rank >= 0 && rank < p_r * p_c, "comm_create_emulated: bad arguments (grid %d x %d, member %d)", p_r, p_c, rank);
    Rccl* r = rccl();
    if (!r) return fail(DNMF_ECOMM, "comm_create_emulated: no RCCL library found (librccl.so.1)");
    dnmf_comm* c = new dnmf_comm();
    c->nranks = p_r * p_c; c->rank = rank; c->p_r = p_r; c->p_c = p_c; c->emulated = 1;
    ncclUniqueId id;
    ncclResult_t e = r->GetUniqueId(&id);
    if (e == ncclSuccess) e = r->CommInitRank(&c->world, 1, id, 0);
    if (e != ncclSuccess) { delete c; return nccl_fail("comm_create_emulated", e); }
    if (hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking) != hipSuccess) { dnmf_comm_destroy(c); return fail(DNMF_EHIP, "comm_create_emulated: stream"); }
    for (int q = 0; q < MAX_CHUNKS; ++q)
        if (hipEventCreateWithFlags(&c->ready[q], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->done[q], hipEventDisableTiming) != hipSuccess) { dnmf_comm_destroy(c); return fail(DNMF_EHIP, "comm_create_emulated: events"); }
    *out = c;
    return DNMF_OK;
}

int dnmf_comm_rccl_version(int* version, char* origin, size_t origin_bytes) {
    Rccl* r = rccl();
    if (!r) return fail(DNMF_ECOMM, "comm_rccl_version: no RCCL library found (librccl.so.1)");
    int v = 0;
    if (r->GetVersion && r->GetVersion(&v) != ncclSuccess) v = 0;
    if (version) *version = v;
    if (origin && origin_bytes) snprintf(origin, origin_bytes, "%s", r->origin);
    return DNMF_OK;
}

int dnmf_comm_create_hosted(int nranks, int rank, int p_r, int p_c, dnmf_collective_fn fn, void* user, dnmf_comm_t** out) {
    REQUIRE(fn && out && nranks >= 1 && rank >= 0 && rank < nranks && p_r >= 1 && p_c >= 1 && p_r * p_c == nranks,
            "comm_create_hosted: bad arguments (nranks %d, rank %d, grid %d x %d)", nranks, rank, p_r, p_c);
    dnmf_comm* c = new dnmf_comm();
    c->nranks = nranks; c->rank = rank; c->p_r = p_r; c->p_c = p_c;
    c->hook = fn; c->hook_user = user;
    if (hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking) != hipSuccess) { dnmf_comm_destroy(c); return fail(DNMF_EHIP, "comm_create_hosted: stream"); }
    for (int q = 0; q < MAX_CHUNKS; ++q)
        if (hipEventCreateWithFlags(&c->ready[q], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->done[q], hipEventDisableTiming) != hipSuccess) { dnmf_comm_destroy(c); return fail(DNMF_EHIP, "comm_create_hosted: events"); }
    *out = c;
    return DNMF_OK;
}

int dnmf_comm_direct_init(dnmf_comm_t* c, size_t max_floats, void* handle_out) {
    REQUIRE(c && handle_out && max_floats >= 2 && c->nranks <= DNMF_DIRECT_MAX_RANKS, "comm_direct_init: bad arguments (%d ranks, at most %d)",
            c ? c->nranks : 0, DNMF_DIRECT_MAX_RANKS);
    REQUIRE(!c->direct_peer[c->rank], "comm_direct_init: already set up");
    static_assert(sizeof(hipIpcMemHandle_t) + 2 * sizeof(unsigned long long) <= DNMF_DIRECT_HANDLE_BYTES, "IPC handle size");
    const size_t cap = (max_floats + 63) / 64 * 64;
    const size_t bytes = direct_hals_off(cap) + 2 * HALS_SLAB_BYTES;
    void* region = nullptr;
    // UNCACHED (fine-grained) device memory: flags and data are read by peers while kernels of this GPU run.  No fallback to an
    // ordinary allocation: its coherence across agents is not what the protocol was validated on -- the rank fails here, the
    // host's agreement round (NativeComm.enable_direct) keeps every rank on the communicator's own allreduce.
    hipError_t e = hipExtMallocWithFlags(&region, bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(DNMF_EHIP, "comm_direct_init: uncached allocation of %zu bytes: %s", bytes, hipGetErrorString(e)); }
    if ((e = hipMemset(region, 0, bytes)) != hipSuccess ||                                         // flags, buffers; the HALS slot slabs: "empty"
        (e = hipMemset((char*)region + direct_hals_off(cap), 0xff, 2 * HALS_SLAB_BYTES)) != hipSuccess) {
        (void)hipFree(region);
        return fail(DNMF_EHIP, "comm_direct_init: memset: %s", hipGetErrorString(e));
    }
    hipIpcMemHandle_t h;
    e = hipIpcGetMemHandle(&h, region);
    if (e != hipSuccess) { (void)hipFree(region); return fail(DNMF_EHIP, "comm_direct_init: hipIpcGetMemHandle: %s", hipGetErrorString(e)); }
    // the exchanged blob: [IPC handle | capacity in floats | magic] -- peers compute offsets into EVERY region from one capacity,
    // so dnmf_comm_direct_connect requires all of them equal
    memset(handle_out, 0, DNMF_DIRECT_HANDLE_BYTES);
    memcpy(handle_out, &h, sizeof(h));
    const unsigned long long tail[2] = {(unsigned long long)cap, DIRECT_MAGIC};
    memcpy((char*)handle_out + sizeof(h), tail, sizeof(tail));
    c->direct_peer[c->rank] = (char*)region;
    c->direct_cap = cap;
    return DNMF_OK;
}

int dnmf_comm_direct_connect(dnmf_comm_t* c, const void* handles) {
    REQUIRE(c && handles && c->direct_peer[c->rank], "comm_direct_connect: call dnmf_comm_direct_init first");
    for (int q = 0; q < c->nranks; ++q) {       // every rank sees every blob: a mismatch anywhere fails the connect everywhere
        unsigned long long tail[2];
        memcpy(tail, (const char*)handles + (size_t)q * DNMF_DIRECT_HANDLE_BYTES + sizeof(hipIpcMemHandle_t), sizeof(tail));
        REQUIRE(tail[1] == DIRECT_MAGIC, "comm_direct_connect: rank %d did not initialise its region", q);
        REQUIRE(tail[0] == (unsigned long long)c->direct_cap, "comm_direct_connect: rank %d sized its region for %llu floats, this rank for %zu "
                "(every rank must pass the same max_floats to dnmf_comm_direct_init)", q, tail[0], c->direct_cap);
    }
    for (int q = 0; q < c->nranks; ++q) {
        if (q == c->rank || c->direct_peer[q]) continue;
        hipIpcMemHandle_t h;
        memcpy(&h, (const char*)handles + (size_t)q * DNMF_DIRECT_HANDLE_BYTES, sizeof(h));
        void* p = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) return fail(DNMF_EHIP, "comm_direct_connect: hipIpcOpenMemHandle(rank %d): %s", q, hipGetErrorString(e));
        c->direct_peer[q] = (char*)p;
    }
    return DNMF_OK;
}

// undo dnmf_comm_direct_init / _connect (a set-up that failed on some rank, or the end of the communicator): unmap the peers,
// free the own region.  The caller makes sure no peer still reads it (NativeComm.close runs a host barrier first).
static void direct_teardown(dnmf_comm* c) {
    c->direct_on = 0;
    for (int q = 0; q < c->nranks && q < DNMF_DIRECT_MAX_RANKS; ++q) {
        if (!c->direct_peer[q]) continue;
        if (q == c->rank) (void)hipFree(c->direct_peer[q]);
        else (void)hipIpcCloseMemHandle(c->direct_peer[q]);
        c->direct_peer[q] = nullptr;
    }
    c->direct_cap = 0;
}

int dnmf_comm_direct_teardown(dnmf_comm_t* c) {
    REQUIRE(c, "comm_direct_teardown: null communicator");
    (void)hipDeviceSynchronize();
    direct_teardown(c);
    return DNMF_OK;
}

int dnmf_comm_set_direct_timeout(dnmf_comm_t* c, double seconds) {
    REQUIRE(c && seconds >= 0.001 && seconds <= 86400.0, "comm_set_direct_timeout: 0.001 .. 86400 seconds");
    c->direct_patience = (unsigned long long)(seconds * 1e8);
    return DNMF_OK;
}

int dnmf_comm_hals_xsweeps(dnmf_comm_t* c, unsigned long long* count) {
    REQUIRE(c && count, "comm_hals_xsweeps: null pointer");
    *count = c->hals_seq;
    return DNMF_OK;
}

int dnmf_comm_set_direct(dnmf_comm_t* c, int on) {
    REQUIRE(c, "comm_set_direct: null communicator");
    if (on) for (int q = 0; q < c->nranks; ++q) REQUIRE(c->direct_peer[q], "comm_set_direct: rank %d is not connected", q);
    c->direct_on = on ? 1 : 0;
    return DNMF_OK;
}

int dnmf_comm_direct_status(dnmf_comm_t* c, int* timed_out) {
    REQUIRE(c && timed_out && c->direct_peer[c->rank], "comm_direct_status: not set up");
    unsigned long long w = 0;
    HIP_OK(hipMemcpy(&w, c->direct_peer[c->rank] + 2048, sizeof(w), hipMemcpyDeviceToHost), "comm_direct_status: copy");
    *timed_out = w != 0;
    return DNMF_OK;
}

int dnmf_comm_allreduce_direct(dnmf_comm_t* c, float* buf, size_t count, void* stream) {
    REQUIRE(c && buf, "comm_allreduce_direct: bad arguments");
    for (int q = 0; q < c->nranks; ++q) REQUIRE(c->direct_peer[q], "comm_allreduce_direct: rank %d is not connected", q);
    if (c->nranks == 1) return DNMF_OK;
    return direct_allreduce(c, buf, count, S(stream));
}

int dnmf_comm_allreduce_direct_f64(dnmf_comm_t* c, double* buf, size_t count, void* stream) {
    REQUIRE(c && buf && count >= 1 && count <= DIRECT_SMALL_MAX, "comm_allreduce_direct_f64: 1 <= count <= %d doubles", DIRECT_SMALL_MAX);
    for (int q = 0; q < c->nranks; ++q) REQUIRE(c->direct_peer[q], "comm_allreduce_direct_f64: rank %d is not connected", q);
    if (c->nranks == 1) return DNMF_OK;
    return direct_allreduce_small_f64(c, buf, count, S(stream));
}

int dnmf_comm_destroy(dnmf_comm_t* c) {
    if (!c) return DNMF_OK;
    direct_teardown(c);
    Rccl* r = rccl();
    for (int q = 0; q < MAX_CHUNKS; ++q) {
        if (c->ready[q]) (void)hipEventDestroy(c->ready[q]);
        if (c->done[q]) (void)hipEventDestroy(c->done[q]);
    }
    if (c->xstream) (void)hipStreamDestroy(c->xstream);
    if (c->agree_buf) (void)hipFree(c->agree_buf);
    if (r) {
        if (c->row) r->CommDestroy(c->row);
        if (c->col) r->CommDestroy(c->col);
        if (c->world) r->CommDestroy(c->world);
    }
    delete c;
    return DNMF_OK;
}

int dnmf_comm_fit_begin(dnmf_comm_t* c) {
    REQUIRE(c, "comm_fit_begin: null communicator");
    ++c->xs_epoch;
    return DNMF_OK;
}

int dnmf_comm_set_overlap_chunks(dnmf_comm_t* c, int chunks) {
    REQUIRE(c && chunks >= 1 && chunks <= MAX_CHUNKS, "comm_set_overlap_chunks: 1 <= chunks <= %d", MAX_CHUNKS);
    c->overlap_chunks = chunks;
    return DNMF_OK;
}

int dnmf_comm_set_always_exchange(dnmf_comm_t* c, int on) {
    REQUIRE(c, "comm_set_always_exchange: null communicator");
    c->always = on != 0;
    return DNMF_OK;
}

int dnmf_comm_set_null_exchange(dnmf_comm_t* c, int on) {
    REQUIRE(c, "comm_set_null_exchange: null communicator");
    c->null_exchange = on != 0;
    return DNMF_OK;
}

int dnmf_comm_info(const dnmf_comm_t* c, int* nranks, int* rank, int* p_r, int* p_c) {
    REQUIRE(c, "comm_info: null communicator");
    if (nranks) *nranks = c->nranks;
    if (rank) *rank = c->rank;
    if (p_r) *p_r = c->p_r;
    if (p_c) *p_c = c->p_c;
    return DNMF_OK;
}

int dnmf_comm_allreduce(dnmf_comm_t* c, float* buf, size_t count, int group, void* stream) {
    REQUIRE(c && buf && group >= 0 && group <= 2, "comm_allreduce: bad arguments");
    return dnmf_allreduce_f32_(c, group, buf, count, S(stream));
}

}  // extern "C"
