// dnmf_comm.h -- the communicator of csrc/dnmf_comm.hip as the grid steps (csrc/dnmf_grid.hip) see it: its state, the groups of the
// grid, and the collectives and HALS W sweeps the steps enqueue.  Private to the library.
#pragma once
#include <rccl/rccl.h>

#include "dnmf_common.h"

namespace {

constexpr int MAX_CHUNKS = 8;                // column chunks of the overlapped H phase, at most (dnmf_comm_set_overlap_chunks)

// The groups of the grid: all ranks, cart_1d_row (the p_r ranks of a grid column), cart_1d_column (the p_c ranks of a grid row) --
// dist_comm.py:16-56
enum { G_WORLD = 0, G_ROW = 1, G_COL = 2 };

inline size_t pad64(size_t x) { return (x + 63) / 64 * 64; }

#define HIP_OK(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(DNMF_EHIP, "%s: %s", what, hipGetErrorString(e_)); } while (0)

}  // namespace

struct dnmf_comm {
    ncclComm_t world = nullptr, row = nullptr, col = nullptr;   // row: the p_r ranks of one grid column; col: the p_c ranks of one grid row
    int nranks = 1, rank = 0, p_r = 1, p_c = 1;
    int overlap_chunks = 1;
    int always = 0;                                              // testing: a one-rank communicator still issues its RCCL calls
    int null_exchange = 0;                                       // measurement: the steps skip their RCCL calls (wrong results on > 1 rank)
    dnmf_collective_fn hook = nullptr;                           // host-supplied collectives instead of RCCL (dnmf_comm_create_hosted)
    void* hook_user = nullptr;
    hipStream_t xstream = nullptr;                               // exchanges of the overlapped H phase run here
    hipEvent_t ready[MAX_CHUNKS] = {}, done[MAX_CHUNKS] = {};
    // direct (two-shot) allreduce over IPC peer buffers (dnmf_comm_direct_*): every rank's region as mapped into this process
    int direct_on = 0;
    size_t direct_cap = 0;                                       // floats per message
    char* direct_peer[DNMF_DIRECT_MAX_RANKS] = {};               // [rank] = the own region
    unsigned long long direct_seq = 0, direct_small_seq = 0;
    unsigned long long direct_patience = 30ull * 100000000ull;   // 30 s of the 100 MHz wall clock (dnmf_comm_set_direct_timeout)
    int emulated = 0;                                            // measurement: ONE member of a p_r x p_c grid, every collective on a one-rank RCCL communicator
    // cross-rank persistent HALS W sweep over the peer regions (dnmf_hals_sweep_exchanged_): the ranks' agreement for the last shape seen
    unsigned long long hals_seq = 0;                             // sweeps issued: its parity selects the slot slab
    long xs_m = -1; int xs_k = -1, xs_ok = 0, xs_first = 0, xs_total = 0;
    // WHEN the ranks agree again is a function of things every rank sees alike -- the fit counter (dnmf_comm_fit_begin: PyNMF calls it on
    // every rank at the start of every fit), the rank k, the process-wide persistent switch -- never of a rank's LOCAL row count: with
    // an asymmetric split two fits of different global m can change the row count on some ranks only, and an agreement
    // that only those ranks enter is a collective mismatch
    int xs_epoch = 0, xs_seen_epoch = -1, xs_pers = -1;
    float* agree_buf = nullptr;                                  // DNMF_DIRECT_MAX_RANKS device floats of the comm's own (the caller's workspace may be absent)
};

// ---- csrc/dnmf_comm.hip.  A group of one member is the identity (unless `always` asks a one-rank communicator to issue its calls
// anyway); a hosted communicator hands every call to the host's function.
#define DNMF_INTERNAL __attribute__((visibility("hidden")))
// in-place SUM over the group: floats; doubles (the column norms of the HALS W sweep, utils.py:388-391)
DNMF_INTERNAL int dnmf_allreduce_f32_(dnmf_comm* cm, int g, float* buf, size_t count, hipStream_t st);
DNMF_INTERNAL int dnmf_allreduce_f64_(dnmf_comm* cm, int g, double* buf, size_t count, hipStream_t st);
// equal blocks of `count` floats: recv[q * count ...] = member q's send (MPI Allgather, dist_nmf.py:163-165, :195-197)
DNMF_INTERNAL int dnmf_allgather_f32_(dnmf_comm* cm, int g, const float* send, float* recv, size_t count, hipStream_t st);
// SUM reduce-scatter of members x count floats: recv = this member's block of the sum (MPI Reduce_scatter, :169, :202)
DNMF_INTERNAL int dnmf_reduce_scatter_f32_(dnmf_comm* cm, int g, const float* send, float* recv, size_t count, int member, hipStream_t st);
// The W sweep of HALS with cross-rank column norms (ss2 = k device doubles), and with local norms
DNMF_INTERNAL int dnmf_hals_sweep_exchanged_(dnmf_comm* cm, float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G,
                                             float eps, double* ss2, void* ws, size_t ws_bytes, void* stream, int column_sweep = 0);
DNMF_INTERNAL int dnmf_hals_sweep_local_(float* W, long m, int k, long ldw, const float* AH, long ldah, const float* G, float eps,
                                         int column_sweep, double* ss2, void* ws, size_t kws, void* stream);
#undef DNMF_INTERNAL
