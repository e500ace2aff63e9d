"""NMFk over dense data with NaN-marked gaps (`params.missing = 'nan'`): test helpers (TEST INFRASTRUCTURE, lives under tests/ only).

`MaskedNmfkOracleOps`: the checker operator set of a MaskedDenseBlock (tests/_masked_dense.py) plus what a sweep asks of an operator
set beyond a fit -- the per-column error sums over the observed positions in float64 numpy (tests/_sparse_nmfk.py::column_err_sums64
on the block's COO form) -- and the capability flag PyNMFk looks for.  `run_nmfk_golden_nan`: tests/_mp.py::run_nmfk_golden with
`missing='nan'` on the fixture's matrix (which has no NaN).  `colerr_case` / `COLERR_*`: the exact operands of the kernel test, shared
by the float64 proof (CPU) and the GPU test, built once per process.
"""
import os
import traceback

import numpy as np
import torch

from tests import _masked_dense as D
from tests._ops_double import _n
from tests._sparse_nmfk import column_err_sums64


class MaskedNmfkOracleOps(D.MaskedDenseOracleOps):
    name = "oracle-masked-nmfk"
    masked_nmfk = True

    def column_err_sums(self, A, W, H):
        if not self._blk(A):
            return super().column_err_sums(A, W, H)
        rows, col, val = self._coo(A)
        num, den = column_err_sums64(rows, col, val, A.shape[1], _n(W), _n(H), True)
        return torch.from_numpy(num), torch.from_numpy(den)


def missing_args(tmp, missing):
    """the parameters of tests/test_gpu_sparse_nmfk.py::_missing_args (mu / fro, k = 1..5, 6 perturbations, 300 iterations) with
    prune off, as missing='nan' asks"""
    from pydnmfk_amd.dist_comm import MPI_comm
    from tests.test_nmfk_cpu import _args
    os.makedirs(str(tmp), exist_ok=True)
    args = _args(tmp, MPI_comm(None, 1, 1))
    assert (args.method, args.norm, args.start_k, args.end_k, args.perturbations) == ("mu", "fro", 1, 5, 6)
    args.prune = False
    if missing:
        args.missing = missing
    return args


def min_silhouettes(nmfk):
    return [float(np.min(np.asarray(nmfk.stats[k]["clusterSilhouetteCoefficients"]))) for k in sorted(nmfk.stats)]


# ---- the reference's golden on two gloo ranks
def _golden_rank(rank, world, port, fixture, q, use_hip, extra):
    try:
        import json
        import tempfile
        import torch.distributed as dist
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMFk import PyNMFk
        from pydnmfk_amd.utils import determine_block_params, parse
        from tests._golden import GOLDEN

        torch.set_num_threads(1)
        if use_hip:
            torch.cuda.set_device(0)
        ops = None if use_hip else MaskedNmfkOracleOps()
        if world > 1:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        z = np.load(os.path.join(GOLDEN, fixture))
        meta = json.loads(str(z["meta"]))
        A = z["A"]
        assert not np.isnan(A).any()
        p_r, p_c = meta["grid"]
        args = parse()
        comms = MPI_comm(None, p_r, p_c)
        args.size, args.rank, args.comm1, args.comm, args.p_r, args.p_c = world, rank, comms.comm, comms, p_r, p_c
        args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
        tmp = [tempfile.mkdtemp() if rank == 0 else None]
        if world > 1:
            dist.broadcast_object_list(tmp, src=0)
        args.fpath, args.fname, args.ftype = tmp[0] + "/", "synth", "npy"
        args.start_k, args.end_k, args.step_k = meta["start_k"], meta["end_k"], 1
        args.sill_thr, args.itr, args.init, args.verbose = meta["sill_thr"], meta["itr"], "rand", False
        args.norm, args.method, args.prune = meta["norm"], meta["method"], False
        args.perturbations, args.noise_var, args.checkpoint = meta["perturbations"], meta["noise_var"], False
        args.results_path = tmp[0] + "/results/"
        args.missing = "nan"
        for key, val in (extra or {}).items():
            setattr(args, key, val)
        s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
        A_ij = np.ascontiguousarray(A[s[0]:e[0] + 1, s[1]:e[1] + 1], dtype=np.float32)
        nmfk = PyNMFk(A_ij, factors=None, params=args, ops=ops)
        assert isinstance(nmfk.A_ij, np.ndarray) and nmfk._masked and nmfk._batch_size() == 1
        nopt = nmfk.fit()
        stats = {k: {key: np.asarray(val) for key, val in st.items()} for k, st in nmfk.stats.items()}
        q.put((rank, (int(nopt), stats), None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_nmfk_golden_nan(fixture, use_hip=False, timeout=600, extra=None):
    """-> [(nopt, {k: statistics}) per rank] on the fixture's grid"""
    import json
    import torch.multiprocessing as mp
    from tests._golden import GOLDEN
    from tests._mp import collect, free_port
    grid = json.loads(str(np.load(os.path.join(GOLDEN, fixture))["meta"]))["grid"]
    world = grid[0] * grid[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_golden_rank, args=(r, world, port, fixture, q, use_hip, extra)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(procs, q, timeout)
    for rank, out, err in res:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
    return [out for _, out, _ in sorted(res, key=lambda r: r[0])]


# ---- exact operands of the per-column error kernel (csrc/dnmf_sums.h: col_sums_kernel<KT, FAST, MaskedErrTerm>)
# EXACT_SHAPES of tests/_masked_dense.py stay at one 128-column block and one 32-row block per chunk.  COLERR_LOOP_CASES are the
# smallest shapes whose plan (dnmf_masked_column_err_plan: {rowblks_per_chunk, nchunks, ncolblk}) leaves one trip of each loop; what
# tests/test_capi_masked_nmfk.py must find in the plan at EVERY rank:
#   last_chunk_blks  row blocks of the last chunk     last_blk_rows  rows of its last block     last_colblk_cols  width of the last column block
COLERR_KS = D.EXACT_KS
COLERR_LOOP_CASES = (
    {"shape": (130, 133), "fast": False,                     # two column blocks, the second 5 wide; five chunks of one block
     "reach": {"rowblks_per_chunk": 1, "nchunks": 5, "ncolblk": 2, "last_chunk_blks": 1, "last_blk_rows": 2, "last_colblk_cols": 5}},
    {"shape": (8261, 133), "fast": False,                    # 259 row blocks > 256 chunks: two per chunk, the last chunk holds one of 5 rows
     "reach": {"rowblks_per_chunk": 2, "nchunks": 130, "ncolblk": 2, "last_chunk_blks": 1, "last_blk_rows": 5, "last_colblk_cols": 5}},
    {"shape": (8260, 132), "fast": True,                     # the same loops through the vector loads (16-byte rows)
     "reach": {"rowblks_per_chunk": 2, "nchunks": 130, "ncolblk": 2, "last_chunk_blks": 1, "last_blk_rows": 4, "last_colblk_cols": 4}},
)
COLERR_SHAPES = tuple(D.EXACT_SHAPES) + tuple(c["shape"] for c in COLERR_LOOP_CASES)


def colerr_reach(m, n, plan):
    d = dict(zip(("rowblks_per_chunk", "nchunks", "ncolblk"), (int(x) for x in plan)))
    nrowblk = -(-m // 32)
    d["last_chunk_blks"] = nrowblk - (d["nchunks"] - 1) * d["rowblks_per_chunk"]
    d["last_blk_rows"] = m - (nrowblk - 1) * 32
    d["last_colblk_cols"] = n - (d["ncolblk"] - 1) * 128
    return d


_COLERR = {}


def colerr_case(m, n, k):
    """(A, mask, W, H) with integer entries under the mask of tests/_masked_dense.py::_exact_mask (at least two columns without an
    observation).  The generator is `exact_problem` where its fp32 tile partials stay below 2^24 (the CPU proof asserts it), else
    `exact_problem_01` (model values 1..k); the tall shapes take the latter throughout.  Built once per process; no test writes to them."""
    key = (m, n, k)
    if key not in _COLERR:
        gen = D.exact_problem if (m, n) in D.EXACT_SHAPES and k <= 64 else D.exact_problem_01
        A, mask, W, H, _ = gen(m, n, k)
        mask = mask.copy()
        mask[:, 7] = False                                   # a second column without an observation (column 3 is the first)
        _COLERR[key] = (A, mask, W, H)
    return _COLERR[key]


def colerr_ref(A, mask, W, H):
    """float64 (num, den) over the observed positions"""
    A64, Dm = A.astype(np.float64), W.astype(np.float64) @ H.astype(np.float64)
    return (mask * (A64 - Dm) ** 2).sum(0), (mask * A64 * A64).sum(0)


def tile_partials(A, mask, W, H):
    """the largest fp32 partial of col_sums_kernel<KT, FAST, MaskedErrTerm>: per column, per 32-row block and per lane half h, the sums of (a - S)^2 and
    of a^2 over the observed ones of the 16 rows crow(r, h) = (r & 3) + 8 (r >> 2) + 4 h"""
    m, n = A.shape
    A64, Dm = A.astype(np.float64), W.astype(np.float64) @ H.astype(np.float64)
    E, Q = mask * (A64 - Dm) ** 2, mask * A64 * A64
    pad = (-m) % 32
    E, Q = np.pad(E, ((0, pad), (0, 0))), np.pad(Q, ((0, pad), (0, 0)))
    # rows of a block as [8 groups of 4]: even groups belong to h = 0, odd groups to h = 1
    E, Q = E.reshape(-1, 4, 2, 4, n), Q.reshape(-1, 4, 2, 4, n)
    return E.sum(axis=(1, 3)).max(), Q.sum(axis=(1, 3)).max()
