"""NMFk over sparse data: test helpers (TEST INFRASTRUCTURE, lives under tests/ only).

`SparseNmfkOracleOps`: the sparse and masked checker back ends (tests/_sparse.py, tests/_masked.py) plus what an NMFk sweep asks of
an operator set beyond a fit -- the per-column error sums of a CSR block in float64 numpy, under both meanings of an unstored
entry -- and the capability flag PyNMFk looks for.  It has no perturbed copy of its own: its blocks live on the CPU, where
`sample` reproduces the reference's numpy stream.  `run_nmfk_golden_sparse`: tests/_mp.py::run_nmfk_golden with the rank's block
handed to PyNMFk as scipy.sparse.csr_matrix.
"""
import os
import traceback

import numpy as np
import torch

from tests._masked import MaskedOracleOps
from tests._ops_double import _n
from tests._sparse import _csr


def column_err_sums64(rows, col, val, n, W, H, masked):
    """(num, den) per column, float64: sum_r (a - d)^2 and sum_r a^2 over ALL rows r (zero meaning: an unstored entry is a zero that
    W H must reproduce, so num = sum_stored a (a - 2 d) + h_c^T (W^T W) h_c) or over the stored positions only (masked)"""
    W64, H64 = W.astype(np.float64), H.astype(np.float64)
    d = np.einsum("ij,ji->i", W64[rows], H64[:, col])
    num, den = np.zeros(n), np.zeros(n)
    np.add.at(den, col, val * val)
    if masked:
        np.add.at(num, col, (val - d) ** 2)
    else:
        np.add.at(num, col, val * (val - 2.0 * d))
        num += np.einsum("ic,ij,jc->c", H64, W64.T @ W64, H64)
    return num, den


class SparseNmfkOracleOps(MaskedOracleOps):
    name = "oracle-sparse-nmfk"
    sparse_nmfk = True

    def column_err_sums(self, A, W, H):
        if not self._sp(A):
            return super().column_err_sums(A, W, H)
        rows, col, val = _csr(A)
        num, den = column_err_sums64(rows, col, val, A.shape[1], _n(W), _n(H), getattr(A, "missing", None) == "unstored")
        return torch.from_numpy(num), torch.from_numpy(den)


def full_scipy(A):
    """the dense block as scipy CSR, with the precondition that EVERY position is stored (no zero in A)"""
    import scipy.sparse as sp
    S = sp.csr_matrix(np.ascontiguousarray(A, dtype=np.float32))
    assert S.nnz == A.size, "the fixture's A has zeros: %d of %d positions stored" % (S.nnz, A.size)
    return S


def run_nmfk_golden_sparse_rank(rank, world, port, fixture, q, use_hip, extra):
    """tests/_mp.py::run_nmfk_golden_rank with the rank's block as scipy.sparse.csr_matrix (numpy I/O: the reference's numpy
    stream) and, without a GPU, the operator set above"""
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
            ops = None
        else:
            ops = SparseNmfkOracleOps()
        if world > 1:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        z = np.load(os.path.join(GOLDEN, fixture))
        meta = json.loads(str(z["meta"]))
        A = z["A"]
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
        for key, val in (extra or {}).items():
            setattr(args, key, val)
        s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
        S_ij = full_scipy(A[s[0]:e[0] + 1, s[1]:e[1] + 1])
        nmfk = PyNMFk(S_ij, factors=None, params=args, ops=ops)
        assert nmfk.A_ij.is_sparse_block and nmfk.sweep.numpy_io
        nopt = nmfk.fit()
        stats = {k: {key: np.asarray(val) for key, val in st.items()} for k, st in nmfk.stats.items()}
        q.put((rank, (int(nopt), stats), None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_nmfk_golden_sparse(fixture, use_hip=False, timeout=600, extra=None):
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
    procs = [ctx.Process(target=run_nmfk_golden_sparse_rank, args=(r, world, port, fixture, q, use_hip, extra)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(procs, q, timeout)
    for rank, out, err in res:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
    return [out for _, out, _ in sorted(res, key=lambda r: r[0])]
