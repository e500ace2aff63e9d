"""Sparse-data test helpers (TEST INFRASTRUCTURE, lives under tests/ only).

`SparseOracleOps`: the checker back end of tests/_ops_double.py with the eight operations that touch the data block
implemented FROM THE CSR ARRAYS of a pydnmfk_amd.sparse.SparseBlock in numpy / float64 (nothing is densified), so the
sparse choreography runs under gloo without a GPU.  `run_case_rank_sparse`: the twin of tests/_mp.py::run_case_rank -- the
same case, the same assertions, the rank's block converted to a sparse object just before PyNMF.  `run_case_sparse` runs
tests/_mp.py::run_case itself (its process handling AND its tolerance table) with that twin as the rank function.
"""
import os
import traceback

import numpy as np
import torch

from tests._golden import load_case, rel_fro
from tests._ops_double import OracleOps, _n


def _csr(A):
    crow, col, val = A.crow.cpu().numpy().astype(np.int64), A.col.cpu().numpy().astype(np.int64), A.val.cpu().numpy().astype(np.float64)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(crow))
    return rows, col, val


def csr_mm64(rows, col, val, nrows, F):
    """out[r] = sum over the stored entries of row r of val * F[col]   (float64; F [ncols x k])"""
    out = np.zeros((nrows, F.shape[1]), dtype=np.float64)
    np.add.at(out, rows, val[:, None] * F[col])
    return out


def csr_kl64(rows, col, val, nrows, L, F, eps):
    d = np.einsum("ij,ij->i", L[rows], F[col])
    return csr_mm64(rows, col, val / (d + eps), nrows, F)


def csr_resid64(rows, col, val, W, H):
    """||A - W H||^2 from the stored entries and the Gram term (float64)"""
    W, HT = W.astype(np.float64), H.astype(np.float64).T
    d = np.einsum("ij,ij->i", W[rows], HT[col])
    return float(np.sum(val * (val - 2.0 * d)) + np.sum((W.T @ W) * (HT.T @ HT)))


class SparseOracleOps(OracleOps):
    name = "oracle-sparse"

    @staticmethod
    def _sp(A):
        return getattr(A, "is_sparse_block", False)

    def aht(self, A, H, out):
        if not self._sp(A):
            return super().aht(A, H, out)
        rows, col, val = _csr(A)
        out.copy_(torch.from_numpy(csr_mm64(rows, col, val, A.shape[0], _n(H).astype(np.float64).T).astype(np.float32)))
        return out

    def wta(self, A, W, out):
        if not self._sp(A):
            return super().wta(A, W, out)
        rows, col, val = _csr(A)
        out.copy_(torch.from_numpy(csr_mm64(col, rows, val, A.shape[1], _n(W).astype(np.float64)).T.astype(np.float32)))
        return out

    def wta_gram(self, A, W, out, G):
        self.gram_wtw(W, G)
        return self.wta(A, W, out)

    def aht_update_w(self, A, H, G, W, eps):
        if not self._sp(A):
            return super().aht_update_w(A, H, G, W, eps)
        AH = torch.empty(W.shape, dtype=torch.float32)
        self.aht(A, H, AH)
        self.mu_update_w(W, AH, G, eps)

    def kl_uht(self, A, W, H, eps, out):
        if not self._sp(A):
            return super().kl_uht(A, W, H, eps, out)
        rows, col, val = _csr(A)
        r = csr_kl64(rows, col, val, A.shape[0], _n(W).astype(np.float64), _n(H).astype(np.float64).T, float(np.float32(eps)))
        out.copy_(torch.from_numpy(r.astype(np.float32)))
        return out

    def kl_wtu(self, A, W, H, eps, out):
        if not self._sp(A):
            return super().kl_wtu(A, W, H, eps, out)
        rows, col, val = _csr(A)
        r = csr_kl64(col, rows, val, A.shape[1], _n(H).astype(np.float64).T, _n(W).astype(np.float64), float(np.float32(eps)))
        out.copy_(torch.from_numpy(r.T.astype(np.float32)))
        return out

    def sqnorm(self, A):
        if not self._sp(A):
            return super().sqnorm(A)
        return torch.tensor([float(np.sum(A.val.cpu().numpy().astype(np.float64) ** 2))], dtype=torch.float64)

    def resid_sqnorm(self, A, W, H):
        if not self._sp(A):
            return super().resid_sqnorm(A, W, H)
        rows, col, val = _csr(A)
        return torch.tensor([max(csr_resid64(rows, col, val, _n(W), _n(H)), 0.0)], dtype=torch.float64)


def to_sparse(A, kind="scipy_csr"):
    """The dense float32 numpy block as a sparse object of the given kind."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    if kind.startswith("scipy"):
        import scipy.sparse as sp
        return {"scipy_csr": sp.csr_matrix, "scipy_csc": sp.csc_matrix, "scipy_coo": sp.coo_matrix}[kind](A)
    t = torch.from_numpy(A)
    return t.to_sparse_csr() if kind == "torch_csr" else t.to_sparse()


def _case_on_rank(rank, name, ops, use_hip, extra=None):
    """What tests/_mp.py::run_case_rank does for one case on one rank, the rank's block handed to PyNMF as
    scipy.sparse.csr_matrix: {"step1" / itr: (rel W, rel H, |d err|)}"""
    from oracle import nmf_oracle as orc
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMF import PyNMF
    from pydnmfk_amd.utils import determine_block_params, parse

    meta, A, W0, H0, z = load_case(name)
    p_r, p_c = meta["grid"]
    comms = MPI_comm(None, p_r, p_c)
    out = {}

    def bag(itr, prune):
        args = parse()
        args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, p_r, p_c, meta["k"]
        args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
        args.itr, args.init, args.verbose, args.prune = itr, "rand", False, prune
        args.norm, args.method, args.W_update = meta["norm"], meta.get("method", "mu"), meta["W_update"]
        for key, val in (extra or {}).items():
            setattr(args, key, val)
        return args

    s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
    (w0, w1), (h0, h1) = orc.factor_ranges(rank, p_r, p_c, meta["m"], meta["n"])
    A_ij = A[s[0]:e[0] + 1, s[1]:e[1] + 1]
    if not meta.get("prune", False):
        from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
        nmf = PyNMF(to_sparse(A_ij), factors=[W0[w0:w1], H0[:, h0:h1]], params=bag(1, False), ops=ops)
        assert nmf.A_ij.is_sparse_block and nmf._ops().name == ("hip-csr" if use_hip else "oracle-sparse")
        W1, H1 = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update()
        out["step1"] = (rel_fro(W1.cpu().numpy(), z["r%d_step1_W" % rank]), rel_fro(H1.cpu().numpy(), z["r%d_step1_H" % rank]), 0.0)
        print("sparse %s rank %d step1: dW=%.2e dH=%.2e" % (name, rank, out["step1"][0], out["step1"][1]), flush=True)
    for itr in meta["itrs"]:
        args = bag(itr, meta.get("prune", False))
        assert [s[0], e[0] + 1, s[1], e[1] + 1] == list(z["r%d_A_range" % rank])
        W, H, err = PyNMF(to_sparse(A_ij), factors=[W0[w0:w1], H0[:, h0:h1]], params=args, ops=ops).fit()
        assert (args.m, args.n) == (meta["m"], meta["n"])
        assert [args.m_loc, args.n_loc] == list(z["r%d_m_loc_n_loc" % rank])
        assert tuple(W.shape) == z["r%d_fit%d_W" % (rank, itr)].shape
        assert W.dtype == z["r%d_fit%d_W" % (rank, itr)].dtype and H.dtype == z["r%d_fit%d_H" % (rank, itr)].dtype
        out[itr] = (rel_fro(W, z["r%d_fit%d_W" % (rank, itr)]), rel_fro(H, z["r%d_fit%d_H" % (rank, itr)]),
                    abs(err - float(z["r0_fit%d_err" % itr])))
        print("sparse %s rank %d fit%s: dW=%.2e dH=%.2e derr=%.2e (err %.6g)" % (name, rank, itr, *out[itr], err), flush=True)
    return out


def run_case_rank_sparse(rank, world, port, name, q, use_hip, extra=None):
    """the sparse twin of tests/_mp.py::run_case_rank; `name` may be a tuple of cases of the same world size, which then share
    the processes (and their start-up): the result is {name: out} in that case"""
    try:
        import torch.distributed as dist
        torch.set_num_threads(1)
        if use_hip:
            torch.cuda.set_device(0)
            ops = None                      # product default for a sparse block: the HIP CSR kernels
        else:
            ops = SparseOracleOps()
        if world > 1:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        if isinstance(name, (tuple, list)):
            out = {nm: _case_on_rank(rank, nm, ops, use_hip, extra) for nm in name}
        else:
            out = _case_on_rank(rank, name, ops, use_hip, extra)
        q.put((rank, out, None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_case_sparse(name, use_hip=False, timeout=240, extra=None, tols=None):
    """tests/_mp.py::run_case -- its spawning, its per-case tolerance table -- over the sparse rank function"""
    from tests import _mp
    dense = _mp.run_case_rank
    _mp.run_case_rank = run_case_rank_sparse
    try:
        _mp.run_case(name, use_hip=use_hip, timeout=timeout, extra=extra, tols=tols)
    finally:
        _mp.run_case_rank = dense


def run_cases_sparse_shared(names, use_hip=True, timeout=400):
    """Several cases of ONE world size on one set of rank processes (a GPU process costs seconds to start): returns
    {name: [(rank, out, None), ...]}, to be judged by `judge_with_run_case`."""
    import torch.multiprocessing as mp
    from tests._mp import free_port
    worlds = {load_case(nm)[0]["grid"][0] * load_case(nm)[0]["grid"][1] for nm in names}
    assert len(worlds) == 1, worlds
    world = worlds.pop()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run_case_rank_sparse, args=(r, world, port, tuple(names), q, use_hip, None)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=timeout) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, out, err in res:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
    return {nm: [(rank, out[nm], None) for rank, out, _ in res] for nm in names}


class _Replay:
    """stands in for the multiprocessing context inside tests/_mp.py::run_case: its 'processes' hand over results that were
    computed before, so that run_case's own loop and tolerance table judge them"""

    def __init__(self, results):
        self.results = list(results)

    def get_context(self, _method):
        return self

    def Queue(self):
        import queue
        return _ReplayQueue(queue.Queue())

    def Process(self, target=None, args=()):
        rank, q = args[0], args[4]
        return _ReplayProc(q, [r for r in self.results if r[0] == rank][0])


class _ReplayQueue:
    def __init__(self, q):
        self.q = q

    def put(self, x):
        self.q.put(x)

    def get(self, timeout=None):
        return self.q.get(timeout=timeout)


class _ReplayProc:
    def __init__(self, q, item):
        self.q, self.item = q, item

    def start(self):
        self.q.put(self.item)

    def join(self, timeout=None):
        pass


def regression_tols(name):
    """`tols` for run_case on a W_update=False HALS golden.  run_case is applied to no such case on dense data and its absolute
    1e-5 on the error cannot hold there: W stays random, the relative error is ~73, and numpy's own float32 evaluation of
    ||A - W H|| / ||A|| from the golden's recorded factors differs from the golden's recorded error by 6.0e-4 (8e-6
    relative: a float32 dot product over 262144 terms on another machine).  The bound is therefore the row tests/test_gpu_parity.py::_tols
    has for this case, applied as that file applies it (relative to max(1, |err|)); step and fit bounds are that row's too."""
    from tests.test_gpu_parity import _tols
    meta, _, _, _, z = load_case(name)
    assert meta.get("method") == "hals" and not meta["W_update"]
    step, fit, err = _tols(meta)
    ref = max(abs(float(z["r0_fit%d_err" % itr])) for itr in meta["itrs"])
    return step, fit, err * max(1.0, ref)


def judge_with_run_case(name, results):
    """tests/_mp.py::run_case's assertions (its tolerance table, not a copy) over `results` = [(rank, out, None), ...]"""
    from tests import _mp
    real = _mp.mp
    _mp.mp = _Replay(results)
    try:
        _mp.run_case(name)
    finally:
        _mp.mp = real
