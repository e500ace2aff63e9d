"""Helpers for sparse data whose unstored entries are MISSING (TEST INFRASTRUCTURE, lives under tests/ only).

A numpy statement of the masked rules, written from the CSR arrays the way tests/_sparse.py::SparseOracleOps is written (nothing
is densified), in the dtype of the factors handed in (float64: the reference the tests compare with; float32: the reference's own
rounding error, `d_ref`).  With Omega the stored positions, d = <W[r], H[:, c]> and eps the float32 machine epsilon:

    fro:  W <- W * (sum_{c in Omega_r} a H[:, c]) / (sum_{c in Omega_r} d H[:, c] + eps)          (H alike, over Omega_c)
    kl:   W <- W * (sum_{c in Omega_r} a / (d + eps) H[:, c]) / (sum_{c in Omega_r} H[:, c] + eps)
    err:  ||P_Omega(A - W H)||_F / ||P_Omega(A)||_F   (both norms)

`MaskedOracleOps`: tests/_sparse.py::SparseOracleOps plus the masked operations of engine.HipCsrOps, so that the choreography of a
flagged block runs on the CPU.  `run_grid`: the ranks of a 1D grid as processes (gloo), each fitting its slice of one problem.
"""
import os
import traceback

import numpy as np
import torch

from tests._golden import load_case, rel_fro
from tests._ops_double import _n
from tests._sparse import SparseOracleOps, _csr

EPS = float(np.finfo(np.float32).eps)


# ---- the rules
def pair(rows, col, val, nrows, L, F, eps, norm):
    """(num, den) [nrows x k] of one side: `rows` / `col` name the stored entries, L [nrows x k] is the factor being updated, F
    [ncols x k] the other one.  The transpose's side: swap `rows` and `col`."""
    dt = L.dtype
    val = val.astype(dt)
    Fc = F[col]
    d = np.einsum("ij,ij->i", L[rows], Fc)
    num, den = np.zeros((nrows, L.shape[1]), dtype=dt), np.zeros((nrows, L.shape[1]), dtype=dt)
    if norm == "kl":
        np.add.at(num, rows, (val / (d + dt.type(eps)))[:, None] * Fc)
        np.add.at(den, rows, Fc)
    else:
        np.add.at(num, rows, val[:, None] * Fc)
        np.add.at(den, rows, d[:, None] * Fc)
    return num, den


def resid(rows, col, val, W, H):
    """sum over the stored positions of (a - d)^2, float64"""
    d = np.einsum("ij,ij->i", W.astype(np.float64)[rows], H.astype(np.float64).T[col])
    return float(np.sum((val.astype(np.float64) - d) ** 2))


def step(csr, shape, W, H, norm, eps=EPS, W_update=True, clamp=False):
    """one MU step in the dtype of W (new arrays): W first, then H with the new W, then the clamp of pyDNMF.py:170-172"""
    rows, col, val = csr
    dt = W.dtype
    e = dt.type(eps)
    W, H = W.copy(), H.astype(dt).copy()
    if W_update:
        num, den = pair(rows, col, val, shape[0], W, np.ascontiguousarray(H.T), eps, norm)
        W = W * (num / (den + e))
    num, den = pair(col, rows, val, shape[1], np.ascontiguousarray(H.T), W, eps, norm)
    H = H * (num / (den + e)).T
    if clamp:
        H, W = np.maximum(H, e), np.maximum(W, e)
    return W, H


def iterate(csr, shape, W, H, itr, norm, eps=EPS, W_update=True):
    """`itr` steps with the clamp after the steps i % 10 == 0 (pyDNMF.py:138-182 without its last lines)"""
    for i in range(itr):
        W, H = step(csr, shape, W, H, norm, eps, W_update, clamp=(i % 10 == 0))
    return W, H


def fit(csr, shape, W0, H0, itr, norm, eps=EPS, W_update=True, dtype=np.float64):
    """PyNMF.fit of a flagged block: the steps, normalize_features (pyDNMF.py:185-194), the masked relative error"""
    rows, col, val = csr
    W, H = iterate(csr, shape, W0.astype(dtype), H0.astype(dtype), itr, norm, eps, W_update)
    s = W.sum(axis=0)
    W = W / (s + W.dtype.type(eps))
    H = H * s[:, None]
    den = float(np.sum(val.astype(np.float64) ** 2))
    return W, H, float(np.sqrt(resid(rows, col, val, W, H)) / np.sqrt(den))


def coo_of(S):
    """(rows, col, val) of a scipy sparse matrix in CSR order, explicit zeros kept, duplicates summed"""
    c = S.tocsr().copy()
    c.sum_duplicates()
    c.sort_indices()
    rows = np.repeat(np.arange(c.shape[0]), np.diff(c.indptr))
    return rows.astype(np.int64), c.indices.astype(np.int64), c.data.astype(np.float32)


def full_csr(A):
    """the dense block with EVERY position stored, its zeros as explicit entries"""
    import scipy.sparse as sp
    m, n = A.shape
    return sp.csr_matrix((np.ascontiguousarray(A, dtype=np.float32).ravel(), np.tile(np.arange(n), m), np.arange(0, m * n + 1, n)), shape=(m, n))


def observed(A, mask):
    """the entries of A where `mask` holds as a scipy CSR matrix; zeros of A under the mask are explicit entries"""
    import scipy.sparse as sp
    r, c = np.nonzero(mask)
    return sp.csr_matrix(sp.coo_matrix((A[r, c].astype(np.float32), (r, c)), shape=A.shape))


# ---- the operator set
class MaskedOracleOps(SparseOracleOps):
    name = "oracle-sparse-masked"

    @staticmethod
    def _sides(A, W, H, transposed):
        rows, col, val = _csr(A)
        W64, HT64 = _n(W).astype(np.float64), np.ascontiguousarray(_n(H).astype(np.float64).T)
        if transposed:
            return col, rows, val, A.shape[1], HT64, W64
        return rows, col, val, A.shape[0], W64, HT64

    def _pair(self, A, W, H, eps, norm, transposed):
        rows, col, val, nrows, L, F = self._sides(A, W, H, transposed)
        num, den = pair(rows, col, val, nrows, L, F, float(np.float32(eps)), str(norm).lower())
        if transposed:
            num, den = num.T, den.T
        return num.astype(np.float32), den.astype(np.float32)

    @staticmethod
    def _halves(buf, shape):
        r, c = shape
        assert buf.is_contiguous() and buf.numel() >= 2 * r * c
        return buf[: r * c].view(r, c), buf[r * c: 2 * r * c].view(r, c)

    def masked_aht_pair(self, A, W, H, eps, norm, buf):
        num, den = self._halves(buf, tuple(W.shape))
        a, b = self._pair(A, W, H, eps, norm, False)
        num.copy_(torch.from_numpy(a))
        den.copy_(torch.from_numpy(b))
        return num, den

    def masked_wta_pair(self, A, W, H, eps, norm, buf):
        num, den = self._halves(buf, tuple(H.shape))
        a, b = self._pair(A, W, H, eps, norm, True)
        num.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        den.copy_(torch.from_numpy(np.ascontiguousarray(b)))
        return num, den

    def ratio_update(self, X, num, den, eps, clamp=False):
        x = _n(X)
        x *= _n(num) / (_n(den) + np.float32(eps))
        if clamp:
            np.maximum(x, np.float32(eps), out=x)
        return X

    def masked_update_w(self, A, W, H, eps, norm):
        a, b = self._pair(A, W, H, eps, norm, False)
        return self.ratio_update(W, torch.from_numpy(a), torch.from_numpy(b), eps)

    def masked_update_h(self, A, W, H, eps, norm, clamp=False):
        a, b = self._pair(A, W, H, eps, norm, True)
        return self.ratio_update(H, torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)), eps, clamp)

    def resid_sqnorm(self, A, W, H):
        if not (self._sp(A) and getattr(A, "missing", None) == "unstored"):
            return super().resid_sqnorm(A, W, H)
        rows, col, val = _csr(A)
        return torch.tensor([resid(rows, col, val, _n(W), _n(H))], dtype=torch.float64)


# ---- problems
def args_for(comms, p_r, p_c, k, itr, norm, W_update=True, prune=False, missing="unstored", method="mu"):
    from pydnmfk_amd.utils import parse
    args = parse()
    args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, p_r, p_c, k
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    args.itr, args.init, args.verbose, args.prune = itr, "rand", False, prune
    args.norm, args.method, args.W_update = norm, method, W_update
    if missing is not None:
        args.missing = missing
    return args


def small_problem():
    """24 x 12, about 40 % stored, row 5 and column 7 without an observation, a few stored zeros; k = 3"""
    rs = np.random.RandomState(24)
    m, n, k = 24, 12, 3
    A = (rs.rand(m, k) @ rs.rand(k, n) + 0.05).astype(np.float32)
    mask = rs.rand(m, n) < 0.4
    mask[5, :] = False
    mask[:, 7] = False
    for r, c in ((0, 0), (3, 9), (11, 2), (23, 11)):
        mask[r, c] = True
        A[r, c] = 0.0
    W0, H0 = rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)
    return A, mask, W0, H0, k


GRID_COMBOS = tuple((norm, wu) for norm in ("fro", "kl") for wu in (True, False))
GRID_ITR = 20


def _grid_rank(rank, world, port, grid, q, use_hip):
    try:
        import torch.distributed as dist
        from oracle import nmf_oracle as orc
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        from pydnmfk_amd.utils import determine_block_params
        if use_hip:
            torch.cuda.set_device(0)
        ops = None if use_hip else MaskedOracleOps()
        if world > 1:
            torch.set_num_threads(1)
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        A, mask, W0, H0, k = small_problem()
        p_r, p_c = grid
        comms = MPI_comm(None, p_r, p_c)
        s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
        (w0, w1), (h0, h1) = orc.factor_ranges(rank, p_r, p_c, A.shape[0], A.shape[1])
        sl = (slice(s[0], e[0] + 1), slice(s[1], e[1] + 1))
        out = {}
        for norm, wu in GRID_COMBOS:
            nmf = PyNMF(observed(A[sl], mask[sl]), factors=[W0[w0:w1], H0[:, h0:h1]], params=args_for(comms, p_r, p_c, k, GRID_ITR, norm, wu),
                        ops=ops)
            assert nmf.A_ij.missing == "unstored" and nmf.A_ij.nnz == int(mask[sl].sum())
            assert nmf._ops().name == ("hip-csr" if use_hip else "oracle-sparse-masked")
            W, H, err = nmf.fit()
            out[(norm, wu)] = ((w0, w1), (h0, h1), np.asarray(W), np.asarray(H), float(err))
        q.put((rank, out, None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_grid(grid, use_hip=False, timeout=240):
    """{(norm, W_update): (W, H, err)} of the 20-iteration masked fits of small_problem() on the grid, assembled from the ranks
    (a replicated factor and the error must agree between the ranks bit for bit)"""
    import queue
    world = grid[0] * grid[1]
    if world == 1:
        q = queue.Queue()
        _grid_rank(0, 1, 0, grid, q, use_hip)
        res = [q.get()]
    else:
        import torch.multiprocessing as mp
        from tests._mp import free_port
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = free_port()
        procs = [ctx.Process(target=_grid_rank, args=(r, world, port, grid, q, use_hip)) for r in range(world)]
        for p in procs:
            p.start()
        res = [q.get(timeout=timeout) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    for rank, out, err in res:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
    A = small_problem()[0]
    k = small_problem()[4]
    full = {}
    for combo in GRID_COMBOS:
        W, H = np.full((A.shape[0], k), np.nan, dtype=np.float32), np.full((k, A.shape[1]), np.nan, dtype=np.float32)
        errs = set()
        for rank, out, _ in res:
            (w0, w1), (h0, h1), Wr, Hr, err = out[combo]
            for dst, src in ((W[w0:w1], Wr), (H[:, h0:h1], Hr)):
                assert np.isnan(dst).all() or np.array_equal(dst, src), (grid, combo, rank)      # replicated: identical on every rank
                dst[...] = src
            errs.add(err)
        assert len(errs) == 1 and np.isfinite(W).all() and np.isfinite(H).all(), (grid, combo, errs)
        full[combo] = (W, H, errs.pop())
    return full


def reference_fits():
    """the one-rank float64 fits of small_problem() from the rules above: {(norm, W_update): (W, H, err)}"""
    A, mask, W0, H0, k = small_problem()
    csr = coo_of(observed(A, mask))
    return {(norm, wu): fit(csr, A.shape, W0, H0, GRID_ITR, norm, W_update=wu) for norm, wu in GRID_COMBOS}


# ---- a golden of the reference on a FULLY STORED block: there the masked rules are the reference's rules up to summation order
FULL_GOLDENS = ("t24x12_1x1_fro_float32", "t24x12_1x1_kl_float32", "swim_1x1_fro_float32")


def full_case(name, ops):
    """What tests/_mp.py::run_case_rank records for a one-rank case -- {"step1" / itr: (rel W, rel H, |d err|)} -- with the block
    handed to PyNMF fully stored (explicit zeros included) under params.missing = 'unstored'; `ops` None: the HIP kernels."""
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    meta, A, W0, H0, z = load_case(name)
    assert meta["grid"] == [1, 1] and not meta.get("prune", False) and meta.get("method", "mu") == "mu"
    comms = MPI_comm(None, 1, 1)
    S = full_csr(A)
    out = {}
    nmf = PyNMF(S, factors=[W0, H0], params=args_for(comms, 1, 1, meta["k"], 1, meta["norm"], meta["W_update"]), ops=ops)
    assert nmf.A_ij.missing == "unstored" and nmf.A_ij.nnz == A.size
    W1, H1 = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update()
    out["step1"] = (rel_fro(W1.cpu().numpy(), z["r0_step1_W"]), rel_fro(H1.cpu().numpy(), z["r0_step1_H"]), 0.0)
    for itr in meta["itrs"]:
        W, H, err = PyNMF(S, factors=[W0, H0], params=args_for(comms, 1, 1, meta["k"], itr, meta["norm"], meta["W_update"]), ops=ops).fit()
        out[itr] = (rel_fro(W, z["r0_fit%d_W" % itr]), rel_fro(H, z["r0_fit%d_H" % itr]), abs(err - float(z["r0_fit%d_err" % itr])))
    return out
