"""Helpers for DENSE data whose missing entries are NaN, `params.missing = 'nan'` (TEST INFRASTRUCTURE, lives under tests/ only).

The rules are those of tests/_masked.py (`pair`, `resid`, `step`, `iterate`, `fit`: a float64 numpy statement over the observed
entries in COO form); this file only carries them over to the dense block: `nan_marked` writes NaN where a mask is false,
`MaskedDenseOracleOps` is the checker operator set of a pydnmfk_amd.masked.MaskedDenseBlock (so the choreography of the block runs on
the CPU and under gloo), `run_grid` runs the ranks of a 1D grid as processes, `exact_problem` builds the exact-by-construction
operands of tests/_exact.py::products under a mask.
"""
import os
import traceback

import numpy as np
import torch

from tests import _exact as E
from tests import _masked as M
from tests._ops_double import _n

EPS = M.EPS


def nan_marked(A, mask):
    """A (float32) with NaN at the positions where `mask` is false"""
    out = np.array(A, dtype=np.float32, copy=True)
    out[~np.asarray(mask, dtype=bool)] = np.nan
    return out


def coo_of_dense(T):
    """(rows, col, val) of the observed (non-NaN) entries of a dense block in row-major order; zeros are observations"""
    T = np.asarray(T)
    r, c = np.nonzero(~np.isnan(T))
    return r.astype(np.int64), c.astype(np.int64), T[r, c].astype(np.float32)


class MaskedDenseOracleOps(M.MaskedOracleOps):
    """tests/_masked.py::MaskedOracleOps for a MaskedDenseBlock: the observed entries in COO form, `pair` / `resid` in float64.  Every
    operation that would read the block as numbers refuses it: the choreography must keep off them."""

    name = "oracle-masked-dense"

    @staticmethod
    def _blk(A):
        return getattr(A, "is_masked_dense", False)

    @staticmethod
    def _coo(A):
        rows, col, val = coo_of_dense(A.tensor.cpu().numpy())
        return rows, col, val.astype(np.float64)

    @staticmethod
    def _sides(A, W, H, transposed):
        assert getattr(A, "is_masked_dense", False) and A.missing == "nan"
        rows, col, val = MaskedDenseOracleOps._coo(A)
        W64, HT64 = _n(W).astype(np.float64), np.ascontiguousarray(_n(H).astype(np.float64).T)
        if transposed:
            return col, rows, val, A.shape[1], HT64, W64
        return rows, col, val, A.shape[0], W64, HT64

    def sqnorm(self, A):
        if not self._blk(A):
            return super().sqnorm(A)
        return torch.tensor([float(np.sum(self._coo(A)[2] ** 2))], dtype=torch.float64)

    def resid_sqnorm(self, A, W, H):
        if not self._blk(A):
            return super().resid_sqnorm(A, W, H)
        rows, col, val = self._coo(A)
        return torch.tensor([M.resid(rows, col, val, _n(W), _n(H))], dtype=torch.float64)

    def _keep_off(self, what, A):
        assert not self._blk(A), "%s was handed the NaN-marked block: it would read the NaNs as data" % what


def _guard(name):
    def method(self, A, *args, **kwargs):
        self._keep_off(name, A)
        return getattr(M.MaskedOracleOps, name)(self, A, *args, **kwargs)
    method.__name__ = name
    return method


for _name in ("aht", "wta", "wta_gram", "aht_update_w", "kl_uht", "kl_wtu", "column_err_sums"):
    setattr(MaskedDenseOracleOps, _name, _guard(_name))


def args_for(comms, p_r, p_c, k, itr, norm, W_update=True, prune=False, missing="nan", method="mu"):
    return M.args_for(comms, p_r, p_c, k, itr, norm, W_update=W_update, prune=prune, missing=missing, method=method)


# ---- 1D grids: the ranks as processes, each fitting its slice of tests/_masked.py::small_problem() with NaN for the mask
def _grid_rank(rank, world, port, grid, q, use_hip):
    try:
        import torch.distributed as dist
        from oracle import nmf_oracle as orc
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        from pydnmfk_amd.utils import determine_block_params
        if use_hip:
            torch.cuda.set_device(0)
        ops = None if use_hip else MaskedDenseOracleOps()
        if world > 1:
            torch.set_num_threads(1)
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        A, mask, W0, H0, k = M.small_problem()
        p_r, p_c = grid
        comms = MPI_comm(None, p_r, p_c)
        s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
        (w0, w1), (h0, h1) = orc.factor_ranges(rank, p_r, p_c, A.shape[0], A.shape[1])
        sl = (slice(s[0], e[0] + 1), slice(s[1], e[1] + 1))
        out = {}
        for norm, wu in M.GRID_COMBOS:
            nmf = PyNMF(nan_marked(A[sl], mask[sl]), factors=[W0[w0:w1], H0[:, h0:h1]],
                        params=args_for(comms, p_r, p_c, k, M.GRID_ITR, norm, wu), ops=ops)
            assert nmf.A_ij.is_masked_dense and nmf.A_ij.missing == "nan" and nmf.A_ij.n_observed == int(mask[sl].sum())
            assert nmf._ops().name == ("hip-masked" if use_hip else "oracle-masked-dense")
            W, H, err = nmf.fit()
            out[(norm, wu)] = ((w0, w1), (h0, h1), np.asarray(W), np.asarray(H), float(err))
        q.put((rank, out, None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_grid(grid, use_hip=False, timeout=240):
    """{(norm, W_update): (W, H, err)} of the 20-iteration fits of small_problem() with NaN for its mask, assembled from the ranks
    (a replicated factor and the error must agree between the ranks bit for bit); every rank process has its own time limit"""
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
        try:
            res = [q.get(timeout=timeout) for _ in procs]
            for p in procs:
                p.join(timeout=60)
        finally:
            for p in procs:
                if p.is_alive():
                    p.kill()
    for rank, out, err in res:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
    A, _, _, _, k = M.small_problem()
    full = {}
    for combo in M.GRID_COMBOS:
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


# ---- a golden of the reference on a block WITHOUT a NaN: there the masked rules are the reference's rules up to summation order
def full_case(name, ops):
    """tests/_masked.py::full_case with the block handed over dense, without a NaN, under params.missing = 'nan'"""
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests._golden import load_case, rel_fro
    meta, A, W0, H0, z = load_case(name)
    assert meta["grid"] == [1, 1] and not meta.get("prune", False) and meta.get("method", "mu") == "mu"
    A = np.ascontiguousarray(A, dtype=np.float32)
    assert not np.isnan(A).any()
    comms = MPI_comm(None, 1, 1)
    out = {}
    nmf = PyNMF(A, factors=[W0, H0], params=args_for(comms, 1, 1, meta["k"], 1, meta["norm"], meta["W_update"]), ops=ops)
    assert nmf.A_ij.missing == "nan" and nmf.A_ij.n_observed == A.size
    W1, H1 = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update()
    out["step1"] = (rel_fro(W1.cpu().numpy(), z["r0_step1_W"]), rel_fro(H1.cpu().numpy(), z["r0_step1_H"]), 0.0)
    for itr in meta["itrs"]:
        W, H, err = PyNMF(A, factors=[W0, H0], params=args_for(comms, 1, 1, meta["k"], itr, meta["norm"], meta["W_update"]), ops=ops).fit()
        out[itr] = (rel_fro(W, z["r0_fit%d_W" % itr]), rel_fro(H, z["r0_fit%d_H" % itr]), abs(err - float(z["r0_fit%d_err" % itr])))
    return out


# ---- exact operands under a mask
EXACT_SHAPES = ((130, 97), (257, 70), (132, 96))          # (the third: rows and ranks of whole 16-byte vectors, the FAST kernels)
EXACT_KS = (3, 32, 64, 128)


def _exact_mask(rs, m, n):
    """a 50 % mask in which rows 5, 64, m - 1 and columns 9, 40, n - 1 keep exactly ONE observation (where a sum is a single term) and
    row 2 and column 3 keep none"""
    mask = rs.rand(m, n) < 0.5
    mask[2, :] = False                                                   # no observation at all
    mask[:, 3] = False
    for r in (5, 64, m - 1):                                             # exactly one observation in the row
        mask[r, :] = False
        mask[r, rs.randint(4, n)] = True
    for c in (9, 40, n - 1):
        keep = mask[[5, 64, m - 1], c].copy()
        mask[:, c] = False
        mask[[5, 64, m - 1], c] = keep                                   # (the single-observation rows stay as they are)
        free = [r for r in range(m) if r not in (2, 5, 64, m - 1)]
        if not keep.any():
            mask[free[rs.randint(len(free))], c] = True
    return mask


def _exact_ref(A, mask, W, H):
    """the float64 answers of the masked pairs: the four `fro` arrays, the `kl` numerators (float64 quotient sums) and denominators,
    the unmasked `fro` sums (which bound the masked ones: all terms are non-negative) and the observation counts per row and column"""
    A64, W64, H64, Mk = A.astype(np.float64), W.astype(np.float64), H.astype(np.float64), mask.astype(np.float64)
    D = W64 @ H64
    PA, PD = Mk * A64, Mk * D
    Q = Mk * A64 / (D + EPS)
    return {"fro": (PA @ H64.T, PD @ H64.T, W64.T @ PA, W64.T @ PD), "kl": (Q @ H64.T, Mk @ H64.T, W64.T @ Q, W64.T @ Mk),
            "unmasked_fro": (A64 @ H64.T, D @ H64.T, W64.T @ A64, W64.T @ D), "row_obs": mask.sum(1), "col_obs": mask.sum(0)}


def exact_problem(m, n, k):
    """tests/_exact.py::products(m, n, k) -- A in 0..7, W and H in 0..3, every unmasked product an integer below 2^24 -- under the mask
    of `_exact_mask`.  Returns A, mask, W, H and the float64 answers of `_exact_ref`."""
    A, W, H = E.products(m, n, k)
    mask = _exact_mask(np.random.RandomState(7 * m + n + k), m, n)
    return A, mask, W, H, _exact_ref(A, mask, W, H)


def exact_problem_01(m, n, k):
    """The same under a tall block, where the Gram denominators of tests/_exact.py::products pass its 2^22: A in 0..7, W and H in
    {0, 1} with W[:, 0] = H[0, :] = 1, so that every model value <W_r, H_c> is an integer in 1..k.  Every unmasked sum is asserted
    below 2^24 (and bounds the masked one: all terms are non-negative), the `kl` denominators as well."""
    rs = np.random.RandomState(31 * m + 7 * n + k)
    A = rs.randint(0, 8, size=(m, n)).astype(np.float32)
    W = rs.randint(0, 2, size=(m, k)).astype(np.float32)
    H = rs.randint(0, 2, size=(k, n)).astype(np.float32)
    W[:, 0] = 1
    H[0, :] = 1
    mask = _exact_mask(rs, m, n)
    ref = _exact_ref(A, mask, W, H)
    for tot, what in zip(ref["unmasked_fro"], ("A H^T", "(W H) H^T", "W^T A", "W^T (W H)")):
        E._bound(tot, 1.0, np.float32, what)
    E._bound(np.float64(max(m, n)), 1.0, np.float32, "observation counts")
    return A, mask, W, H, ref


# ---- exact operands at the smallest shapes whose launch plans (dnmf_masked_plan) enter the tile loop of masked_uht_kernel, the
# row-block loop of masked_wtu_kernel and the grid-stride trip of masked_reduce_kernel; EXACT_SHAPES above stay at one trip of each.
# Per case: shape, ranks, generator, whether the operands qualify for the 16-byte vector (FAST) kernels at k % 4 == 0, and what
# tests/test_capi_masked.py must find in the plan at EVERY one of its ranks.  Derived there from the plan's six numbers:
#   last_split_tiles  tiles of the last column split         last_tile_cols   width of its last tile (< 32: ragged, and not the first)
#   last_chunk_blks   row blocks of the last row chunk       last_blk_rows    rows of its last block
#   w_reduce_trips    grid-stride trips of the W side's ending, from dnmf_masked_reduce_grid(m, k) workgroups of 256 threads
EXACT_LOOP_CASES = (
    {"shape": (70, 2085), "ks": EXACT_KS, "gen": "products", "fast": False,          # W side, generic: cur goes 0, 1, 0
     "reach": {"tiles_per_split": 3, "nsplit": 22, "last_split_tiles": 3, "last_tile_cols": 5}},
    {"shape": (68, 2084), "ks": EXACT_KS, "gen": "products", "fast": True,           # W side through the vector loads
     "reach": {"tiles_per_split": 3, "nsplit": 22, "last_split_tiles": 3, "last_tile_cols": 4}},
    {"shape": (2130, 70), "ks": EXACT_KS, "gen": "products", "fast": False,          # H side, generic: a short last chunk
     "reach": {"nrowblk": 67, "rowblks_per_chunk": 2, "nchunks": 34, "last_chunk_blks": 1, "last_blk_rows": 18}},
    {"shape": (2132, 96), "ks": EXACT_KS, "gen": "products", "fast": True,           # H side through the vector paths
     "reach": {"nrowblk": 67, "rowblks_per_chunk": 2, "nchunks": 34, "last_chunk_blks": 1, "last_blk_rows": 20}},
    {"shape": (16400, 41), "ks": (128,), "gen": "01", "fast": False,                 # m k elements: a second trip of the reduce
     "reach": {"tiles_per_split": 2, "nsplit": 1, "zdim": 2, "last_split_tiles": 2, "last_tile_cols": 9,
               "nrowblk": 513, "rowblks_per_chunk": 9, "nchunks": 57, "last_chunk_blks": 9, "last_blk_rows": 16,
               "w_reduce_trips": 2}},
)
EXACT_LOOP_SHAPES = tuple(c["shape"] for c in EXACT_LOOP_CASES)
PLAN_FIELDS = ("tiles_per_split", "nsplit", "zdim", "rowblks_per_chunk", "nchunks", "nrowblk")


def loop_case(shape):
    return next(c for c in EXACT_LOOP_CASES if c["shape"] == tuple(shape))


def plan_reach(m, n, k, plan, reduce_grid):
    """the six numbers of dnmf_masked_plan as a dict, with the derived entries the table above names; `reduce_grid` is the library's
    dnmf_masked_reduce_grid"""
    d = dict(zip(PLAN_FIELDS, (int(x) for x in plan)))
    last_cols = n - (d["nsplit"] - 1) * d["tiles_per_split"] * 32
    d["last_split_tiles"] = -(-last_cols // 32)
    d["last_tile_cols"] = last_cols - (d["last_split_tiles"] - 1) * 32
    d["last_chunk_blks"] = d["nrowblk"] - (d["nchunks"] - 1) * d["rowblks_per_chunk"]
    d["last_blk_rows"] = m - (d["nrowblk"] - 1) * 32
    d["w_reduce_trips"] = -(-m * k // (256 * int(reduce_grid(m, k))))
    d["h_reduce_trips"] = -(-k * n // (256 * int(reduce_grid(k, n))))
    return d


_LOOP_PROBLEMS = {}


def loop_problem(m, n, k):
    """(A, mask, W, H, ref) of a case of EXACT_LOOP_CASES from its generator, built once per process and shared: no test writes to them"""
    key = (m, n, k)
    if key not in _LOOP_PROBLEMS:
        gen = exact_problem_01 if loop_case((m, n))["gen"] == "01" else exact_problem
        _LOOP_PROBLEMS[key] = gen(m, n, k)
    return _LOOP_PROBLEMS[key]


def exact_resid_block(A, mask, W, H):
    """(block, r): W H + r at the observed positions with r in {0, 1, 2}, NaN elsewhere -- integers, so the kernel's differences are
    exactly r and the masked residual is sum(mask * r^2)"""
    m, n = mask.shape
    r = np.random.RandomState(3 * m + n).randint(0, 3, size=(m, n))
    D = W.astype(np.float64) @ H.astype(np.float64)
    return nan_marked((D + r).astype(np.float32), mask), r
