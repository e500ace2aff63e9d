"""Helpers for the Itakura-Saito objective, `params.norm = 'is'` (TEST INFRASTRUCTURE, lives under tests/ only).

A float64 numpy statement of the rule on the WHOLE matrix.  With S = W H, R = 1 / (S + eps) element-wise and eps the machine epsilon
of the factors' arithmetic (float32's in the fp32 path):

    W <- W * sqrt(((A R R) H^T) / (R H^T + eps))      then, with the new W,      H <- H * sqrt((W^T (A R R)) / (W^T R + eps))
    D_IS(A | S + eps) = sum (q - log q - 1),  q = A R

`ISOracleOps`: tests/_ops_double.py::OracleOps plus the Itakura-Saito operations of engine.HipOps in numpy float64, so that the
choreography (dist_nmf.IS_MU_update) runs on the CPU and under gloo.  It takes float32 AND float64 blocks (`is_dtypes`): with
float64 data PyNMF computes in float64 throughout (factors, pair buffers, allreduce), which is what lets a grid be compared with the
whole-matrix statement to 1e-10 -- through float32 buffers the partial sums of two ranks round differently from the whole sum at 6e-8.
`run_grid`: the ranks of a 1D grid as processes.  `exact`: operands at which both pairs are exact in fp32, element by element.
"""
import os
import traceback

import numpy as np
import torch

from tests import _exact as E
from tests._ops_double import OracleOps, _n

EPS = float(np.finfo(np.float32).eps)


# ---- the rule
def pair(A, W, H, side, eps=EPS):
    """(num, den) in float64: m x k for side 'w', k x n for side 'h'"""
    A, W, H = (np.asarray(x, dtype=np.float64) for x in (A, W, H))
    R = 1.0 / (W @ H + eps)
    U = A * R * R
    return (U @ H.T, R @ H.T) if side == "w" else (W.T @ U, W.T @ R)


def step(A, W, H, eps=EPS, W_update=True, clamp=False):
    """one step in float64 (new arrays): W first, then H with the new W, then the clamp of pyDNMF.py:170-172"""
    W, H = np.array(W, dtype=np.float64), np.array(H, dtype=np.float64)
    if W_update:
        num, den = pair(A, W, H, "w", eps)
        W = W * np.sqrt(num / (den + eps))
    num, den = pair(A, W, H, "h", eps)
    H = H * np.sqrt(num / (den + eps))
    if clamp:
        H, W = np.maximum(H, eps), np.maximum(W, eps)
    return W, H


def iterate(A, W, H, itr, eps=EPS, W_update=True):
    for i in range(itr):
        W, H = step(A, W, H, eps, W_update, clamp=(i % 10 == 0))
    return W, H


def divergence(A, W, H, eps=EPS):
    q = np.asarray(A, dtype=np.float64) / (np.asarray(W, dtype=np.float64) @ np.asarray(H, dtype=np.float64) + eps)
    return float(np.sum(q - np.log(q) - 1.0))


def fit(A, W0, H0, itr, eps=EPS, W_update=True):
    """PyNMF.fit under norm='is': the steps, normalize_features (pyDNMF.py:185-194), the Frobenius relative error (:205-218)"""
    A64 = np.asarray(A, dtype=np.float64)
    W, H = iterate(A64, W0, H0, itr, eps, W_update)
    s = W.sum(axis=0)
    W = W / (s + eps)
    H = H * s[:, None]
    return W, H, float(np.linalg.norm(A64 - W @ H) / np.linalg.norm(A64))


# ---- the operator set
class ISOracleOps(OracleOps):
    name = "oracle-is"
    is_dtypes = (torch.float32, torch.float64)

    def empty(self, shape, like):
        return torch.empty(shape, dtype=torch.float64 if like.dtype == torch.float64 else torch.float32)

    def zeros(self, shape, like):
        return torch.zeros(shape, dtype=torch.float64 if like.dtype == torch.float64 else torch.float32)

    def clamp_min(self, X, eps):
        x = _n(X)
        np.maximum(x, x.dtype.type(eps), out=x)

    def scale_cols_div(self, W, s, eps):
        w = _n(W)
        w /= _n(s)[None, :] + w.dtype.type(eps)

    @staticmethod
    def _halves(buf, shape):
        r, c = shape
        assert buf.is_contiguous() and buf.numel() >= 2 * r * c
        return buf[: r * c].view(r, c), buf[r * c: 2 * r * c].view(r, c)

    @staticmethod
    def _store(dst, src):
        dst.copy_(torch.from_numpy(np.ascontiguousarray(src)).to(dst.dtype))
        return dst

    def is_aht_pair(self, A, W, H, eps, buf):
        num, den = self._halves(buf, tuple(W.shape))
        a, b = pair(_n(A), _n(W), _n(H), "w", eps)
        return self._store(num, a), self._store(den, b)

    def is_wta_pair(self, A, W, H, eps, buf):
        num, den = self._halves(buf, tuple(H.shape))
        a, b = pair(_n(A), _n(W), _n(H), "h", eps)
        return self._store(num, a), self._store(den, b)

    def is_ratio_update(self, X, num, den, eps, clamp=False):
        x = _n(X).astype(np.float64) * np.sqrt(_n(num).astype(np.float64) / (_n(den).astype(np.float64) + eps))
        if clamp:
            x = np.maximum(x, eps)
        return self._store(X, x)

    def is_update_w(self, A, W, H, eps):
        a, b = pair(_n(A), _n(W), _n(H), "w", eps)
        return self.is_ratio_update(W, torch.from_numpy(a), torch.from_numpy(b), eps)

    def is_update_h(self, A, W, H, eps, clamp=False):
        a, b = pair(_n(A), _n(W), _n(H), "h", eps)
        return self.is_ratio_update(H, torch.from_numpy(a), torch.from_numpy(b), eps, clamp)

    def is_divergence(self, A, W, H, eps):
        return torch.tensor([divergence(_n(A), _n(W), _n(H), eps)], dtype=torch.float64)


# ---- problems
def problem(m=50, n=39, k=3, seed=5, noise=4.0):
    """a strictly positive m x n block: a rank-k product with multiplicative gamma noise (shape `noise`, mean 1), and initial factors"""
    rs = np.random.RandomState(seed)
    A = ((rs.rand(m, k) + 0.1) @ (rs.rand(k, n) + 0.1)) * rs.gamma(noise, 1.0 / noise, size=(m, n))
    A = np.maximum(A, 1e-3)
    return A, rs.rand(m, k) + 0.05, rs.rand(k, n) + 0.05, k


def args_for(comms, p_r, p_c, k, itr, W_update=True, norm="is", method="mu", **extra):
    from pydnmfk_amd.utils import parse
    args = parse()
    args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, p_r, p_c, k
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    args.itr, args.init, args.verbose, args.prune = itr, "rand", False, False
    args.norm, args.method, args.W_update = norm, method, W_update
    for key, val in extra.items():
        setattr(args, key, val)
    return args


def one_rank_args(k, itr, **kw):
    from pydnmfk_amd.dist_comm import MPI_comm
    grid = kw.pop("grid", (1, 1))
    return args_for(MPI_comm(None, 1, 1), grid[0], grid[1], k, itr, **kw)


GRID_ITR = 20
GRID_COMBOS = (True, False)                                  # W_update


def _slices(rank, grid, shape):
    from oracle import nmf_oracle as orc
    from pydnmfk_amd.utils import determine_block_params
    p_r, p_c = grid
    s, e = determine_block_params(rank, (p_r, p_c), shape).determine_block_index_range_asymm()
    (w0, w1), (h0, h1) = orc.factor_ranges(rank, p_r, p_c, shape[0], shape[1])
    return (slice(s[0], e[0] + 1), slice(s[1], e[1] + 1)), (w0, w1), (h0, h1)


def _setup_rank(rank, world, port, use_hip):
    import torch.distributed as dist
    if use_hip:
        torch.cuda.set_device(0)
    if world > 1:
        torch.set_num_threads(1)
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)


def _teardown_rank(world):
    import torch.distributed as dist
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _grid_rank(rank, world, port, grid, q, use_hip, shape_k):
    """this rank's slice of problem(): the GRID_ITR-step fits with W_update on and off, then the divergence of the last one"""
    try:
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        _setup_rank(rank, world, port, use_hip)
        dt = np.float32 if use_hip else np.float64            # (the HIP kernels are float32; the checker set runs in float64)
        A, W0, H0, k = problem(*shape_k)
        comms = MPI_comm(None, grid[0], grid[1])
        sl, (w0, w1), (h0, h1) = _slices(rank, grid, A.shape)
        out = {}
        for wu in GRID_COMBOS:
            nmf = PyNMF(A[sl].astype(dt), factors=[W0[w0:w1].astype(dt), H0[:, h0:h1].astype(dt)],
                        params=args_for(comms, grid[0], grid[1], k, GRID_ITR, wu), ops=None if use_hip else ISOracleOps())
            assert nmf._ops().name == ("hip" if use_hip else "oracle-is")
            W, H, err = nmf.fit()
            out[wu] = ((w0, w1), (h0, h1), np.asarray(W), np.asarray(H), float(err), nmf.is_divergence())
        q.put((rank, out, None))
        _teardown_rank(world)
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def _bad_data_rank(rank, world, port, grid, q, use_hip, value):
    """every rank's slice of problem() is fine but ONE entry of the last rank's, set to `value`: what each rank's PyNMF raises"""
    try:
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        _setup_rank(rank, world, port, use_hip)
        A, W0, H0, k = problem()
        A[-1, -1] = value
        comms = MPI_comm(None, grid[0], grid[1])
        sl, (w0, w1), (h0, h1) = _slices(rank, grid, A.shape)
        try:
            PyNMF(A[sl].astype(np.float32), factors=[W0[w0:w1].astype(np.float32), H0[:, h0:h1].astype(np.float32)],
                  params=args_for(comms, grid[0], grid[1], k, 3), ops=None if use_hip else ISOracleOps())
            got = (None, "")
        except Exception as ex:  # noqa: BLE001
            got = (type(ex).__name__, str(ex))
        q.put((rank, got, None))
        _teardown_rank(world)
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def spawn(target, grid, args, timeout=240):
    """[(rank, result)] of `target(rank, world, port, grid, queue, *args)` run as one process per rank of the grid (one rank: in this
    process); every rank process has its own time limit and none is left running"""
    import queue
    world = grid[0] * grid[1]
    if world == 1:
        q = queue.Queue()
        target(0, 1, 0, grid, q, *args)
        res = [q.get()]
    else:
        import torch.multiprocessing as mp
        from tests._mp import free_port
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = free_port()
        procs = [ctx.Process(target=target, args=(r, world, port, grid, q) + tuple(args)) for r in range(world)]
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
    return sorted((rank, out) for rank, out, _ in res)


def run_grid(grid, use_hip=False, shape_k=(50, 39, 3), timeout=240):
    """{W_update: (W, H, err, divergence)} of the GRID_ITR-step fits of problem(*shape_k) on the grid, assembled from the ranks (a
    replicated factor, the error and the divergence must agree between the ranks bit for bit)"""
    res = spawn(_grid_rank, grid, (use_hip, shape_k), timeout)
    m, n, k = shape_k
    full = {}
    for wu in GRID_COMBOS:
        dt = res[0][1][wu][2].dtype
        W, H = np.full((m, k), np.nan, dtype=dt), np.full((k, n), np.nan, dtype=dt)
        errs, divs = set(), set()
        for rank, out in res:
            (w0, w1), (h0, h1), Wr, Hr, err, div = out[wu]
            for dst, src in ((W[w0:w1], Wr), (H[:, h0:h1], Hr)):
                assert np.isnan(dst).all() or np.array_equal(dst, src), (grid, wu, rank)      # replicated: identical on every rank
                dst[...] = src
            errs.add(err)
            divs.add(div)
        assert len(errs) == 1 and len(divs) == 1 and np.isfinite(W).all() and np.isfinite(H).all(), (grid, wu, errs, divs)
        full[wu] = (W, H, errs.pop(), divs.pop())
    return full


def reference_fits(shape_k=(50, 39, 3), eps=EPS, dtype=np.float64):
    """the whole-matrix float64 fits of problem(*shape_k), its arrays first rounded to `dtype` (float32: what the HIP ranks are
    handed): {W_update: (W, H, err, divergence)}"""
    A, W0, H0, k = problem(*shape_k)
    A, W0, H0 = (x.astype(dtype).astype(np.float64) for x in (A, W0, H0))
    out = {}
    for wu in GRID_COMBOS:
        W, H, err = fit(A, W0, H0, GRID_ITR, eps, wu)
        out[wu] = (W, H, err, divergence(A, W, H, eps))
    return out


# ---- exact operands: both pairs exact in fp32, element by element, in any summation order
def exact_factors(rs, m, n, k, qmax=3):
    """(W, H, S = W H) in float64 from the stream `rs`: W has one nonzero per row, 2^(0..2) in a random column j(r); H = 2^(1..qmax).
    Every S is a power of two in [2, 2^(2 + qmax)] whose float32 image absorbs eps (asserted).  No bound on any sum: the shape is free."""
    jr = rs.randint(0, k, size=m)
    W = np.zeros((m, k))
    W[np.arange(m), jr] = 2.0 ** rs.randint(0, 3, size=m)
    H = 2.0 ** rs.randint(1, qmax + 1, size=(k, n))
    S = W @ H
    assert np.all(S >= 2) and np.array_equal(np.log2(S), np.round(np.log2(S)))
    assert np.array_equal((S.astype(np.float32) + np.float32(EPS)), S.astype(np.float32))          # eps is absorbed
    return W, H, S


def exact(m, n, k, seed=0, qmax=3):
    """The operands of tests/_exact.py::kl with A in 1..7: W has one nonzero per row, 2^(0..2) in a random column j(r); H = 2^(1..qmax).
    Every S = W[r][j(r)] H[j(r)][c] is then a power of two in [2, 2^(2 + qmax)]: eps is absorbed (it is at most half an ulp of 2, whose
    last bit is even), r = 1 / S (v_rcp_f32 is exact at powers of two: tests/test_gpu_exact.py) and a r r are exact, num is a sum of
    multiples of 2^-(2 (2 + qmax)) and den of 2^-(2 + qmax).  All terms are non-negative, so every partial sum in every order is exact
    when the total stays below 2^24 of its unit: asserted here with E._bound.  Returns A, W, H (float32) and the float64 answers
    {"w": (num, den), "h": (num, den)}."""
    rs = np.random.RandomState(seed + 13 * m + 5 * n + 3 * k + 1)
    A = rs.randint(1, 8, size=(m, n)).astype(np.float64)
    W, H, S = exact_factors(rs, m, n, k, qmax)
    R = 1.0 / S
    U = A * R * R
    ref = {"w": (U @ H.T, R @ H.T), "h": (W.T @ U, W.T @ R)}
    un, ud = 2.0 ** -(2 * (2 + qmax)), 2.0 ** -(2 + qmax)
    for side in ("w", "h"):
        E._bound(ref[side][0], un, np.float32, "IS num, side " + side)
        E._bound(ref[side][1], ud, np.float32, "IS den, side " + side)
        for x, unit in zip(ref[side], (un, ud)):
            assert np.array_equal(x / unit, np.round(x / unit)) and np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return A.astype(np.float32), W.astype(np.float32), H.astype(np.float32), ref


# ---- the shapes of the exact test: one trip of every loop, and the smallest shapes at which the launch geometry (dnmf_is_plan reports
# it: the masked one, with at least four row chunks on the H side and one part of the output columns at KP = 128) enters the W side's tile loop with a ragged last tile, the H side's row-block
# loop with a short last chunk, the FAST variants of both, and the second grid-stride trip of the ending.  `reach`: what
# tests/test_capi_is.py must find in the plan at EVERY one of the case's ranks (the names of tests/_masked_dense.py::plan_reach).
EXACT_SHAPES = ((130, 97), (257, 70), (132, 96))          # (the third: rows and ranks of whole 16-byte vectors, the FAST kernels)
EXACT_KS = (3, 32, 64, 128)
EXACT_LOOP_CASES = (
    {"shape": (70, 2085), "ks": EXACT_KS, "fast": False,          # W side, generic: the LDS stage index goes 0, 1, 0
     "reach": {"tiles_per_split": 3, "nsplit": 22, "last_split_tiles": 3, "last_tile_cols": 5}},
    {"shape": (68, 2084), "ks": EXACT_KS, "fast": True,           # W side through the vector loads
     "reach": {"tiles_per_split": 3, "nsplit": 22, "last_split_tiles": 3, "last_tile_cols": 4}},
    {"shape": (2130, 70), "ks": EXACT_KS, "fast": False,          # H side, generic: a short last chunk
     "reach": {"nrowblk": 67, "rowblks_per_chunk": 2, "nchunks": 34, "last_chunk_blks": 1, "last_blk_rows": 18}},
    {"shape": (2132, 96), "ks": EXACT_KS, "fast": True,           # H side through the vector paths
     "reach": {"nrowblk": 67, "rowblks_per_chunk": 2, "nchunks": 34, "last_chunk_blks": 1, "last_blk_rows": 20}},
    {"shape": (16400, 41), "ks": (128,), "fast": False,           # m k elements: a second trip of the ending
     "reach": {"nsplit": 2, "zdim": 1, "last_tile_cols": 9,
               "nrowblk": 513, "rowblks_per_chunk": 9, "nchunks": 57, "last_chunk_blks": 9, "last_blk_rows": 16,
               "w_reduce_trips": 2}},
)
PLAN_FIELDS = ("tiles_per_split", "nsplit", "zdim", "rowblks_per_chunk", "nchunks", "nrowblk", "w_reduce_grid", "h_reduce_grid")


def plan_reach(m, n, k, plan):
    """the eight numbers of dnmf_is_plan as a dict, with the derived entries the table above names"""
    d = dict(zip(PLAN_FIELDS, (int(x) for x in plan)))
    last_cols = n - (d["nsplit"] - 1) * d["tiles_per_split"] * 32
    d["last_split_tiles"] = -(-last_cols // 32)
    d["last_tile_cols"] = last_cols - (d["last_split_tiles"] - 1) * 32
    d["last_chunk_blks"] = d["nrowblk"] - (d["nchunks"] - 1) * d["rowblks_per_chunk"]
    d["last_blk_rows"] = m - (d["nrowblk"] - 1) * 32
    d["w_reduce_trips"] = -(-m * k // (256 * d["w_reduce_grid"]))
    d["h_reduce_trips"] = -(-k * n // (256 * d["h_reduce_grid"]))
    return d


_EXACT = {}


def exact_problem(m, n, k):
    """exact(m, n, k), built once per process and shared: no test writes to it"""
    if (m, n, k) not in _EXACT:
        _EXACT[(m, n, k)] = exact(m, n, k)
    return _EXACT[(m, n, k)]
