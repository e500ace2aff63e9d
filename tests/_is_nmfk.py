"""NMFk under the Itakura-Saito objective (`params.norm = 'is'`): test helpers (TEST INFRASTRUCTURE, lives under tests/ only).

`scaled_problem`: the planted problem of the sweeps -- rank 3, column scales over three decades, multiplicative gamma(10) noise: the
setting in which the Frobenius (and KL) per-column error weights the columns by their scale and the Itakura-Saito one does not.
`ISNmfkOracleOps`: tests/_is.py::ISOracleOps plus what a sweep asks of an operator set beyond a fit -- the per-column divergence sums
in float64 numpy -- and the capability flag PyNMFk looks for.  `column_div`: the float64 statement.  `coldiv_case`: the exact operands
of the kernel test.  The rank functions run a grid's column divergence and a perturbation-shared sweep as processes.
"""
import os
import traceback

import numpy as np
import torch

from tests import _is as I
from tests._ops_double import _n

EPS = I.EPS


def scaled_problem(seed=1):
    """120 x 90, rank 3, strictly positive float32: min 6.0e-5, max 1.73 at seed 1"""
    rs = np.random.RandomState(seed); m, n, k = 120, 90, 3
    x = np.arange(m)[:, None]
    W = np.exp(-0.5 * ((x - m * (np.arange(k)[None, :] + 0.5) / k) / (m / 10.0)) ** 2) + 0.05
    cs = 10.0 ** (-3.0 * rs.rand(n))[None, :]
    S = (W @ (rs.rand(k, n) + 0.05)) * cs
    A = (S * rs.gamma(10.0, 0.1, size=(m, n))).astype(np.float32)
    return A


def column_div(A, W, H, eps=EPS):
    """float64 column SUMS of q - log q - 1, q = A / (W H + eps)"""
    q = np.asarray(A, dtype=np.float64) / (np.asarray(W, dtype=np.float64) @ np.asarray(H, dtype=np.float64) + eps)
    return (q - np.log(q) - 1.0).sum(0)


class ISNmfkOracleOps(I.ISOracleOps):
    name = "oracle-is-nmfk"
    is_nmfk = True

    def is_column_div(self, A, W, H, eps):
        return torch.from_numpy(column_div(_n(A), _n(W), _n(H), eps))


def sweep_args(tmp, norm="is", comms=None, **extra):
    """the parameters of tests/test_nmfk_cpu.py::_args (mu, k = 1..5, 6 perturbations, 300 iterations, sill_thr 0.8) under `norm`"""
    from pydnmfk_amd.dist_comm import MPI_comm
    from tests.test_nmfk_cpu import _args
    os.makedirs(str(tmp), exist_ok=True)
    args = _args(tmp, comms if comms is not None else MPI_comm(None, 1, 1))
    assert (args.method, args.start_k, args.end_k, args.perturbations, args.itr, args.sill_thr) == ("mu", 1, 5, 6, 300, 0.8)
    args.norm = norm
    for key, val in extra.items():
        setattr(args, key, val)
    return args


def small_args(tmp, comms=None, norm="is", **extra):
    """a short sweep (k = 2..3, 4 perturbations, 60 iterations) for the tests that compare two runs of it"""
    return sweep_args(tmp, norm, comms, start_k=2, end_k=3, itr=60, perturbations=4, **extra)


def min_silhouettes(nmfk):
    return [round(float(np.min(np.asarray(nmfk.stats[k]["clusterSilhouetteCoefficients"]))), 2) for k in sorted(nmfk.stats)]


# ---- PyNMF.is_column_divergence() on a grid
def _coldiv_rank(rank, world, port, grid, q, use_hip):
    """this rank's slice of tests/_is.py::problem(): a GRID_ITR-step fit, then (W rows, H columns, W, H, column divergence, divergence)"""
    try:
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        I._setup_rank(rank, world, port, use_hip)
        dt = np.float32 if use_hip else np.float64            # (the HIP kernels are float32; the checker set runs in float64)
        A, W0, H0, k = I.problem()
        comms = MPI_comm(None, grid[0], grid[1])
        sl, (w0, w1), (h0, h1) = I._slices(rank, grid, A.shape)
        nmf = PyNMF(A[sl].astype(dt), factors=[W0[w0:w1].astype(dt), H0[:, h0:h1].astype(dt)],
                    params=I.args_for(comms, grid[0], grid[1], k, I.GRID_ITR), ops=None if use_hip else ISNmfkOracleOps())
        assert nmf._ops().name == ("hip" if use_hip else "oracle-is-nmfk")
        W, H, _ = nmf.fit()
        col = nmf.is_column_divergence()
        assert isinstance(col, np.ndarray) and col.dtype == np.float64 and col.shape == (A.shape[1],)
        q.put((rank, ((w0, w1), (h0, h1), np.asarray(W), np.asarray(H), col, nmf.is_divergence()), None))
        I._teardown_rank(world)
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_coldiv(grid, use_hip=False, timeout=240):
    """(A as the ranks held it in float64, W, H assembled, [column divergence per rank], [divergence per rank])"""
    res = I.spawn(_coldiv_rank, grid, (use_hip,), timeout)
    A, _, _, k = I.problem()
    dt = np.float32 if use_hip else np.float64
    m, n = A.shape
    W, H = np.full((m, k), np.nan), np.full((k, n), np.nan)
    for _, ((w0, w1), (h0, h1), Wr, Hr, _, _) in res:
        W[w0:w1], H[:, h0:h1] = Wr, Hr
    assert np.isfinite(W).all() and np.isfinite(H).all()
    return A.astype(dt).astype(np.float64), W, H, [out[4] for _, out in res], [out[5] for _, out in res]


# ---- nmfk_split='data': the short sweep with scaled_problem(1) cut into the blocks of a 1D grid
def _data_grid_rank(rank, world, port, grid, q, use_hip, results_root):
    try:
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMFk import PyNMFk
        I._setup_rank(rank, world, port, use_hip)
        A = scaled_problem(1)
        comms = MPI_comm(None, grid[0], grid[1])
        sl = I._slices(rank, grid, A.shape)[0]
        args = small_args(os.path.join(results_root, "%dx%d" % tuple(grid)), comms=comms)
        args.size, args.rank = world, rank
        nmfk = PyNMFk(np.ascontiguousarray(A[sl]), params=args, ops=None if use_hip else ISNmfkOracleOps())
        nopt = nmfk.fit()
        q.put((rank, (int(nopt), {k: {key: np.asarray(v) for key, v in st.items()} for k, st in nmfk.stats.items()}), None))
        I._teardown_rank(world)
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


# ---- nmfk_split='perturbations'
def _split_rank(rank, world, port, q, results_root, use_hip):
    try:
        import torch.distributed as dist
        from pydnmfk_amd.dist_comm import COMM_WORLD, SoloGrid
        from pydnmfk_amd.pyDNMFk import PyNMFk
        torch.set_num_threads(1)
        if use_hip:
            torch.cuda.set_device(0)
        if world > 1:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
            comms = SoloGrid(rank)
            args = small_args(os.path.join(results_root, "w%d" % world), comms=comms, nmfk_split="perturbations")
            args.size, args.rank, args.comm1 = world, rank, COMM_WORLD()
        else:
            args = small_args(os.path.join(results_root, "w%d" % world))
        nmfk = PyNMFk(scaled_problem(1), params=args, ops=None if use_hip else ISNmfkOracleOps())
        assert nmfk._batch_size() == 1
        nopt = nmfk.fit()
        q.put((rank, (int(nopt), {k: {key: np.asarray(v) for key, v in st.items()} for k, st in nmfk.stats.items()}), None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_split(results_root, use_hip=False, timeout=300):
    """{world: [(nopt, {k: statistics}) per rank]} of the short sweep on one rank and shared by two"""
    import torch.multiprocessing as mp
    from tests._mp import collect, free_port
    outs = {}
    for world in (1, 2):
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = free_port()
        procs = [ctx.Process(target=_split_rank, args=(r, world, port, q, str(results_root), use_hip)) for r in range(world)]
        for p in procs:
            p.start()
        res = collect(procs, q, timeout)
        for rank, out, err in res:
            assert err is None, "rank %d failed:\n%s" % (rank, err)
        outs[world] = [out for _, out, _ in sorted(res, key=lambda r: r[0])]
    return outs


def assert_split_equals_one_rank(outs):
    one = outs[1][0]
    assert set(one[1]) == {2, 3} and all("is_div" in st and "avgDiv" in st for st in one[1].values())
    for o in outs[2]:
        assert o[0] == one[0]
        for k in one[1]:
            assert set(o[1][k]) == set(one[1][k])
            for key, val in one[1][k].items():
                assert np.allclose(np.asarray(o[1][k][key]), np.asarray(val), rtol=1e-9, atol=0, equal_nan=True), (k, key)


# ---- exact operands of the per-column divergence kernel (csrc/dnmf_sums.h: col_sums_kernel with the term BetaDivTerm<BETA_DIV_IS, 1>)
_COLDIV = {}


def coldiv_case(m, n, k):
    """(A, W, H, count): W, H of tests/_is.py::exact (every S a power of two in [2, 32], eps absorbed); A = S but for a planted set
    where A = 2 S, so q is exactly 1 or 2 and a term exactly 0 or t2 = 1 - logf(2).  The planted set has at most one position per column
    and 32-row block (every fp32 partial is 0 or t2), none in columns 3 and 7, and one in EVERY row block of column 0.  count[c]: the planted positions of column c.  Built once per process; no test writes to them."""
    key = (m, n, k)
    if key not in _COLDIV:
        _, W, H, _ = I.exact_problem(m, n, k)
        S = W.astype(np.float64) @ H.astype(np.float64)
        rs = np.random.RandomState(7 * m + 3 * n + k)
        plant = np.zeros((m, n), dtype=bool)
        nrowblk = -(-m // 32)
        assert n > 8
        empty = (3, 7)
        for rb in range(nrowblk):
            rows = min(32, m - 32 * rb)
            for c in range(n):
                if c in empty or (c != 0 and rs.rand() < 0.5):
                    continue
                plant[32 * rb + rs.randint(rows), c] = True
        A = np.where(plant, 2.0 * S, S)
        assert A.max() <= 64 and np.array_equal(A.astype(np.float32).astype(np.float64), A)
        count = plant.sum(0)
        assert count[0] == nrowblk and (count == 0).sum() >= 2
        assert np.pad(plant, ((0, (-m) % 32), (0, 0))).reshape(-1, 32, n).sum(1).max() <= 1
        _COLDIV[key] = (A.astype(np.float32), W, H, count)
    return _COLDIV[key]
