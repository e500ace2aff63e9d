"""NMFk under a beta-divergence (`params.norm = 'beta'` with `params.beta`): test helpers (TEST INFRASTRUCTURE, lives under tests/ only).

The per-column statistic of the sweep, for a column c with s' = W H + eps and a^beta := 0 at a = 0 (beta > 0):

    stat[c] = sum_i d_beta(a_ic | s'_ic) / sum_i a_ic^beta

`column_sums` / `column_stat`: its float64 statement (numerator with the magnitudes of its terms, denominator; the ratio).
`BetaNmfkOracleOps`: tests/_beta.py::BetaOracleOps plus what a sweep asks of an operator set beyond a fit -- the two per-column sums in
float64 numpy on tests/_beta.py::terms_of -- and the capability flag PyNMFk looks for (and the Itakura-Saito pair of tests/_is_nmfk.py,
which beta = 0 is handed to).  `coldiv_case`: the exact operands of the kernel test.  The rank functions run a grid's statistic and a
perturbation-shared sweep as processes, modelled on tests/_is_nmfk.py.
"""
import os
import traceback

import numpy as np
import torch

from tests import _beta as B
from tests import _is as I
from tests import _is_nmfk as K
from tests._ops_double import _n

EPS = B.EPS
scaled_problem = K.scaled_problem
min_silhouettes = K.min_silhouettes


def power_sums(A, beta):
    """float64 column sums of a^beta, 0 at a = 0 (a itself at beta = 1, the row count at beta = 0)"""
    A = np.asarray(A, dtype=np.float64)
    if beta == 0:
        return np.full(A.shape[1], float(A.shape[0]))
    return np.where(A > 0, np.where(A > 0, A, 1.0) ** beta, 0.0).sum(0)


def column_sums(A, W, H, beta, eps=EPS):
    """(div[c], the column's sum of the magnitudes of the divergence's terms, pw[c]) in float64"""
    t = B.terms_of(A, np.asarray(W, dtype=np.float64) @ np.asarray(H, dtype=np.float64) + eps, beta)
    return sum(x.sum(0) for x in t), sum(np.abs(x).sum(0) for x in t), power_sums(A, beta)


def column_stat(A, W, H, beta, eps=EPS):
    """the float64 statement of the per-column statistic"""
    div, _, pw = column_sums(A, W, H, beta, eps)
    return div / pw


class BetaNmfkOracleOps(B.BetaOracleOps):
    name = "oracle-beta-nmfk"
    beta_nmfk = True
    is_nmfk = True                      # (beta = 0 is renamed to norm='is' and swept on that path)

    def beta_column_div(self, A, W, H, eps, beta):
        div, _, pw = column_sums(_n(A), _n(W), _n(H), beta, eps)
        return torch.from_numpy(np.ascontiguousarray(div)), torch.from_numpy(np.ascontiguousarray(pw))

    def is_column_div(self, A, W, H, eps):
        return torch.from_numpy(K.column_div(_n(A), _n(W), _n(H), eps))


def sweep_args(tmp, beta, comms=None, **extra):
    """tests/_is_nmfk.py::sweep_args (mu, k = 1..5, 6 perturbations, 300 iterations, sill_thr 0.8) under norm='beta'"""
    return K.sweep_args(tmp, extra.pop("norm", "beta"), comms, beta=beta, **extra)


def small_args(tmp, beta, comms=None, **extra):
    """a short sweep (k = 2..3, 4 perturbations, 60 iterations) for the tests that compare two runs of it"""
    return sweep_args(tmp, beta, comms, start_k=2, end_k=3, itr=60, perturbations=4, **extra)


# ---- PyNMF.beta_column_divergence() on a grid
def _colstat_rank(rank, world, port, grid, q, use_hip, betas):
    """this rank's slice of tests/_beta.py::problem(): for every beta a GRID_ITR-step fit, then (W rows, H columns, W, H, statistic,
    its numerator's total as beta_divergence() reports it)"""
    try:
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        I._setup_rank(rank, world, port, use_hip)
        dt = np.float32 if use_hip else np.float64            # (the HIP kernels are float32; the checker set runs in float64)
        A, W0, H0, k = B.problem()
        comms = MPI_comm(None, grid[0], grid[1])
        sl, (w0, w1), (h0, h1) = I._slices(rank, grid, A.shape)
        out = {}
        for beta in betas:
            nmf = PyNMF(A[sl].astype(dt), factors=[W0[w0:w1].astype(dt), H0[:, h0:h1].astype(dt)],
                        params=B.args_for(comms, grid[0], grid[1], k, B.GRID_ITR, beta), ops=None if use_hip else BetaNmfkOracleOps())
            assert nmf._ops().name == ("hip" if use_hip else "oracle-beta-nmfk") and nmf.norm == "beta"
            W, H, _ = nmf.fit()
            col = nmf.beta_column_divergence()
            assert isinstance(col, np.ndarray) and col.dtype == np.float64 and col.shape == (A.shape[1],)
            out[beta] = ((w0, w1), (h0, h1), np.asarray(W), np.asarray(H), col, nmf.beta_divergence())
        q.put((rank, out, None))
        I._teardown_rank(world)
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_colstat(grid, betas, use_hip=False, timeout=240):
    """{beta: (A as the ranks held it in float64, W, H assembled, [statistic per rank], [divergence per rank])}"""
    res = I.spawn(_colstat_rank, grid, (use_hip, tuple(betas)), timeout)
    A, _, _, k = B.problem()
    dt = np.float32 if use_hip else np.float64
    m, n = A.shape
    full = {}
    for beta in betas:
        W, H = np.full((m, k), np.nan), np.full((k, n), np.nan)
        for _, out in res:
            (w0, w1), (h0, h1), Wr, Hr, _, _ = out[beta]
            W[w0:w1], H[:, h0:h1] = Wr, Hr
        assert np.isfinite(W).all() and np.isfinite(H).all()
        full[beta] = (A.astype(dt).astype(np.float64), W, H, [out[beta][4] for _, out in res], [out[beta][5] for _, out in res])
    return full


# ---- nmfk_split='perturbations'
SPLIT_BETA = 0.5


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
            args = small_args(os.path.join(results_root, "w%d" % world), SPLIT_BETA, comms=comms, nmfk_split="perturbations")
            args.size, args.rank, args.comm1 = world, rank, COMM_WORLD()
        else:
            args = small_args(os.path.join(results_root, "w%d" % world), SPLIT_BETA)
        nmfk = PyNMFk(scaled_problem(1), params=args, ops=None if use_hip else BetaNmfkOracleOps())
        assert nmfk._batch_size() == 1
        nopt = nmfk.fit()
        q.put((rank, (int(nopt), {k: {key: np.asarray(v) for key, v in st.items()} for k, st in nmfk.stats.items()}), None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_split(results_root, use_hip=False, timeout=300):
    """{world: [(nopt, {k: statistics}) per rank]} of the short sweep at beta = SPLIT_BETA on one rank and shared by two"""
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
    """tests/_is_nmfk.py::assert_split_equals_one_rank with this norm's keys (rtol 1e-9, equal_nan)"""
    one = outs[1][0]
    assert set(one[1]) == {2, 3} and all("beta_div" in st and "avgDiv" in st and "beta" in st for st in one[1].values())
    for o in outs[2]:
        assert o[0] == one[0]
        for k in one[1]:
            assert set(o[1][k]) == set(one[1][k])
            for key, val in one[1][k].items():
                assert np.allclose(np.asarray(o[1][k][key]), np.asarray(val), rtol=1e-9, atol=0, equal_nan=True), (k, key)


# ---- exact operands of the per-column kernel (csrc/dnmf_sums.h: col_sums_kernel with the terms BetaDivTerm<FORM, 2>; the general form: beta_coldiv_kernel)
_COLDIV = {}


def coldiv_case(m, n, k):
    """(A, W, H, splant, asum): the operands of tests/_is_nmfk.py::coldiv_case -- W, H of tests/_is.py::exact (every S a power of two in
    [2, 32], eps absorbed); A = S but for a planted set where A = 2 S; at most one planted position per column and 32-row block, none in
    columns 3 and 7, one in EVERY row block of column 0.  splant[c]: the sum of s over the planted positions of column c (an integer);
    asum[c] = sum_i a_ic (an integer below 2^24: exact in every order in fp32 and float64).  Built once per process; no test writes to
    them."""
    key = (m, n, k)
    if key not in _COLDIV:
        A, W, H, count = K.coldiv_case(m, n, k)
        S = W.astype(np.float64) @ H.astype(np.float64)
        plant = A.astype(np.float64) != S
        assert np.array_equal(plant.sum(0), count) and np.array_equal(A.astype(np.float64)[plant], 2.0 * S[plant])
        splant = np.where(plant, S, 0.0).sum(0)
        asum = A.astype(np.float64).sum(0)
        assert splant[0] > 0 and (splant == 0).sum() >= 2 and asum.max() < 2.0 ** 24 and np.array_equal(asum, np.round(asum))
        _COLDIV[key] = (A, W, H, splant, asum)
    return _COLDIV[key]
