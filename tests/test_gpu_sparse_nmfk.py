"""NMFk over sparse data on the GPU: the two kernels the sweep adds to the fits (csrc/dnmf_csr.h: the keyed perturbation of a CSR
image, the per-column error from the transpose's image) and the sweep itself through pydnmfk_amd.pyDNMFk.

Perturbation: a stored entry's value must be, BIT FOR BIT, what the dense kernels give its position in the densified block
(engine.HIP_OPS.perturb_uniform) -- in the block's image and, in transpose order, in the transpose's.
Column error: on the exact-by-construction operands of tests/_exact.py (`sparse_products`: every product and sum below an integer
under 2^53) num and den must EQUAL the float64 integers, under both meanings of an unstored entry, on the block and on its
transpose (long rows in the transpose's image), k on both sides of every KPAD boundary, factors as pitched / unaligned views in
NaN-poisoned buffers.
Sweeps: the reference's golden statistics on a fully stored matrix; device input against the dense device sweep (identical
perturbed copies, see test_device_input_equals_the_dense_device_sweep for the bound on avgErr); missing data; prune, poisson,
perturbations shared by two ranks, the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _exact as ex

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 16, 17, 32, 33, 64, 65, 128, 129, 256]
CASES = [pytest.param(k, i % 2 == 0, id="k%d-%s" % (k, "aligned" if i % 2 == 0 else "unaligned")) for i, k in enumerate(KS)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pydnmfk_amd.engine import HIP_CSR_OPS
    assert HIP_CSR_OPS.sparse_nmfk
    return HIP_CSR_OPS


@pytest.fixture(scope="module")
def pattern():
    return ex.lens_pattern()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------- perturbation
def _many_rows():
    return ex.sparse_pattern(np.random.RandomState(11).randint(0, 6, size=2 * 8192 + 5), 70, seed=1)


def _beyond_grid():
    """more rows than the launch has waves (65536 workgroups of 4): every wave loops over its rows"""
    m = 4 * 65536 + 7
    mask = np.zeros((m, 5), dtype=bool)
    mask[np.arange(m), np.random.RandomState(2).randint(0, 5, size=m)] = True
    mask[::3] = False
    return mask


def _vector_shape():
    """a dense shape the 8-element vector kernel takes (cols % 8 == 0): the CSR kernel must give ITS values too"""
    return np.random.RandomState(3).rand(33, 64) < 0.3


@pytest.mark.parametrize("which", ["lens", "many_rows", "beyond_grid", "vector"])
def test_perturbation_is_the_dense_kernels_value_at_the_stored_positions(ops, pattern, which):
    from pydnmfk_amd.engine import HIP_OPS
    from tests.test_gpu_exact_sparse import _block
    mask = {"lens": lambda: pattern, "many_rows": _many_rows, "beyond_grid": _beyond_grid, "vector": _vector_shape}[which]()
    m, n = mask.shape
    if which == "lens":
        assert (m, n) == (27, 3100) and max(ex.LENS) > 3 * 1024
    if which == "many_rows":
        assert (m, n) == (16389, 70)
    A = np.where(mask, np.random.RandomState(4).rand(m, n) + 0.5, 0.0).astype(np.float32)
    blk = _block(A, mask)
    r, c = np.nonzero(mask)
    L = r.astype(np.int64) * n + c
    assert (L % 2 == 0).any() and (L % 2 == 1).any()                       # both halves of a hash are used
    dense = blk.to_dense()
    rt, ct = torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda()
    tr, tc = np.nonzero(mask.T)                                            # the transpose's order: column by column, rows ascending
    for seed in (0, 1000, 2 ** 40 + 1):
        ref = HIP_OPS.perturb_uniform(dense, 0.03, seed)
        per = ops.perturb_uniform(blk, 0.03, seed)
        assert torch.equal(_bits(per.val), _bits(ref[rt, ct])), (which, seed)
        assert torch.equal(_bits(per.t_val), _bits(ref[torch.from_numpy(tc).cuda(), torch.from_numpy(tr).cuda()])), (which, seed)
        for name in ("crow", "col", "t_crow", "t_col", "long_rows", "long_segptr", "t_long_rows", "t_long_segptr"):
            assert getattr(per, name) is getattr(blk, name), name          # shared with the source, not copied
        assert per.missing == blk.missing and per.val.data_ptr() != blk.val.data_ptr() and getattr(per, "_sqnorm", None) is None
        assert not torch.equal(per.val, blk.val) and float((per.val / blk.val).min()) >= 1.03 - 1e-6 and float((per.val / blk.val).max()) <= 1.09 + 1e-6
    other = ops.perturb_uniform(blk, 0.03, 1)
    assert not torch.equal(other.val, per.val)
    blk_m = _block(A, mask, missing="unstored")
    assert ops.perturb_uniform(blk_m, 0.03, 0).missing == "unstored"
    d = torch.rand(5, 7, device="cuda")                                    # a dense tensor still takes the inherited path
    assert torch.equal(ops.perturb_uniform(d, 0.03, 5), HIP_OPS.perturb_uniform(d, 0.03, 5))


# ------------------------------------------------------------------------------------------------------------- column error
def _colerr_ref(A, mask, W, H, masked):
    A64, D = A.astype(np.float64), W.astype(np.float64) @ H.astype(np.float64)
    E = (A64 - D) ** 2
    return ((mask * E).sum(0) if masked else E.sum(0)), (A64 * A64).sum(0)


@pytest.mark.parametrize("side", ["A", "At"])
@pytest.mark.parametrize("k,aligned", CASES)
def test_column_err_sums_are_the_float64_integers(ops, pattern, k, aligned, side):
    from tests.test_gpu_exact_sparse import _P, _checked, _oriented, _problem
    for missing in (None, "unstored"):
        A, mask, W, H, blk = _oriented(side, *_problem(ex.sparse_products, pattern, k, stored_zeros=missing is not None), missing=missing)
        assert (blk.t_n_long >= 5) == (side == "At") and (blk.t_n_long == 0) == (side == "A")   # At: long rows in the transpose's image
        num, den = _colerr_ref(A, mask, W, H, missing is not None)
        assert np.array_equal(num, np.round(num)) and num.max() < 2.0 ** 53
        empty = mask.sum(0) == 0
        assert empty.sum() >= 2
        Wv, Hv = _P(W, aligned), _P(H, aligned)
        gn, gd = ops.column_err_sums(blk, Wv.view, Hv.view)
        gn2, gd2 = ops.column_err_sums(blk, Wv.view, Hv.view)
        assert gn.dtype == torch.float64 and tuple(gn.shape) == (mask.shape[1],)
        assert torch.equal(gn.view(torch.int64), gn2.view(torch.int64)) and torch.equal(gd.view(torch.int64), gd2.view(torch.int64))
        gn, gd = gn.cpu().numpy(), gd.cpu().numpy()
        bad = np.flatnonzero(gn != num)
        assert bad.size == 0, "num (missing=%r): %d columns differ; first %d: got %r, expected %r" % (missing, bad.size, bad[0], gn[bad[0]], num[bad[0]])
        bad = np.flatnonzero(gd != den)
        assert bad.size == 0, "den (missing=%r): %d columns differ; first %d: got %r, expected %r" % (missing, bad.size, bad[0], gd[bad[0]], den[bad[0]])
        assert not gd[empty].any()                                         # no stored entry: den = 0, num = the Gram term or 0
        if missing is not None:
            assert not gn[empty].any()
        _checked(((Wv, "W"), (Hv, "H")))


def test_column_err_of_a_fully_stored_block_equals_the_dense_path(tmp_path):
    """PyNMF.column_err(): sparse against dense on the same exact operands -- both are float64 sums of the same exact terms"""
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests._masked import args_for
    m, n, k = 53, 37, 5
    A, W, H = ex.sparse_products(np.ones((m, n), dtype=bool), k)
    assert (A != 0).all()
    comms = MPI_comm(None, 1, 1)
    got = {}
    for name, data, missing in (("dense", A, None), ("sparse", sp.csr_matrix(A), None), ("masked", sp.csr_matrix(A), "unstored")):
        nmf = PyNMF(data, factors=[W, H], params=args_for(comms, 1, 1, k, 1, "fro", missing=missing))
        got[name] = nmf.column_err()
    assert np.isfinite(got["dense"]).all() and got["dense"].shape == (n,)
    for name in ("sparse", "masked"):
        assert np.allclose(got[name], got["dense"], rtol=1e-12, atol=0), name


# ------------------------------------------------------------------------------------------------------------- sweeps
def test_golden_statistics_on_a_fully_stored_matrix(tmp_path, golden_dir):
    """nmfk_1x1.npz's A as scipy CSR through the HIP engine (numpy I/O: the reference's numpy stream)"""
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._sparse_nmfk import full_scipy
    from tests.test_nmfk_cpu import _args, check_against_golden
    z = np.load(golden_dir + "/nmfk_1x1.npz")
    nmfk = PyNMFk(full_scipy(z["A"]), factors=None, params=_args(tmp_path, MPI_comm(None, 1, 1)))
    assert nmfk.A_ij.is_sparse_block and nmfk.A_ij.device.type == "cuda" and nmfk._batch_size() == 1
    nopt = nmfk.fit()
    assert nopt == 3
    check_against_golden(nmfk, nopt, z)


def test_device_input_equals_the_dense_device_sweep(tmp_path, golden_dir):
    """torch sparse CSR input on the GPU with params.rng = 'device': the perturbed copies are the dense device sweep's bit for bit at
    the stored positions (all of them here) and the initial factors are the same draws, so the two sweeps differ by summation order
    inside the fits only.  Same estimate; avgErr per k within 0.05 of the dense sweep's below and at the planted rank (the level
    tests/test_gpu_nmfk.py::test_nmfk_device_resident_input holds k = 1, 2 to against the reference), and within the same 0.05 of
    the reference's own below the planted rank."""
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMFk import PyNMFk, sample
    from tests.test_nmfk_cpu import _args
    z = np.load(golden_dir + "/nmfk_1x1.npz")
    A = z["A"]
    assert (A != 0).all()
    dense = torch.from_numpy(A).cuda()
    runs = {}
    for name, data in (("dense", dense), ("sparse", torch.from_numpy(A).cuda().to_sparse_csr())):
        args = _args(tmp_path / name, MPI_comm(None, 1, 1))
        args.rng = "device"
        os.makedirs(str(tmp_path / name), exist_ok=True)
        nmfk = PyNMFk(data, factors=None, params=args)
        runs[name] = (nmfk.fit(), nmfk)
    blk = runs["sparse"][1].A_ij
    assert blk.is_sparse_block and blk.nnz == A.size
    for p in range(6):
        d = sample(dense, 0.03, "uniform", seed=p * 1000).fit()
        s = sample(blk, 0.03, "uniform", seed=p * 1000, sparse=runs["sparse"][1].sweep).fit()
        assert torch.equal(_bits(s.val), _bits(d.reshape(-1))) and torch.equal(_bits(s.t_val), _bits(d.t().reshape(-1))), p
    assert runs["sparse"][0] == runs["dense"][0] == 3
    for k in range(1, 6):
        es, ed = runs["sparse"][1].stats[k]["avgErr"], runs["dense"][1].stats[k]["avgErr"]
        print("k=%d avgErr sparse %.6g dense %.6g rel diff %.3g" % (k, es, ed, es / ed - 1))
        if k <= 3:
            assert abs(es / ed - 1) < 0.05, k
        if k <= 2:
            assert abs(es / float(z["k%d_avgErr" % k]) - 1) < 0.05, k
    assert np.min(runs["sparse"][1].stats[3]["clusterSilhouetteCoefficients"]) > 0.8


MISSING_SEED = 7


def missing_problem():
    """Planted rank 3, 120 x 90 (three Gaussian bumps over the rows times uniform H, 1 % noise), 40 % observed -- NOT at random:
    a position is observed with probability 0.6 where row and column have the same parity and 0.2 elsewhere, so the pattern
    itself carries structure that zero-filling turns into data (a mask drawn uniformly at random only scales the matrix in
    expectation, and the zero-filled sweep finds the rank as well).  The draw was checked on the CPU before its seed was fixed,
    with the float64-accumulating operator set of tests/_sparse_nmfk.py over the rules of tests/_masked.py (300 iterations, the
    parameters of _missing_args): the masked sweep estimates 3 (minimum silhouettes 1.0 / 0.97 / 0.97 / -0.45 / -0.49 at
    k = 1..5), the zero-filled sweep of the same entries 2 (1.0 / 0.99 / 0.55 / 0.49 / 0.48).  Seed 8 gives 3 and 2 as well."""
    rs = np.random.RandomState(MISSING_SEED)
    m, n, k = 120, 90, 3
    x = np.arange(m)[:, None]
    W = np.exp(-0.5 * ((x - m * (np.arange(k)[None, :] + 0.5) / k) / (m / 10.0)) ** 2)
    A = (W @ rs.rand(k, n) + 0.01 * rs.rand(m, n)).astype(np.float32)
    same = (np.arange(m)[:, None] % 2) == (np.arange(n)[None, :] % 2)
    return A, rs.rand(m, n) < np.where(same, 0.6, 0.2)


def _missing_args(tmp, missing):
    from pydnmfk_amd.dist_comm import MPI_comm
    from tests.test_nmfk_cpu import _args
    os.makedirs(str(tmp), exist_ok=True)
    args = _args(tmp, MPI_comm(None, 1, 1))                    # mu / fro, k = 1..5, 6 perturbations
    assert (args.method, args.norm, args.start_k, args.end_k, args.perturbations) == ("mu", "fro", 1, 5, 6)
    if missing:
        args.missing = missing
    return args


def test_missing_data_sweep_finds_the_planted_rank(tmp_path):
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._masked import observed
    A, mask = missing_problem()
    assert 0.35 < mask.mean() < 0.45
    S = observed(A, mask)
    zero = PyNMFk(S, params=_missing_args(tmp_path / "zero", None))
    assert zero.A_ij.missing is None
    assert zero.fit() != 3                                     # precondition: read as zeros, the same entries do not give the rank
    nmfk = PyNMFk(S, params=_missing_args(tmp_path / "masked", "unstored"))
    assert nmfk.A_ij.missing == "unstored" and nmfk.A_ij.nnz == int(mask.sum())
    assert nmfk.fit() == 3


def _sparse_counts():
    """integer counts with planted rank 3, about 35 % of the positions zero; row 4 and column 9 empty"""
    rs = np.random.RandomState(12)
    lam = 6.0 * rs.rand(60, 3) @ rs.rand(3, 40)
    A = np.where(rs.rand(60, 40) < 0.65, rs.poisson(lam), 0).astype(np.float32)
    A[4, :] = 0
    A[:, 9] = 0
    return A


def _small_args(tmp, comms=None, **extra):
    """`comms`: the fits' grid (default: the 1 x 1 grid of a one-process job)"""
    from pydnmfk_amd.dist_comm import MPI_comm
    from tests.test_nmfk_cpu import _args
    os.makedirs(str(tmp), exist_ok=True)
    args = _args(tmp, comms if comms is not None else MPI_comm(None, 1, 1))
    args.start_k, args.end_k, args.itr, args.perturbations = 2, 3, 60, 4
    for key, val in extra.items():
        setattr(args, key, val)
    return args


def test_prune_drops_the_empty_rows_of_every_perturbed_copy(tmp_path):
    """prune=True: a perturbed block has its source's pattern, so every fit prunes the same rows / columns; their error is nan"""
    from pydnmfk_amd.pyDNMFk import PyNMFk
    A = _sparse_counts()
    nmfk = PyNMFk(sp.csr_matrix(A), params=_small_args(tmp_path, prune=True))
    assert nmfk.fit() in (2, 3)
    for k in (2, 3):
        st = nmfk.stats[k]
        assert np.isfinite(st["avgErr"]) and np.asarray(st["L_err"]).shape == (40,)
        assert np.isnan(st["L_err"][9]) and np.isfinite(np.delete(st["L_err"], 9)).all()
    assert tuple(nmfk.AvgW.shape) == (60, 3) and not np.asarray(nmfk.AvgW.cpu() if hasattr(nmfk.AvgW, "cpu") else nmfk.AvgW)[4].any()


def test_poisson_sampling_on_integer_counts(tmp_path):
    from pydnmfk_amd.pyDNMFk import PyNMFk, sample
    A = _sparse_counts()
    A = A[np.arange(60) != 4][:, np.arange(40) != 9]
    nmfk = PyNMFk(torch.from_numpy(A).cuda().to_sparse_csr(), params=_small_args(tmp_path, sampling="poisson", rng="device"))
    blk = nmfk.A_ij
    per = sample(blk, 0.03, "poisson", seed=1000, sparse=nmfk.sweep).fit()
    assert per.col is blk.col and per.nnz == blk.nnz and torch.equal(per.val, per.val.round()) and not torch.equal(per.val, blk.val)
    assert (per.val == 0).any()                                # a draw of 0 stays stored
    assert torch.equal(per.to_dense().t().contiguous()[blk.to_dense().t() != 0], per.t_val)
    assert nmfk.fit() in (2, 3)
    assert all(np.isfinite(nmfk.stats[k]["L_err"]).all() and 0 < nmfk.stats[k]["avgErr"] < 1 for k in (2, 3))


def _split_rank(rank, world, port, q, results_root):
    try:
        import torch.distributed as dist
        from pydnmfk_amd.dist_comm import COMM_WORLD, SoloGrid
        from pydnmfk_amd.pyDNMFk import PyNMFk
        torch.cuda.set_device(0)
        if world > 1:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        if world > 1:
            # every rank holds the whole matrix on a 1 x 1 grid of its own; the job's communicator is the world (tests/_mp.py)
            comms = SoloGrid(rank)
            args = _small_args(os.path.join(results_root, "w%d" % world), comms=comms, nmfk_split="perturbations")
            args.size, args.rank, args.comm1 = world, rank, COMM_WORLD()
        else:
            args = _small_args(os.path.join(results_root, "w%d" % world))
        nmfk = PyNMFk(sp.csr_matrix(_sparse_counts()), params=args)
        nopt = nmfk.fit()
        q.put((rank, (int(nopt), {k: {key: np.asarray(v) for key, v in st.items()} for k, st in nmfk.stats.items()}), None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, None, traceback.format_exc()))


def test_perturbations_shared_by_two_ranks_equal_the_one_rank_sweep(tmp_path):
    """nmfk_split='perturbations' with world = 2 on the one GPU: the gathered factors are dense, the statistics the one-rank run's"""
    import torch.multiprocessing as mp
    from tests._mp import collect, free_port
    outs = {}
    for world in (1, 2):
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = free_port()
        procs = [ctx.Process(target=_split_rank, args=(r, world, port, q, str(tmp_path))) for r in range(world)]
        for p in procs:
            p.start()
        res = collect(procs, q, 300)
        for rank, out, err in res:
            assert err is None, "rank %d failed:\n%s" % (rank, err)
        outs[world] = [out for _, out, _ in sorted(res, key=lambda r: r[0])]
    one = outs[1][0]
    for o in outs[2]:
        assert o[0] == one[0]
        for k in one[1]:
            for key, val in one[1][k].items():
                assert np.allclose(np.asarray(o[1][k][key]), np.asarray(val), rtol=1e-12, atol=0, equal_nan=True), (k, key)


def test_cli_spnpz_nmfk_end_to_end(tmp_path, golden_dir):
    """main.py --ftype spnpz --process=pyDNMFk: a scipy.sparse.save_npz file in, the estimate and the per-k results out"""
    z = np.load(golden_dir + "/nmfk_1x1.npz")
    A = z["A"].astype(np.float32).copy()
    A[A < np.quantile(A, 0.1)] = 0                              # a tenth of the entries become (true) zeros
    sp.save_npz(str(tmp_path / "synth.npz"), sp.csr_matrix(A))
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--process=pyDNMFk", "--p_r=1", "--p_c=1", "--fpath=%s/" % tmp_path,
           "--fname=synth", "--ftype=spnpz", "--itr=100", "--norm=fro", "--method=mu", "--start_k=2", "--end_k=3", "--perturbations=4",
           "--noise_var=0.03", "--sill_thr=0.8", "--results_path=%s/res/" % tmp_path]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Estimated k with NMFk is" in out.stdout
    for k in (2, 3):
        base = tmp_path / "res" / "synth" / str(k)
        assert (base / "W_reg_factors" / "W_0.npy").exists() and (base / "H_reg_factors" / "H_0.npy").exists()
        assert np.load(base / "W_reg_factors" / "W_0.npy").shape == (A.shape[0], k)
