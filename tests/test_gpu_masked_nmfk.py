"""NMFk over dense data with NaN-marked gaps (`params.missing = 'nan'`) on the GPU: the masked per-column error
(csrc/dnmf_sums.h: col_sums_kernel<KT, FAST, MaskedErrTerm>) on exact operands element by element and on random data against float64, the perturbation
of a NaN-marked tensor, the whole masked fit as one library call (dnmf_masked_mu_fit) against the step loop, and the sweeps through
pydnmfk_amd.pyDNMFk."""
import ctypes
import os
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

from tests import _exact as E  # noqa: E402
from tests import _masked as M  # noqa: E402
from tests import _masked_dense as D  # noqa: E402
from tests import _masked_nmfk as N  # noqa: E402

EPS = M.EPS
HUGE = 3.0e38                                              # finite poison: read as data it would swamp any sum


def _ops():
    from pydnmfk_amd.engine import HIP_MASKED_OPS
    assert HIP_MASKED_OPS.masked_nmfk
    return HIP_MASKED_OPS


def _block(An):
    from pydnmfk_amd.masked import MaskedDenseBlock
    return MaskedDenseBlock(torch.from_numpy(np.ascontiguousarray(An)).cuda())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _plan(m, n, k):
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 3)()
    assert lib.dnmf_masked_column_err_plan(m, n, k, out) == 0
    return N.colerr_reach(m, n, out)


# ------------------------------------------------------------------------------------------------------------- the kernel, exact
def _colerr_into(Ap, Wp, Hp, k, aligned):
    """dnmf_masked_column_err on views, num and den poisoned float64 views themselves: (num, den) after the check that nothing outside
    them was written"""
    from pydnmfk_amd._lib import check, lib
    m, n = Ap.rows, Ap.cols
    num, den = E.Poisoned.out(torch, 1, n, torch.float64, aligned=aligned), E.Poisoned.out(torch, 1, n, torch.float64, aligned=aligned)
    nbytes = lib.dnmf_masked_column_err_ws_bytes(m, n, k)
    ws = torch.full((nbytes // 8 + 16,), float("nan"), dtype=torch.float64, device="cuda")
    check(lib.dnmf_masked_column_err(Ap.view.data_ptr(), m, n, Ap.ld, Wp.view.data_ptr(), Wp.ld, Hp.view.data_ptr(), Hp.ld, k,
                                     num.view.data_ptr(), den.view.data_ptr(), ws.data_ptr(), nbytes, None))
    torch.cuda.synchronize()
    assert torch.isnan(ws[nbytes // 8:]).all()                                        # nothing behind the slab
    return num.check("num k=%d" % k)[0], den.check("den k=%d" % k)[0]


@pytest.mark.parametrize("shape", N.COLERR_SHAPES, ids=lambda s: "%dx%d" % s)
def test_column_err_sums_are_the_float64_integers(shape):
    """Integer A under a mask with at least two all-NaN columns (tests/test_masked_nmfk_cpu.py proves every fp32 partial an integer below
    2^24 and every float64 sum below 2^53): num and den equal the float64 integers element by element, on aligned views and on views at
    an odd base with pitch = width + 3, with finite-huge and with NaN around the views; empty columns are (0, 0); two calls are
    bit-identical; nothing outside num / den is written; and the CSR kernel under missing='unstored' gives the same numbers on the
    same observations.  The loop shapes are asserted against dnmf_masked_column_err_plan at every rank they run."""
    from pydnmfk_amd.engine import HIP_CSR_OPS
    from pydnmfk_amd.masked import MaskedDenseBlock
    from pydnmfk_amd.sparse import SparseBlock
    m, n = shape
    case = next((c for c in N.COLERR_LOOP_CASES if c["shape"] == shape), None)
    for k in N.COLERR_KS:
        if case is not None:
            p = _plan(m, n, k)
            for what, want in case["reach"].items():
                assert p[what] == want, (shape, k, what, p)
        A, mask, W, H = N.colerr_case(m, n, k)
        rn, rd = N.colerr_ref(A, mask, W, H)
        empty = mask.sum(0) == 0
        assert empty.sum() >= 2
        An = D.nan_marked(A, mask)
        for aligned, fill in ((True, float("nan")), (True, HUGE), (False, float("nan")), (False, HUGE)):
            Ap, Wp, Hp = (E.Poisoned(torch, x, aligned=aligned, fill=fill) for x in (An, W, H))
            if not aligned:
                assert all(p_.view.data_ptr() % 16 and p_.ld == p_.cols + 3 for p_ in (Ap, Wp, Hp))
            gn, gd = _colerr_into(Ap, Wp, Hp, k, aligned)
            gn2, gd2 = _colerr_into(Ap, Wp, Hp, k, aligned)
            tag = "%dx%d k=%d %s %s" % (m, n, k, "aligned" if aligned else "odd", "nan" if np.isnan(fill) else "huge")
            for got, ref, what in ((gn, rn, "num"), (gd, rd, "den")):
                bad = np.flatnonzero(got != ref)
                assert bad.size == 0, "%s %s: %d columns differ; first %d: got %r, expected %r" % (tag, what, bad.size, bad[0], got[bad[0]], ref[bad[0]])
            assert not gn[empty].any() and not gd[empty].any(), tag
            assert np.array_equal(gn.view(np.int64), gn2.view(np.int64)) and np.array_equal(gd.view(np.int64), gd2.view(np.int64)), tag
            for p_, what in ((Ap, "A"), (Wp, "W"), (Hp, "H")):                        # the operands are not written
                outside = p_.buf.cpu().numpy()[~p_.mask]
                assert (np.isnan(outside) if np.isnan(fill) else outside == np.float32(fill)).all(), (tag, what)
        # through the operator set, and against the CSR kernel on the same observations
        blk = MaskedDenseBlock(Ap.view)
        on, od = _ops().column_err_sums(blk, Wp.view, Hp.view)
        assert on.dtype == torch.float64 and tuple(on.shape) == (n,)
        assert np.array_equal(on.cpu().numpy(), rn) and np.array_equal(od.cpu().numpy(), rd)
        csr = SparseBlock.from_any(M.observed(A, mask), torch.device("cuda", 0), keep_zeros=True, missing="unstored")
        assert csr.nnz == int(mask.sum())
        Wd, Hd = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
        cn, cd = HIP_CSR_OPS.column_err_sums(csr, Wd, Hd)
        assert torch.equal(_bits(cn), _bits(on)) and torch.equal(_bits(cd), _bits(od)), (shape, k)
    d = torch.rand(9, 7, device="cuda")                                               # a plain tensor keeps the inherited path
    from pydnmfk_amd.engine import HIP_OPS
    Wd, Hd = torch.rand(9, 2, device="cuda"), torch.rand(2, 7, device="cuda")
    a, b = _ops().column_err_sums(d, Wd, Hd), HIP_OPS.column_err_sums(d, Wd, Hd)
    assert torch.allclose(a[0], b[0], rtol=1e-12) and torch.allclose(a[1], b[1], rtol=1e-12)


# ------------------------------------------------------------------------------------------------------------- the kernel, random
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (129, 33), (300, 257)], ids=lambda s: "%dx%d" % s)
def test_column_err_sums_against_float64(shape):
    """random data, densities 0 .. 1, k = 1 .. 128: num within the project's bound for the masked residual (1e-5 relative Frobenius),
    den within 2e-6 (one fp32 square and a 16-term fp32 sum per tile: at most 17 * 2^-24)."""
    from tests.test_gpu_masked import _observed_block
    rs = np.random.RandomState(900 + shape[0])
    m, n = shape
    worst = {"num": 0.0, "den": 0.0}
    for density in (0.0, 0.05, 0.5, 1.0):
        A, mask = _observed_block(rs, m, n, density)
        blk = _block(D.nan_marked(A, mask))
        for k in (1, 3, 16, 17, 32, 33, 64, 100, 128):
            W, H = (rs.rand(m, k) + 0.01).astype(np.float32), (rs.rand(k, n) + 0.01).astype(np.float32)
            gn, gd = (t.cpu().numpy() for t in _ops().column_err_sums(blk, torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()))
            rn, rd = N.colerr_ref(A, mask, W, H)
            assert np.isfinite(gn).all() and np.isfinite(gd).all()
            empty = mask.sum(0) == 0
            assert not gn[empty].any() and not gd[empty].any()
            dn = np.linalg.norm(gn - rn) / np.linalg.norm(rn) if rn.any() else np.abs(gn).max()
            dd = np.linalg.norm(gd - rd) / np.linalg.norm(rd) if rd.any() else np.abs(gd).max()
            worst["num"], worst["den"] = max(worst["num"], dn), max(worst["den"], dd)
            assert dn <= 1e-5 and dd <= 2e-6, (shape, density, k, dn, dd)
    print("masked column error %dx%d maxima: num %.2e den %.2e" % (m, n, worst["num"], worst["den"]))


def test_column_err_of_a_fully_observed_block_equals_the_dense_path():
    """PyNMF.column_err() under missing='nan' against the dense path on the same exact operands: float64 sums of the same exact terms"""
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests._masked import args_for
    m, n, k = 53, 37, 5
    A, W, H = E.sparse_products(np.ones((m, n), dtype=bool), k)
    comms = MPI_comm(None, 1, 1)
    got = {}
    for name, missing in (("dense", None), ("nan", "nan")):
        nmf = PyNMF(A, factors=[W, H], params=args_for(comms, 1, 1, k, 1, "fro", missing=missing))
        assert nmf._masked_dense == (missing == "nan")
        got[name] = nmf.column_err()
    assert np.isfinite(got["dense"]).all() and got["dense"].shape == (n,)
    assert np.allclose(got["nan"], got["dense"], rtol=1e-12, atol=0)
    # a column without an observation: 0 / 0, what numpy returns
    An = A.copy()
    An[:, 4] = np.nan
    err = PyNMF(An, factors=[W, H], params=args_for(comms, 1, 1, k, 1, "fro", missing="nan")).column_err()
    assert np.isnan(err[4]) and np.allclose(np.delete(err, 4), np.delete(got["dense"], 4), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------------------- perturbation
@pytest.mark.parametrize("shape", [(33, 64), (37, 23)], ids=lambda s: "%dx%d" % s)
def test_perturbation_keeps_nan_and_the_zero_filled_values(shape):
    """HipOps.perturb_uniform on a NaN-marked CUDA tensor (33 x 64: rows of whole 8-element vectors, the vector kernel; 37 x 23: the
    element kernel), also into `out=`: isnan is the source's, observed positions are bit-equal to the perturbation of the zero-filled
    tensor with the same seed"""
    from pydnmfk_amd.engine import HIP_OPS
    from pydnmfk_amd.pyDNMFk import sample
    rs = np.random.RandomState(3)
    mask = rs.rand(*shape) < 0.4
    A = (rs.rand(*shape) + 0.5).astype(np.float32)
    Xn, X0 = torch.from_numpy(D.nan_marked(A, mask)).cuda(), torch.from_numpy(np.where(mask, A, 0).astype(np.float32)).cuda()
    obs = torch.from_numpy(mask).cuda()
    for seed in (0, 1000, 2 ** 40 + 1):
        ref = HIP_OPS.perturb_uniform(X0, 0.03, seed)
        per = HIP_OPS.perturb_uniform(Xn, 0.03, seed)
        out = torch.full(shape, 7.0, device="cuda")
        into = HIP_OPS.perturb_uniform(Xn, 0.03, seed, out=out)
        assert into.data_ptr() == out.data_ptr()
        via = sample(Xn, 0.03, "uniform", seed=seed % 2 ** 32, missing="nan").fit() if seed < 2 ** 32 else per   # (`sample` seeds numpy too)
        for got in (per, into, via):
            assert torch.equal(torch.isnan(got), ~obs), seed
            assert torch.equal(_bits(got[obs]), _bits(ref[obs])), seed
        assert not torch.equal(per[obs], Xn[obs])
    poi = sample(torch.from_numpy(D.nan_marked(np.round(4 * A), mask)).cuda(), 0.03, "poisson", seed=1000, missing="nan").fit()
    assert torch.equal(torch.isnan(poi), ~obs) and torch.equal(poi[obs], poi[obs].round())


# ------------------------------------------------------------------------------------------------------------- whole fit
@pytest.mark.parametrize("shape,k", [((300, 200), 4), ((130, 97), 32)], ids=["300x200-k4", "130x97-k32"])
def test_whole_fit_equals_the_step_loop(shape, k):
    """dnmf_masked_mu_fit against fit_loop='python': the same launches in the same order, so the factors are bit-identical; recon_err
    within 1e-9 relative (both errors end in float64 atomic sums of fewer than 2^20 non-negative partials in varying order:
    2^20 * 2^-53)."""
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMF import PyNMF
    m, n = shape
    rs = np.random.RandomState(40 + k)
    mask = rs.rand(m, n) < 0.5
    mask[2, :] = False
    mask[:, 3] = False
    An = D.nan_marked((rs.rand(m, k) @ rs.rand(k, n) + 0.05).astype(np.float32), mask)
    W0, H0 = rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)
    comms = MPI_comm(None, 1, 1)
    for norm in ("fro", "kl"):
        for wu in (True, False):
            for itr in (1, 11, 30):
                out = {}
                for loop in (None, "python"):
                    args = D.args_for(comms, 1, 1, k, itr, norm, W_update=wu)
                    if loop:
                        args.fit_loop = loop
                    nmf = PyNMF(torch.from_numpy(An).cuda(), factors=[torch.from_numpy(W0).cuda(), torch.from_numpy(H0).cuda()], params=args)
                    assert nmf._ops().name == "hip-masked" and nmf._whole_fit_ok(nmf._ops()) == (loop is None)
                    out[loop] = nmf.fit()
                (W1, H1, e1), (W2, H2, e2) = out[None], out["python"]
                tag = (shape, k, norm, wu, itr)
                assert torch.isfinite(W1).all() and torch.isfinite(H1).all(), tag
                assert not torch.equal(H1.cpu(), torch.from_numpy(H0)) and not torch.equal(W1.cpu(), torch.from_numpy(W0)), tag   # (the fits ran)
                assert torch.equal(_bits(W1), _bits(W2)) and torch.equal(_bits(H1), _bits(H2)), tag
                assert abs(e1 - e2) <= 1e-9 * e2, (tag, e1, e2)
    # a 1D grid keeps the step loop
    args = D.args_for(comms, 1, 1, k, 3, "fro")
    nmf = PyNMF(torch.from_numpy(An).cuda(), params=args)
    nmf.p = 2
    assert not nmf._whole_fit_ok(nmf._ops())


# ------------------------------------------------------------------------------------------------------------- sweeps
def _missing():
    from tests.test_gpu_sparse_nmfk import missing_problem
    return missing_problem()


def test_missing_data_sweep_finds_the_planted_rank(tmp_path):
    """missing_problem() NaN-marked, numpy input: 3; zero-filled: not 3.  Wall times of the masked sweep with the whole-fit call and
    with fit_loop='python' are printed (no threshold)."""
    from pydnmfk_amd.pyDNMFk import PyNMFk
    A, mask = _missing()
    zero = PyNMFk(np.where(mask, A, 0).astype(np.float32), params=N.missing_args(tmp_path / "zero", None))
    assert zero.fit() != 3                                     # precondition: read as zeros, the same entries do not give the rank
    An = D.nan_marked(A, mask)
    walls = {}
    for loop in (None, "python"):
        args = N.missing_args(tmp_path / ("masked-%s" % loop), "nan")
        if loop:
            args.fit_loop = loop
        nmfk = PyNMFk(An, params=args)
        assert nmfk.A_ij is An and nmfk._batch_size() == 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nopt = nmfk.fit()
        torch.cuda.synchronize()
        walls[loop] = time.perf_counter() - t0
        assert nopt == 3, (loop, N.min_silhouettes(nmfk))
        assert all(np.isfinite(nmfk.stats[k]["L_err"]).all() for k in range(1, 6))
    print("missing-data sweep (120 x 90, k = 1..5, 6 perturbations, 300 iterations): %.2f s whole-fit calls, %.2f s fit_loop='python'"
          % (walls[None], walls["python"]))


def test_matrix_without_a_nan_meets_the_reference_statistics(tmp_path, golden_dir):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests.test_nmfk_cpu import _args, check_against_golden
    z = np.load(golden_dir + "/nmfk_1x1.npz")
    args = _args(tmp_path, MPI_comm(None, 1, 1))
    args.missing = "nan"
    nmfk = PyNMFk(np.ascontiguousarray(z["A"], dtype=np.float32), factors=None, params=args)
    nopt = nmfk.fit()
    assert nopt == 3
    check_against_golden(nmfk, nopt, z)


def test_two_ranks_of_a_data_grid_meet_the_reference_statistics(golden_dir):
    """nmfk_2x1.npz under missing='nan' on a 2 x 1 grid (nmfk_split='data'), both ranks on the one GPU: every fit runs the masked pairs
    with their allreduce, `column_err` fills the rank's column range and allreduces both sums; the bounds of
    tests/test_gpu_nmfk.py for this fixture on the GPU"""
    from tests.test_nmfk_cpu import check_nmfk_fixture
    check_nmfk_fixture(N.run_nmfk_golden_nan("nmfk_2x1.npz", use_hip=True, timeout=600), np.load(golden_dir + "/nmfk_2x1.npz"), tight=False)


def test_device_input_against_the_csr_sweep(tmp_path):
    """A NaN-marked CUDA tensor with params.rng = 'device' against the CSR sweep of the same observations under missing='unstored':
    the perturbed observed values are bit-equal (one keyed stream), the initial factors are the same draws, so the sweeps differ by
    summation order inside the fits only.  Both estimate 3; avgErr per k <= 3 within 0.05 (the level
    tests/test_gpu_sparse_nmfk.py::test_device_input_equals_the_dense_device_sweep holds)."""
    from pydnmfk_amd.pyDNMFk import PyNMFk, sample
    A, mask = _missing()
    Xn = torch.from_numpy(D.nan_marked(A, mask)).cuda()
    S = torch.sparse_coo_tensor(torch.from_numpy(np.stack(np.nonzero(mask))), torch.from_numpy(A[mask]), size=A.shape).cuda()
    runs = {}
    for name, data, missing in (("nan", Xn, "nan"), ("csr", S, "unstored")):
        args = N.missing_args(tmp_path / name, missing)
        args.rng = "device"
        nmfk = PyNMFk(data, factors=None, params=args)
        runs[name] = (nmfk.fit(), nmfk)
    blk = runs["csr"][1].A_ij
    assert blk.is_sparse_block and blk.nnz == int(mask.sum()) and runs["nan"][1].A_ij is Xn
    obs = torch.from_numpy(mask).cuda()
    for p in range(6):
        d = sample(Xn, 0.03, "uniform", seed=p * 1000, missing="nan").fit()
        s = sample(blk, 0.03, "uniform", seed=p * 1000, sparse=runs["csr"][1].sweep).fit()
        assert torch.equal(torch.isnan(d), ~obs) and torch.equal(_bits(s.val), _bits(d[obs])), p
    assert runs["nan"][0] == runs["csr"][0] == 3
    for k in range(1, 6):
        en, es = runs["nan"][1].stats[k]["avgErr"], runs["csr"][1].stats[k]["avgErr"]
        print("k=%d avgErr nan %.6g csr %.6g rel diff %.3g" % (k, en, es, en / es - 1))
        if k <= 3:
            assert abs(en / es - 1) < 0.05, k


def _gappy_counts():
    """integer counts with planted rank 3 and 35 % of the positions missing; column 9 without an observation"""
    rs = np.random.RandomState(12)
    lam = 6.0 * rs.rand(60, 3) @ rs.rand(3, 40)
    A = rs.poisson(lam).astype(np.float32)
    mask = rs.rand(60, 40) < 0.65
    mask[:, 9] = False
    return D.nan_marked(A, mask), mask


def _small_args(tmp, comms=None, **extra):
    from tests.test_gpu_sparse_nmfk import _small_args as base
    return base(tmp, comms, missing="nan", prune=False, **extra)


def test_poisson_sampling_on_integer_counts_with_gaps(tmp_path):
    from pydnmfk_amd.pyDNMFk import PyNMFk
    An, mask = _gappy_counts()
    nmfk = PyNMFk(torch.from_numpy(An).cuda(), params=_small_args(tmp_path, sampling="poisson", rng="device"))
    assert nmfk.fit() in (2, 3)
    seen = mask.sum(0) > 0
    for k in (2, 3):
        st = nmfk.stats[k]
        assert np.isfinite(np.asarray(st["L_err"])[seen]).all() and np.isnan(np.asarray(st["L_err"])[~seen]).all() and 0 < st["avgErr"] < 1, k


def _split_rank(rank, world, port, q, results_root):
    try:
        import torch.distributed as dist
        from pydnmfk_amd.dist_comm import COMM_WORLD, SoloGrid
        from pydnmfk_amd.pyDNMFk import PyNMFk
        torch.cuda.set_device(0)
        if world > 1:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
            comms = SoloGrid(rank)
            args = _small_args(os.path.join(results_root, "w%d" % world), comms=comms, nmfk_split="perturbations")
            args.size, args.rank, args.comm1 = world, rank, COMM_WORLD()
        else:
            args = _small_args(os.path.join(results_root, "w%d" % world))
        nmfk = PyNMFk(_gappy_counts()[0], params=args)
        nopt = nmfk.fit()
        q.put((rank, (int(nopt), {k: {key: np.asarray(v) for key, v in st.items()} for k, st in nmfk.stats.items()}), None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, None, traceback.format_exc()))


def test_perturbations_shared_by_two_ranks_equal_the_one_rank_sweep(tmp_path):
    """nmfk_split='perturbations' with world = 2 on the one GPU: the statistics are the one-rank run's (the factors are bit-identical;
    recon_err ends in float64 atomics, hence 1e-9 there and on what follows from it)"""
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
                assert np.allclose(np.asarray(o[1][k][key]), np.asarray(val), rtol=1e-9, atol=0, equal_nan=True), (k, key)
