"""NMFk under the Itakura-Saito objective (`params.norm = 'is'`) on the GPU: the per-column divergence (csrc/dnmf_sums.h:
col_sums_kernel with the term BetaDivTerm<BETA_DIV_IS, 1>) on exact operands bit for bit and on random data against float64, PyNMF.is_column_divergence() on one rank and on
both 1D grids, the planted sweep through pydnmfk_amd.pyDNMFk from numpy and from device input, and the perturbation split."""
import ctypes
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _exact as E  # noqa: E402
from tests import _is as I  # noqa: E402
from tests import _is_nmfk as K  # noqa: E402
from tests import _masked_nmfk as N  # noqa: E402

EPS = I.EPS
HUGE = 3.0e38                                              # finite poison: read as data it would swamp any sum
BOUND = 1e-5                                               # the project's bound for the IS divergence (tests/test_gpu_is.py)
LOOP_SHAPES = tuple(c["shape"] for c in N.COLERR_LOOP_CASES)


def _ops():
    from pydnmfk_amd.engine import HIP_OPS
    assert HIP_OPS.is_nmfk
    return HIP_OPS


def _plan(m, n, k):
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 3)()
    assert lib.dnmf_is_column_div_plan(m, n, k, out) == 0
    return N.colerr_reach(m, n, out)


# ------------------------------------------------------------------------------------------------------------- the kernel, exact
def _coldiv_into(Ap, Wp, Hp, k, aligned):
    """dnmf_is_column_div on views, div a poisoned float64 view itself: div after the check that nothing outside it or behind the
    workspace was written"""
    from pydnmfk_amd._lib import check, lib
    m, n = Ap.rows, Ap.cols
    div = E.Poisoned.out(torch, 1, n, torch.float64, aligned=aligned)
    nbytes = lib.dnmf_is_column_div_ws_bytes(m, n, k)
    ws = torch.full((nbytes // 8 + 16,), float("nan"), dtype=torch.float64, device="cuda")
    check(lib.dnmf_is_column_div(Ap.view.data_ptr(), m, n, Ap.ld, Wp.view.data_ptr(), Wp.ld, Hp.view.data_ptr(), Hp.ld, k, EPS,
                                 div.view.data_ptr(), ws.data_ptr(), nbytes, None))
    torch.cuda.synchronize()
    assert torch.isnan(ws[nbytes // 8:]).all()                                        # nothing behind the slab
    return div.check("div k=%d" % k)[0]


@pytest.mark.parametrize("shape", I.EXACT_SHAPES + LOOP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_column_divergence_is_exact_at_the_planted_positions(shape):
    """W, H of tests/_is.py::exact (S a power of two in [2, 32], eps absorbed), A = S but for a planted set where A = 2 S: q is exactly
    1 or 2 (v_rcp_f32 is exact at powers of two), a term exactly 0 or t2 = 1 - logf(2), every fp32 partial 0 or t2 (at most one planted
    position per column and 32-row block) and every float64 sum count * t2 exactly.  On aligned views and on views at an odd base with
    pitch = width + 3, inside NaN and inside finite-huge poison: columns without a planted position are exactly 0.0; with
    u = div[0] / count[0] (column 0 has one in every row block) div[c] == count[c] * u bit for bit; u is a float32 within 2^-21 of
    1 - ln 2 (eight ulp of logf in the binade of 0.69; the subtraction from 1 is exact); two calls are bit-identical; nothing outside
    div, behind the workspace or in the operands is written.  The loop shapes are asserted against the plan at every rank they run."""
    m, n = shape
    case = next((c for c in N.COLERR_LOOP_CASES if c["shape"] == shape), None)
    for k in I.EXACT_KS:
        if case is not None:
            p = _plan(m, n, k)
            for what, want in case["reach"].items():
                assert p[what] == want, (shape, k, what, p)
        A, W, H, count = K.coldiv_case(m, n, k)
        empty = count == 0
        assert empty.sum() >= 2 and count[0] == -(-m // 32)
        for aligned, fill in ((True, float("nan")), (True, HUGE), (False, float("nan")), (False, HUGE)):
            Ap, Wp, Hp = (E.Poisoned(torch, x, aligned=aligned, fill=fill) for x in (A, W, H))
            if not aligned:
                assert all(p_.view.data_ptr() % 16 and p_.ld == p_.cols + 3 for p_ in (Ap, Wp, Hp))
            g1 = _coldiv_into(Ap, Wp, Hp, k, aligned)
            g2 = _coldiv_into(Ap, Wp, Hp, k, aligned)
            tag = "%dx%d k=%d %s %s" % (m, n, k, "aligned" if aligned else "odd", "nan" if np.isnan(fill) else "huge")
            assert g1.dtype == np.float64 and np.array_equal(g1.view(np.int64), g2.view(np.int64)), tag
            assert np.array_equal(g1[empty].view(np.int64), np.zeros(int(empty.sum()), dtype=np.int64)), (tag, g1[empty])      # +0.0
            u = g1[0] / count[0]
            bad = np.flatnonzero(g1 != count * u)
            assert bad.size == 0, "%s: %d columns differ; first %d: got %r, expected %r" % (tag, bad.size, bad[0], g1[bad[0]], count[bad[0]] * u)
            assert float(np.float64(np.float32(u))) == u, (tag, u)
            assert abs(u - (1.0 - np.log(2.0))) <= 2.0 ** -21, (tag, u)
            for p_, what in ((Ap, "A"), (Wp, "W"), (Hp, "H")):                        # the operands are not written
                outside = p_.buf.cpu().numpy()[~p_.mask]
                assert (np.isnan(outside) if np.isnan(fill) else outside == np.float32(fill)).all(), (tag, what)
                assert np.array_equal(p_.view.cpu().numpy(), {"A": A, "W": W, "H": H}[what]), (tag, what)
        # through the operator set: column SUMS, float64, on the device
        got = _ops().is_column_div(Ap.view, Wp.view, Hp.view, EPS)
        assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (n,)
        assert np.array_equal(got.cpu().numpy().view(np.int64), g1.view(np.int64)), (shape, k)


# ------------------------------------------------------------------------------------------------------------- the kernel, random
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (129, 33), (300, 257)], ids=lambda s: "%dx%d" % s)
def test_column_divergence_against_float64(shape):
    """random positive data (tests/test_gpu_is.py::_random_problem), k = 1 .. 128: within the project's bound for the IS divergence
    (1e-5 relative, the same term with 16 fp32 terms per partial instead of 64); the column sums add up to is_divergence() within
    8e-6 (the two kernels' fp32 partials of at most 64 non-negative terms each are within 64 * 2^-24)."""
    from tests.test_gpu_is import _random_problem
    m, n = shape
    worst = {"columns": 0.0, "sum": 0.0}
    for k in (1, 3, 16, 17, 32, 33, 64, 100, 128):
        A, W, H = _random_problem(m, n, k)
        Ad, Wd, Hd = (torch.from_numpy(x).cuda() for x in (A, W, H))
        got = _ops().is_column_div(Ad, Wd, Hd, EPS).cpu().numpy()
        ref = K.column_div(A, W, H)
        assert got.shape == (n,) and np.isfinite(got).all()
        d = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        total = float(_ops().is_divergence(Ad, Wd, Hd, EPS).cpu())
        s = abs(got.sum() - total) / total
        worst["columns"], worst["sum"] = max(worst["columns"], d), max(worst["sum"], s)
        assert d <= BOUND and s <= 8e-6, (shape, k, d, s)
    print("is column divergence %dx%d maxima: against float64 %.2e, sum against is_divergence %.2e" % (m, n, worst["columns"], worst["sum"]))


# ------------------------------------------------------------------------------------------------------------- PyNMF
@pytest.mark.parametrize("grid", [(1, 1), (2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_pynmf_column_divergence_on_one_rank_and_on_grids(grid):
    """50 x 39, k = 3, 20 steps, the ranks of a grid stacked on the one GPU (one time limit per rank process): the mean divergence
    per entry of every column within 1e-5 of the float64 statement from the returned factors, identical on every rank"""
    A, W, H, cols, divs = K.run_coldiv(grid, use_hip=True, timeout=300)
    m, n = A.shape
    ref = K.column_div(A, W, H) / m
    assert len(cols) == grid[0] * grid[1] and all(np.array_equal(c, cols[0]) for c in cols) and len(set(divs)) == 1
    d = float(np.linalg.norm(cols[0] - ref) / np.linalg.norm(ref))
    print("is column divergence (gpu) %dx%d: against float64 %.2e; sum x m against is_divergence %.2e"
          % (grid + (d, abs(cols[0].sum() * m - divs[0]) / divs[0])))
    assert cols[0].shape == (n,) and d <= 1e-5, (grid, d)


# ------------------------------------------------------------------------------------------------------------- sweeps
def test_planted_sweep_estimates_three(tmp_path):
    """scaled_problem(1), numpy input: 3 through the whole-fit call and through fit_loop='python' (wall times printed, no threshold);
    L_err is the float64 recomputation from AvgW / AvgH within 1e-5.  (The Frobenius and KL sweeps of this array estimate 2:
    tests/test_is_nmfk_cpu.py)"""
    from pydnmfk_amd.pyDNMFk import PyNMFk
    A = K.scaled_problem(1)
    walls = {}
    for loop in (None, "python"):
        args = K.sweep_args(tmp_path / ("is-%s" % loop))
        if loop:
            args.fit_loop = loop
        nmfk = PyNMFk(A, params=args)
        assert nmfk.A_ij is A and nmfk._batch_size() == 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nopt = nmfk.fit()
        torch.cuda.synchronize()
        walls[loop] = time.perf_counter() - t0
        print("is sweep (%s): estimate %d, minimum silhouettes %s" % (loop or "whole-fit calls", nopt, K.min_silhouettes(nmfk)))
        assert nopt == 3, (loop, K.min_silhouettes(nmfk))
        ref = K.column_div(A, np.asarray(nmfk.AvgW), np.asarray(nmfk.AvgH)) / A.shape[0]             # (k = 5: the last of the sweep)
        d = float(np.linalg.norm(nmfk.stats[5]["L_err"] - ref) / np.linalg.norm(ref))
        print("is sweep (%s): L_err at k = 5 against float64 %.2e" % (loop or "whole-fit calls", d))
        assert d <= 1e-5, (loop, d)
        for k in range(1, 6):
            st = nmfk.stats[k]
            assert np.isfinite(st["L_err"]).all() and len(st["is_div"]) == 6 and np.isfinite(st["is_div"]).all() and np.isfinite(st["avgDiv"])
    print("is sweep (120 x 90, k = 1..5, 6 perturbations, 300 iterations): %.2f s whole-fit calls, %.2f s fit_loop='python'"
          % (walls[None], walls["python"]))


def test_device_input_sweep_completes_with_finite_statistics(tmp_path):
    """a CUDA tensor with params.rng = 'device': the sweep completes, every statistic is finite, the perturbed copies are strictly
    positive.  The estimate is printed, not asserted: the device stream is another draw, and on the CPU two of eight draws of this
    problem family miss."""
    from pydnmfk_amd.pyDNMFk import PyNMFk, sample
    X = torch.from_numpy(K.scaled_problem(1)).cuda()
    nmfk = PyNMFk(X, params=K.sweep_args(tmp_path, rng="device"))
    assert nmfk.A_ij is X
    nopt = nmfk.fit()
    print("is sweep, device input: estimate %d, minimum silhouettes %s" % (nopt, K.min_silhouettes(nmfk)))
    assert 1 <= nopt <= 5
    for k in range(1, 6):
        for key, val in nmfk.stats[k].items():
            val = val.detach().cpu().numpy() if isinstance(val, torch.Tensor) else np.asarray(val, dtype=np.float64)
            assert np.isfinite(val).all(), (k, key)
    for p in range(6):
        per = sample(X, 0.03, "uniform", seed=p * 1000).fit()
        assert per.is_cuda and float(per.min()) > 0.0 and not torch.equal(per, X), p


def test_perturbations_shared_by_two_ranks_equal_the_one_rank_sweep(tmp_path):
    """nmfk_split='perturbations' with two processes on the one GPU: the statistics are the one-rank sweep's (rtol 1e-9)"""
    K.assert_split_equals_one_rank(K.run_split(tmp_path, use_hip=True))
