"""NMFk under a beta-divergence (`params.norm = 'beta'`) on the GPU: the per-column kernels (csrc/dnmf_sums.h: col_sums_kernel, beta_coldiv_kernel) on
exact operands bit for bit at beta = 1 and on random data against float64 over the accepted range, its workspace contract,
PyNMF.beta_column_divergence() on one rank and on both 1D grids, the planted sweep through pydnmfk_amd.pyDNMFk from numpy and from
device input against the float64 checker set's estimate of the same array, and main.py --process pyDNMFk --norm beta.

Measured maxima (one MI355X; also in DESIGN.md section 7): see the table there -- this file prints every figure before it asserts."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _beta as B  # noqa: E402
from tests import _beta_nmfk as K  # noqa: E402
from tests import _exact as E  # noqa: E402
from tests import _is as I  # noqa: E402
from tests import _masked_nmfk as N  # noqa: E402
from tests import test_gpu_workspace as G  # noqa: E402
from tests.test_gpu_workspace import env  # noqa: E402,F401  (the module's fixture: engine and library on cuda:0)

EPS = B.EPS
HUGE = 3.0e38                                              # finite poison: read as data it would swamp any sum
BOUND = 1e-5                                               # the project's bound for the divergence (tests/test_gpu_beta.py)
LOOP_SHAPES = tuple(c["shape"] for c in N.COLERR_LOOP_CASES)
T1 = 2.0 * np.log(2.0) - 1.0                               # d_1(2 s | s) / s = 2 ln 2 - 1


def _ops():
    from pydnmfk_amd.engine import HIP_OPS
    assert HIP_OPS.beta_nmfk
    return HIP_OPS


def _plan(m, n, k):
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 3)()
    assert lib.dnmf_beta_column_div_plan(m, n, k, out) == 0
    return N.colerr_reach(m, n, out)


# ------------------------------------------------------------------------------------------------------------- the kernel, exact
def _coldiv_into(Ap, Wp, Hp, k, beta, aligned):
    """dnmf_beta_column_div on views, div and pw poisoned float64 views themselves: (div, pw) after the check that nothing outside
    them or behind the workspace was written"""
    from pydnmfk_amd._lib import check, lib
    m, n = Ap.rows, Ap.cols
    div, pw = (E.Poisoned.out(torch, 1, n, torch.float64, aligned=aligned) for _ in range(2))
    nbytes = lib.dnmf_beta_column_div_ws_bytes(m, n, k)
    ws = torch.full((nbytes // 8 + 16,), float("nan"), dtype=torch.float64, device="cuda")
    check(lib.dnmf_beta_column_div(Ap.view.data_ptr(), m, n, Ap.ld, Wp.view.data_ptr(), Wp.ld, Hp.view.data_ptr(), Hp.ld, k, EPS, beta,
                                   div.view.data_ptr(), pw.view.data_ptr(), ws.data_ptr(), nbytes, None))
    torch.cuda.synchronize()
    assert torch.isnan(ws[nbytes // 8:]).all()                                        # nothing behind the slab
    return div.check("div k=%d" % k)[0], pw.check("pw k=%d" % k)[0]


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


@pytest.mark.parametrize("shape", I.EXACT_SHAPES + LOOP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_column_sums_are_exact_at_the_planted_positions(shape):
    """beta = 1, the KL form (no power function: exactness needs only x / x == 1 and logf(1) == 0).  W, H of tests/_is.py::exact (S a
    power of two in [2, 32], eps absorbed), A = S but for a planted set where A = 2 S: a term a log(a / s) - a + s is exactly 0 where
    A = S and s * t1 where A = 2 S, t1 the value at s = 1 (scaling by a power of two commutes with every rounding of the expression),
    every fp32 partial holds at most one planted position and every float64 sum is t1 times an integer.  On aligned views and on views
    at an odd base with pitch = width + 3, inside NaN and inside finite-huge poison: columns without a planted position are exactly
    +0.0; with u = div[0] / splant[0] (column 0 has a planted position in every row block) div[c] == u * splant[c] bit for bit; u is a
    float32 within 2^-20 of 2 ln 2 - 1 (twice eight ulp of logf in the binade of 0.69; the other operations are exact); pw[c] is the
    integer sum_i a_ic exactly; two calls are bit-identical; nothing outside div and pw, behind the workspace or in the operands is
    written.  The loop shapes are asserted against the plan at every rank they run."""
    m, n = shape
    case = next((c for c in N.COLERR_LOOP_CASES if c["shape"] == shape), None)
    for k in I.EXACT_KS:
        if case is not None:
            p = _plan(m, n, k)
            for what, want in case["reach"].items():
                assert p[what] == want, (shape, k, what, p)
        A, W, H, splant, asum = K.coldiv_case(m, n, k)
        empty = splant == 0
        assert empty.sum() >= 2 and splant[0] > 0
        for aligned, fill in ((True, float("nan")), (True, HUGE), (False, float("nan")), (False, HUGE)):
            Ap, Wp, Hp = (E.Poisoned(torch, x, aligned=aligned, fill=fill) for x in (A, W, H))
            if not aligned:
                assert all(p_.view.data_ptr() % 16 and p_.ld == p_.cols + 3 for p_ in (Ap, Wp, Hp))
            g1, w1 = _coldiv_into(Ap, Wp, Hp, k, 1.0, aligned)
            g2, w2 = _coldiv_into(Ap, Wp, Hp, k, 1.0, aligned)
            tag = "%dx%d k=%d %s %s" % (m, n, k, "aligned" if aligned else "odd", "nan" if np.isnan(fill) else "huge")
            assert g1.dtype == np.float64 and w1.dtype == np.float64, tag
            assert np.array_equal(_bits(g1), _bits(g2)) and np.array_equal(_bits(w1), _bits(w2)), tag
            assert np.array_equal(_bits(g1[empty]), np.zeros(int(empty.sum()), dtype=np.int64)), (tag, g1[empty])      # +0.0
            u = g1[0] / splant[0]
            bad = np.flatnonzero(g1 != u * splant)
            assert bad.size == 0, "%s: %d columns differ; first %d: got %r, expected %r" % (tag, bad.size, bad[0], g1[bad[0]], u * splant[bad[0]])
            assert float(np.float64(np.float32(u))) == u, (tag, u)
            assert abs(u - T1) <= 2.0 ** -20, (tag, u)
            assert np.array_equal(w1, asum), (tag, np.flatnonzero(w1 != asum)[:4])
            for p_, what in ((Ap, "A"), (Wp, "W"), (Hp, "H")):                        # the operands are not written
                outside = p_.buf.cpu().numpy()[~p_.mask]
                assert (np.isnan(outside) if np.isnan(fill) else outside == np.float32(fill)).all(), (tag, what)
                assert np.array_equal(p_.view.cpu().numpy(), {"A": A, "W": W, "H": H}[what]), (tag, what)
        # through the operator set: column SUMS, float64, on the device
        got = _ops().beta_column_div(Ap.view, Wp.view, Hp.view, EPS, 1.0)
        assert all(g.dtype == torch.float64 and g.is_cuda and tuple(g.shape) == (n,) for g in got)
        assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(g1)) and np.array_equal(_bits(got[1].cpu().numpy()), _bits(w1)), (shape, k)


@pytest.mark.parametrize("beta", [-1.0, 2.0, 3.0], ids=lambda b: "beta=%g" % b)
def test_integer_beta_on_the_planted_operands_is_recorded(beta):
    """the general form at an integer beta on the same operands (every a and s a power of two): the answers are exact IF log2f and exp2f
    are exact at powers of two and at small integers, which is not documented.  Recorded (printed), not asserted, as
    tests/test_gpu_beta.py::test_integer_beta_on_power_of_two_operands_is_recorded does; the sums stay within BOUND of float64 -- div[c]
    of the magnitudes of its terms, pw[c] of itself"""
    for m, n in I.EXACT_SHAPES:
        for k in I.EXACT_KS:
            A, W, H, _, _ = K.coldiv_case(m, n, k)
            ref, scale, pw_ref = K.column_sums(A, W, H, beta, 0.0)                   # (eps is absorbed: s' == s in float32)
            Ap, Wp, Hp = (E.Poisoned(torch, x, aligned=False) for x in (A, W, H))
            div, pw = _coldiv_into(Ap, Wp, Hp, k, beta, False)
            exact = np.array_equal(div, ref) and np.array_equal(pw, pw_ref)
            dd, dp = float(np.max(np.abs(div - ref) / scale)), float(np.max(np.abs(pw - pw_ref) / pw_ref))
            print("beta=%g %dx%d k=%d on power-of-two operands: %s (div %.2e of its terms, pw %.2e)"
                  % (beta, m, n, k, "exact, column by column" if exact else "not exact", dd, dp))
            assert dd <= BOUND and dp <= BOUND, (beta, m, n, k, dd, dp)


# ------------------------------------------------------------------------------------------------------------- the kernel, random
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (129, 33), (300, 257)], ids=lambda s: "%dx%d" % s)
def test_column_sums_against_float64(shape):
    """random data (tests/test_gpu_beta.py::_random_problem; A with exact zeros for beta > 0), k = 1 .. 128, beta over the accepted
    range and 0: div[c] within BOUND of the column's sum of the magnitudes of the float64 terms (the project's bound for the divergence,
    applied as tests/test_gpu_beta.py applies it), pw[c] within BOUND of itself, and the column sums add up to dnmf_beta_divergence
    within BOUND of the magnitudes of all terms"""
    from tests.test_gpu_beta import _random_problem, _with_zeros
    m, n = shape
    worst = {"div": (0.0, 0.0), "pw": (0.0, 0.0), "sum": (0.0, 0.0)}
    for k in (1, 3, 16, 17, 32, 33, 64, 100, 128):
        A0, W, H = _random_problem(m, n, k)
        Wd, Hd = (torch.from_numpy(x).cuda() for x in (W, H))
        for beta in B.GPU_BETAS + (0.0,):
            A = _with_zeros(A0) if beta > 0 else A0
            Ad = torch.from_numpy(A).cuda()
            div, pw = (x.cpu().numpy() for x in _ops().beta_column_div(Ad, Wd, Hd, EPS, beta))
            ref, scale, pw_ref = K.column_sums(A, W, H, beta)
            assert div.shape == (n,) and pw.shape == (n,) and np.isfinite(div).all() and np.isfinite(pw).all()
            dd = float(np.max(np.abs(div - ref) / scale))
            dp = float(np.max(np.abs(pw - pw_ref) / np.where(pw_ref > 0, pw_ref, 1.0)))
            total = float(_ops().beta_divergence(Ad, Wd, Hd, EPS, beta).cpu())
            ds = abs(div.sum() - total) / B.divergence_scale(A, W, H, beta)
            for key, val in (("div", dd), ("pw", dp), ("sum", ds)):
                worst[key] = max(worst[key], (val, beta))
            assert dd <= BOUND and dp <= BOUND and ds <= BOUND, (shape, k, beta, dd, dp, ds)
    print("beta column sums %dx%d maxima (value, at beta):" % shape, {k_: "%.2e at %g" % v for k_, v in sorted(worst.items())})


# ------------------------------------------------------------------------------------------------------------- workspace contract
def _coldiv_ws_case(shape, k):
    m, n = shape

    def make(engine, lib):
        ops = engine.HIP_OPS
        A, W, H, splant, asum = K.coldiv_case(m, n, k)
        Ap, Wp, Hp = G._P(A), G._P(W), G._P(H)
        ref, scale, pw_ref = K.column_sums(A, W, H, 0.5, 0.0)

        @G._nout(4)
        def call():
            d1, p1 = ops.beta_column_div(Ap.view, Wp.view, Hp.view, EPS, 1.0)
            d2, p2 = ops.beta_column_div(Ap.view, Wp.view, Hp.view, EPS, 0.5)
            return [x.cpu().numpy() for x in (d1, p1, d2, p2)]

        def chk(d1, p1, d2, p2, w):
            u = d1[0] / splant[0]
            assert not d1[splant == 0].any() and np.array_equal(d1, u * splant) and abs(u - T1) <= 2.0 ** -20, (w, u)
            assert np.array_equal(p1, asum), w
            assert np.max(np.abs(d2 - ref) / scale) <= BOUND and np.max(np.abs(p2 - pw_ref) / pw_ref) <= BOUND, w
        S = G.Steps()
        S.add("beta column div", call, chk)
        return S.prob()
    return G.Case("beta-coldiv-%dx%d-k%d" % (m, n, k), ("dnmf_beta_column_div",), make, align16=True,
                  query=lambda lib: {lib.dnmf_beta_column_div_ws_bytes(m, n, k)})


WS_CASES = [_coldiv_ws_case((200, 136), 5), _coldiv_ws_case(LOOP_SHAPES[1], 32)]


@pytest.mark.parametrize("case", WS_CASES, ids=[c.id for c in WS_CASES])
def test_column_div_workspace_contract(env, case):  # noqa: F811
    """poisoned, zeroed, 0x7F-filled and leftover workspaces of exactly the query, four times the query and a 16-byte base: the driver
    of tests/test_gpu_workspace.py"""
    G.test_workspace_contract(env, case)


# ------------------------------------------------------------------------------------------------------------- PyNMF
@pytest.mark.parametrize("grid", [(1, 1), (2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_pynmf_statistic_on_one_rank_and_on_grids(grid):
    """50 x 39, k = 3, 20 steps at beta in {0.5, 3}, the ranks of a grid stacked on the one GPU (one time limit per rank process): the
    statistic of every column within 1e-5 of the float64 statement from the returned factors, identical on every rank"""
    for beta, (A, W, H, cols, divs) in K.run_colstat(grid, (0.5, 3.0), use_hip=True, timeout=300).items():
        ref = K.column_stat(A, W, H, beta)
        assert len(cols) == grid[0] * grid[1] and all(np.array_equal(c, cols[0]) for c in cols) and len(set(divs)) == 1
        d = float(np.linalg.norm(cols[0] - ref) / np.linalg.norm(ref))
        print("beta=%g statistic (gpu) %dx%d: against float64 %.2e" % ((beta,) + grid + (d,)))
        assert cols[0].shape == (A.shape[1],) and d <= 1e-5, (grid, beta, d)


# ------------------------------------------------------------------------------------------------------------- sweeps
SWEEP_BETA = -0.75
_CHECKER = {}


def _checker_estimate(tmp):
    """the float64 checker set's sweep of scaled_problem(1) at SWEEP_BETA (about 2 s on the CPU), once per process"""
    if not _CHECKER:
        from pydnmfk_amd.pyDNMFk import PyNMFk
        nmfk = PyNMFk(K.scaled_problem(1), params=K.sweep_args(tmp / "checker", SWEEP_BETA), ops=K.BetaNmfkOracleOps())
        _CHECKER["nopt"] = int(nmfk.fit())
        print("beta=%g sweep, checker set: estimate %d, minimum silhouettes %s" % (SWEEP_BETA, _CHECKER["nopt"], K.min_silhouettes(nmfk)))
    return _CHECKER["nopt"]


@pytest.mark.parametrize("source", ["numpy", "device"])
def test_planted_sweep_estimates_what_the_checker_set_estimates(source, tmp_path):
    """scaled_problem(1) at beta = -0.75, from a numpy array and from a CUDA tensor (params.rng = 'device': perturbed and initialised on
    the device, another draw): the estimate is the checker set's on the same array, 3; L_err is the float64 recomputation from AvgW /
    AvgH within 1e-5; every statistic is finite"""
    from pydnmfk_amd.pyDNMFk import PyNMFk
    want = _checker_estimate(tmp_path)
    assert want == 3
    A = K.scaled_problem(1)
    X = A if source == "numpy" else torch.from_numpy(A).cuda()
    nmfk = PyNMFk(X, params=K.sweep_args(tmp_path / source, SWEEP_BETA, **({} if source == "numpy" else {"rng": "device"})))
    assert nmfk.A_ij is X and nmfk._batch_size() == 1 and nmfk.params.norm == "beta"
    nopt = nmfk.fit()
    print("beta=%g sweep (gpu, %s input): estimate %d, minimum silhouettes %s" % (SWEEP_BETA, source, nopt, K.min_silhouettes(nmfk)))
    AvgW, AvgH = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (nmfk.AvgW, nmfk.AvgH))
    ref = K.column_stat(A, AvgW, AvgH, SWEEP_BETA)                                      # (k = 5: the last of the sweep)
    d = float(np.linalg.norm(nmfk.stats[5]["L_err"] - ref) / np.linalg.norm(ref))
    print("beta=%g sweep (gpu, %s input): L_err at k = 5 against float64 %.2e" % (SWEEP_BETA, source, d))
    assert nopt == want, (source, nopt, K.min_silhouettes(nmfk))
    assert d <= 1e-5, (source, d)
    for k in range(1, 6):
        st = nmfk.stats[k]
        assert np.isfinite(st["L_err"]).all() and len(st["beta_div"]) == 6 and np.isfinite(st["beta_div"]).all() and np.isfinite(st["avgDiv"])
        assert st["beta"] == SWEEP_BETA


# ------------------------------------------------------------------------------------------------------------- main.py
def test_main_pydnmfk_norm_beta_end_to_end(tmp_path):
    """main.py --process pyDNMFk --norm beta --beta 0.5 on one rank, in a fresh child process under its own time limit: reads a .npy,
    sweeps k = 2..3 on the GPU and writes a results file per k with the norm's keys"""
    import os
    import subprocess
    import sys
    from pydnmfk_amd.data_io import read_cluster_results
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    np.save(tmp_path / "spectra.npy", K.scaled_problem(1))
    cmd = [sys.executable, os.path.join(root, "main.py"), "--process=pyDNMFk", "--p_r=1", "--p_c=1", "--fpath=%s/" % tmp_path,
           "--fname=spectra", "--ftype=npy", "--start_k=2", "--end_k=3", "--itr=60", "--perturbations=4", "--sill_thr=0.8", "--norm=beta",
           "--beta=0.5", "--method=mu", "--init=rand", "--results_path=%s/res/" % tmp_path]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Rank estimated by NMFk" in out.stdout, out.stdout[-1000:]
    found = 0
    for dirpath, _, files in os.walk(tmp_path / "res"):
        if files and os.path.basename(dirpath) in ("2", "3"):
            z = read_cluster_results(dirpath + "/")
            assert len(np.asarray(z["beta_div"])) == 4 and float(z["beta"]) == 0.5 and np.isfinite(np.asarray(z["L_err"])).all()
            assert np.asarray(z["L_err"]).shape == (90,)
            found += 1
    assert found == 2, (found, out.stdout[-1000:])


# ------------------------------------------------------------------------------------- one walk, one term: 'is' and beta = 0 agree
@pytest.mark.parametrize("k", [3, 40, 100], ids=lambda k: "k=%d" % k)
def test_is_and_beta_zero_share_their_bits(k):
    """The Itakura-Saito entry points and the beta ones at beta = 0 run the same tile walks (csrc/dnmf_sums.h: tile_sum_kernel and
    col_sums_kernel) with the same term, BetaDivTerm<BETA_DIV_IS, .> -- the per-column walk once with one sum per column and once with
    two.  On strictly positive random operands, 70 x 300 (three column blocks, the last ragged; three 32-row blocks, the last ragged; a
    partly filled last workgroup), KT = 1, 2, 4, on contiguous tensors and on views at an odd base with an odd pitch (the generic
    loads): is_divergence == beta_divergence(., 0.0) and is_column_div == beta_column_div(., 0.0)[0] bit for bit, and the second
    output, the column's sum of a^0, is the row count.  No tolerance."""
    m, n = 70, 300
    rs = np.random.RandomState(1000 + k)
    A, W, H = (rs.uniform(0.25, 2.0, s).astype(np.float32) for s in ((m, n), (m, k), (k, n)))
    ops = _ops()
    for aligned in (True, False):
        if aligned:
            Ad, Wd, Hd = (torch.from_numpy(x).cuda() for x in (A, W, H))
        else:
            Ad, Wd, Hd = (E.Poisoned(torch, x, aligned=False, fill=float("nan"), ld=x.shape[1] + 3 + x.shape[1] % 2).view for x in (A, W, H))
            assert all(t.data_ptr() % 16 and t.stride(0) % 2 == 1 for t in (Ad, Wd, Hd))
        d_is = ops.is_divergence(Ad, Wd, Hd, EPS).cpu().numpy()
        d_b0 = ops.beta_divergence(Ad, Wd, Hd, EPS, 0.0).cpu().numpy()
        c_is = ops.is_column_div(Ad, Wd, Hd, EPS).cpu().numpy()
        c_b0, pw = (x.cpu().numpy() for x in ops.beta_column_div(Ad, Wd, Hd, EPS, 0.0))
        tag = "k=%d %s" % (k, "contiguous" if aligned else "odd views")
        print("%s: divergence %r / %r, column sums differ in %d of %d" % (tag, d_is[0], d_b0[0], int((_bits(c_is) != _bits(c_b0)).sum()), n))
        assert np.isfinite(d_is).all() and d_is[0] > 0.0 and np.isfinite(c_is).all() and (c_is > 0.0).all(), tag
        assert np.array_equal(_bits(d_is), _bits(d_b0)), (tag, d_is, d_b0)
        assert c_is.shape == (n,) and np.array_equal(_bits(c_is), _bits(c_b0)), (tag, np.flatnonzero(c_is != c_b0)[:4])
        assert np.array_equal(pw, np.full(n, float(m))), (tag, np.flatnonzero(pw != m)[:4])
