"""The beta-divergence (`params.norm = 'beta'`, `params.beta`) without a GPU: the choreography (dist_nmf.BETA_MU_update) with the
float64 checker operator set of tests/_beta.py through PyNMF on one rank and on gloo 1D grids against the whole-matrix float64
statement, the divergence along a fit for every beta (with zeros in the data for beta > 0), beta = 0 as norm='is', every refusal, the
ValueErrors for beta and for the data on both ranks of a grid, main.py's flags."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _beta as B  # noqa: E402
from tests import _is as I  # noqa: E402
from tests._golden import rel_fro  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = float(np.finfo(np.float64).eps)


# ---- 0. the statement itself
def test_the_statement_meets_the_named_members_of_the_family():
    """gamma at the branch points; the divergence at beta = 2 is half the squared error, at beta -> 1 and beta -> 0 it tends to the KL and
    Itakura-Saito forms; the pair at beta = 0 is the Itakura-Saito pair of tests/_is.py"""
    assert [B.gamma(b) for b in (-2, -1, 0, 0.5, 1, 1.5, 2, 3, 4)] == [0.25, 1 / 3, 0.5, 1 / 1.5, 1, 1, 1, 0.5, 1 / 3]
    A, W, H, k = B.problem()
    S = W @ H + B.EPS
    assert abs(B.divergence(A, W, H, 2.0) - 0.5 * np.sum((A - S) ** 2)) <= 1e-12 * B.divergence(A, W, H, 2.0)
    assert abs(B.divergence(A, W, H, 1.0) - np.sum(A * np.log(A / S) - A + S)) <= 1e-12 * B.divergence(A, W, H, 1.0)
    assert abs(B.divergence(A, W, H, 0.0) - I.divergence(A, W, H)) <= 1e-12 * I.divergence(A, W, H)
    for beta, limit in ((1.0, 1.0 + 1e-6), (0.0, 1e-6)):
        assert abs(B.divergence(A, W, H, limit) - B.divergence(A, W, H, beta)) <= 1e-4 * B.divergence(A, W, H, beta)
    for side in ("w", "h"):
        for got, ref in zip(B.pair(A, W, H, side, 0.0), I.pair(A, W, H, side)):
            assert rel_fro(got, ref) <= 1e-14
    Az = B.problem(zeros=0.2)[0]
    assert np.isfinite(B.divergence(Az, W, H, 0.5)) and np.isfinite(B.divergence(Az, W, H, 1.0)) and np.isfinite(B.divergence(Az, W, H, 3.0))


# ---- 1. grids against the whole-matrix statement
@pytest.fixture(scope="module")
def reference_fits():
    return B.reference_fits(B.CPU_BETAS, eps=EPS64)        # (float64 data: PyNMF's eps is the float64 machine epsilon, pyDNMF.py:68)


@pytest.mark.parametrize("grid", [(1, 1), (2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_grids_against_the_whole_matrix_statement(grid, reference_fits):
    """50 x 39, k = 3, 20 iterations, beta in {-1, 0.5, 1, 1.5, 3}, W_update on and off, in float64 from end to end: each grid's
    factors, error and divergence equal the whole-matrix statement to 1e-10 (the bound of the Itakura-Saito suite for the same
    construction); replicated factors agree bit for bit between the ranks (run_grid asserts it)"""
    got = B.run_grid(grid, B.CPU_BETAS, use_hip=False)
    assert set(got) == set(reference_fits)
    for (beta, wu), (Wr, Hr, err_r, div_r, _) in reference_fits.items():
        W, H, err, div = got[(beta, wu)]
        assert W.dtype == np.float64 and H.dtype == np.float64
        dw, dh, de, dd = rel_fro(W, Wr), rel_fro(H, Hr), abs(err - err_r) / err_r, abs(div - div_r) / div_r
        print("beta=%g %dx%d W_update=%s: dW=%.2e dH=%.2e derr=%.2e ddiv=%.2e (err %.6g, D %.6g)"
              % ((beta,) + grid + (wu, dw, dh, de, dd, err_r, div_r)))
        assert dw <= 1e-10 and dh <= 1e-10 and de <= 1e-10 and dd <= 1e-10, (grid, beta, wu, dw, dh, de, dd)
    A, W0, H0, k = B.problem()
    s = W0.sum(axis=0)
    for beta in B.CPU_BETAS:
        assert not np.array_equal(got[(beta, True)][0], got[(beta, False)][0])     # W_update=False: W moved by the normalisation only
        assert rel_fro(got[(beta, False)][0], W0 / (s + EPS64)) <= 1e-14
    assert not np.array_equal(got[(0.5, True)][1], got[(1.5, True)][1])            # beta reaches the rule


def test_float32_data_take_the_same_path_in_float32():
    """the checker set on float32 data (the dtype of the HIP kernels): float32 factors come back, close to the float64 statement"""
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = B.problem()
    nmf = PyNMF(A.astype(np.float32), factors=[W0, H0], params=B.one_rank_args(k, 20, 0.5), ops=B.BetaOracleOps())
    assert nmf.norm == "beta" and nmf.beta == 0.5 and nmf.c_dtype == torch.float32 and not nmf._whole_fit_ok(nmf._ops())
    W, H, err = nmf.fit()
    Wr, Hr, err_r = B.fit(A.astype(np.float32), W0.astype(np.float32), H0.astype(np.float32), 0.5, 20)
    assert W.dtype == np.float32 and rel_fro(W, Wr) <= 1e-5 and rel_fro(H, Hr) <= 1e-5 and abs(err - err_r) <= 1e-5 * err_r


# ---- 2. the divergence never increases
@pytest.mark.parametrize("zeros", [0.0, 0.2], ids=["positive", "a fifth zeros"])
@pytest.mark.parametrize("beta", B.CPU_BETAS, ids=lambda b: "beta=%g" % b)
def test_the_divergence_never_increases_along_a_fit(beta, zeros):
    """50 steps of the choreography, the divergence read by PyNMF.beta_divergence() after each: no step increases it (the
    majorisation-minimisation form), and it equals the statement's at every step; with 20 % zeros in A for beta > 0"""
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    if zeros and beta <= 0:
        with pytest.raises(ValueError, match="strictly positive"):
            A, W0, H0, k = B.problem(zeros=zeros)
            PyNMF(A, factors=[W0, H0], params=B.one_rank_args(k, 50, beta), ops=B.BetaOracleOps())
        return
    A, W0, H0, k = B.problem(zeros=zeros)
    nmf = PyNMF(A, factors=[W0, H0], params=B.one_rank_args(k, 50, beta), ops=B.BetaOracleOps())
    d = [nmf.beta_divergence()]
    assert abs(d[0] - B.divergence(A, W0, H0, beta, EPS64)) <= 1e-12 * d[0]
    W, H = W0, H0
    for i in range(50):
        nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update(clamp=(i % 10 == 0))
        W, H = B.step(A, W, H, beta, EPS64, True, clamp=(i % 10 == 0))
        d.append(nmf.beta_divergence())
        assert abs(d[-1] - B.divergence(A, W, H, beta, EPS64)) <= 1e-10 * d[-1], i
    rel = np.diff(d) / np.array(d[:-1])
    print("beta=%g zeros=%g divergence: %.6g -> %.6g over 50 steps; relative change per step between %.3e and %.3e"
          % (beta, zeros, d[0], d[-1], rel.min(), rel.max()))
    assert np.all(np.diff(d) <= 0), rel.max()
    assert d[-1] < 0.9 * d[0]


# ---- 3. beta = 0 is norm='is'
def test_beta_zero_is_handed_to_the_itakura_saito_path():
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = B.problem()
    nmf = PyNMF(A, factors=[W0, H0], params=B.one_rank_args(k, 7, 0.0), ops=B.BetaOracleOps())
    assert nmf.norm == "is" and nmf.params.norm == "is" and nmf._is and not nmf._beta
    got = nmf.fit()
    ref = PyNMF(A, factors=[W0, H0], params=I.one_rank_args(k, 7), ops=B.BetaOracleOps()).fit()
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    assert nmf.is_divergence() > 0
    with pytest.raises(ValueError, match="beta_divergence.*norm='is'"):
        nmf.beta_divergence()
    with pytest.raises(ValueError, match="strictly positive"):                       # and keeps that path's data check
        PyNMF(B.problem(zeros=0.2)[0], factors=[W0, H0], params=B.one_rank_args(k, 7, 0), ops=B.BetaOracleOps())


# ---- 4. the refusals
def test_refusals_name_the_norm_and_the_combination():
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._ops_double import OracleOps
    sp = pytest.importorskip("scipy.sparse")
    A, W0, H0, k = B.problem()
    A = A.astype(np.float32)
    ops = B.BetaOracleOps()

    def args(k, itr, **kw):
        return B.one_rank_args(k, itr, kw.pop("beta", 0.5), **kw)
    with pytest.raises(NotImplementedError, match="norm='beta'.*2D grid"):
        PyNMF(A, params=args(k, 3, grid=(2, 2)), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='beta'.*sparse"):
        PyNMF(sp.csr_matrix(A), params=args(k, 3), ops=ops)
    An = A.copy()
    An[3, 4] = np.nan
    with pytest.raises(NotImplementedError, match="norm='beta'.*missing='nan'"):
        PyNMF(An, params=args(k, 3, missing="nan"), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='beta'.*missing='unstored'"):
        PyNMF(sp.csr_matrix(A), params=args(k, 3, missing="unstored"), ops=ops)
    # float64 data: refused unless the operator set names the dtype (the HIP sets name float32 alone; OracleOps names none)
    with pytest.raises(NotImplementedError, match="norm='beta'.*float64"):
        PyNMF(A.astype(np.float64), params=args(k, 3), ops=OracleOps())
    with pytest.raises(NotImplementedError, match="norm='beta'.*float64"):
        PyNMF(A.astype(np.float64), params=args(k, 3), ops=I.ISOracleOps())             # (the Itakura-Saito operations are not these)
    with pytest.raises(NotImplementedError, match="norm='beta'.*bfloat16"):
        PyNMF(torch.from_numpy(A).to(torch.bfloat16), params=args(k, 3), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='beta'.*bfloat16"):
        PyNMF(A, params=args(k, 3, precision="bfloat16"), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='beta'.*bf16x6"):
        PyNMF(A, params=args(k, 3, gemm="bf16x6"), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='beta'.*k = 129"):
        PyNMF(np.ones((4, 200), dtype=np.float32), params=args(129, 3), ops=ops)
    for method in ("hals", "bcd"):
        with pytest.raises(NotImplementedError, match="norm='beta'.*%s" % method):
            PyNMF(A, params=args(k, 3, method=method), ops=ops)
    with pytest.raises(NotImplementedError, match="PyNMFk.*norm='beta'"):
        PyNMFk(A, params=args(k, 3), ops=ops)
    # the choreography refuses by itself, whatever PyNMF let through
    t = [torch.from_numpy(x) for x in (A, W0.astype(np.float32), H0.astype(np.float32))]
    for method in ("hals", "bcd"):
        a = args(k, 3, method=method)
        a.m, a.n, a.eps = A.shape[0], A.shape[1], B.EPS
        with pytest.raises(NotImplementedError, match="norm='beta'.*%s" % method):
            nmf_algorithms_1D(*t, params=a, ops=ops).update()
    a = args(k, 3)
    a.m, a.n, a.eps = A.shape[0], A.shape[1], B.EPS
    with pytest.raises(NotImplementedError, match="norm='beta'.*oracle-double"):        # an operator set without the operations is named
        nmf_algorithms_1D(*t, params=a, ops=OracleOps()).update()
    a.beta = None
    with pytest.raises(ValueError, match="norm='beta'.*params.beta"):
        nmf_algorithms_1D(*t, params=a, ops=ops).update()
    # the bf16x6 operator set names no dtype for these operations
    from pydnmfk_amd import engine
    assert engine.HipOps.beta_dtypes == (torch.float32,) and engine.HipOpsBf16x6.beta_dtypes == ()
    for name in ("beta_aht_pair", "beta_wta_pair", "beta_pair_into", "beta_update_w", "beta_update_h", "beta_ratio_update",
                 "beta_divergence", "beta_fit"):
        assert callable(getattr(engine.HipOps, name)), name
    # fit_batch runs such fits one by one
    fits = [PyNMF(A, factors=[W0, H0], params=args(k, 4), ops=ops) for _ in range(2)]
    one = PyNMF(A, factors=[W0, H0], params=args(k, 4), ops=ops).fit()
    for res in PyNMF.fit_batch(fits):
        assert np.array_equal(res[0], one[0]) and np.array_equal(res[1], one[1]) and res[2] == one[2]
    # beta_divergence belongs to norm='beta'
    with pytest.raises(ValueError, match="beta_divergence.*norm='kl'"):
        PyNMF(A, factors=[W0, H0], params=args(k, 3, norm="kl"), ops=ops).beta_divergence()


@pytest.mark.parametrize("beta", [-2.5, 4.001, 7.5, float("nan"), float("inf")], ids=lambda b: "beta=%g" % b)
def test_beta_outside_the_range_is_a_value_error_naming_the_range(beta):
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = B.problem()
    with pytest.raises(ValueError, match=r"-2 <= beta <= 4"):
        PyNMF(A, factors=[W0, H0], params=B.one_rank_args(k, 3, beta), ops=B.BetaOracleOps())


def test_the_ends_of_the_range_are_accepted():
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = B.problem()
    for beta in B.BETA_RANGE:
        W, H, err = PyNMF(A, factors=[W0, H0], params=B.one_rank_args(k, 5, beta), ops=B.BetaOracleOps()).fit()
        Wr, Hr, err_r = B.fit(A, W0, H0, beta, 5, EPS64)
        assert rel_fro(W, Wr) <= 1e-10 and rel_fro(H, Hr) <= 1e-10 and abs(err - err_r) <= 1e-10 * err_r, beta


def test_a_missing_beta_is_a_value_error():
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = B.problem()
    args = I.one_rank_args(k, 3, norm="beta")
    assert getattr(args, "beta", None) is None
    with pytest.raises(ValueError, match="norm='beta' needs params.beta"):
        PyNMF(A, factors=[W0, H0], params=args, ops=B.BetaOracleOps())


# (beta, the bad entry, what the message must name): a zero is bad under beta <= 0 only, a negative entry under every beta
BAD_DATA = [(-1.0, 0.0, "strictly positive"), (-1.0, -0.5, "strictly positive"), (0.5, -0.5, "non-negative"), (3.0, -0.5, "non-negative")]


@pytest.mark.parametrize("beta,value,word", BAD_DATA, ids=lambda v: "%g" % v if isinstance(v, float) else None)
def test_one_rank_refuses_bad_data(beta, value, word):
    (rank, (name, text)), = I.spawn(B._bad_rank, (1, 1), (False, beta, value))
    assert name == "ValueError" and word in text and ("%g" % value) in text and ("beta = %g" % beta) in text, (name, text)


def test_a_zero_is_legal_data_for_positive_beta():
    (rank, (name, text)), = I.spawn(B._bad_rank, (1, 1), (False, 0.5, 0.0))
    assert name is None, (name, text)


@pytest.mark.parametrize("beta,value,word", BAD_DATA[:1] + BAD_DATA[2:3], ids=lambda v: "%g" % v if isinstance(v, float) else None)
def test_every_rank_of_a_grid_refuses_bad_data_together(beta, value, word):
    """2 x 1: the bad entry sits in the LAST rank's slice; both ranks raise the ValueError (rank 0 names its own, legal, minimum and the
    count of bad ranks), and no rank is left in a collective: both come back within the time limit of spawn()"""
    res = I.spawn(B._bad_rank, (2, 1), (False, beta, value), timeout=120)
    assert [r for r, _ in res] == [0, 1]
    for rank, (name, text) in res:
        assert name == "ValueError" and word in text and "1 of 2 ranks" in text, (rank, name, text)
    assert ("block is %g (" % value) in res[1][1][1] and ("block is %g (" % value) not in res[0][1][1]


@pytest.mark.parametrize("beta,match", [(5.0, "-2 <= beta <= 4"), (None, "needs params.beta")], ids=["range", "missing"])
def test_every_rank_of_a_grid_refuses_a_bad_beta(beta, match):
    res = I.spawn(B._bad_rank, (2, 1), (False, beta, None), timeout=120)
    assert [r for r, _ in res] == [0, 1]
    for rank, (name, text) in res:
        assert name == "ValueError" and match in text, (rank, name, text)


# ---- 5. main.py --norm beta --beta
def test_main_has_the_beta_flags():
    sys.path.insert(0, ROOT)
    try:
        import main as cli
    finally:
        sys.path.remove(ROOT)
    (text,) = [row[4] for row in cli.FLAGS if row[0] == "norm"]
    assert "beta" in text.replace(",", " ").replace("/", " ").split()
    (row,) = [row for row in cli.FLAGS if row[0] == "beta"]
    assert row[1] is float and row[2] is None and "-2 <= beta <= 4" in row[4]
    args = cli.build_parser().parse_args(["--p_r=1", "--p_c=1", "--norm=beta", "--beta=0.5"])
    assert args.norm == "beta" and args.beta == 0.5
    assert cli.build_parser().parse_args(["--p_r=1", "--p_c=1"]).beta is None
