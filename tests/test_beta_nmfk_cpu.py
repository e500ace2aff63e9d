"""NMFk under a beta-divergence (`params.norm = 'beta'`) without a GPU: the sweep on the float64 checker operator set
(tests/_beta_nmfk.py::BetaNmfkOracleOps) on the planted problem, the identities of the per-column statistic
(PyNMF.beta_column_divergence), the statistic on 1D grids under gloo against the whole-matrix statement, the statistics a sweep adds,
what it refuses, and the perturbation-shared sweep."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _beta as B  # noqa: E402
from tests import _beta_nmfk as K  # noqa: E402
from tests import _is as I  # noqa: E402
from tests import _is_nmfk as KI  # noqa: E402

EPS64 = float(np.finfo(np.float64).eps)


# ---- (a) the planted rank
@pytest.mark.parametrize("beta, want", [(-0.75, 3), (1.5, 2)], ids=lambda v: str(v))
def test_beta_sweep_on_the_planted_problem(beta, want, tmp_path):
    """scaled_problem(1): rank 3, column scales over three decades, gamma(10) multiplicative noise; numpy input, mu, k = 1..5,
    6 perturbations, 300 iterations, sill_thr 0.8.  Measured minimum silhouettes at k = 1..5:
    beta = -0.75: 1.0 / 0.43 / 0.91 / -0.07 / -0.24 (estimate 3);  beta = 1.5: 1.0 / 0.97 / 0.67 / 0.36 / 0.03 (estimate 2: towards the
    Frobenius end of the family the large columns carry the objective, as under norm='fro' and 'kl')"""
    from pydnmfk_amd.pyDNMFk import PyNMFk
    A = K.scaled_problem(1)
    assert A.shape == (120, 90) and A.dtype == np.float32 and A.min() > 0
    nmfk = PyNMFk(A, params=K.sweep_args(tmp_path, beta), ops=K.BetaNmfkOracleOps())
    assert nmfk.params.norm == "beta" and nmfk.beta == beta and nmfk._batch_size() == 1
    got = nmfk.fit()
    print("scaled_problem(1) norm=beta beta=%g: estimate %d, minimum silhouettes %s" % (beta, got, K.min_silhouettes(nmfk)))
    assert got == want, (beta, got, K.min_silhouettes(nmfk))


# ---- (b) identities
def _one_rank(A, W0, H0, k, itr, beta, **kw):
    from pydnmfk_amd.pyDNMF import PyNMF
    nmf = PyNMF(A, factors=[W0.copy(), H0.copy()], params=B.one_rank_args(k, itr, beta, **kw), ops=K.BetaNmfkOracleOps())
    nmf.fit()
    return nmf


def test_beta_two_is_half_the_squared_column_error():
    """float64 data on the checker set: beta_column_divergence() at beta = 2 equals column_err()^2 / 2 to 1e-12 (the eps in s' = W H + eps
    is 2.2e-16 there, against residuals of 1e-2)"""
    A, W0, H0, k = B.problem()
    nmf = _one_rank(A, W0, H0, k, 20, 2.0)
    stat, err = nmf.beta_column_divergence(), np.asarray(nmf.column_err(), dtype=np.float64)
    d = float(np.max(np.abs(stat - 0.5 * err ** 2) / (0.5 * err ** 2)))
    print("beta = 2: statistic against column_err()^2 / 2: %.2e" % d)
    assert stat.shape == (A.shape[1],) and d <= 1e-12, d


def test_beta_zero_is_renamed_and_swept_as_itakura_saito(tmp_path):
    """norm='beta' with beta = 0 is norm='is': the same statistics keys and numbers as a sweep constructed under norm='is', L_err being
    is_column_divergence()'s (the float64 statement of tests/_is_nmfk.py)"""
    from pydnmfk_amd.pyDNMFk import PyNMFk
    A = K.scaled_problem(1)
    got = PyNMFk(A, params=K.small_args(tmp_path / "beta0", 0.0), ops=K.BetaNmfkOracleOps())
    assert got.params.norm == "is" and got._is and not got._beta
    ref = PyNMFk(A, params=KI.small_args(tmp_path / "is"), ops=K.BetaNmfkOracleOps())
    assert got.fit() == ref.fit()
    for k in (2, 3):
        assert set(got.stats[k]) == set(ref.stats[k]) and "is_div" in got.stats[k] and "beta_div" not in got.stats[k]
        assert np.array_equal(got.stats[k]["L_err"], ref.stats[k]["L_err"]) and got.stats[k]["is_div"] == ref.stats[k]["is_div"]
    want = KI.column_div(A, np.asarray(got.AvgW), np.asarray(got.AvgH)) / A.shape[0]
    assert np.linalg.norm(got.stats[3]["L_err"] - want) <= 1e-10 * np.linalg.norm(want)


@pytest.mark.parametrize("beta", [-1.0, 0.5, 3.0], ids=lambda b: "beta=%g" % b)
def test_the_statistic_does_not_see_a_columns_scale(beta):
    """a column of A and of H scaled by 10: numerator and denominator both scale by 10^beta; only eps in s' = W H + eps breaks the
    exactness (the fit's eps against the model values), so the statistic changes by less than 1e-3 relative (measured
    3e-4 on the issue's problem); the unscaled sums themselves change by 10^beta"""
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = B.problem()
    base = _one_rank(A, W0, H0, k, 20, beta)
    W, H = np.asarray(base.W_i, dtype=np.float64), np.asarray(base.H_j, dtype=np.float64)
    s0 = base.beta_column_divergence()
    A2, H2 = A.copy(), H.copy()
    A2[:, 4] *= 10.0
    H2[:, 4] *= 10.0
    nmf = PyNMF(A2, factors=[W.copy(), H2], params=B.one_rank_args(k, 0, beta), ops=K.BetaNmfkOracleOps())
    s1 = nmf.beta_column_divergence()
    d = float(np.max(np.abs(s1 - s0) / s0))
    print("beta=%g: column 4 of A and H times 10 changes the statistic by %.2e (column 4: %.2e)" % (beta, d, abs(s1[4] - s0[4]) / s0[4]))
    assert d < 1e-3, (beta, d)
    n0, n1 = K.column_sums(A, W, H, beta)[0][4], K.column_sums(A2, W, H2, beta)[0][4]
    assert abs(n1 / n0 / 10.0 ** beta - 1) < 1e-3                                        # (the sums do see it)


def test_the_statistic_is_reported_under_beta_only():
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = I.problem()
    for norm, hint in (("kl", "norm='kl'"), ("is", "is_column_divergence")):
        nmf = PyNMF(A.astype(np.float32), factors=[W0, H0], params=I.one_rank_args(k, 2, norm=norm), ops=K.BetaNmfkOracleOps())
        with pytest.raises(ValueError, match="beta_column_divergence.*%s" % hint):
            nmf.beta_column_divergence()


def test_a_column_without_a_positive_entry_is_nan():
    """beta > 0, prune off: a column of zeros has no scale to divide by -- nan, as from column_err()"""
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = B.problem()
    A = A.astype(np.float32)
    A[:, 6] = 0.0
    nmf = PyNMF(A, factors=[W0.astype(np.float32), H0.astype(np.float32)], params=B.one_rank_args(k, 3, 1.5, prune=False), ops=K.BetaNmfkOracleOps())
    nmf.fit()
    stat = nmf.beta_column_divergence()
    assert np.isnan(stat[6]) and np.isfinite(np.delete(stat, 6)).all()


# ---- (c) the statistic on grids
@pytest.mark.parametrize("grid", [(2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_statistic_on_grids_equals_the_whole_matrix_statement(grid):
    """float64 data on two gloo ranks, beta in {-1, 0.5, 3}: the statistic of every column equals the whole-matrix float64 statement from
    the assembled factors to 1e-10 (the bound of tests/_is.py for float64 grids) and is identical on both ranks; the numerators add up to
    beta_divergence() to 1e-12 (statistic times the statement's own denominator, so the check is on the reported numbers)"""
    for beta, (A, W, H, cols, divs) in K.run_colstat(grid, (-1.0, 0.5, 3.0), use_hip=False).items():
        n = A.shape[1]
        num, _, pw = K.column_sums(A, W, H, beta, EPS64)
        ref = num / pw
        assert len(cols) == 2 and np.array_equal(cols[0], cols[1]) and divs[0] == divs[1]
        d = np.linalg.norm(cols[0] - ref) / np.linalg.norm(ref)
        s = abs((cols[0] * pw).sum() - divs[0]) / divs[0]
        print("beta=%g statistic %dx%d: against the whole matrix %.2e, sum of the numerators against beta_divergence %.2e" % ((beta,) + grid + (d, s)))
        assert cols[0].shape == (n,) and (cols[0] > 0).all()
        assert d <= 1e-10 and s <= 1e-12, (grid, beta, d, s)


# ---- (d) statistics and refusals
def test_statistics_of_a_sweep_and_its_results_file(tmp_path):
    from pydnmfk_amd.data_io import read_cluster_results
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._ops_double import OracleOps
    A = K.scaled_problem(1)
    beta = -0.75
    nmfk = PyNMFk(A, params=K.small_args(tmp_path / "beta", beta), ops=K.BetaNmfkOracleOps())
    assert nmfk.params.norm == "beta" and nmfk._batch_size() == 1
    nmfk.fit()
    for k in (2, 3):
        st = nmfk.stats[k]
        assert len(st["beta_div"]) == 4 and np.isfinite(st["beta_div"]).all() and min(st["beta_div"]) > 0
        assert st["avgDiv"] == float(np.mean(st["beta_div"])) and st["beta"] == beta and "is_div" not in st
        assert np.asarray(st["L_err"]).shape == (90,) and np.isfinite(st["L_err"]).all() and (np.asarray(st["L_err"]) > 0).all()
        assert len(st["recon_err"]) == 4 and 0 < st["avgErr"] < 1 and np.isfinite(st["AIC"])             # (the Frobenius definitions)
        z = read_cluster_results(str(tmp_path / "beta") + "/results/synth/%d/" % k)
        assert np.array_equal(z["beta_div"], np.asarray(st["beta_div"])) and float(z["avgDiv"]) == st["avgDiv"] and float(z["beta"]) == beta
        assert np.array_equal(z["L_err"], st["L_err"])
    # L_err is the statistic of the regression fit's factors (the last k's are still held): the float64 statement
    ref = K.column_stat(A, np.asarray(nmfk.AvgW), np.asarray(nmfk.AvgH), beta)
    assert np.linalg.norm(nmfk.stats[3]["L_err"] - ref) <= 1e-10 * np.linalg.norm(ref)
    fro = PyNMFk(A, params=KI.small_args(tmp_path / "fro", norm="fro"), ops=OracleOps())
    fro.fit()
    for k in (2, 3):
        assert not {"beta_div", "avgDiv", "beta", "is_div"} & set(fro.stats[k])
        z = read_cluster_results(str(tmp_path / "fro") + "/results/synth/%d/" % k)
        assert sorted(z) == sorted(["clusterSilhouetteCoefficients", "avgSilhouetteCoefficients", "L_err", "L_errDist", "avgErr", "ErrTol", "AIC"])


class _NoFlag(K.BetaNmfkOracleOps):
    name = "no-flag"
    beta_nmfk = False


def test_refusals_at_construction_name_what_is_refused(tmp_path):
    from pydnmfk_amd.pyDNMFk import PyNMFk
    sp = pytest.importorskip("scipy.sparse")
    A = K.scaled_problem(1)
    ops = K.BetaNmfkOracleOps()

    def args(beta=0.5, **kw):
        return K.sweep_args(tmp_path, beta, **kw)

    a = args()
    a.p_r = a.p_c = 2
    with pytest.raises(NotImplementedError, match="norm='beta'.*2D grid"):
        PyNMFk(A, params=a, ops=ops)
    with pytest.raises(NotImplementedError, match="norm='beta'.*k = 129"):
        PyNMFk(A, params=args(end_k=129), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='beta'.*sparse"):
        PyNMFk(sp.csr_matrix(A), params=args(), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='beta'.*missing='nan'"):
        PyNMFk(A, params=args(missing="nan"), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='beta'.*hals"):
        PyNMFk(A, params=args(method="hals"), ops=ops)
    for beta in (-1.0, -0.0001):
        with pytest.raises(NotImplementedError, match="norm='beta'.*sampling='poisson'"):
            PyNMFk(A, params=args(beta, sampling="poisson"), ops=ops)
    Z = A.copy()
    Z[5, 6] = 0.0
    with pytest.raises(ValueError, match="norm='beta'.*beta = -1.*strictly positive"):
        PyNMFk(Z, params=args(-1.0), ops=ops)
    PyNMFk(Z, params=args(0.5), ops=ops)                                                  # a zero is data for beta > 0
    Z[5, 6] = -0.5
    with pytest.raises(ValueError, match="norm='beta'.*beta = 0.5.*non-negative"):
        PyNMFk(Z, params=args(0.5), ops=ops)
    with pytest.raises(ValueError, match="norm='beta' needs params.beta"):
        PyNMFk(A, params=KI.sweep_args(tmp_path, "beta"), ops=ops)
    for beta in (4.5, -2.01, float("nan")):
        with pytest.raises(ValueError, match="norm='beta'.*outside the accepted range"):
            PyNMFk(A, params=args(beta), ops=ops)
    # an operator set without the operation, or without the flag, is named -- before anything else is looked at
    with pytest.raises(NotImplementedError, match="^PyNMFk with norm='beta' is not provided by operator set 'oracle-beta'"):
        PyNMFk(A, params=args(), ops=B.BetaOracleOps())
    with pytest.raises(NotImplementedError, match="^PyNMFk with norm='beta' is not provided by operator set 'no-flag'"):
        PyNMFk(sp.csr_matrix(A), params=args(7.0, method="hals"), ops=_NoFlag())
    # Poisson sampling of non-negative data is accepted for beta > 0
    nmfk = PyNMFk(A, params=args(1.0, sampling="poisson"), ops=ops)
    assert nmfk._beta and nmfk.beta == 1.0 and nmfk.sampling == "poisson"


def test_the_engine_names_which_operator_sets_sweep():
    """the fp32 set has the operation and the flag; the split (bf16x6) and float64 sets do not sweep under norm='beta'"""
    from pydnmfk_amd import engine
    assert engine.HipOps.beta_nmfk is True and callable(engine.HipOps.beta_column_div)
    assert engine.HipOpsBf16x6.beta_nmfk is False
    assert not getattr(engine.HipOpsF64, "beta_nmfk", False) and not hasattr(engine.HipOpsF64, "beta_column_div")


# ---- (e) the perturbation split
def test_perturbations_shared_by_two_ranks_equal_the_one_rank_sweep(tmp_path):
    """nmfk_split='perturbations' on two gloo ranks at beta = 0.5: every statistic, the divergences of the perturbations' fits among
    them, is the one-rank sweep's (rtol 1e-9 with equal_nan, as tests/_is_nmfk.py::assert_split_equals_one_rank holds its split)"""
    K.assert_split_equals_one_rank(K.run_split(tmp_path, use_hip=False))
