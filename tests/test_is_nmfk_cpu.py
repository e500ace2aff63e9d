"""NMFk under the Itakura-Saito objective (`params.norm = 'is'`) without a GPU: the sweep on the float64 checker operator set
(tests/_is_nmfk.py::ISNmfkOracleOps) finds the planted rank where the Frobenius and KL sweeps of the same array do not,
PyNMF.is_column_divergence() on 1D grids under gloo against the whole-matrix statement, the statistics a sweep adds and what it
refuses, and the perturbation-shared sweep."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _is as I  # noqa: E402
from tests import _is_nmfk as K  # noqa: E402

EPS64 = float(np.finfo(np.float64).eps)


# ---- (a) the planted rank
def test_is_sweep_finds_the_planted_rank_where_fro_and_kl_do_not(tmp_path):
    """scaled_problem(1): rank 3, column scales over three decades, gamma(10) multiplicative noise; numpy input, mu, k = 1..5,
    6 perturbations, 300 iterations, sill_thr 0.8.  Measured minimum silhouettes at k = 1..5:
    IS 1.0 / 0.87 / 0.90 / -0.16 / -0.30 (estimate 3), Frobenius 1.0 / 0.97 / 0.73 / 0.49 / 0.19 (2), KL 1.0 / 0.97 / 0.57 / 0.23 / -0.18 (2)"""
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._ops_double import OracleOps
    A = K.scaled_problem(1)
    assert A.shape == (120, 90) and A.dtype == np.float32 and A.min() > 0
    got = {}
    for norm, ops in (("is", K.ISNmfkOracleOps()), ("fro", OracleOps()), ("kl", OracleOps())):
        nmfk = PyNMFk(A, params=K.sweep_args(tmp_path / norm, norm), ops=ops)
        got[norm] = nmfk.fit()
        print("scaled_problem(1) norm=%s: estimate %d, minimum silhouettes %s" % (norm, got[norm], K.min_silhouettes(nmfk)))
    assert got == {"is": 3, "fro": 2, "kl": 2}, got


# ---- (b) the column divergence on grids
@pytest.mark.parametrize("grid", [(2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_column_divergence_on_grids_equals_the_whole_matrix_statement(grid):
    """float64 data on two gloo ranks: the mean divergence per entry of every column equals the whole-matrix float64 statement from
    the assembled factors to 1e-10 (the bound of tests/_is.py for float64 grids), is identical on every rank, and its sum times m is
    is_divergence() to 1e-12"""
    A, W, H, cols, divs = K.run_coldiv(grid, use_hip=False)
    m, n = A.shape
    ref = K.column_div(A, W, H, EPS64) / m
    assert len(cols) == 2 and np.array_equal(cols[0], cols[1]) and divs[0] == divs[1]
    d = np.linalg.norm(cols[0] - ref) / np.linalg.norm(ref)
    s = abs(cols[0].sum() * m - divs[0]) / divs[0]
    print("is column divergence %dx%d: against the whole matrix %.2e, sum against is_divergence %.2e" % (grid + (d, s)))
    assert cols[0].shape == (n,) and (cols[0] > 0).all()
    assert d <= 1e-10 and s <= 1e-12, (grid, d, s)


def test_column_divergence_is_reported_under_is_only():
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = I.problem()
    nmf = PyNMF(A.astype(np.float32), factors=[W0, H0], params=I.one_rank_args(k, 2, norm="kl"), ops=K.ISNmfkOracleOps())
    with pytest.raises(ValueError, match="is_column_divergence.*norm='kl'"):
        nmf.is_column_divergence()


# ---- (c) statistics and refusals
def test_statistics_of_a_sweep_and_its_results_file(tmp_path):
    from pydnmfk_amd.data_io import read_cluster_results
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._ops_double import OracleOps
    A = K.scaled_problem(1)
    nmfk = PyNMFk(A, params=K.small_args(tmp_path / "is", norm="itakura-saito"), ops=K.ISNmfkOracleOps())
    assert nmfk.params.norm == "is" and nmfk._batch_size() == 1
    nmfk.fit()
    for k in (2, 3):
        st = nmfk.stats[k]
        assert len(st["is_div"]) == 4 and np.isfinite(st["is_div"]).all() and min(st["is_div"]) > 0
        assert st["avgDiv"] == float(np.mean(st["is_div"])) and np.isfinite(st["avgDiv"])
        assert np.asarray(st["L_err"]).shape == (90,) and np.isfinite(st["L_err"]).all() and (np.asarray(st["L_err"]) > 0).all()
        assert len(st["recon_err"]) == 4 and 0 < st["avgErr"] < 1 and np.isfinite(st["AIC"])             # (the Frobenius definitions)
        z = read_cluster_results(str(tmp_path / "is") + "/results/synth/%d/" % k)
        assert np.array_equal(z["is_div"], np.asarray(st["is_div"])) and float(z["avgDiv"]) == st["avgDiv"]
        assert np.array_equal(z["L_err"], st["L_err"])
    # L_err is the mean divergence per entry of the regression fit's factors (the last k's are still held): the float64 statement
    ref = K.column_div(A, np.asarray(nmfk.AvgW), np.asarray(nmfk.AvgH)) / A.shape[0]
    assert np.linalg.norm(nmfk.stats[3]["L_err"] - ref) <= 1e-10 * np.linalg.norm(ref)
    fro = PyNMFk(A, params=K.small_args(tmp_path / "fro", norm="fro"), ops=OracleOps())
    fro.fit()
    for k in (2, 3):
        assert "is_div" not in fro.stats[k] and "avgDiv" not in fro.stats[k]
        z = read_cluster_results(str(tmp_path / "fro") + "/results/synth/%d/" % k)
        assert sorted(z) == sorted(["clusterSilhouetteCoefficients", "avgSilhouetteCoefficients", "L_err", "L_errDist", "avgErr", "ErrTol", "AIC"])


def test_refusals_at_construction_name_what_is_refused(tmp_path):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMFk import PyNMFk
    sp = pytest.importorskip("scipy.sparse")
    A = K.scaled_problem(1)
    ops = K.ISNmfkOracleOps()
    with pytest.raises(NotImplementedError, match="norm='is'.*sampling='poisson'"):
        PyNMFk(A, params=K.sweep_args(tmp_path, sampling="poisson"), ops=ops)
    a = K.sweep_args(tmp_path)
    a.p_r = a.p_c = 2
    with pytest.raises(NotImplementedError, match="norm='is'.*2D grid"):
        PyNMFk(A, params=a, ops=ops)
    with pytest.raises(NotImplementedError, match="norm='is'.*k = 129"):
        PyNMFk(A, params=K.sweep_args(tmp_path, end_k=129), ops=ops)
    for value in (0.0, -0.5):
        B = A.copy()
        B[5, 6] = value
        with pytest.raises(ValueError, match="strictly positive"):
            PyNMFk(B, params=K.sweep_args(tmp_path), ops=ops)
    # what PyNMF refuses under the norm, in its words
    with pytest.raises(NotImplementedError, match="norm='is'.*sparse"):
        PyNMFk(sp.csr_matrix(A), params=K.sweep_args(tmp_path), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='is'.*missing='nan'"):
        PyNMFk(A, params=K.sweep_args(tmp_path, missing="nan"), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='is'.*bfloat16"):
        PyNMFk(A, params=K.sweep_args(tmp_path, precision="bfloat16"), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='is'.*float64"):
        PyNMFk(A.astype(np.float64), params=K.sweep_args(tmp_path), ops=_NoFloat64())
    with pytest.raises(NotImplementedError, match="norm='is'.*bf16x6"):
        PyNMFk(A, params=K.sweep_args(tmp_path, gemm="bf16x6"), ops=ops)
    for method in ("hals", "bcd"):
        with pytest.raises(NotImplementedError, match="norm='is'.*%s" % method):
            PyNMFk(A, params=K.sweep_args(tmp_path, method=method), ops=ops)
    # an operator set without the operation, or without the flag, is named
    with pytest.raises(NotImplementedError, match="^PyNMFk with norm='is' is not provided by operator set 'oracle-is'"):
        PyNMFk(A, params=K.sweep_args(tmp_path), ops=I.ISOracleOps())
    with pytest.raises(NotImplementedError, match="^PyNMFk with norm='is' is not provided by operator set 'no-flag'"):
        PyNMFk(A, params=K.sweep_args(tmp_path), ops=_NoFlag())
    assert MPI_comm(None, 1, 1).size == 1


class _NoFloat64(K.ISNmfkOracleOps):
    is_dtypes = (torch.float32,)


class _NoFlag(K.ISNmfkOracleOps):
    name = "no-flag"
    is_nmfk = False


def test_the_engine_names_which_operator_sets_sweep():
    """the fp32 set has the operation and the flag; the split (bf16x6) and float64 sets do not sweep under norm='is'"""
    from pydnmfk_amd import engine
    assert engine.HipOps.is_nmfk is True and callable(engine.HipOps.is_column_div)
    assert engine.HipOpsBf16x6.is_nmfk is False
    assert not getattr(engine.HipOpsF64, "is_nmfk", False) and not hasattr(engine.HipOpsF64, "is_column_div")


@pytest.mark.parametrize("grid", [(2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_data_split_sweep_on_a_grid_agrees_between_its_ranks(grid, tmp_path):
    """nmfk_split='data' (the default) with scaled_problem(1) cut into the blocks of a 1D grid: the short sweep completes, every rank
    holds the same estimate and the same GLOBAL statistics (L_err over all 90 columns, the perturbations' divergences), all finite"""
    res = I.spawn(K._data_grid_rank, grid, (False, str(tmp_path)), timeout=240)
    (n0, s0), (n1, s1) = res[0][1], res[1][1]
    assert n0 == n1 and set(s0) == set(s1) == {2, 3}
    for k in (2, 3):
        for key in ("L_err", "is_div", "avgDiv", "recon_err", "avgErr", "AIC"):
            assert np.array_equal(s0[k][key], s1[k][key]) and np.isfinite(s0[k][key]).all(), (k, key)
        assert s0[k]["L_err"].shape == (90,) and (s0[k]["L_err"] > 0).all() and s0[k]["is_div"].shape == (4,)


# ---- (d) the perturbation split
def test_perturbations_shared_by_two_ranks_equal_the_one_rank_sweep(tmp_path):
    """nmfk_split='perturbations' on two gloo ranks: every statistic, the divergences of the perturbations' fits among them, is the
    one-rank sweep's (rtol 1e-9 with equal_nan, as tests/test_gpu_masked_nmfk.py holds its split)"""
    K.assert_split_equals_one_rank(K.run_split(tmp_path, use_hip=False))
