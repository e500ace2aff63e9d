"""NMFk over dense data with NaN-marked gaps (`params.missing = 'nan'`) without a GPU: the driver (pydnmfk_amd.pyDNMFk) over the checker
operator set of tests/_masked_nmfk.py -- the missing-data sweep in float64, the reference's own statistics on a matrix without a NaN
(one rank and 2 x 1 over gloo), `sample` on a NaN-marked array, the refusals, and the float64 proof that the operands of the kernel
test (tests/test_gpu_masked_nmfk.py) keep every fp32 partial an integer below 2^24."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _masked_dense as D  # noqa: E402
from tests import _masked_nmfk as N  # noqa: E402

# minimum silhouettes at k = 1..5 of the float64 sweeps of missing_problem() (300 iterations, 6 perturbations).  MASKED_SIL: the sweep of
# tests/_sparse_nmfk.py::SparseNmfkOracleOps over the CSR form of the same observations under missing='unstored' (the reference of this
# test: 1.0 / 0.970 / 0.970 / -0.453 / -0.492 to three decimals); ZERO_SIL: the zero-filled dense sweep on tests/_ops_double.py::OracleOps
MASKED_SIL = (1.0, 0.969844200, 0.969594766, -0.453246968, -0.492369526)
ZERO_SIL = (1.0, 0.994, 0.548, 0.492, 0.483)


def _missing():
    from tests.test_gpu_sparse_nmfk import missing_problem
    A, mask = missing_problem()
    assert A.shape == (120, 90) and 0.35 < mask.mean() < 0.45
    return A, mask


def test_missing_data_sweep_finds_the_planted_rank(tmp_path):
    """missing_problem() NaN-marked, numpy input: the draws of `sample` and of the rand init are those of the CSR sweep under
    missing='unstored' (np.random.random_sample over the dense shape, np.multiply keeps NaN), the rules are the same float64 statement
    over the same observations: the same estimate and the same silhouettes.  Read as zeros, the same entries give 2."""
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._ops_double import OracleOps
    A, mask = _missing()
    An = D.nan_marked(A, mask)
    nmfk = PyNMFk(An, params=N.missing_args(tmp_path / "masked", "nan"), ops=N.MaskedNmfkOracleOps())
    assert nmfk.A_ij is An and nmfk._batch_size() == 1
    nopt = nmfk.fit()
    sil = N.min_silhouettes(nmfk)
    print("masked sweep: estimate %d, minimum silhouettes %s" % (nopt, ["%.6f" % s for s in sil]))
    assert nopt == 3
    for k, (got, want) in enumerate(zip(sil, MASKED_SIL), start=1):
        assert abs(got - want) < 1e-6, (k, got, want)
    for k in range(1, 6):
        st = nmfk.stats[k]
        assert np.asarray(st["L_err"]).shape == (90,) and np.isfinite(st["L_err"]).all() and 0 < st["avgErr"] < 1
        assert st["AIC"] == 2 * k + 120 * 90 * np.log(st["avgErr"] / (120 * 90))                       # m n, not |Omega|
    zero = PyNMFk(np.where(mask, A, 0).astype(np.float32), params=N.missing_args(tmp_path / "zero", None), ops=OracleOps())
    nz = zero.fit()
    zsil = N.min_silhouettes(zero)
    print("zero-filled sweep: estimate %d, minimum silhouettes %s" % (nz, ["%.6f" % s for s in zsil]))
    assert nz == 2
    for k, (got, want) in enumerate(zip(zsil, ZERO_SIL), start=1):
        assert abs(got - want) < 5e-4 + 1e-6, (k, got, want)          # (quoted to three decimals)


def test_matrix_without_a_nan_meets_the_reference_statistics(tmp_path, golden_dir):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests.test_nmfk_cpu import _args, check_against_golden
    z = np.load(golden_dir + "/nmfk_1x1.npz")
    assert not np.isnan(z["A"]).any()
    args = _args(tmp_path, MPI_comm(None, 1, 1))
    args.missing = "nan"
    nmfk = PyNMFk(np.ascontiguousarray(z["A"], dtype=np.float32), factors=None, params=args, ops=N.MaskedNmfkOracleOps())
    check_against_golden(nmfk, nmfk.fit(), z)


def test_two_ranks_meet_the_reference_statistics(golden_dir):
    from tests.test_nmfk_cpu import check_nmfk_fixture
    check_nmfk_fixture(N.run_nmfk_golden_nan("nmfk_2x1.npz", use_hip=False, timeout=600), np.load(golden_dir + "/nmfk_2x1.npz"), tight=True)


def _gappy(seed=5, shape=(37, 23), counts=False):
    rs = np.random.RandomState(seed)
    mask = rs.rand(*shape) < 0.4
    A = (rs.randint(0, 6, size=shape) if counts else rs.rand(*shape) + 0.5).astype(np.float32)
    return A, mask


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_sample_uniform_keeps_nan_and_the_reference_stream():
    from pydnmfk_amd.pyDNMFk import host_uniform_values, sample
    import scipy.sparse as sp
    A, mask = _gappy()
    An = D.nan_marked(A, mask)
    per = sample(An, 0.03, "uniform", seed=4000, missing="nan").fit()
    after = np.random.get_state()
    assert per.dtype == np.float32 and np.array_equal(np.isnan(per), ~mask)
    zero = np.where(mask, A, 0).astype(np.float32)
    dense = sample(zero, 0.03, "uniform", seed=4000).fit()
    assert _same_state(after, np.random.get_state())                               # the generator ends where the dense path leaves it
    assert np.array_equal(per[mask], dense[mask])                                  # observed: the values the zero-filled matrix gets
    S = sp.csr_matrix((A[mask], np.nonzero(mask)), shape=A.shape)
    np.random.seed(4000)
    vals = host_uniform_values(S.indptr, S.indices, S.data, S.shape, 0.03)
    r, c = S.nonzero()
    assert np.array_equal(per[r, c], vals)                                         # and those of the CSR path on the COO form
    pt = sample(torch.from_numpy(An), 0.03, "uniform", seed=4000, missing="nan").fit()
    assert torch.equal(torch.isnan(pt), torch.from_numpy(~mask))


def test_sample_poisson_draws_from_the_zero_filled_rates():
    from pydnmfk_amd.pyDNMFk import sample
    A, mask = _gappy(counts=True)
    An = D.nan_marked(A, mask)
    per = sample(An, 0.03, "poisson", seed=1000, missing="nan").fit()
    after = np.random.get_state()
    assert per.dtype == np.float32 and np.array_equal(np.isnan(per), ~mask)
    assert np.array_equal(per[mask], np.round(per[mask])) and (per[mask] >= 0).all() and (per[mask] == 0).any()
    zero = np.where(mask, A, 0).astype(np.float32)
    dense = sample(zero, 0.03, "poisson", seed=1000).fit()
    assert _same_state(after, np.random.get_state()) and np.array_equal(per[mask], dense[mask])
    # torch input: the generator sees the zero-filled rates
    pt = sample(torch.from_numpy(An), 0.03, "poisson", seed=1000, missing="nan").fit()
    g = torch.Generator()
    g.manual_seed(1000)
    want = torch.poisson(torch.from_numpy(zero), generator=g)
    assert torch.equal(torch.isnan(pt), torch.from_numpy(~mask)) and torch.equal(pt[torch.from_numpy(mask)], want[torch.from_numpy(mask)])


def test_refusals_at_construction(tmp_path):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._ops_double import OracleOps
    from tests.test_nmfk_cpu import _args
    A, mask = _gappy()
    An = D.nan_marked(A, mask)
    comms = MPI_comm(None, 1, 1)

    def args(**kw):
        a = _args(tmp_path, comms)
        a.missing = "nan"
        for key, val in kw.items():
            setattr(a, key, val)
        return a
    # an operator set without the capability is named
    for ops in (D.MaskedDenseOracleOps(), OracleOps()):
        with pytest.raises(NotImplementedError, match="PyNMFk.*missing='nan'.*operator set '%s'" % ops.name):
            PyNMFk(An, params=args(), ops=ops)
    ops = N.MaskedNmfkOracleOps()
    nmfk = PyNMFk(An, params=args(), ops=ops)
    assert nmfk.A_ij is An and nmfk._masked and nmfk._batch_size() == 1
    # what PyNMF refuses under missing='nan' is refused at construction, in PyNMF's words
    with pytest.raises(NotImplementedError, match="missing='nan'.*prune"):
        PyNMFk(An, params=args(prune=True), ops=ops)
    with pytest.raises(NotImplementedError, match="missing='nan'.*2D grid"):
        PyNMFk(An, params=args(p_r=2, p_c=2), ops=ops)
    with pytest.raises(NotImplementedError, match="missing='nan'.*k = 129"):
        PyNMFk(An, params=args(end_k=129), ops=ops)
    with pytest.raises(NotImplementedError, match="missing='nan'.*nnsvd"):
        PyNMFk(An, params=args(init="nnsvd"), ops=ops)
    with pytest.raises(NotImplementedError, match="missing='nan'.*float64"):
        PyNMFk(An.astype(np.float64), params=args(), ops=ops)
    with pytest.raises(NotImplementedError, match="missing='nan'.*bfloat16"):
        PyNMFk(An, params=args(precision="bfloat16"), ops=ops)
    with pytest.raises(NotImplementedError, match="missing='nan'.*bf16x6"):
        PyNMFk(An, params=args(gemm="bf16x6"), ops=ops)
    with pytest.raises(NotImplementedError, match="missing='nan'.*hals"):
        PyNMFk(An, params=args(method="hals"), ops=ops)


def test_oracle_column_err_runs_over_the_observed_positions():
    from pydnmfk_amd.masked import MaskedDenseBlock
    A, mask = _gappy()
    mask[:, 4] = False
    rs = np.random.RandomState(1)
    W, H = rs.rand(A.shape[0], 3).astype(np.float32), rs.rand(3, A.shape[1]).astype(np.float32)
    num, den = N.MaskedNmfkOracleOps().column_err_sums(MaskedDenseBlock(torch.from_numpy(D.nan_marked(A, mask))), torch.from_numpy(W), torch.from_numpy(H))
    rn, rd = N.colerr_ref(A, mask, W, H)
    assert np.allclose(num.numpy(), rn, rtol=1e-12, atol=1e-13) and np.allclose(den.numpy(), rd, rtol=1e-12) and num[4] == 0 and den[4] == 0


@pytest.mark.parametrize("shape", N.COLERR_SHAPES, ids=lambda s: "%dx%d" % s)
def test_colerr_exact_operands_keep_every_partial_an_integer_below_2_24(shape):
    """col_sums_kernel<KT, FAST, MaskedErrTerm> adds, per column and lane half, the (a - S)^2 and a^2 of the observed ones of 16 rows in float32 (fmaf on
    integers: exact while every intermediate stays below 2^24), and float64 from there on.  Asserted here for the operands the GPU test
    uses: the model values are integers (so every difference is), the largest 16-row partial is below 2^24, the column sums are
    integers below 2^53, and at least two columns have no observation."""
    m, n = shape
    for k in N.COLERR_KS:
        A, mask, W, H = N.colerr_case(m, n, k)
        assert (A >= 0).all() and (W >= 0).all() and (H >= 0).all() and np.array_equal(A, np.round(A))
        Dm = W.astype(np.float64) @ H.astype(np.float64)
        assert np.array_equal(Dm, np.round(Dm)) and Dm.max() < 2.0 ** 24            # S itself is exact in the accumulators
        pn, pd = N.tile_partials(A, mask, W, H)
        assert pn < 2.0 ** 24 and pd < 2.0 ** 24, (shape, k, pn, pd)
        num, den = N.colerr_ref(A, mask, W, H)
        assert np.array_equal(num, np.round(num)) and np.array_equal(den, np.round(den)) and num.max() < 2.0 ** 53 and den.max() < 2.0 ** 53
        empty = mask.sum(0) == 0
        assert empty.sum() >= 2 and not num[empty].any() and not den[empty].any() and (mask.sum(0) == 1).any()
        print("colerr operands %dx%d k=%d: largest fp32 partial %d / %d, largest column sum %d" % (m, n, k, pn, pd, num.max()))
