"""The Itakura-Saito objective (`params.norm = 'is'`) without a GPU: the choreography (dist_nmf.IS_MU_update) with the float64 checker
operator set of tests/_is.py through PyNMF on one rank and on gloo 1D grids against the whole-matrix float64 statement, the
divergence along a fit, every refusal, the positivity verdict on a grid, main.py's flag, and the float64 proof that the exact
operands of the GPU test are exact."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _is as I  # noqa: E402
from tests._golden import rel_fro  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = float(np.finfo(np.float64).eps)


# ---- 1. grids against the whole-matrix statement
@pytest.fixture(scope="module")
def reference_fits():
    return I.reference_fits(eps=EPS64)                     # (float64 data: PyNMF's eps is the float64 machine epsilon, pyDNMF.py:68)


@pytest.mark.parametrize("grid", [(1, 1), (2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_grids_against_the_whole_matrix_statement(grid, reference_fits):
    """50 x 39, k = 3, strictly positive, 20 iterations, W_update on and off, in float64 from end to end: each grid's factors, error
    and divergence equal the whole-matrix statement to 1e-10 (the sums of two ranks differ from the whole sum by float64 rounding
    only); replicated factors agree bit for bit between the ranks (run_grid asserts it)"""
    got = I.run_grid(grid, use_hip=False)
    for wu, (Wr, Hr, err_r, div_r) in reference_fits.items():
        W, H, err, div = got[wu]
        assert W.dtype == np.float64 and H.dtype == np.float64
        dw, dh, de, dd = rel_fro(W, Wr), rel_fro(H, Hr), abs(err - err_r) / err_r, abs(div - div_r) / div_r
        print("is %dx%d W_update=%s: dW=%.2e dH=%.2e derr=%.2e ddiv=%.2e (err %.6g, D %.6g)" % (grid + (wu, dw, dh, de, dd, err_r, div_r)))
        assert dw <= 1e-10 and dh <= 1e-10 and de <= 1e-10 and dd <= 1e-10, (grid, wu, dw, dh, de, dd)
    assert not np.array_equal(got[True][0], got[False][0])                 # W_update=False: W moved by the normalisation only
    A, W0, H0, k = I.problem()
    s = W0.sum(axis=0)
    assert rel_fro(got[False][0], W0 / (s + EPS64)) <= 1e-14


def test_float32_data_take_the_same_path_in_float32():
    """the checker set on float32 data (the dtype of the HIP kernels): float32 factors come back, close to the float64 statement"""
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = I.problem()
    nmf = PyNMF(A.astype(np.float32), factors=[W0, H0], params=I.one_rank_args(k, 20), ops=I.ISOracleOps())
    assert nmf.norm == "is" and nmf.c_dtype == torch.float32 and not nmf._whole_fit_ok(nmf._ops())
    W, H, err = nmf.fit()
    Wr, Hr, err_r = I.fit(A.astype(np.float32), W0.astype(np.float32), H0.astype(np.float32), 20)
    assert W.dtype == np.float32 and rel_fro(W, Wr) <= 1e-5 and rel_fro(H, Hr) <= 1e-5 and abs(err - err_r) <= 1e-5 * err_r


def test_itakura_saito_is_an_alias():
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = I.problem()
    out = [PyNMF(A, factors=[W0, H0], params=I.one_rank_args(k, 5, norm=norm), ops=I.ISOracleOps()).fit() for norm in ("is", "itakura-saito", "IS")]
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[2][1])


# ---- 2. the divergence never increases
def test_the_divergence_never_increases_along_a_fit():
    """50 steps of the choreography, the divergence read by PyNMF.is_divergence() after each: no step increases it (the
    majorisation-minimisation form), and it equals the statement's at every step"""
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = I.problem()
    nmf = PyNMF(A, factors=[W0, H0], params=I.one_rank_args(k, 50), ops=I.ISOracleOps())
    d = [nmf.is_divergence()]
    assert abs(d[0] - I.divergence(A, W0, H0, EPS64)) <= 1e-12 * d[0]
    W, H = W0, H0
    for i in range(50):
        nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update(clamp=(i % 10 == 0))
        W, H = I.step(A, W, H, EPS64, True, clamp=(i % 10 == 0))
        d.append(nmf.is_divergence())
        assert abs(d[-1] - I.divergence(A, W, H, EPS64)) <= 1e-10 * d[-1], i
    rel = np.diff(d) / np.array(d[:-1])
    print("is divergence: %.6g -> %.6g over 50 steps; largest relative change per step %.3e" % (d[0], d[-1], rel.max()))
    assert np.all(np.diff(d) <= 0), rel.max()
    assert d[-1] < 0.9 * d[0]


# ---- 3. the refusals
def test_refusals_name_the_norm_and_the_combination():
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._ops_double import OracleOps
    sp = pytest.importorskip("scipy.sparse")
    A, W0, H0, k = I.problem()
    A = A.astype(np.float32)
    ops = I.ISOracleOps()
    args = I.one_rank_args
    with pytest.raises(NotImplementedError, match="norm='is'.*2D grid"):
        PyNMF(A, params=args(k, 3, grid=(2, 2)), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='is'.*sparse"):
        PyNMF(sp.csr_matrix(A), params=args(k, 3), ops=ops)
    An = A.copy()
    An[3, 4] = np.nan
    with pytest.raises(NotImplementedError, match="norm='is'.*missing='nan'"):
        PyNMF(An, params=args(k, 3, missing="nan"), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='is'.*missing='unstored'"):
        PyNMF(sp.csr_matrix(A), params=args(k, 3, missing="unstored"), ops=ops)
    # float64 data: refused unless the operator set names the dtype (the HIP sets name float32 alone; OracleOps names none)
    with pytest.raises(NotImplementedError, match="norm='is'.*float64"):
        PyNMF(A.astype(np.float64), params=args(k, 3), ops=OracleOps())
    with pytest.raises(NotImplementedError, match="norm='is'.*bfloat16"):
        PyNMF(torch.from_numpy(A).to(torch.bfloat16), params=args(k, 3), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='is'.*bfloat16"):
        PyNMF(A, params=args(k, 3, precision="bfloat16"), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='is'.*bf16x6"):
        PyNMF(A, params=args(k, 3, gemm="bf16x6"), ops=ops)
    with pytest.raises(NotImplementedError, match="norm='is'.*k = 129"):
        PyNMF(np.ones((4, 200), dtype=np.float32), params=args(129, 3), ops=ops)
    for method in ("hals", "bcd"):
        with pytest.raises(NotImplementedError, match="norm='is'.*%s" % method):
            PyNMF(A, params=args(k, 3, method=method), ops=ops)
    with pytest.raises(NotImplementedError, match="PyNMFk.*norm='is'"):
        PyNMFk(A, params=args(k, 3), ops=ops)
    # the choreography refuses by itself, whatever PyNMF let through
    for method in ("hals", "bcd"):
        a = args(k, 3, method=method)
        a.m, a.n, a.eps = A.shape[0], A.shape[1], I.EPS
        with pytest.raises(NotImplementedError, match="norm='is'.*%s" % method):
            nmf_algorithms_1D(torch.from_numpy(A), torch.from_numpy(W0.astype(np.float32)), torch.from_numpy(H0.astype(np.float32)),
                              params=a, ops=ops).update()
    a = args(k, 3)
    a.m, a.n, a.eps = A.shape[0], A.shape[1], I.EPS
    with pytest.raises(NotImplementedError, match="norm='is'.*oracle-double"):          # an operator set without the operations is named
        nmf_algorithms_1D(torch.from_numpy(A), torch.from_numpy(W0.astype(np.float32)), torch.from_numpy(H0.astype(np.float32)),
                          params=a, ops=OracleOps()).update()
    # fit_batch runs such fits one by one
    fits = [PyNMF(A, factors=[W0, H0], params=args(k, 4), ops=ops) for _ in range(2)]
    one = PyNMF(A, factors=[W0, H0], params=args(k, 4), ops=ops).fit()
    for res in PyNMF.fit_batch(fits):
        assert np.array_equal(res[0], one[0]) and np.array_equal(res[1], one[1]) and res[2] == one[2]
    # is_divergence belongs to norm='is'
    with pytest.raises(ValueError, match="is_divergence.*norm='kl'"):
        PyNMF(A, factors=[W0, H0], params=args(k, 3, norm="kl"), ops=ops).is_divergence()


def test_every_other_norm_keeps_the_old_text():
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = I.problem()
    with pytest.raises(Exception, match=r"Not a valid norm: Choose \(fro/kl\)"):
        PyNMF(A.astype(np.float32), factors=[W0, H0], params=I.one_rank_args(k, 3, norm="l1"), ops=I.ISOracleOps()).fit()


@pytest.mark.parametrize("value", [0.0, -0.5], ids=["zero", "negative"])
def test_one_rank_refuses_data_that_are_not_strictly_positive(value):
    (rank, (name, text)), = I.spawn(I._bad_data_rank, (1, 1), (False, value))
    assert name == "ValueError" and "strictly positive" in text and ("%g" % value) in text, (name, text)


@pytest.mark.parametrize("value", [0.0, -0.5], ids=["zero", "negative"])
def test_every_rank_of_a_grid_refuses_together(value):
    """2 x 1: the bad entry sits in the LAST rank's slice; both ranks raise the ValueError (rank 0 names its own, positive, minimum and
    the count of bad ranks), and no rank is left in a collective: both come back within the time limit of spawn()"""
    res = I.spawn(I._bad_data_rank, (2, 1), (False, value), timeout=120)
    assert [r for r, _ in res] == [0, 1]
    for rank, (name, text) in res:
        assert name == "ValueError" and "strictly positive" in text and "1 of 2 ranks" in text, (rank, name, text)
    assert ("block is %g (" % value) in res[1][1][1] and ("block is %g (" % value) not in res[0][1][1]


# ---- 4. main.py --norm is
def test_main_names_is_in_the_norm_help():
    sys.path.insert(0, ROOT)
    try:
        import main as cli
    finally:
        sys.path.remove(ROOT)
    (text,) = [row[4] for row in cli.FLAGS if row[0] == "norm"]
    assert "is" in text.replace(",", " ").replace("/", " ").split() and "Itakura-Saito" in text


# ---- 5. the exact operands of tests/test_gpu_is.py are exact: float64 proof
@pytest.mark.parametrize("shape", I.EXACT_SHAPES + tuple(c["shape"] for c in I.EXACT_LOOP_CASES), ids=lambda s: "%dx%d" % s)
def test_exact_operands_are_exact_in_any_order(shape):
    """every sum of both pairs stays below 2^24 of its unit (I.exact asserts it with E._bound; the largest, at 70 x 2085, is
    0.29 * 2^24); and an fp32 sum over the terms in shuffled order equals the float64 one, element by element"""
    m, n = shape
    ks = next((c["ks"] for c in I.EXACT_LOOP_CASES if c["shape"] == shape), I.EXACT_KS)
    for k in ks:
        A, W, H, ref = I.exact(m, n, k)
        assert A.min() >= 1 and A.max() <= 7
        un, ud = 2.0 ** -10, 2.0 ** -5
        top = max(ref["w"][0].max() / un, ref["h"][0].max() / un, ref["w"][1].max() / ud, ref["h"][1].max() / ud)
        print("is exact %dx%d k=%d: largest sum is %.3f * 2^24 of its unit" % (m, n, k, top / 2 ** 24))
        assert top < 2 ** 24, (shape, k, top / 2 ** 24)
        # fp32 arithmetic of the kernel's element-wise step, then fp32 sums in a shuffled order
        S = (W @ H).astype(np.float32)
        R = (np.float32(1) / (S + np.float32(I.EPS))).astype(np.float32)
        U = (A * R * R).astype(np.float32)
        assert np.array_equal(R.astype(np.float64), 1.0 / (W.astype(np.float64) @ H.astype(np.float64)))
        perm = np.random.RandomState(m + n + k).permutation(n)
        num = np.zeros((m, k), dtype=np.float32)
        den = np.zeros((m, k), dtype=np.float32)
        for c in perm[: min(n, 256)]:                              # (a prefix of a shuffled order: partial sums are exact as well)
            num += U[:, c:c + 1] * H[:, c][None, :]
            den += R[:, c:c + 1] * H[:, c][None, :]
        cols = perm[: min(n, 256)]
        assert np.array_equal(num.astype(np.float64), (U[:, cols].astype(np.float64) @ H[:, cols].astype(np.float64).T))
        assert np.array_equal(den.astype(np.float64), (R[:, cols].astype(np.float64) @ H[:, cols].astype(np.float64).T))
        for side in ("w", "h"):
            for x in ref[side]:
                assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
