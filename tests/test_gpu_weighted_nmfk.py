"""NMFk under per-entry weights on the GPU: dnmf_weighted_column_div against float64 numpy and its unweighted twins, and the sweeps."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _exact as E, _masked_nmfk as N, _weighted as Wt  # noqa: E402,E401

PLANS = {(70, 300): [1, 3, 3], (8250, 130): [2, 129, 2], (8250, 132): [2, 129, 2]}


@pytest.mark.parametrize("odd", [False, True], ids=["contiguous", "odd-views"])
@pytest.mark.parametrize("k", [3, 40, 100])
@pytest.mark.parametrize("shape", PLANS, ids=lambda s: "%dx%d" % s)
def test_column_div_against_float64_and_its_unweighted_twins(shape, k, odd):
    """25 % zero weights over NaN / inf / 0 / -1, column 5 without a positive weight; odd: views at an odd base, pitch = width + 3"""
    from pydnmfk_amd._lib import check, lib
    from pydnmfk_amd.engine import HIP_MASKED_OPS, HIP_OPS
    from pydnmfk_amd.masked import MaskedDenseBlock
    from pydnmfk_amd.pyDNMF import PyNMF
    (m, n), plan, rs = shape, (ctypes.c_long * 3)(), np.random.RandomState(sum(shape) + k)
    assert lib.dnmf_weighted_column_div_plan(m, n, k, plan) == 0 and list(plan) == PLANS[shape] and m % 32 != 0   # chunks > 1, a short tail
    W, H = (rs.rand(m, k) + 0.05).astype(np.float32), (rs.rand(k, n) + 0.05).astype(np.float32)
    A, V = ((W @ H) * (0.5 + rs.rand(m, n))).astype(np.float32), Wt.weights(shape, k, zero=0.25) * (np.arange(n) != 5)
    on, S = V > 0, W.astype(np.float64) @ H.astype(np.float64)
    A[~on] = rs.choice(np.array([np.nan, np.inf, 0.0, -1.0], dtype=np.float32), size=int((~on).sum()))
    A64, V64, seen = np.where(on, A, 1.0).astype(np.float64), V.astype(np.float64), on.any(0)
    dA, dV, dW, dH = (E.Poisoned(torch, x, aligned=False).view if odd else torch.from_numpy(x).cuda() for x in (A, V, W, H))
    nbytes = lib.dnmf_weighted_column_div_ws_bytes(m, n, k)
    for norm, beta in (("fro", 0.0), ("kl", 0.0), ("is", 0.0), ("beta", -2.0), ("beta", 0.5), ("beta", 4.0)):
        b = Wt._power(norm, beta)
        terms = [(A64 - S) ** 2] if norm == "fro" else Wt.B.terms_of(A64, S + Wt.EPS, b)
        rn, mag = np.where(on, V64 * sum(terms), 0.0).sum(0), np.where(on, V64 * sum(np.abs(t) for t in terms), 0.0).sum(0)
        rd = np.where(on, V64 * A64 ** b, 0.0).sum(0)
        out = torch.full((2, n + 2), float("nan"), dtype=torch.float64, device="cuda")
        ws = torch.full((nbytes // 8 + 16,), float("nan"), dtype=torch.float64, device="cuda")
        check(lib.dnmf_weighted_column_div(dA.data_ptr(), m, n, dA.stride(0), dV.data_ptr(), dV.stride(0), dW.data_ptr(), dW.stride(0),
                                           dH.data_ptr(), dH.stride(0), k, Wt.EPS, ("fro", "kl", "is", "beta").index(norm), beta,
                                           out[0, 1:].data_ptr(), out[1, 1:].data_ptr(), ws.data_ptr(), nbytes, None))
        again = torch.stack(HIP_OPS.weighted_column_div(dA, dV, dW, dH, Wt.EPS, norm, beta))          # a second call: the same bits
        assert torch.isnan(ws[nbytes // 8:]).all() and torch.isnan(out[:, [0, -1]]).all() and torch.equal(out[:, 1:-1], again)
        gn, gd = again.cpu().numpy()
        en, ed = (np.abs(gn - rn)[seen] / mag[seen]).max(), (np.abs(gd - rd)[seen] / rd[seen]).max()
        assert np.isfinite(gn).all() and gd[5] == 0 and not seen[5] and en <= 1e-5 and ed <= 1e-5, (norm, beta, en, ed)
        stat = PyNMF(dA, factors=[dW, dH], params=Wt.args(k, 1, norm, beta, weights=dV)).weighted_column_divergence()   # the same sums
        ref = np.sqrt(gn[seen] / gd[seen]) if norm == "fro" else gn[seen] / gd[seen]
        assert np.isnan(stat[~seen]).all() and np.array_equal(stat[seen], ref), (norm, beta)
    if not odd:     # bit for bit: fro at 0/1 weights is dnmf_masked_column_err on A with NaN at v = 0; is at unit weights is dnmf_is_column_div
        nan, pos = (torch.from_numpy(np.where(on, A, fill).astype(np.float32)).cuda() for fill in (np.nan, 1.0))
        wn, wd = HIP_OPS.weighted_column_div(dA, (dV > 0).float(), dW, dH, Wt.EPS, "fro", 0.0)
        mn, md = HIP_MASKED_OPS.column_err_sums(MaskedDenseBlock(nan), dW, dH)
        assert torch.equal(wn, mn) and torch.equal(wd, md) and wn.any()
        wn, wd = HIP_OPS.weighted_column_div(pos, torch.ones_like(pos), dW, dH, Wt.EPS, "is", 0.0)
        assert torch.equal(wn, HIP_OPS.is_column_div(pos, dW, dH, Wt.EPS)) and bool((wd == m).all())


def _sweep(tmp, data, **extra):
    from pydnmfk_amd.pyDNMFk import PyNMFk
    args = N.missing_args(tmp, extra.pop("missing", None))
    vars(args).update(extra)
    nmfk = PyNMFk(torch.from_numpy(data.astype(np.float32)).cuda(), params=args)
    return nmfk.fit(), nmfk.stats


def test_sweeps_with_01_weights_equal_the_masked_sweep_and_inverse_variance_weights_find_the_rank(tmp_path):
    """missing_problem() as weights = ~isnan(A) over garbage and as missing='nan': the factors, and so the column errors, are bit-equal"""
    from tests.test_gpu_sparse_nmfk import missing_problem
    A, mask = missing_problem()
    junk = np.resize(np.array([np.nan, -7.0, np.inf, 0.0], dtype=np.float32), A.shape)
    nw, w = _sweep(tmp_path / "w", np.where(mask, A, junk), weights=mask.astype(np.float32))
    nr, r = _sweep(tmp_path / "nan", np.where(mask, A, np.nan), missing="nan")
    assert nw == nr == 3 and all(len(w[k]["weighted_div"]) == 6 for k in w)
    for k, key in ((k, key) for k in range(1, 6) for key in ("L_err", "clusterSilhouetteCoefficients", "avgSilhouetteCoefficients")):
        assert np.array_equal(np.asarray(w[k][key]), np.asarray(r[k][key])), (k, key)
    # general weights: the same planted array under Gaussian noise of sigma 0.005, and 2 in every fourth column; v = 1 / sigma^2
    sigma = np.where(np.arange(90) % 4 == 0, 2.0, 0.005)[None, :] * np.ones((120, 1))
    A = np.abs(A + sigma * np.random.RandomState(21).randn(120, 90))
    assert _sweep(tmp_path / "v", A, weights=(sigma.min() / sigma) ** 2)[0] == 3 and _sweep(tmp_path / "plain", A)[0] != 3   # 
