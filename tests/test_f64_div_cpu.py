"""norm='is' and norm='beta' on float64 data without a GPU: what the operator sets name, the rank refusal, the workspace queries, and the
long-double statement tests/test_gpu_f64_div.py holds the kernels to."""
import types

import numpy as np
import pytest
import torch

from tests import _beta as B

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)


def statement(A, W, H, beta, eps=EPS64):
    """The pair of both sides, the rule applied to each factor (H with the OLD W) and the divergence with the sum of its terms'
    magnitudes, in long double; beta None: norm='is' (beta = 0).  The formulas of tests/_beta.py."""
    A, W, H = (np.asarray(x, dtype=LD) for x in (A, W, H))
    beta = 0.0 if beta is None else beta
    S = W @ H + LD(eps)
    P = S ** LD(beta - 2.0)
    Un, Ud = A * P, S * P
    out = {"w": (Un @ H.T, Ud @ H.T), "h": (W.T @ Un, W.T @ Ud)}
    g = LD(B.gamma(beta))
    out["upd_w"] = W * (out["w"][0] / (out["w"][1] + LD(eps))) ** g
    out["upd_h"] = H * (out["h"][0] / (out["h"][1] + LD(eps))) ** g
    pos = A > 0
    if beta == 0:
        t = (A / S, -np.log(A / S), -np.ones_like(S))
    elif beta == 1:
        t = (np.where(pos, A * np.log(np.where(pos, A, 1) / S), 0), -A, S)
    else:
        c = LD(beta) * LD(beta - 1.0)
        t = (np.where(pos, np.where(pos, A, 1) ** LD(beta), 0) / c, LD(beta - 1.0) * S ** LD(beta) / c, -LD(beta) * A * S ** LD(beta - 1.0) / c)
    out["div"], out["div_scale"] = sum(x.sum() for x in t), sum(np.abs(x).sum() for x in t)
    return out


@pytest.mark.parametrize("beta", (None, -2.0, 0.3, 1.0, 3.0))
def test_the_long_double_statement_agrees_with_the_float64_one(beta):
    A, W, H, _ = B.problem(130, 97, 16, seed=7, zeros=0.3 if beta and beta > 0 else 0.0)
    ref, b = statement(A, W, H, beta), (0.0 if beta is None else beta)
    for side in ("w", "h"):
        for got, want in zip(B.pair(A, W, H, side, b, EPS64), ref[side]):
            assert float(np.linalg.norm(got - want) / np.linalg.norm(want)) <= 5e-15, (beta, side)
    assert abs(B.divergence(A, W, H, b, EPS64) - float(ref["div"])) <= 5e-15 * float(ref["div_scale"])


def test_the_operator_sets_name_their_dtypes_and_ranks():
    from pydnmfk_amd import engine
    from pydnmfk_amd._lib import lib
    from pydnmfk_amd.pyDNMF import PyNMF
    assert engine.HipOpsF64.is_dtypes == (torch.float64,) and engine.HipOpsF64.beta_dtypes == (torch.float64,)
    assert engine.HipOps.is_dtypes == (torch.float32,) and engine.HipOps.beta_dtypes == (torch.float32,)
    for name in ("aht_pair", "wta_pair", "pair_into", "update_w", "update_h", "ratio_update", "divergence"):
        assert callable(getattr(engine.HipOpsF64, "is_" + name)) and callable(getattr(engine.HipOpsF64, "beta_" + name)), name
    for fn in (lib.dnmf_is_f64_ws_bytes, lib.dnmf_beta_f64_ws_bytes):
        assert fn(130, 97, 0) == 0 and fn(130, 97, 65) == 0 and fn(130, 97, 1) > 0 and fn(130, 97, 64) > 0
    stub = types.SimpleNamespace(name="stub", is_dtypes=(torch.float64,), beta_dtypes=(torch.float64,), is_max_k=64, beta_max_k=64)
    par = types.SimpleNamespace(gemm=None)
    for norm in ("is", "beta"):
        PyNMF._div_refusals(norm, par, False, None, torch.float64, stub, "mu", 2, 1, 64)
        with pytest.raises(NotImplementedError, match="norm='%s' with k = 65.*float64.*1 <= k <= 64" % norm):
            PyNMF._div_refusals(norm, par, False, None, torch.float64, stub, "mu", 2, 1, 65)
        with pytest.raises(NotImplementedError, match="norm='%s' with k = 129.*1 <= k <= 128" % norm):
            PyNMF._div_refusals(norm, par, False, None, torch.float32, engine.HipOps, "mu", 1, 1, 129)
