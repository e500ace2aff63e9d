"""Per-entry weights (`params.weights`) without a GPU: the choreography (dist_nmf.WEIGHTED_MU_update) with the float64 checker operator
set of tests/_weighted.py through PyNMF on one rank and on gloo 1D grids against the whole-matrix float64 statement, the weighted
objective along a fit, every refusal and every ValueError, the C ABI's table and main.py's flag."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _weighted as Wt  # noqa: E402
from tests.test_capi import EINVAL, EWS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = Wt.EPS64
NAMES = ["dnmf_weighted_" + n for n in ("ws_bytes", "ws_bytes_fit", "plan", "aht_pair", "wta_pair", "update_w", "update_h", "resid_sqnorm",
                                        "divergence", "mu_fit")]


@pytest.mark.parametrize("grid", [(1, 1), (2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_grids_against_the_whole_matrix_statement(grid):
    """50 x 39, k = 3, 20 steps, fro / kl / is / beta (0.5, 3), 30 % zero weights with NaN under them, float64 from end to end: factors,
    weighted error and objective within 1e-10 of the whole-matrix statement"""
    for key, d in Wt.run_grid(grid).items():
        print("%s beta=%g" % key, "%dx%d" % grid, "dW=%.2e dH=%.2e derr=%.2e dobj=%.2e" % d)
        assert max(d) <= 1e-10, (grid, key, d)


@pytest.mark.parametrize("norm,beta", Wt.NORMS, ids=lambda v: str(v))
def test_the_weighted_objective_never_increases(norm, beta):
    """50 steps of the choreography, PyNMF.weighted_divergence() after each: it equals the statement's and no step increases it"""
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    A, V, W0, H0, k = Wt.problem()
    nmf = PyNMF(A, factors=[W0, H0], params=Wt.args(k, 50, norm, beta, weights=V.astype(np.float32)), ops=Wt.WeightedOracleOps())
    d, (W, H) = [nmf.weighted_divergence()], (W0, H0)
    for i in range(50):
        nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update(clamp=(i % 10 == 0))
        W, H = Wt.step(A, V, W, H, norm, beta, EPS64, True, clamp=(i % 10 == 0))
        d.append(nmf.weighted_divergence())
        assert abs(d[-1] - Wt.objective(A, V, W, H, norm, beta, EPS64)) <= 1e-10 * d[-1], i
    print("%s beta=%g: %.6g -> %.6g, largest relative change %.3e" % (norm, beta, d[0], d[-1], (np.diff(d) / np.array(d[:-1])).max()))
    assert np.all(np.diff(d) <= 0) and d[-1] < 0.9 * d[0]


REFUSALS = [(dict(missing="nan"), "weights.*missing='nan'.*weight 0"), (dict(method="hals"), "weights.*hals"), (dict(method="bcd"), "weights.*bcd"),
            (dict(grid=(2, 2)), "weights.*2D grid"), (dict(gemm="bf16x6"), "weights.*bf16x6"), (dict(prune=True), "weights.*prune=True"),
            (dict(init="nnsvd"), "weights.*nnsvd"), (dict(k=129), "weights.*k = 129"), (dict(precision="bfloat16"), "weights.*bfloat16")]


@pytest.mark.parametrize("change,match", REFUSALS, ids=lambda v: str(v) if isinstance(v, dict) else None)
def test_refusals_name_the_combination(change, match):
    from pydnmfk_amd.pyDNMF import PyNMF
    A, V, W0, H0, k = Wt.problem(zero=0.0)
    change = dict(change)
    a = Wt.args(change.pop("k", k), 3, "kl", 0.0, weights=V.astype(np.float32), **change)
    with pytest.raises(NotImplementedError, match=match):
        PyNMF(A.astype(np.float32), params=a, ops=Wt.WeightedOracleOps())


def test_refusals_of_the_data_type_the_sparse_block_rank_estimation_and_the_choreography():
    from pydnmfk_amd import engine
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._ops_double import OracleOps
    sp = pytest.importorskip("scipy.sparse")
    A, V, W0, H0, k = Wt.problem(zero=0.0)
    V32 = V.astype(np.float32)
    with pytest.raises(NotImplementedError, match="weights.*float64"):
        PyNMF(A, params=Wt.args(k, 3, "kl", 0.0, weights=V32), ops=OracleOps())
    with pytest.raises(NotImplementedError, match="weights.*sparse"):
        PyNMF(sp.csr_matrix(A.astype(np.float32)), params=Wt.args(k, 3, "kl", 0.0, weights=V32), ops=Wt.WeightedOracleOps())
    with pytest.raises(NotImplementedError, match="PyNMFk.*weights"):
        PyNMFk(A.astype(np.float32), params=Wt.args(k, 3, "kl", 0.0, weights=V32), ops=Wt.WeightedOracleOps())
    a = Wt.args(k, 3, "kl", 0.0, weights_block=torch.from_numpy(V32))                  # the choreography refuses by itself
    a.m, a.n, a.eps = A.shape[0], A.shape[1], Wt.EPS
    t = [torch.from_numpy(x.astype(np.float32)) for x in (A, W0, H0)]
    for ops, change, match in ((OracleOps(), {}, "weights.*oracle-double"), (Wt.WeightedOracleOps(), dict(method="hals"), "weights.*hals")):
        for key, val in change.items():
            setattr(a, key, val)
        with pytest.raises(NotImplementedError, match=match):
            nmf_algorithms_1D(*t, params=a, ops=ops).update()
    assert engine.HipOps.weighted_dtypes == (torch.float32,) and engine.HipOpsBf16x6.weighted_dtypes == ()


BAD = {"nan": np.nan, "inf": np.inf, "negative": -1.0, "a = 0 under is": 0.0, "a < 0 under kl": -0.5}


@pytest.mark.parametrize("what,word", [("nan", "finite"), ("inf", "finite"), ("negative", ">= 0"), ("all zero", "no positive weight"),
                                       ("shape", "shape"), ("a = 0 under is", "strictly positive"), ("a < 0 under kl", "non-negative")])
def test_bad_weights_or_data_are_a_value_error(what, word):
    from pydnmfk_amd.pyDNMF import PyNMF
    A, V, W0, H0, k = Wt.problem()
    pos = tuple(np.argwhere(V > 0)[-1])
    if what in BAD:
        (A if what.startswith("a ") else V)[pos] = BAD[what]
    V = V[:, :-1] if what == "shape" else V * (what != "all zero")
    with pytest.raises(ValueError, match="weights.*" + word):
        PyNMF(A.astype(np.float32), factors=[W0, H0], params=Wt.args(k, 3, "is" if "is" in what else "kl", 0.0, weights=V.astype(np.float32)),
              ops=Wt.WeightedOracleOps())


def test_the_abi_is_declared_exported_and_bound_in_a_table_of_its_own():
    from pydnmfk_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dnmf_weighted_api.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(dnmf_[a-z0-9_]+)\s*\(", txt))) == sorted(NAMES) == sorted(_lib.WEIGHTED_SIGNATURES)
    core = open(os.path.join(ROOT, "include", "dnmf.h")).read()
    assert core.index('"dnmf_beta_nmfk_api.h"') < core.index('#include "dnmf_weighted_api.h"')
    assert not set(_lib.WEIGHTED_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.BETA_SIGNATURES) | set(_lib.BETA_NMFK_SIGNATURES))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and getattr(_lib.lib, name).argtypes == _lib.WEIGHTED_SIGNATURES[name], name
    lib, P16, out = _lib.lib, 0x10000, (ctypes.c_long * 8)()
    for norm, twin in enumerate((lib.dnmf_masked_plan, lib.dnmf_masked_plan, lib.dnmf_is_plan, lib.dnmf_beta_plan)):
        ref = (ctypes.c_long * 8)()
        for m, n, k in ((130, 97, 3), (70, 2085, 64), (2130, 70, 128), (32768, 16384, 128)):
            assert lib.dnmf_weighted_plan(m, n, k, norm, out) == 0 and twin(m, n, k, ref) == 0
            assert list(out)[:6] == list(ref)[:6], (norm, m, n, k)                 # the mode's own geometry, number for number
    good = [P16, 130, 97, 97, P16, 97, P16, 32, P16, 97, 32, 1e-7, 3, 0.5, P16, P16, 32, P16, 1 << 40, None]
    for at, val, code, word in ((17, P16 + 4, EWS, b"16-byte boundary"), (13, 7.5, EINVAL, b"-2 <= beta <= 4"), (12, 4, EINVAL, b"norm=4"),
                                (10, 129, EINVAL, b"rank k=129"), (4, None, EINVAL, b"null pointer"), (18, 8, EWS, b"workspace 8 < ")):
        call = list(good)
        call[at] = val
        if at == 10:
            call[7] = 129
        assert lib.dnmf_weighted_aht_pair(*call) == code and word in lib.dnmf_last_error(), (at, lib.dnmf_last_error())
    assert lib.dnmf_weighted_ws_bytes(10, 10, 129) == 0 == lib.dnmf_weighted_ws_bytes_fit(0, 10, 4)


def test_main_has_the_weights_flag():
    sys.path.insert(0, ROOT)
    try:
        import main as cli
    finally:
        sys.path.remove(ROOT)
    ap = cli.build_parser()
    assert ap.parse_args(["--p_r=1", "--p_c=1"]).weights is None
    for extra, word in ((["--missing=nan"], "weight 0"), (["--process=pyDNMFk"], "rank estimation"), (["--ftype=spnpz"], "sparse")):
        with pytest.raises(SystemExit, match=word):
            cli.check_missing_flag(ap.parse_args(["--p_r=1", "--p_c=1", "--weights=v"] + extra))
