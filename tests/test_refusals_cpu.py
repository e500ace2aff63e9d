"""What PyNMF and PyNMFk refuse and accept at construction, as a transcript: for every case of CASES the class name and the complete
str() of what the construction raises, or None where it is accepted, compared for equality with tests/golden/refusals.json.

The fixture was generated from the PARENT of the commit that added this test (a checkout of that parent, this module's `transcript()`
run there on this case list), never from the code under test: the drivers' kind decision was rewritten in that commit, and the
transcript is what held the wording, the exception types and the precedence between competing refusals still.

The cases: per kind (weights, is, beta, missing='nan', sparse, sparse with missing='unstored', plain) every option the kind refuses, the
combinations in which two refusals compete, the operator sets without the capability flag, the constructions without a GPU (ops=None
with torch.cuda.is_available() held False, so that the outcome is the same where a GPU exists), and one accepted construction per kind.
The operator sets are the checker doubles of tests/; no fit runs."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

from tests import _beta_nmfk as BK  # noqa: E402
from tests import _is as I  # noqa: E402
from tests import _is_nmfk as IK  # noqa: E402
from tests import _masked_dense as D  # noqa: E402
from tests import _masked_nmfk as MK  # noqa: E402
from tests import _sparse_nmfk as SK  # noqa: E402
from tests import _weighted as Wt  # noqa: E402
from tests._golden import GOLDEN  # noqa: E402
from tests._ops_double import OracleOps  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "refusals.json")


class WeightedNmfkOps(Wt.WeightedOracleOps):                   # (no fit runs here: PyNMFk looks for the two names)
    name, weighted_nmfk, weighted_column_div = "oracle-weighted-nmfk", True, None


class F64BoundOps(BK.BetaNmfkOracleOps):                        # the rank bound of the float64 pairs, as the product's float64 set names it
    name, is_max_k, beta_max_k = "oracle-f64-bound", 64, 64


OPS = {"plain": OracleOps, "weighted": WeightedNmfkOps, "weighted-fit": Wt.WeightedOracleOps, "is": IK.ISNmfkOracleOps, "is-fit": I.ISOracleOps,
       "beta": BK.BetaNmfkOracleOps, "nan": MK.MaskedNmfkOracleOps, "nan-fit": D.MaskedDenseOracleOps, "sparse": SK.SparseNmfkOracleOps,
       "f64-bound": F64BoundOps, "none": lambda: None}

# what a case may hold: form ('dense' | 'nan' | 'sparse' | 'cpu-tensor' | 'cpu-sparse-tensor'), dtype, weights, bad (an entry planted
# under a positive weight), ops (a key of OPS), k, grid; everything else is set on the params bag as it is
KINDS = {"weights": dict(weights=True, norm="kl", ops="weighted", prune=False),
         "is": dict(norm="is", ops="is"),
         "beta": dict(norm="beta", beta=0.5, ops="beta"),
         "nan": dict(form="nan", norm="fro", missing="nan", ops="nan"),
         "sparse": dict(form="sparse", norm="fro", ops="sparse"),
         "unstored": dict(form="sparse", norm="fro", missing="unstored", ops="sparse"),
         "plain": dict(norm="fro", ops="plain")}
OPTIONS = {"bf16": dict(precision="bfloat16"), "f64": dict(dtype="float64"), "gemm": dict(gemm="bf16x6"), "hals": dict(method="hals"),
           "bcd": dict(method="bcd"), "grid": dict(grid=(2, 2)), "nnsvd": dict(init="nnsvd"), "prune": dict(prune=True), "k129": dict(k=129),
           "poisson": dict(sampling="poisson"), "sign": dict(bad=0.0), "noflag": dict(ops="plain")}
REFUSED = {"weights": "bf16 gemm hals bcd grid nnsvd prune k129 sign noflag",
           "is": "bf16 gemm hals bcd grid k129 poisson sign noflag",
           "beta": "bf16 gemm hals bcd grid k129 poisson sign noflag",
           "nan": "bf16 f64 gemm hals bcd grid nnsvd prune k129 noflag",
           "sparse": "bf16 f64 gemm grid nnsvd noflag",
           "unstored": "hals bcd noflag",
           "plain": ""}
BOTH = ("PyNMF", "PyNMFk")


def _cases():
    out = {}

    def add(name, classes=BOTH, **case):
        for cls in classes:
            assert cls + ":" + name not in out, name
            out[cls + ":" + name] = dict(case, cls=cls)
    for kind, base in KINDS.items():
        add(kind + " accepted", **base)
        for opt in REFUSED[kind].split():
            add("%s + %s" % (kind, opt), classes=("PyNMFk",) if opt == "poisson" else BOTH, **dict(base, **OPTIONS[opt]))
        add(kind + " without a GPU", **dict(base, ops="none"))
    # the capability flag alone missing: an operator set that fits under the kind but has no per-column statistic of a sweep
    add("weights + a set lacking weighted_nmfk", **dict(KINDS["weights"], ops="weighted-fit"))
    add("is + a set lacking is_nmfk", **dict(KINDS["is"], ops="is-fit"))
    add("beta + a set lacking beta_nmfk", **dict(KINDS["beta"], ops="is"))
    add("nan + a set lacking masked_nmfk", **dict(KINDS["nan"], ops="nan-fit"))
    # float64 data
    for kind in ("is", "beta"):
        add(kind + " float64 + k = 65", **dict(KINDS[kind], dtype="float64", ops="f64-bound", k=65))
        add(kind + " float64 + k = 64", **dict(KINDS[kind], dtype="float64", ops="f64-bound", k=64))
        add(kind + " float64 + a float32 set", **dict(KINDS[kind], dtype="float64", ops="plain"))
    add("weights + float64 + a float32 set", **dict(KINDS["weights"], dtype="float64", ops="plain"))
    add("weights + float64", **dict(KINDS["weights"], dtype="float64"))
    # the sampling and the sign, norm by norm
    add("beta = -1 + poisson", classes=("PyNMFk",), **dict(KINDS["beta"], beta=-1.0, sampling="poisson"))
    add("beta = 0 + poisson", classes=("PyNMFk",), **dict(KINDS["beta"], beta=0.0, sampling="poisson"))
    add("beta = 1 + poisson", classes=("PyNMFk",), **dict(KINDS["beta"], beta=1.0, sampling="poisson"))
    add("beta = -1 + a zero", **dict(KINDS["beta"], beta=-1.0, bad=0.0))
    add("beta = 0 + a zero", **dict(KINDS["beta"], beta=0.0, bad=0.0))
    add("beta = 0.5 + a zero", **dict(KINDS["beta"], bad=0.0))
    add("beta = 0.5 + a negative entry", **dict(KINDS["beta"], bad=-1.0))
    add("beta = 0 accepted", **dict(KINDS["beta"], beta=0.0))
    add("itakura-saito accepted", **dict(KINDS["is"], norm="itakura-saito"))
    add("beta without params.beta", **dict(KINDS["beta"], beta=None))
    add("beta = 5", **dict(KINDS["beta"], beta=5.0))
    for norm, beta, bad in (("is", None, 0.0), ("beta", -1.0, 0.0), ("beta", 0.5, -1.0), ("kl", None, -0.5), ("fro", None, float("nan"))):
        add("weights + %s%s + %g under a positive weight" % (norm, "" if beta is None else " %g" % beta, bad),
            **dict(KINDS["weights"], norm=norm, beta=beta, bad=bad))
    add("weights + is accepted", **dict(KINDS["weights"], norm="is"))
    add("weights + beta accepted", **dict(KINDS["weights"], norm="beta", beta=3.0))
    add("weights + kl + poisson", classes=("PyNMFk",), **dict(KINDS["weights"], sampling="poisson"))
    add("weights + beta = 0.5 + poisson", classes=("PyNMFk",), **dict(KINDS["weights"], norm="beta", beta=0.5, sampling="poisson"))
    add("weights + an unknown norm", **dict(KINDS["weights"], norm="l1"))
    add("weights of another shape", **dict(KINDS["weights"], weights="shape"))
    add("weights all zero", **dict(KINDS["weights"], weights="zero"))
    # two refusals compete
    add("weights + sparse", **dict(KINDS["weights"], form="sparse"))
    add("weights + missing='nan'", **dict(KINDS["weights"], form="nan", missing="nan"))
    add("is + sparse", **dict(KINDS["is"], form="sparse"))
    add("beta + sparse", **dict(KINDS["beta"], form="sparse"))
    add("is + missing='nan'", **dict(KINDS["is"], form="nan", missing="nan"))
    add("beta + missing='nan'", **dict(KINDS["beta"], form="nan", missing="nan"))
    add("weights + is + poisson", classes=("PyNMFk",), **dict(KINDS["weights"], norm="is", sampling="poisson"))
    add("weights + beta = -1 + poisson + prune", classes=("PyNMFk",), **dict(KINDS["weights"], norm="beta", beta=-1.0, sampling="poisson", prune=True))
    add("weights + sparse + a set lacking weighted_nmfk", **dict(KINDS["weights"], form="sparse", ops="weighted-fit"))
    add("weights + is + hals", **dict(KINDS["weights"], norm="is", method="hals"))
    add("missing='nan' + sparse", **dict(KINDS["sparse"], missing="nan"))
    add("missing='nan' + sparse + a set lacking sparse_nmfk", **dict(KINDS["sparse"], missing="nan", ops="plain"))
    add("is + sparse + a set lacking is_nmfk", **dict(KINDS["is"], form="sparse", ops="sparse"))
    add("is + hals + k = 129 + a 2D grid", **dict(KINDS["is"], method="hals", k=129, grid=(2, 2)))
    add("nan + prune + k = 129", **dict(KINDS["nan"], prune=True, k=129))
    add("nan + prune + a set lacking masked_nmfk", **dict(KINDS["nan"], prune=True, ops="nan-fit"))
    add("nan + bf16 + kl", **dict(KINDS["nan"], precision="bfloat16", norm="kl"))
    for kind in KINDS:
        add(kind + " + nmfk_split unknown + hals + prune", classes=("PyNMFk",), **dict(KINDS[kind], nmfk_split="ranks", method="hals", prune=True))
    # the rest of what the constructors refuse by themselves
    add("plain + bf16 + kl", **dict(KINDS["plain"], precision="bfloat16", norm="kl"))
    add("missing unknown", **dict(KINDS["plain"], missing="zero"))
    add("missing='unstored' + dense", **dict(KINDS["plain"], missing="unstored"))
    add("sparse + bf16 + a 2D grid", **dict(KINDS["sparse"], precision="bfloat16", grid=(2, 2)))
    # a CPU tensor and no operator set: refused before the GPU is looked for
    for kind in ("weights", "is", "nan", "plain"):
        add(kind + " + a CPU tensor without a GPU", **dict(KINDS[kind], form="nan-tensor" if kind == "nan" else "cpu-tensor", ops="none"))
    add("sparse + a CPU tensor without a GPU", **dict(KINDS["sparse"], form="cpu-sparse-tensor", ops="none"))
    return out


CASES = _cases()


def _construct(tmp, case):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMF import PyNMF
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests.test_nmfk_cpu import _args
    case = dict(case)
    cls, form, dtype = case.pop("cls"), case.pop("form", "dense"), case.pop("dtype", "float32")
    k, grid, bad, weights = case.pop("k", 3), case.pop("grid", (1, 1)), case.pop("bad", None), case.pop("weights", False)
    ops = OPS[case.pop("ops")]()
    A = I.problem()[0]                                       # 50 x 39, strictly positive
    V = Wt.weights(A.shape, 12, 0.3)
    if weights:
        A = np.where(V > 0, A, -1.0)                         # (what lies under a zero weight is not looked at)
    if bad is not None:
        A[tuple(np.argwhere(V > 0)[0])] = bad
    if form in ("nan", "nan-tensor"):
        A[np.random.RandomState(3).rand(*A.shape) < 0.2] = np.nan
    A = A.astype(dtype)
    if form == "sparse":
        A = sp.csr_matrix(A)
    elif form in ("cpu-tensor", "nan-tensor"):
        A = torch.from_numpy(A)
    elif form == "cpu-sparse-tensor":
        A = torch.from_numpy(A).to_sparse_csr()
    if cls == "PyNMF":
        a = I.one_rank_args(k, 3, grid=grid, norm=case.pop("norm"), prune=case.pop("prune", False))
    else:
        a = _args(tmp, MPI_comm(None, 1, 1))
        (a.p_r, a.p_c), a.start_k, a.end_k, a.norm, a.prune = grid, 2, k, case.pop("norm"), case.pop("prune", False)
    if weights:
        a.weights = V[:, :-1] if weights == "shape" else V * 0 if weights == "zero" else V
    vars(a).update(case)
    (PyNMF if cls == "PyNMF" else PyNMFk)(A, params=a, ops=ops)


def transcript(tmp, no_gpu):
    """{case: [the exception's class name, its str()] or None}; `no_gpu(True / False)` holds torch.cuda.is_available() False for the
    cases without an operator set"""
    out = {}
    for name, case in CASES.items():
        no_gpu(case["ops"] == "none")
        np.random.seed(0)
        try:
            _construct(tmp, case)
            out[name] = None
        except Exception as ex:  # noqa: BLE001
            out[name] = [type(ex).__name__, str(ex)]
    no_gpu(False)
    return out


def test_the_transcript_of_refusals_is_the_recorded_one(tmp_path, monkeypatch):
    def no_gpu(on):
        monkeypatch.undo()
        if on:
            monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    got = transcript(tmp_path, no_gpu)
    want = json.load(open(FIXTURE))
    assert sorted(got) == sorted(want)
    for name in CASES:
        print(name, "->", got[name])
    wrong = {name: (got[name], want[name]) for name in CASES if got[name] != want[name]}
    assert not wrong, wrong
    # the list is what the fixture's docstring says it is: every kind has refusals of each type and an accepted construction
    kinds = [v[0] for v in want.values() if v is not None]
    assert {"NotImplementedError", "ValueError", "TypeError", "RuntimeError"} <= set(kinds) and sum(v is None for v in want.values()) >= 16
