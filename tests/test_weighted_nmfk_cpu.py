"""NMFk under per-entry weights without a GPU: what PyNMFk refuses and accepts at construction, and the ctypes table."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _weighted as Wt  # noqa: E402
from tests.test_weighted_cpu import REFUSALS, ROOT  # noqa: E402


class NmfkOps(Wt.WeightedOracleOps):                            # (no fit runs here: PyNMFk looks for the two names)
    name, weighted_nmfk, weighted_column_div = "oracle-weighted-nmfk", True, None


def nmfk(tmp, A, V, norm, beta=None, ops=None, **kw):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests.test_nmfk_cpu import _args
    a = _args(tmp, MPI_comm(None, 1, 1))
    (a.p_r, a.p_c), a.norm, a.beta, a.end_k, a.weights = kw.pop("grid", (1, 1)), norm, beta, kw.pop("k", 2), V.astype(np.float32)
    vars(a).update(kw)
    return PyNMFk(A, params=a, ops=ops or NmfkOps())


CASES = REFUSALS + [(dict(ops=Wt.WeightedOracleOps()), "PyNMFk.*weights.*oracle-weighted"), (dict(sparse=True), "weights.*sparse"),
                    (dict(norm="is", sampling="poisson"), "norm='is' and sampling='poisson'"),
                    (dict(norm="beta", beta=-1.0, sampling="poisson"), "beta = -1 and sampling='poisson'"),
                    (dict(norm="is", bad=0.0), "needs strictly positive data"),
                    (dict(norm="beta", beta=-1.0, bad=0.0), "needs strictly positive data"),
                    (dict(norm="beta", beta=0.5, bad=-1.0), "needs non-negative data")]


@pytest.mark.parametrize("change,match", CASES, ids=lambda v: str(sorted(v)) if isinstance(v, dict) else None)
def test_what_is_refused_and_accepted_at_construction(tmp_path, change, match):
    """PyNMF's refusals in its words (NotImplementedError); a `bad` entry under a POSITIVE weight (ValueError), while -1 under v = 0
    is not looked at; 'poisson' is accepted under kl"""
    sp = pytest.importorskip("scipy.sparse")
    change = dict(change)
    A, V, _, _, _ = Wt.problem()
    A = np.where(V > 0, A, -1.0).astype(np.float32)
    if "bad" in change:
        assert nmfk(tmp_path, A, V, change["norm"], change.get("beta"))._batch_size() == 1 and nmfk(tmp_path, A, V, "kl", sampling="poisson")._weighted
        A[tuple(np.argwhere(V > 0)[0])] = change.pop("bad")
    with pytest.raises(ValueError if "needs" in match else NotImplementedError, match=match):
        nmfk(tmp_path, sp.csr_matrix(A) if change.pop("sparse", False) else A, V, change.pop("norm", "kl"), **change)


def test_the_ctypes_table_matches_the_header():
    from pydnmfk_amd import _lib, engine
    txt = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/dnmf_weighted_nmfk_api.h").read(), flags=re.S)
    table = _lib.WEIGHTED_NMFK_SIGNATURES
    assert sorted(set(re.findall(r"\b(dnmf_[a-z0-9_]+)\s*\(", txt))) == sorted(table) and len(table) == 3 and engine.HipOps.weighted_nmfk
    assert open(ROOT + "/include/dnmf.h").read().count('#include "dnmf_weighted_nmfk_api.h"') == 1
    assert all(getattr(_lib.lib, name).argtypes == sig for name, sig in table.items())
