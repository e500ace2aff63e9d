"""The Huber entry points (csrc/dnmf_huber.hip: dnmf_huber_*) and norm='huber' without a GPU: header, table and exports agree; every bad
argument is refused by the host-side checks before any launch (made-up pointers: the pattern of tests/test_capi.py), naming the entry
point; PyNMF and PyNMFk raise the refusals of the norm."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _is as I  # noqa: E402
from tests.test_capi import EWS, ODD, P16, ROOT, _refused  # noqa: E402
from tests.test_capi_beta import _slabs  # noqa: E402  (the plans are dnmf_beta_plan's by construction: csrc/dnmf_huber.h)

TWINS = dict(uht_pair="aht_pair", wtu_pair="wta_pair", update_w="update_w", update_h="update_h", loss="divergence", mu_fit="mu_fit")


def test_header_table_and_exports_agree():
    from pydnmfk_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dnmf_huber_api.h")).read(), flags=re.S)
    names = sorted("dnmf_huber_" + n for n in list(TWINS) + ["ws_bytes"])
    assert sorted(set(re.findall(r"\b(dnmf_[a-z0-9_]+)\s*\(", txt))) == names == sorted(_lib.HUBER_SIGNATURES)
    assert open(os.path.join(ROOT, "include", "dnmf.h")).read().count('#include "dnmf_huber_api.h"') == 1
    others = [getattr(_lib, t) for t in dir(_lib) if t.endswith("SIGNATURES") and t != "HUBER_SIGNATURES"]
    assert len(others) >= 9 and not any(set(_lib.HUBER_SIGNATURES) & set(t) for t in others)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, twin in TWINS.items():
        assert hasattr(raw, "dnmf_huber_" + name) and getattr(_lib.lib, "dnmf_huber_" + name).argtypes == _lib.BETA_SIGNATURES["dnmf_beta_" + twin]
        assert "float eps, float delta" in re.sub(r"\s+", " ", txt.split("dnmf_huber_" + name + "(")[1].split(")")[0]), name
    assert _lib.lib.dnmf_huber_ws_bytes.restype is ctypes.c_size_t


def test_argument_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    m, n, k = 70, 2085, 32
    assert not any(lib.dnmf_huber_ws_bytes(*bad) for bad in ((0, 10, 4), (10, 0, 4), (-1, 10, 4), (10, 10, 0), (10, 10, 129), (10, 10, -1)))
    (w_slab, h_slab, d_slab), fit_ws = _slabs(m, n, k), lib.dnmf_huber_ws_bytes(m, n, k)
    assert fit_ws == lib.dnmf_beta_ws_bytes_fit(m, n, k) >= max(w_slab, h_slab, d_slab)
    head = dict(A=P16, m=m, n=n, lda=n, W=P16, ldw=k, H=P16, ldh=n, k=k, eps=1e-7, delta=0.5)
    tail = dict(ws=P16, ws_bytes=1 << 40, stream=None)
    calls = {"uht_pair": (w_slab, dict(head, num=P16, den=P16, ldo=k, **tail)), "wtu_pair": (h_slab, dict(head, num=P16, den=P16, ldo=n, **tail)),
             "update_w": (w_slab, dict(head, **tail)), "update_h": (h_slab, dict(head, clamp=0, **tail)),
             "loss": (d_slab, dict(head, out=P16, **tail)), "mu_fit": (fit_ws, dict(head, w_update=1, itr=3, sq_out=P16, **tail))}
    for name, (need, good) in calls.items():
        fn, who = "dnmf_huber_" + name, "huber_" + name
        for delta in (0.0, -1.0, float("nan"), float("-inf")):
            _refused(lib, fn, who, good, delta=delta)
            assert b"delta" in lib.dnmf_last_error()
        nulls = [{a: None} for a in ("A", "W", "H", "num", "den", "out", "sq_out") if a in good]
        for bad in nulls + [dict(k=0), dict(k=129), dict(k=-1), dict(m=0), dict(n=-3), dict(lda=n - 1), dict(ldw=k - 1), dict(ldh=n - 1)]:
            _refused(lib, fn, who, good, **bad)
        for delta in (0.5, float("inf")):                                       # (an accepted delta gets as far as the workspace check)
            _refused(lib, fn, who, dict(good, delta=delta), rc=EWS, ws_bytes=need - 1)
            assert str(need).encode() in lib.dnmf_last_error()
        for bad in (dict(ws=None), dict(ws=ODD), dict(ws_bytes=0)):
            _refused(lib, fn, who, good, rc=EWS, **bad)


def _construct(cls="PyNMF", A=None, k=3, **kw):
    """the class on a 12 x 9 block, norm='huber', delta = 0.5 unless `kw` says otherwise, with an operator set that only names what it takes"""
    from pydnmfk_amd import pyDNMF, pyDNMFk
    A = np.random.RandomState(0).rand(12, 9).astype(np.float32) if A is None else A
    stub = types.SimpleNamespace(name="stub", huber_dtypes=(torch.float32,), weighted_dtypes=(torch.float32,))
    params = I.one_rank_args(k, 3, **dict(dict(norm="huber", delta=0.5), **kw))
    return getattr(pyDNMF if cls == "PyNMF" else pyDNMFk, cls)(A, factors=[np.ones((A.shape[0], k), np.float32), np.ones((k, A.shape[1]), np.float32)], ops=stub, params=params)


def test_pynmf_takes_the_norm_and_refuses_what_it_does_not_serve():
    sp = pytest.importorskip("scipy.sparse")
    from pydnmfk_amd.pyDNMF import _NATIVE_FITS
    nmf = _construct()
    assert (nmf.kind.norm, nmf.kind.family, nmf.kind.batchable, nmf.delta) == ("huber", "huber", False, 0.5) and ("mu", "huber") in _NATIVE_FITS
    assert _construct(delta=float("inf")).delta == float("inf") and _construct(fit_loop="slab").delta == 0.5
    A = np.random.RandomState(0).rand(12, 9).astype(np.float32)
    nan, neg = A.copy(), A.copy()
    nan[1, 1], neg[2, 3] = np.nan, -1.0
    for why, kw in (("sparse data", dict(A=sp.csr_matrix(A))), ("missing='nan'", dict(A=nan, missing="nan", prune=False)),
                    ("bfloat16", dict(precision="bfloat16")), ("float64", dict(A=A.astype(np.float64))), ("--gemm bf16x6", dict(gemm="bf16x6")),
                    ("'hals'", dict(method="hals")), ("'bcd'", dict(method="bcd")), ("2D grid", dict(grid=(2, 2))), ("k = 129", dict(k=129)),
                    ("not for 'huber'", dict(weights=np.ones_like(A), prune=False)), ("PyNMFk with norm='huber'", dict(cls="PyNMFk"))):
        with pytest.raises(NotImplementedError, match="(?=.*huber).*" + re.escape(why)):        # (names the option and the norm)
            _construct(**kw)
    for match, kw in (("params.delta", dict(delta=None)), ("params.delta", dict(delta=0.0)), ("params.delta", dict(delta=-2.0)),
                      ("params.delta", dict(delta=float("nan"))), ("finite non-negative", dict(A=neg)), ("finite non-negative", dict(A=nan))):
        with pytest.raises(ValueError, match=match):
            _construct(**kw)
