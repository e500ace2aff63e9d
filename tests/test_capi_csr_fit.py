"""The whole sparse fits' C ABI (include/dnmf_csr_fit_api.h, _lib.CSR_FIT_SIGNATURES) without a GPU: header against table, the plan's
arithmetic, and what dnmf_csr_mu_fit_batch refuses before any HIP call."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_table_and_exports_agree():
    from pydnmfk_amd import _lib
    declared = sorted(set(re.findall(r"\b(dnmf_[a-z0-9_]+)\s*\(", _text("dnmf_csr_fit_api.h"))))
    assert declared == sorted(_lib.CSR_FIT_SIGNATURES) == ["dnmf_csr_fit_plan", "dnmf_csr_fit_ws_bytes", "dnmf_csr_mu_fit_batch"]
    for name, sig in _lib.CSR_FIT_SIGNATURES.items():
        assert getattr(_lib.lib, name).argtypes == sig, name
    assert _lib.lib.dnmf_csr_fit_ws_bytes.restype is ctypes.c_size_t
    others = [getattr(_lib, t) for t in dir(_lib) if t.endswith("SIGNATURES") and t != "CSR_FIT_SIGNATURES"]
    assert len(others) >= 7 and not any(set(t) & set(_lib.CSR_FIT_SIGNATURES) for t in others)
    assert _text("dnmf.h").count('#include "dnmf_csr_fit_api.h"') == 1


@pytest.mark.parametrize("k, kpad, bt", [(1, 16, 8), (16, 16, 8), (17, 32, 4), (33, 64, 4), (65, 128, 2), (129, 256, 2), (256, 256, 2)])
def test_plan_arithmetic(k, kpad, bt):
    from pydnmfk_amd._lib import csr_fit_plan, lib
    m, n = 70, 1100
    for batch in (1, bt, bt + 1):
        p = csr_fit_plan(m, n, k, batch)
        pb = 1 if batch == 1 else bt                               # a single problem: the plain packed images
        tiles = -(-batch // pb)
        assert (p["kpad"], p["g"], p["bt"], p["tiles"]) == (kpad, kpad // 4, pb, tiles)
        for rows, key in ((m, "w_image_bytes"), (n, "h_image_bytes")):
            exact = tiles * rows * pb * kpad * 4
            assert exact <= p[key] < exact + 256
        assert bt * kpad * 4 >= 128                                # what one stored entry gathers for a tile is whole 128-byte lines
        ws = lib.dnmf_csr_fit_ws_bytes(m, n, k, batch, 3)
        assert ws > p["w_image_bytes"] + p["h_image_bytes"] and ws >= lib.dnmf_csr_fit_ws_bytes(m, n, k, batch, 0)
    out = (ctypes.c_long * 6)()
    for bad in ((0, n, k, 1), (m, n, 0, 1), (m, n, 257, 1), (m, n, k, 0)):
        assert lib.dnmf_csr_fit_plan(*bad, out) == -1 and lib.dnmf_csr_fit_ws_bytes(*bad, 0) == 0


def _args(**change):
    """a full argument list over never-dereferenced host addresses (every case below is refused before any HIP call)"""
    p = 4096
    a = dict(m=8, n=8, k=3, batch=1, nnz=5, crow=p, col=p, long_rows=None, long_segptr=None, n_long=0, nseg=0, t_crow=p, t_col=p,
             t_long_rows=None, t_long_segptr=None, t_n_long=0, t_nseg=0, val=p, t_val=p, val_stride=8, W=p, ldw=3, w_stride=24, H=p, ldh=8,
             h_stride=24, norm=0, missing=0, eps=1e-7, w_update=1, itr=5, ws=p, ws_bytes=1 << 40, sq_out=p, stream=None)
    a.update(change)
    return list(a.values())


@pytest.mark.parametrize("change, text", [(dict(W=None), b"null pointer"), (dict(t_col=None), b"null pointer"), (dict(sq_out=None), b"null pointer"),
                                          (dict(ws=None), b"null pointer"), (dict(k=0), b"rank k=0"), (dict(k=257), b"rank k=257"),
                                          (dict(batch=0), b"batch=0"), (dict(ws_bytes=1024), b"workspace 1024 <"),
                                          (dict(norm=2), b"norm=2"), (dict(n_long=1), b"long-row lists")],
                         ids=["W", "t_col", "sq_out", "ws", "k0", "k257", "batch", "ws_bytes", "norm", "long"])
def test_bad_arguments_are_refused_before_any_hip_call(change, text):
    from pydnmfk_amd._lib import lib
    assert lib.dnmf_csr_mu_fit_batch(*_args(**change)) == -1
    err = lib.dnmf_last_error()
    assert b"csr_mu_fit_batch" in err and text in err, err
