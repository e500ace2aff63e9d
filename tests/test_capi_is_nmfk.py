"""The entry points NMFk under norm='is' adds (csrc/dnmf_is.hip: dnmf_is_column_div{,_ws_bytes,_plan}) without a GPU: every bad
argument is refused by the host-side checks before any launch -- the pointers are made-up addresses that nothing may dereference (the
pattern of tests/test_capi.py) --, the workspace query equals the slab recomputed from the plan (ONE double per chunk and column), and
the plan is the masked per-column one: the loop shapes of tests/_masked_nmfk.py::COLERR_LOOP_CASES reach what their table says."""
import ctypes

import pytest

from tests import _masked_nmfk as N
from tests.test_capi import EINVAL, EWS, ODD, P16, _align256, _refused

KS = (3, 32, 64, 128)
SHAPES = ((1, 1), (7, 5), (129, 33), (300, 257), (120, 90)) + tuple(c["shape"] for c in N.COLERR_LOOP_CASES)


def _plan(m, n, k):
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 3)(*([-7] * 3))
    assert lib.dnmf_is_column_div_plan(m, n, k, out) == 0, lib.dnmf_last_error()
    return N.colerr_reach(m, n, out)


def test_symbols_are_bound_with_their_result_types():
    from pydnmfk_amd import _lib
    for name in ("dnmf_is_column_div_ws_bytes", "dnmf_is_column_div_plan", "dnmf_is_column_div"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert _lib.lib.dnmf_is_column_div_ws_bytes.restype is ctypes.c_size_t
    assert len(_lib.SIGNATURES["dnmf_is_column_div"]) == 14


@pytest.mark.parametrize("case", N.COLERR_LOOP_CASES, ids=lambda c: "%dx%d" % c["shape"])
def test_loop_shapes_reach_what_the_masked_table_says(case):
    from pydnmfk_amd._lib import lib
    m, n = case["shape"]
    assert (n % 4 == 0) == case["fast"]
    for k in KS:
        p = _plan(m, n, k)
        for what, want in case["reach"].items():
            assert p[what] == want, "%dx%d k=%d: %s is %d, the table says %d (plan %s)" % (m, n, k, what, p[what], want, p)
        masked = (ctypes.c_long * 3)()
        assert lib.dnmf_masked_column_err_plan(m, n, k, masked) == 0 and N.colerr_reach(m, n, masked) == p       # the same plan


def test_plan_refusals():
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 3)()
    good = dict(m=130, n=133, k=32, out=ctypes.addressof(out))
    for bad in (dict(k=0), dict(k=129), dict(k=-1), dict(m=0), dict(n=0), dict(m=-3), dict(out=None)):
        _refused(lib, "dnmf_is_column_div_plan", "is_column_div_plan", good, **bad)
    _refused(lib, "dnmf_is_column_div_plan", "is_column_div_plan", good, k=129)
    assert b"Itakura-Saito kernels" in lib.dnmf_last_error()                       # the wording of the other dnmf_is_* entry points


def test_workspace_query_is_one_double_per_chunk_and_column():
    from pydnmfk_amd._lib import lib
    q = lib.dnmf_is_column_div_ws_bytes
    for bad in ((0, 10, 4), (10, 0, 4), (-1, 10, 4), (10, -1, 4), (10, 10, 0), (10, 10, 129), (10, 10, -1)):
        assert q(*bad) == 0, bad
    for m, n in SHAPES:
        for k in KS:
            p = _plan(m, n, k)
            assert q(m, n, k) == _align256(p["nchunks"] * p["ncolblk"] * 128 * 8) >= 256, (m, n, k)
            # the masked slab holds a pair: the plan moved to a header leaves it as it was
            assert lib.dnmf_masked_column_err_ws_bytes(m, n, k) == _align256(p["nchunks"] * 2 * p["ncolblk"] * 128 * 8), (m, n, k)


def test_argument_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    fn, who = "dnmf_is_column_div", "is_column_div"
    m, n, k = 8261, 133, 32
    good = dict(A=P16, m=m, n=n, lda=n, W=P16, ldw=k, H=P16, ldh=n, k=k, eps=1e-7, div=P16, ws=P16, ws_bytes=1 << 40, stream=None)
    for a in ("A", "W", "H", "div"):
        _refused(lib, fn, who, good, **{a: None})
    for bad_k in (0, 129, -1):
        _refused(lib, fn, who, good, k=bad_k)
        assert b"Itakura-Saito kernels" in lib.dnmf_last_error()
    _refused(lib, fn, who, good, ldw=k - 1)
    _refused(lib, fn, who, good, ldh=n - 1)
    _refused(lib, fn, who, good, lda=n - 1)
    for a in ("m", "n"):
        for v in (0, -3):
            _refused(lib, fn, who, good, **{a: v})
    p = _plan(m, n, k)
    need = p["nchunks"] * p["ncolblk"] * 128 * 8
    _refused(lib, fn, who, good, rc=EWS, ws_bytes=need - 1)
    assert str(need).encode() in lib.dnmf_last_error()
    _refused(lib, fn, who, good, rc=EWS, ws=None)
    _refused(lib, fn, who, good, rc=EWS, ws=ODD)
    _refused(lib, fn, who, good, rc=EWS, ws_bytes=0)
    assert EINVAL != 0 and EWS != 0
