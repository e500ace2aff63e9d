"""The entry points NMFk over a NaN-marked block adds (csrc/dnmf_masked.hip: dnmf_masked_column_err{,_ws_bytes,_plan},
dnmf_masked_{ws_bytes_fit,mu_fit}) without a GPU: every bad argument is refused by the host-side checks before any launch -- the
pointers are made-up addresses that nothing may dereference (the pattern of tests/test_capi.py) --, the workspace query equals the
slab recomputed from the plan, and the plan shows which shapes of tests/test_gpu_masked_nmfk.py enter which loop of
col_sums_kernel (tests/_masked_nmfk.py::COLERR_LOOP_CASES)."""
import ctypes

import pytest

from tests import _masked_dense as D
from tests import _masked_nmfk as N
from tests.test_capi import EINVAL, EWS, ODD, P16, _align256, _refused

KS = (1, 3, 16, 17, 32, 33, 64, 100, 128)
SHAPES = ((1, 1), (7, 5), (129, 33), (300, 257), (53, 37), (120, 90)) + N.COLERR_SHAPES


def _plan(m, n, k):
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 3)(*([-7] * 3))
    assert lib.dnmf_masked_column_err_plan(m, n, k, out) == 0, lib.dnmf_last_error()
    return N.colerr_reach(m, n, out)


def _slab(m, n, k):
    """one float64 pair per chunk and column of the 128-padded width (include/dnmf.h)"""
    p = _plan(m, n, k)
    return p["nchunks"] * 2 * p["ncolblk"] * 128 * 8


def test_column_err_plan_refusals_and_invariants():
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 3)()
    good = dict(m=130, n=133, k=32, out=ctypes.addressof(out))
    for bad in (dict(k=0), dict(k=129), dict(k=-1), dict(m=0), dict(n=0), dict(m=-3), dict(out=None)):
        _refused(lib, "dnmf_masked_column_err_plan", "masked_column_err_plan", good, **bad)
    for m, n in SHAPES + ((40000, 17), (5, 40000), (1 << 20, 3)):
        plans = [_plan(m, n, k) for k in KS]
        assert all(p == plans[0] for p in plans), (m, n)                 # the plan does not depend on the rank
        p, nrowblk = plans[0], -(-m // 32)
        assert p["ncolblk"] == -(-n // 128) and 1 <= p["last_colblk_cols"] <= 128, (m, n, p)
        # every row block belongs to exactly one chunk, none of which is empty
        assert 1 <= p["nchunks"] <= 256 and 1 <= p["last_chunk_blks"] <= p["rowblks_per_chunk"] and 1 <= p["last_blk_rows"] <= 32, (m, n, p)
        assert (p["nchunks"] - 1) * p["rowblks_per_chunk"] < nrowblk <= p["nchunks"] * p["rowblks_per_chunk"], (m, n, p)


def test_column_err_workspace_query_is_the_slab_of_the_plan():
    from pydnmfk_amd._lib import lib
    q = lib.dnmf_masked_column_err_ws_bytes
    for bad in ((0, 10, 4), (10, 0, 4), (-1, 10, 4), (10, -1, 4), (10, 10, 0), (10, 10, 129), (10, 10, -1)):
        assert q(*bad) == 0, bad
    for m, n in SHAPES:
        for k in KS:
            assert q(m, n, k) == _align256(_slab(m, n, k)) >= 256, (m, n, k)


@pytest.mark.parametrize("case", N.COLERR_LOOP_CASES, ids=lambda c: "%dx%d" % c["shape"])
def test_loop_shapes_reach_what_their_table_entry_says(case):
    m, n = case["shape"]
    assert (n % 4 == 0) == case["fast"]
    for k in N.COLERR_KS:
        p = _plan(m, n, k)
        for what, want in case["reach"].items():
            assert p[what] == want, "%dx%d k=%d: %s is %d, the table says %d (plan %s)" % (m, n, k, what, p[what], want, p)


def test_loop_shapes_between_them_leave_one_trip_of_each_loop():
    reach = [c["reach"] for c in N.COLERR_LOOP_CASES]
    assert all(r["ncolblk"] >= 2 and r["last_colblk_cols"] < 128 for r in reach)                       # a ragged second column block
    assert any(r["rowblks_per_chunk"] >= 2 for r in reach)                                             # the row-block loop
    assert any(r["rowblks_per_chunk"] >= 2 and r["nchunks"] >= 2 and r["last_chunk_blks"] < r["rowblks_per_chunk"]
               and r["last_blk_rows"] < 32 for r in reach)                                             # ragged last chunk, ragged last block
    for m, n in D.EXACT_SHAPES:                                                                        # the shapes they add to
        p = _plan(m, n, 32)
        assert p["rowblks_per_chunk"] == 1 and p["ncolblk"] == 1 and p["nchunks"] == -(-m // 32) >= 2, (m, n, p)


def test_column_err_argument_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    fn, who = "dnmf_masked_column_err", "masked_column_err"
    m, n, k = 8261, 133, 32
    good = dict(A=P16, m=m, n=n, lda=n, W=P16, ldw=k, H=P16, ldh=n, k=k, num=P16, den=P16, ws=P16, ws_bytes=1 << 40, stream=None)
    for a in ("A", "W", "H", "num", "den"):
        _refused(lib, fn, who, good, **{a: None})
    for bad_k in (0, 129, -1):
        _refused(lib, fn, who, good, k=bad_k)
    _refused(lib, fn, who, good, ldw=k - 1)
    _refused(lib, fn, who, good, ldh=n - 1)
    _refused(lib, fn, who, good, lda=n - 1)
    for a in ("m", "n"):
        for v in (0, -3):
            _refused(lib, fn, who, good, **{a: v})
    need = _slab(m, n, k)
    _refused(lib, fn, who, good, rc=EWS, ws_bytes=need - 1)
    assert str(need).encode() in lib.dnmf_last_error()
    _refused(lib, fn, who, good, rc=EWS, ws=None)
    _refused(lib, fn, who, good, rc=EWS, ws=ODD)
    _refused(lib, fn, who, good, rc=EWS, ws_bytes=0)
    assert EINVAL != 0 and EWS != 0


def test_masked_fit_argument_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    q = lib.dnmf_masked_ws_bytes_fit
    for bad in ((0, 10, 4), (10, 0, 4), (-1, 10, 4), (10, -1, 4), (10, 10, 0), (10, 10, 129), (10, 10, -1)):
        assert q(*bad) == 0, bad
    for m, n in SHAPES:
        for k in KS:
            # the step's slabs and room for the normalisation and the three sums behind them
            assert q(m, n, k) % 256 == 0 and q(m, n, k) > lib.dnmf_masked_ws_bytes(m, n, k), (m, n, k)
    fn, who = "dnmf_masked_mu_fit", "masked_mu_fit"
    m, n, k = 300, 200, 4
    need = q(m, n, k)
    good = dict(A=P16, m=m, n=n, lda=n, W=P16, ldw=k, H=P16, ldh=n, k=k, eps=1e-7, kl=0, w_update=1, itr=5, sq_out=P16, ws=P16,
                ws_bytes=need, stream=None)
    for kl in (0, 1):
        good = dict(good, kl=kl)
        for a in ("A", "W", "H", "sq_out"):
            _refused(lib, fn, who, good, **{a: None})
        for bad_k in (0, 129, -1):
            _refused(lib, fn, who, good, k=bad_k)
        _refused(lib, fn, who, good, ldw=k - 1)
        _refused(lib, fn, who, good, ldh=n - 1)
        _refused(lib, fn, who, good, lda=n - 1)
        _refused(lib, fn, who, good, itr=-1)
        for a in ("m", "n"):
            for v in (0, -3):
                _refused(lib, fn, who, good, **{a: v})
        _refused(lib, fn, who, good, rc=EWS, ws_bytes=need - 1)
        assert str(need).encode() in lib.dnmf_last_error()
        _refused(lib, fn, who, good, rc=EWS, ws=None)
        _refused(lib, fn, who, good, rc=EWS, ws=ODD)
        _refused(lib, fn, who, good, rc=EWS, ws_bytes=0)
