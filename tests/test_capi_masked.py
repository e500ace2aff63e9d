"""The entry points of the NaN-marked dense path (csrc/dnmf_masked.hip: dnmf_masked_*) without a GPU: every bad argument is refused by
the host-side checks with a non-zero code, before any launch -- the pointers are made-up addresses that nothing may dereference (the
pattern of tests/test_capi.py) --, the workspace query equals the slab sizes recomputed from the launch plans, and the plans
(dnmf_masked_plan) show which shapes of the suite enter the tile loop of masked_uht_kernel, the row-block loop of masked_wtu_kernel
and the second grid-stride trip of masked_reduce_kernel (tests/_masked_dense.py::EXACT_LOOP_CASES) -- and which do not."""
import ctypes

import pytest

from tests import _masked_dense as D
from tests.test_capi import EINVAL, EWS, ODD, P16, _align256, _refused

KS = (1, 3, 16, 17, 32, 33, 64, 100, 128)                 # the ranks of tests/test_gpu_masked_dense.py
OLD_SHAPES = ((1, 1), (7, 5), (129, 33), (300, 257), (300, 200), (24, 12), (1024, 256)) + D.EXACT_SHAPES
ALL_SHAPES = OLD_SHAPES + D.EXACT_LOOP_SHAPES


def _plan(m, n, k):
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 6)(*([-7] * 6))
    assert lib.dnmf_masked_plan(m, n, k, out) == 0, lib.dnmf_last_error()
    return D.plan_reach(m, n, k, out, lib.dnmf_masked_reduce_grid)


def _kp(k):
    return 32 if k <= 32 else (64 if k <= 64 else 128)


def _slabs(m, n, k):
    """(W side, H side) partial slabs in bytes from the plan (include/dnmf.h): nsplit * 2 * m * KP and nchunks * 2 * KP * ldp floats,
    ldp = n rounded up to the H side's column block of 4096 / KP columns"""
    p, kp = _plan(m, n, k), _kp(k)
    cw = 4096 // kp
    ldp = -(-n // cw) * cw
    return p["nsplit"] * 2 * m * kp * 4, p["nchunks"] * 2 * kp * ldp * 4


# ---- 1. the plan query itself
def test_masked_plan_refusals_and_invariants():
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 6)()
    good = dict(m=70, n=2085, k=32, out=ctypes.addressof(out))
    for bad in (dict(k=0), dict(k=129), dict(k=-1), dict(m=0), dict(n=0), dict(m=-3), dict(out=None)):
        _refused(lib, "dnmf_masked_plan", "masked_plan", good, **bad)
    for m, n in ALL_SHAPES + ((40000, 17), (5, 40000), (1 << 20, 3)):
        for k in KS:
            p = _plan(m, n, k)
            tiles = -(-n // 32)
            assert p["nrowblk"] == -(-m // 32) and p["zdim"] == (2 if k > 64 else 1), (m, n, k, p)
            # every tile and every row block belongs to exactly one split / chunk, none of which is empty
            assert 1 <= p["nsplit"] <= 32 and (p["nsplit"] - 1) * p["tiles_per_split"] < tiles <= p["nsplit"] * p["tiles_per_split"], (m, n, k, p)
            assert 1 <= p["last_split_tiles"] <= p["tiles_per_split"] and 1 <= p["last_tile_cols"] <= 32, (m, n, k, p)
            assert 1 <= p["nchunks"] <= 64 and 1 <= p["last_chunk_blks"] <= p["rowblks_per_chunk"], (m, n, k, p)
            assert (p["nchunks"] - 1) * p["rowblks_per_chunk"] < p["nrowblk"] <= p["nchunks"] * p["rowblks_per_chunk"], (m, n, k, p)


# ---- 2. the workspace query
def test_masked_workspace_query_is_the_larger_slab():
    from pydnmfk_amd._lib import lib
    q = lib.dnmf_masked_ws_bytes
    for bad in ((0, 10, 4), (10, 0, 4), (-1, 10, 4), (10, -1, 4), (10, 10, 0), (10, 10, 129), (10, 10, -1)):
        assert q(*bad) == 0, bad
    for m, n in ALL_SHAPES:
        for k in KS:
            assert q(m, n, k) == _align256(max(_slabs(m, n, k))) >= 256, (m, n, k)


# ---- 3. which shapes reach the loops
@pytest.mark.parametrize("shape", D.EXACT_LOOP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_loop_shapes_reach_what_their_table_entry_says(shape):
    case = D.loop_case(shape)
    m, n = shape
    assert case["reach"] and (n % 4 == 0) == case["fast"]                # (the vector kernels need whole 16-byte rows of A and H)
    for k in case["ks"]:
        p = _plan(m, n, k)
        for what, want in case["reach"].items():
            assert p[what] == want, "%dx%d k=%d: %s is %d, the table says %d (plan %s)" % (m, n, k, what, p[what], want, p)
    # what the entries mean for the kernels: more than one tile per workgroup / more than one row block per wave
    r = case["reach"]
    if "tiles_per_split" in r:
        assert r["tiles_per_split"] >= 2 and r["last_split_tiles"] >= 2 and r["last_tile_cols"] < 32
    if "rowblks_per_chunk" in r:
        assert r["rowblks_per_chunk"] >= 2 and r["last_blk_rows"] < 32


def test_loop_shapes_between_them_reach_a_short_last_chunk_and_a_second_reduce_trip():
    reach = [c["reach"] for c in D.EXACT_LOOP_CASES]
    assert any(r["last_chunk_blks"] < r["rowblks_per_chunk"] for r in reach if "rowblks_per_chunk" in r)
    assert any(r.get("w_reduce_trips", 1) >= 2 for r in reach)


def test_masked_reduce_grid_query():
    """the grid of the ending as the launches size it: a workgroup per 256 output elements up to a cap, never empty"""
    from pydnmfk_amd._lib import lib
    q = lib.dnmf_masked_reduce_grid
    for bad in ((0, 4), (4, 0), (-1, 4), (4, -1)):
        assert q(*bad) == 0, bad
    cap = q(1 << 20, 128)
    for rows, cols in ((1, 1), (1, 256), (1, 257), (70, 128), (16400, 128), (128, 41), (1 << 20, 3)):
        assert q(rows, cols) == min(-(-rows * cols // 256), cap) >= 1, (rows, cols)


@pytest.mark.parametrize("shape", OLD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_earlier_shapes_stay_at_one_trip_of_each_loop(shape):
    """every shape tests/test_gpu_masked_dense.py had before EXACT_LOOP_SHAPES: one tile per column split, one row block per wave, one
    trip of the reduce -- the gap those shapes close.  A retune of the plans that moves it shows here."""
    m, n = shape
    for k in KS:
        p = _plan(m, n, k)
        assert p["tiles_per_split"] == 1 and p["rowblks_per_chunk"] == 1, (shape, k, p)
        assert p["w_reduce_trips"] == 1 and p["h_reduce_trips"] == 1, (shape, k, p)


# ---- 4. refusals
def _calls(m=70, n=2085, k=32):
    """{entry point: (name in dnmf_last_error, ordered good arguments)}"""
    head = dict(A=P16, m=m, n=n, lda=n, W=P16, ldw=k, H=P16, ldh=n, k=k)
    tail = dict(ws=P16, ws_bytes=1 << 40, stream=None)
    return {
        "dnmf_masked_aht_pair": ("masked_aht_pair", dict(head, eps=1e-7, kl=0, num=P16, den=P16, ldo=k, **tail)),
        "dnmf_masked_wta_pair": ("masked_wta_pair", dict(head, eps=1e-7, kl=0, num=P16, den=P16, ldo=n, **tail)),
        "dnmf_masked_update_w": ("masked_update_w", dict(head, eps=1e-7, kl=0, **tail)),
        "dnmf_masked_update_h": ("masked_update_h", dict(head, eps=1e-7, kl=0, clamp=0, **tail)),
        "dnmf_masked_resid_sqnorm": ("masked_resid_sqnorm", dict(head, sq=P16, stream=None)),
        "dnmf_masked_sqnorm": ("masked_sqnorm", dict(A=P16, m=m, n=n, lda=n, out=P16, stream=None)),
    }


def test_masked_argument_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    m, n, k = 70, 2085, 32
    w_slab, h_slab = _slabs(m, n, k)
    for fn, (who, good) in _calls(m, n, k).items():
        for kl in ((0, 1) if "kl" in good else (0,)):
            if "kl" in good:
                good = dict(good, kl=kl)
            for a in ("A", "W", "H", "num", "den", "sq", "out"):                 # null operands and outputs
                if a in good:
                    _refused(lib, fn, who, good, **{a: None})
            if "k" in good:
                for bad_k in (0, 129, -1):
                    _refused(lib, fn, who, good, k=bad_k)
                _refused(lib, fn, who, good, ldw=k - 1)
                _refused(lib, fn, who, good, ldh=n - 1)
            _refused(lib, fn, who, good, lda=n - 1)
            for a in ("m", "n"):
                for v in (0, -3):
                    _refused(lib, fn, who, good, **{a: v})
            if "ldo" in good:
                _refused(lib, fn, who, good, ldo=good["ldo"] - 1)
            if "ws" in good:                                                     # workspace: one byte short, null, misaligned
                need = w_slab if fn in ("dnmf_masked_aht_pair", "dnmf_masked_update_w") else h_slab
                _refused(lib, fn, who, good, rc=EWS, ws_bytes=need - 1)
                assert str(need).encode() in lib.dnmf_last_error()
                _refused(lib, fn, who, good, rc=EWS, ws=None)
                _refused(lib, fn, who, good, rc=EWS, ws=ODD)
                _refused(lib, fn, who, good, rc=EWS, ws_bytes=0)
    assert EINVAL != 0 and EWS != 0
