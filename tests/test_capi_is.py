"""The entry points of the Itakura-Saito path (csrc/dnmf_is.hip: dnmf_is_*) without a GPU: every symbol is bound, every bad argument
is refused by the host-side checks with a non-zero code before any launch -- the pointers are made-up addresses that nothing may
dereference (the pattern of tests/test_capi.py) --, the workspace queries equal the sizes recomputed from the launch plan, and the
plan (dnmf_is_plan: the masked launch geometry with whole workgroups on the H side and one pass over S at KP = 128) shows which shapes of
tests/test_gpu_is.py enter the tile loop of the W side, the row-block loop of the H side and the second grid-stride trip of the
ending (tests/_is.py::EXACT_LOOP_CASES) -- and which stay at one trip of each."""
import ctypes

import pytest

from tests import _is as I
from tests.test_capi import EINVAL, EWS, ODD, P16, _align256, _refused

KS = (1, 3, 16, 17, 32, 33, 64, 100, 128)
LOOP_SHAPES = tuple(c["shape"] for c in I.EXACT_LOOP_CASES)
ONE_TRIP_SHAPES = ((1, 1), (7, 5), (50, 39), (200, 136)) + I.EXACT_SHAPES
SYMBOLS = ("dnmf_is_ws_bytes", "dnmf_is_ws_bytes_fit", "dnmf_is_plan", "dnmf_is_aht_pair", "dnmf_is_wta_pair", "dnmf_is_update_w",
           "dnmf_is_update_h", "dnmf_is_ratio_update", "dnmf_is_divergence", "dnmf_is_mu_fit")


def _plan(m, n, k):
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 8)(*([-7] * 8))
    assert lib.dnmf_is_plan(m, n, k, out) == 0, lib.dnmf_last_error()
    return I.plan_reach(m, n, k, out)


def _kp(k):
    return 32 if k <= 32 else (64 if k <= 64 else 128)


def _slabs(m, n, k):
    """(W side, H side, divergence) workspace in bytes from the plan (include/dnmf.h): nsplit * 2 * m * KP and nchunks * 2 * KP * ldp
    floats, ldp = n rounded up to the H side's column block of 4096 / KP columns; one double per 32 x 128 tile"""
    p, kp = _plan(m, n, k), _kp(k)
    cw = 4096 // kp
    ldp = -(-n // cw) * cw
    return p["nsplit"] * 2 * m * kp * 4, p["nchunks"] * 2 * kp * ldp * 4, -(-m // 32) * -(-n // 128) * 8


def test_every_symbol_is_declared_and_bound():
    import os
    from pydnmfk_amd._lib import SIGNATURES, lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dnmf.h")).read()
    for name in SYMBOLS:
        assert name in SIGNATURES and callable(getattr(lib, name)) and (name + "(") in header, name
    assert lib.dnmf_is_ws_bytes.restype is ctypes.c_size_t and lib.dnmf_is_ws_bytes_fit.restype is ctypes.c_size_t


def test_is_plan_is_the_masked_plan_with_whole_workgroups_and_refuses_bad_arguments():
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 8)()
    good = dict(m=70, n=2085, k=32, out=ctypes.addressof(out))
    for bad in (dict(k=0), dict(k=129), dict(k=-1), dict(m=0), dict(n=0), dict(m=-3), dict(out=None)):
        _refused(lib, "dnmf_is_plan", "is_plan", good, **bad)
    six = (ctypes.c_long * 6)()
    for m, n in LOOP_SHAPES + ONE_TRIP_SHAPES + ((40000, 17), (5, 40000), (32768, 16384)):
        for k in KS:
            assert lib.dnmf_is_plan(m, n, k, out) == 0 and lib.dnmf_masked_plan(m, n, k, six) == 0
            kp = _kp(k)
            ncolblk, nrowblk, tiles, rowtiles = -(-n // (4096 // kp)), -(-m // 32), -(-n // 32), -(-m // 128)
            # H side: the masked plan, but never fewer than four row chunks (a whole workgroup of waves)
            rpc = max(1, -(-nrowblk // min(max(4, 1024 // ncolblk), 64)))
            assert (out[3], out[4], out[5]) == (rpc, -(-nrowblk // rpc), nrowblk), (m, n, k)
            if ncolblk <= 256:
                assert list(out)[3:6] == list(six)[3:], (m, n, k)
            # W side: the masked plan with ONE part of the output columns at KP = 128 (S formed once), hence twice the column splits
            tps = -(-tiles // min(max(1, 512 // rowtiles), tiles, 32))
            assert (out[0], out[1], out[2]) == (tps, -(-n // (32 * tps)), 1), (m, n, k)
            if kp <= 64:
                assert list(out)[:3] == list(six)[:3], (m, n, k)
            else:
                assert six[2] == 2
            assert out[6] == lib.dnmf_masked_reduce_grid(m, k) >= 1 and out[7] == lib.dnmf_masked_reduce_grid(k, n) >= 1
    assert lib.dnmf_is_plan(32768, 16384, 128, out) == 0 and list(out)[:5] == [256, 2, 1, 256, 4]       # (the masked plan: 512, 1, 2, 512, 2)


def test_workspace_queries():
    from pydnmfk_amd._lib import lib
    for q in (lib.dnmf_is_ws_bytes, lib.dnmf_is_ws_bytes_fit):
        for bad in ((0, 10, 4), (10, 0, 4), (-1, 10, 4), (10, -1, 4), (10, 10, 0), (10, 10, 129), (10, 10, -1)):
            assert q(*bad) == 0, bad
    for m, n in LOOP_SHAPES + ONE_TRIP_SHAPES:
        for k in KS:
            step = _align256(max(_slabs(m, n, k)))
            assert lib.dnmf_is_ws_bytes(m, n, k) == step >= 256, (m, n, k)
            # the whole fit: the step's slabs, 1024 partial rows of the column sums, the sums, the two squared norms
            kp = _kp(k)
            assert lib.dnmf_is_ws_bytes_fit(m, n, k) == step + _align256(1024 * kp * 4) + _align256(kp * 4) + 256, (m, n, k)


@pytest.mark.parametrize("case", I.EXACT_LOOP_CASES, ids=lambda c: "%dx%d" % c["shape"])
def test_loop_shapes_reach_what_their_table_entry_says(case):
    m, n = case["shape"]
    assert case["reach"] and (n % 4 == 0) == case["fast"]                # (the vector kernels need whole 16-byte rows of A and H)
    for k in case["ks"]:
        p = _plan(m, n, k)
        for what, want in case["reach"].items():
            assert p[what] == want, "%dx%d k=%d: %s is %d, the table says %d (plan %s)" % (m, n, k, what, p[what], want, p)
    r = case["reach"]
    if "tiles_per_split" in r:                   # more than one tile per workgroup, the last one ragged and not the first
        assert r["tiles_per_split"] >= 2 and r["last_split_tiles"] >= 2 and r["last_tile_cols"] < 32
    if "rowblks_per_chunk" in r:                 # more than one row block per wave, the last one short of rows
        assert r["rowblks_per_chunk"] >= 2 and r["last_blk_rows"] < 32


def test_loop_shapes_between_them_reach_every_loop():
    reach = [c["reach"] for c in I.EXACT_LOOP_CASES]
    for fast in (False, True):
        mine = [c["reach"] for c in I.EXACT_LOOP_CASES if c["fast"] == fast]
        assert any("tiles_per_split" in r for r in mine) and any("rowblks_per_chunk" in r for r in mine), fast   # both sides, both variants
    assert any(r["last_chunk_blks"] < r["rowblks_per_chunk"] for r in reach if "rowblks_per_chunk" in r)
    assert any(r.get("w_reduce_trips", 1) >= 2 for r in reach)


@pytest.mark.parametrize("shape", ONE_TRIP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_other_shapes_stay_at_one_trip_of_each_loop(shape):
    m, n = shape
    for k in KS:
        p = _plan(m, n, k)
        assert p["tiles_per_split"] == 1 and p["rowblks_per_chunk"] == 1 and p["w_reduce_trips"] == 1 and p["h_reduce_trips"] == 1, (shape, k, p)


def _calls(m=70, n=2085, k=32):
    """{entry point: (name in dnmf_last_error, ordered good arguments)}"""
    head = dict(A=P16, m=m, n=n, lda=n, W=P16, ldw=k, H=P16, ldh=n, k=k, eps=1e-7)
    tail = dict(ws=P16, ws_bytes=1 << 40, stream=None)
    return {
        "dnmf_is_aht_pair": ("is_aht_pair", dict(head, num=P16, den=P16, ldo=k, **tail)),
        "dnmf_is_wta_pair": ("is_wta_pair", dict(head, num=P16, den=P16, ldo=n, **tail)),
        "dnmf_is_update_w": ("is_update_w", dict(head, **tail)),
        "dnmf_is_update_h": ("is_update_h", dict(head, clamp=0, **tail)),
        "dnmf_is_divergence": ("is_divergence", dict(head, out=P16, **tail)),
        "dnmf_is_mu_fit": ("is_mu_fit", dict(head, w_update=1, itr=3, sq_out=P16, **tail)),
    }


def test_argument_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    m, n, k = 70, 2085, 32
    w_slab, h_slab, d_slab = _slabs(m, n, k)
    need_of = {"dnmf_is_aht_pair": w_slab, "dnmf_is_update_w": w_slab, "dnmf_is_wta_pair": h_slab, "dnmf_is_update_h": h_slab,
               "dnmf_is_divergence": d_slab, "dnmf_is_mu_fit": lib.dnmf_is_ws_bytes_fit(m, n, k)}
    for fn, (who, good) in _calls(m, n, k).items():
        for a in ("A", "W", "H", "num", "den", "out", "sq_out"):                 # null operands and outputs
            if a in good:
                _refused(lib, fn, who, good, **{a: None})
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
        if "itr" in good:
            _refused(lib, fn, who, good, itr=-1)
        need = need_of[fn]                                                       # workspace: one byte short, null, misaligned
        _refused(lib, fn, who, good, rc=EWS, ws_bytes=need - 1)
        assert str(need).encode() in lib.dnmf_last_error()
        _refused(lib, fn, who, good, rc=EWS, ws=None)
        _refused(lib, fn, who, good, rc=EWS, ws=ODD)
        _refused(lib, fn, who, good, rc=EWS, ws_bytes=0)
    good = dict(X=P16, rows=8, cols=5, ldx=5, num=P16, den=P16, ldo=5, eps=1e-7, clamp=0, stream=None)
    for bad in (dict(X=None), dict(num=None), dict(den=None), dict(rows=0), dict(cols=0), dict(rows=-1), dict(ldx=4), dict(ldo=4)):
        _refused(lib, "dnmf_is_ratio_update", "is_ratio_update", good, **bad)
    assert EINVAL != 0 and EWS != 0
