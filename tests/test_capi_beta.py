"""The entry points of the beta-divergence path (csrc/dnmf_beta.hip: dnmf_beta_*) without a GPU: every symbol is bound, every bad
argument -- a beta outside [-2, 4] among them -- is refused by the host-side checks with a non-zero code before any launch (the pointers
are made-up addresses that nothing may dereference: the pattern of tests/test_capi.py), the workspace queries equal the sizes
recomputed from the launch plan, and the plan (dnmf_beta_plan) IS the Itakura-Saito plan at every shape: the register report of the
PAIR_BETA kernels shows no scratch at JT = 4, KP = 128 (csrc/dnmf_beta.h), so nothing forced the masked plan's JT = 2."""
import ctypes

import pytest

from tests import _is as I
from tests.test_capi import EINVAL, EWS, ODD, P16, _align256, _refused

KS = (1, 3, 16, 17, 32, 33, 64, 100, 128)
LOOP_SHAPES = tuple(c["shape"] for c in I.EXACT_LOOP_CASES)
ONE_TRIP_SHAPES = ((1, 1), (7, 5), (50, 39), (200, 136), (300, 200)) + I.EXACT_SHAPES
SYMBOLS = ("dnmf_beta_ws_bytes", "dnmf_beta_ws_bytes_fit", "dnmf_beta_plan", "dnmf_beta_aht_pair", "dnmf_beta_wta_pair", "dnmf_beta_update_w",
           "dnmf_beta_update_h", "dnmf_beta_ratio_update", "dnmf_beta_divergence", "dnmf_beta_mu_fit")
BAD_BETAS = (-2.5, -2.0001, 4.0001, 7.5, float("nan"), float("inf"), float("-inf"))
GOOD_BETAS = (-2.0, -1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0)


def _plan(m, n, k, fn="dnmf_beta_plan"):
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 8)(*([-7] * 8))
    assert getattr(lib, fn)(m, n, k, out) == 0, lib.dnmf_last_error()
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
    from pydnmfk_amd._lib import BETA_SIGNATURES, SIGNATURES, lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dnmf_beta_api.h")).read()
    for name in SYMBOLS:
        assert name in BETA_SIGNATURES and callable(getattr(lib, name)) and (name + "(") in header, name
    assert lib.dnmf_beta_ws_bytes.restype is ctypes.c_size_t and lib.dnmf_beta_ws_bytes_fit.restype is ctypes.c_size_t
    # `float beta` follows `eps` in every entry point that takes eps
    for name in SYMBOLS[3:]:
        twin = SIGNATURES["dnmf_is_" + name[len("dnmf_beta_"):]]
        at = max(i for i, a in enumerate(twin) if a is ctypes.c_float) + 1
        assert BETA_SIGNATURES[name] == twin[:at] + [ctypes.c_float] + twin[at:], name
        proto = header.split(name + "(")[1].split(")")[0]
        assert "float eps" in proto and proto.split("float eps")[1].lstrip(", \n").startswith("float beta"), (name, proto)


def test_beta_plan_is_the_itakura_saito_plan_and_refuses_bad_arguments():
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 8)()
    good = dict(m=70, n=2085, k=32, out=ctypes.addressof(out))
    for bad in (dict(k=0), dict(k=129), dict(k=-1), dict(m=0), dict(n=0), dict(m=-3), dict(out=None)):
        _refused(lib, "dnmf_beta_plan", "beta_plan", good, **bad)
    ref = (ctypes.c_long * 8)()
    for m, n in LOOP_SHAPES + ONE_TRIP_SHAPES + ((40000, 17), (5, 40000), (32768, 16384)):
        for k in KS:
            assert lib.dnmf_beta_plan(m, n, k, out) == 0 and lib.dnmf_is_plan(m, n, k, ref) == 0
            assert list(out) == list(ref), (m, n, k)
            assert out[2] == 1                                           # one part of the output columns at every KP: JT = KT
    assert lib.dnmf_beta_plan(32768, 16384, 128, out) == 0 and list(out)[:5] == [256, 2, 1, 256, 4]


def test_workspace_queries():
    from pydnmfk_amd._lib import lib
    for q in (lib.dnmf_beta_ws_bytes, lib.dnmf_beta_ws_bytes_fit):
        for bad in ((0, 10, 4), (10, 0, 4), (-1, 10, 4), (10, -1, 4), (10, 10, 0), (10, 10, 129), (10, 10, -1)):
            assert q(*bad) == 0, bad
    for m, n in LOOP_SHAPES + ONE_TRIP_SHAPES:
        for k in KS:
            step = _align256(max(_slabs(m, n, k)))
            assert lib.dnmf_beta_ws_bytes(m, n, k) == step >= 256, (m, n, k)
            assert step == lib.dnmf_is_ws_bytes(m, n, k)
            # the whole fit: the step's slabs, 1024 partial rows of the column sums, the sums, the two squared norms
            kp = _kp(k)
            assert lib.dnmf_beta_ws_bytes_fit(m, n, k) == step + _align256(1024 * kp * 4) + _align256(kp * 4) + 256, (m, n, k)


@pytest.mark.parametrize("case", I.EXACT_LOOP_CASES, ids=lambda c: "%dx%d" % c["shape"])
def test_loop_shapes_reach_what_their_table_entry_says(case):
    """the shapes of tests/test_gpu_beta.py's exact test reach, under dnmf_beta_plan, the ragged last tile, the short last chunk, both
    FAST variants and the ending's second grid-stride trip (the table of tests/_is.py)"""
    m, n = case["shape"]
    assert case["reach"] and (n % 4 == 0) == case["fast"]
    for k in case["ks"]:
        p = _plan(m, n, k)
        for what, want in case["reach"].items():
            assert p[what] == want, "%dx%d k=%d: %s is %d, the table says %d (plan %s)" % (m, n, k, what, p[what], want, p)


@pytest.mark.parametrize("shape", ONE_TRIP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_other_shapes_stay_at_one_trip_of_each_loop(shape):
    m, n = shape
    for k in KS:
        p = _plan(m, n, k)
        assert p["tiles_per_split"] == 1 and p["rowblks_per_chunk"] == 1 and p["w_reduce_trips"] == 1 and p["h_reduce_trips"] == 1, (shape, k, p)


def _calls(m=70, n=2085, k=32, beta=0.5):
    """{entry point: (name in dnmf_last_error, ordered good arguments)}"""
    head = dict(A=P16, m=m, n=n, lda=n, W=P16, ldw=k, H=P16, ldh=n, k=k, eps=1e-7, beta=beta)
    tail = dict(ws=P16, ws_bytes=1 << 40, stream=None)
    return {
        "dnmf_beta_aht_pair": ("beta_aht_pair", dict(head, num=P16, den=P16, ldo=k, **tail)),
        "dnmf_beta_wta_pair": ("beta_wta_pair", dict(head, num=P16, den=P16, ldo=n, **tail)),
        "dnmf_beta_update_w": ("beta_update_w", dict(head, **tail)),
        "dnmf_beta_update_h": ("beta_update_h", dict(head, clamp=0, **tail)),
        "dnmf_beta_divergence": ("beta_divergence", dict(head, out=P16, **tail)),
        "dnmf_beta_mu_fit": ("beta_mu_fit", dict(head, w_update=1, itr=3, sq_out=P16, **tail)),
    }


def test_argument_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    m, n, k = 70, 2085, 32
    w_slab, h_slab, d_slab = _slabs(m, n, k)
    need_of = {"dnmf_beta_aht_pair": w_slab, "dnmf_beta_update_w": w_slab, "dnmf_beta_wta_pair": h_slab, "dnmf_beta_update_h": h_slab,
               "dnmf_beta_divergence": d_slab, "dnmf_beta_mu_fit": lib.dnmf_beta_ws_bytes_fit(m, n, k)}
    for fn, (who, good) in _calls(m, n, k).items():
        for beta in BAD_BETAS:                                                   # beta outside [-2, 4]: the argument error, naming the range
            _refused(lib, fn, who, good, beta=beta)
            assert b"-2 <= beta <= 4" in lib.dnmf_last_error(), (fn, beta)
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
        for beta in GOOD_BETAS:                                                  # (an accepted beta gets as far as the workspace check)
            _refused(lib, fn, who, dict(good, beta=beta), rc=EWS, ws_bytes=need - 1)
            assert str(need).encode() in lib.dnmf_last_error()
        _refused(lib, fn, who, good, rc=EWS, ws=None)
        _refused(lib, fn, who, good, rc=EWS, ws=ODD)
        _refused(lib, fn, who, good, rc=EWS, ws_bytes=0)
    good = dict(X=P16, rows=8, cols=5, ldx=5, num=P16, den=P16, ldo=5, eps=1e-7, beta=0.5, clamp=0, stream=None)
    for bad in (dict(X=None), dict(num=None), dict(den=None), dict(rows=0), dict(cols=0), dict(rows=-1), dict(ldx=4), dict(ldo=4)):
        _refused(lib, "dnmf_beta_ratio_update", "beta_ratio_update", good, **bad)
    for beta in BAD_BETAS:
        _refused(lib, "dnmf_beta_ratio_update", "beta_ratio_update", good, beta=beta)
        assert b"-2 <= beta <= 4" in lib.dnmf_last_error()
    assert EINVAL != 0 and EWS != 0
