"""The entry points NMFk under norm='beta' adds (csrc/dnmf_beta.hip: dnmf_beta_column_div{,_ws_bytes,_plan}, declared in
include/dnmf_beta_nmfk_api.h and bound from pydnmfk_amd._lib.BETA_NMFK_SIGNATURES) without a GPU: declared, exported and bound with
`float beta` after `eps`; every bad argument refused by the host-side checks before any launch, in the stated order -- the pointers
are made-up addresses that nothing may dereference (the pattern of tests/test_capi.py) --; the workspace query equals the masked
per-column error's pair slab, recomputed here in Python; the plan is dnmf_is_column_div_plan's."""
import ctypes
import os
import re

import pytest

from tests import _is as I
from tests import _masked_nmfk as N
from tests.test_capi import EINVAL, EWS, ODD, P16, _align256, _refused
from tests.test_capi_beta import BAD_BETAS, GOOD_BETAS, ONE_TRIP_SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 3, 32, 64, 128)
LOOP_SHAPES = tuple(c["shape"] for c in N.COLERR_LOOP_CASES)
NAMES = ("dnmf_beta_column_div_ws_bytes", "dnmf_beta_column_div_plan", "dnmf_beta_column_div")


def pair_slab(m, n):
    """plan_masked_colerr(m, n, 2) of csrc/dnmf_masked.h in Python: (rowblks_per_chunk, nchunks, ncolblk, bytes)"""
    ncolblk, nrowblk = -(-n // 128), -(-m // 32)
    want = min(max(1, 2048 // ncolblk), 256)
    rpc = max(1, -(-nrowblk // want))
    nchunks = -(-nrowblk // rpc)
    return rpc, nchunks, ncolblk, nchunks * 2 * ncolblk * 128 * 8


def test_symbols_are_declared_exported_and_bound():
    from pydnmfk_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dnmf_beta_nmfk_api.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(dnmf_[a-z0-9_]+)\s*\(", txt))) == sorted(NAMES)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dnmf.h")).read(), flags=re.S)
    assert '#include "dnmf_beta_nmfk_api.h"' in core and core.index('"dnmf_beta_api.h"') < core.index('"dnmf_beta_nmfk_api.h"')
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert sorted(_lib.BETA_NMFK_SIGNATURES) == sorted(NAMES)
    assert not set(_lib.BETA_NMFK_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.BETA_SIGNATURES))
    for name in NAMES:
        assert hasattr(raw, name) and callable(getattr(_lib.lib, name)), name
        assert getattr(_lib.lib, name).argtypes == _lib.BETA_NMFK_SIGNATURES[name], name
    assert _lib.lib.dnmf_beta_column_div_ws_bytes.restype is ctypes.c_size_t
    sig = _lib.BETA_NMFK_SIGNATURES["dnmf_beta_column_div"]
    # A m n lda W ldw H ldh k eps beta div pw ws ws_bytes stream
    assert len(sig) == 16 and sig[9] is ctypes.c_float and sig[10] is ctypes.c_float and sig[8] is ctypes.c_int
    assert sig[11] is ctypes.c_void_p and sig[12] is ctypes.c_void_p and sig[13] is ctypes.c_void_p and sig[14] is ctypes.c_size_t
    decl = re.search(r"int dnmf_beta_column_div\((.*?)\);", txt, flags=re.S).group(1)
    assert re.search(r"float eps,\s*float beta,\s*double\* div,\s*double\* pw,\s*void\* ws,\s*size_t ws_bytes", decl), decl


def test_plan_is_the_itakura_saito_per_column_plan():
    from pydnmfk_amd._lib import lib
    out, ref = (ctypes.c_long * 3)(*([-7] * 3)), (ctypes.c_long * 3)(*([-9] * 3))
    for m, n in LOOP_SHAPES + ONE_TRIP_SHAPES + ((40000, 17), (5, 40000), (32768, 16384)):
        for k in KS:
            assert lib.dnmf_beta_column_div_plan(m, n, k, out) == 0 and lib.dnmf_is_column_div_plan(m, n, k, ref) == 0
            assert list(out) == list(ref) == list(pair_slab(m, n)[:3]), (m, n, k)
    for case in N.COLERR_LOOP_CASES:
        m, n = case["shape"]
        assert lib.dnmf_beta_column_div_plan(m, n, 32, out) == 0
        p = N.colerr_reach(m, n, out)
        for what, want in case["reach"].items():
            assert p[what] == want, (case["shape"], what, p)


def test_plan_refusals():
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_long * 3)()
    good = dict(m=130, n=133, k=32, out=ctypes.addressof(out))
    for bad in (dict(k=0), dict(k=129), dict(k=-1), dict(m=0), dict(n=0), dict(m=-3), dict(out=None)):
        _refused(lib, "dnmf_beta_column_div_plan", "beta_column_div_plan", good, **bad)
    _refused(lib, "dnmf_beta_column_div_plan", "beta_column_div_plan", good, k=129)
    assert b"beta-divergence kernels" in lib.dnmf_last_error()                     # the wording of the other dnmf_beta_* entry points


def test_workspace_query_is_the_masked_pair_slab():
    from pydnmfk_amd._lib import lib
    q = lib.dnmf_beta_column_div_ws_bytes
    for bad in ((0, 10, 4), (10, 0, 4), (-1, 10, 4), (10, -1, 4), (10, 10, 0), (10, 10, 129), (10, 10, -1)):
        assert q(*bad) == 0, bad
    for m, n in ONE_TRIP_SHAPES + LOOP_SHAPES:
        for k in KS:
            assert q(m, n, k) == _align256(pair_slab(m, n)[3]) >= 256, (m, n, k)
            assert q(m, n, k) == lib.dnmf_masked_column_err_ws_bytes(m, n, k), (m, n, k)                # the plan as it is
            assert _align256(pair_slab(m, n)[3] // 2) == lib.dnmf_is_column_div_ws_bytes(m, n, k), (m, n, k)


def _good(m=8261, n=133, k=32, beta=0.5):
    return dict(A=P16, m=m, n=n, lda=n, W=P16, ldw=k, H=P16, ldh=n, k=k, eps=1e-7, beta=beta, div=P16, pw=P16, ws=P16, ws_bytes=1 << 40,
                stream=None)


def test_a_misaligned_workspace_is_refused_before_anything_else():
    """the loop of tests/test_beta_workspace_cpu.py over this table: a pointer nothing may dereference and 8 for every integer, so a
    refusal that came later would be another one, or a fault; then with every other argument bad as well"""
    from pydnmfk_amd import _lib
    lib = _lib.lib
    ws_taking = [name for name, args in _lib.BETA_NMFK_SIGNATURES.items()
                 if any(args[i] is ctypes.c_void_p and args[i + 1] is ctypes.c_size_t for i in range(len(args) - 1))]
    assert ws_taking == ["dnmf_beta_column_div"]
    for name in ws_taking:
        args = _lib.BETA_NMFK_SIGNATURES[name]
        at = next(i for i in range(len(args) - 1) if args[i] is ctypes.c_void_p and args[i + 1] is ctypes.c_size_t)
        call = [P16 if a is ctypes.c_void_p else 1 << 20 if a is ctypes.c_size_t else 1e-7 if a in (ctypes.c_float, ctypes.c_double) else 8
                for a in args]
        for odd in (ODD, P16 + 8, P16 + 1):
            call[at] = odd
            rc = getattr(lib, name)(*call)
            err = lib.dnmf_last_error()
            assert rc == EWS and b"16-byte boundary" in err, "%s with ws at %#x returned %d (%r)" % (name, odd, rc, err)
    for other in (dict(beta=7.5), dict(beta=float("nan")), dict(k=129), dict(A=None), dict(m=0), dict(ws_bytes=0)):
        _refused(lib, "dnmf_beta_column_div", "beta_column_div", _good(), rc=EWS, **dict(other, ws=ODD))
        assert b"16-byte boundary" in lib.dnmf_last_error(), other


def test_beta_out_of_range_is_refused_next():
    from pydnmfk_amd._lib import lib
    fn, who = "dnmf_beta_column_div", "beta_column_div"
    for beta in BAD_BETAS:
        for other in ({}, dict(k=129), dict(A=None), dict(div=None), dict(n=0), dict(ws_bytes=0), dict(ws=None)):
            _refused(lib, fn, who, _good(), **dict(other, beta=beta))
            assert b"outside the accepted range -2 <= beta <= 4" in lib.dnmf_last_error(), (beta, other)
    for beta in GOOD_BETAS:                                       # inside the range the next check speaks
        _refused(lib, fn, who, _good(beta=beta), k=129)
        assert b"rank k=129" in lib.dnmf_last_error(), beta


def test_then_pointers_and_shapes_then_a_short_workspace():
    from pydnmfk_amd._lib import lib
    fn, who = "dnmf_beta_column_div", "beta_column_div"
    good = _good()
    m, n, k = good["m"], good["n"], good["k"]
    for a in ("A", "W", "H", "div", "pw"):
        _refused(lib, fn, who, good, **{a: None})
        _refused(lib, fn, who, good, ws_bytes=0, **{a: None})                       # (before the workspace's size)
        assert b"null pointer or bad shape" in lib.dnmf_last_error()
    for bad_k in (0, 129, -1):
        _refused(lib, fn, who, good, k=bad_k)
        assert b"beta-divergence kernels" in lib.dnmf_last_error()
    _refused(lib, fn, who, good, ldw=k - 1)
    _refused(lib, fn, who, good, ldh=n - 1)
    _refused(lib, fn, who, good, lda=n - 1)
    for a in ("m", "n"):
        for v in (0, -3):
            _refused(lib, fn, who, good, **{a: v})
    need = pair_slab(m, n)[3]
    _refused(lib, fn, who, good, rc=EWS, ws_bytes=need - 1)
    assert str(need).encode() in lib.dnmf_last_error()
    _refused(lib, fn, who, good, rc=EWS, ws=None)
    _refused(lib, fn, who, good, rc=EWS, ws_bytes=0)
    assert EINVAL != 0 and EWS != 0 and I.EPS > 0
