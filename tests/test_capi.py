"""The C-ABI library loads and exports every symbol include/dnmf.h declares; argument validation
works without touching a GPU (no compute calls here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "dnmf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dnmf_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported_and_bound():
    from pydnmfk_amd import _lib
    names = _declared()
    assert len(names) >= 24
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), "symbol %s declared in include/dnmf.h but not exported" % n
        assert n in _lib.SIGNATURES, "symbol %s has no ctypes signature in pydnmfk_amd/_lib.py" % n
    assert sorted(_lib.SIGNATURES) == names


def test_argument_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    assert lib.dnmf_version() >= 100
    assert [lib.dnmf_kp(k) for k in (1, 4, 32, 33, 64, 65, 128, 129, 256)] == [32, 32, 32, 64, 64, 128, 128, 256, 256]
    assert lib.dnmf_kp(0) < 0 and lib.dnmf_kp(257) < 0
    # wide ranks (128 < k <= 256): the workspace carries the m x n quotient image of the KL products; the library-sequenced grid
    # steps and the float64 path stop at the tuned kernels' rank
    assert lib.dnmf_ws_bytes(4096, 1024, 200) >= lib.dnmf_ws_bytes(4096, 1024, 128) + 4 * 4096 * 1024
    assert lib.dnmf_ws_bytes_1d(4096, 1024, 200) == 0 and lib.dnmf_f64_ws_bytes(4096, 1024, 200) == 0
    assert lib.dnmf_aht_update_w(None, 8, 8, 8, None, 200, 8, None, None, 200, 1e-7, None) == -1 and b"fused form" in lib.dnmf_last_error()
    assert lib.dnmf_ws_bytes(0, 10, 4) == 0
    assert lib.dnmf_ws_bytes(262144, 8192, 64) > 64 * 8192 * 4
    # null pointers / bad rank are rejected before any HIP call
    assert lib.dnmf_aht(None, 8, 8, 8, None, 4, 8, None, 4, None) == -1
    assert b"aht" in lib.dnmf_last_error()
    assert lib.dnmf_mu_fro_step(None, 8, 8, 8, None, 4, None, 8, 300, 1e-7, 1, 0, None, 0, None) == -1
    # the exchange entry points (csrc/dnmf_comm.hip): argument checks come before any RCCL / HIP call
    assert lib.dnmf_ws_bytes_1d(0, 10, 4) == 0
    assert lib.dnmf_ws_bytes_1d(32768, 8192, 64) >= lib.dnmf_ws_bytes(32768, 8192, 64) + 4 * (64 * 8192 + 64 * 64)
    assert lib.dnmf_comm_create(None, 2, 0, 2, 1, None) == -1 and b"comm_create" in lib.dnmf_last_error()
    assert lib.dnmf_comm_unique_id(None) == -1
    assert lib.dnmf_comm_allreduce(None, None, 4, 0, None) == -1
    assert lib.dnmf_mu_fro_step_1d(None, 8, 8, 8, None, 4, None, 8, 4, 1e-7, 1, 0, None, 0, None, None) == -1
    assert lib.dnmf_mu_kl_step_1d(None, 8, 8, 8, None, 4, None, 8, 4, 1e-7, 1, 0, None, 0, None, None) == -1
    # 2D steps: the workspace query is host arithmetic (ragged grids included; 0 for a grid with more members than rows / columns
    # or a bad grid), null arguments are refused
    assert lib.dnmf_ws_bytes_2d(32768, 32768, 128, 4, 2) >= lib.dnmf_ws_bytes(32768, 32768, 128) + 4 * 128 * (2 * 32768 + 2 * 32768)
    assert lib.dnmf_ws_bytes_2d(1000, 1000, 8, 3, 2) > lib.dnmf_ws_bytes(1000, 1000, 8)
    assert lib.dnmf_ws_bytes_2d(2, 1000, 8, 2, 3) == 0 and lib.dnmf_ws_bytes_2d(1000, 1024, 8, 2, 0) == 0
    assert lib.dnmf_mu_fro_step_2d(None, 8, 8, 8, None, 8, 4, None, 8, 8, 4, 1e-7, 1, 0, None, 0, None, None) == -1
    assert b"mu_fro_step_2d" in lib.dnmf_last_error()
    assert lib.dnmf_mu_kl_step_2d(None, 8, 8, 8, None, 8, 4, None, 8, 8, 4, 1e-7, 1, 0, None, 0, None, None) == -1
    assert lib.dnmf_hals_fro_step_1d(None, 8, 8, 8, None, 4, None, 8, 4, 1e-7, 1, 0, 0, None, 0, None, None) == -1
    assert lib.dnmf_hals_fro_step_2d(None, 8, 8, 8, None, 8, 4, None, 8, 8, 4, 1e-7, 1, 0, None, 0, None, None) == -1
    assert lib.dnmf_hals_fro_step_1d_bf16a(None, 8, 8, 8, None, 4, None, 8, 4, 1e-7, 1, 0, 0, None, 0, None, None) == -1
    assert lib.dnmf_mu_fro_step_2d_bf16a(None, 8, 8, 8, None, 8, 4, None, 8, 8, 4, 1e-7, 1, 0, None, 0, None, None) == -1
    assert lib.dnmf_wta_gram(None, 8, 8, 8, None, 4, 4, None, 8, None, None, 0, None) == -1
    assert lib.dnmf_clock_probe(None, 4, 1, None) == -1
    # the plan query of the HALS W sweep: its refusals come before the device is asked
    plan = (ctypes.c_int * 6)()
    for bad in ((8, 4, 4, 4, 1, 1, None), (8, 0, 4, 4, 1, 1, plan), (8, 257, 300, 300, 1, 1, plan), (0, 4, 4, 4, 1, 1, plan), (8, 4, 3, 4, 1, 1, plan),
                (8, 4, 4, 3, 1, 1, plan)):
        assert lib.dnmf_hals_sweep_plan(*bad) == -1 and b"hals_sweep_plan:" in lib.dnmf_last_error(), bad
    assert lib.dnmf_hals_sweep_plan(600, 129, 129, 129, 1, 1, plan) == 0 and list(plan) == [0, 256, 3, -1, 0, 0]     # a wide rank: column launches, no device needed
    assert lib.dnmf_comm_destroy(None) == 0


# ---- the sparse (CSR) entry points (csrc/dnmf_csr.hip).  Every call below is refused by the host-side checks, before any launch: the
# pointers are made-up addresses that nothing may dereference.
P16, ODD = 0x10000, 0x10004                          # a 16-byte aligned address and one that is not
EINVAL, EWS = -1, -2


def _csr_calls():
    """{entry point: (name in dnmf_last_error, ordered good arguments)}; rows = 8, k = 4, no long rows"""
    lists = dict(long_rows=None, long_segptr=None, n_long=0, nseg=0)
    tail = dict(ws=P16, ws_bytes=1 << 20, stream=None)
    csr = dict(rowptr=P16, col=P16, val=P16, rows=8)
    return {
        "dnmf_csr_mm": ("csr_mm", dict(csr, Fp=P16, k=4, out=P16, ldo=4, out_trans=0, **lists, **tail)),
        "dnmf_csr_kl_mm": ("csr_kl_mm", dict(csr, Lp=P16, Fp=P16, k=4, eps=1e-7, out=P16, ldo=4, out_trans=0, **lists, **tail)),
        "dnmf_csr_masked_mm": ("csr_masked_mm", dict(csr, Lp=P16, Fp=P16, k=4, eps=1e-7, kl=0, num=P16, den=P16, ldo=4, out_trans=0,
                                                     **lists, **tail)),
        "dnmf_csr_masked_update": ("csr_masked_update", dict(csr, Lp=P16, Fp=P16, k=4, eps=1e-7, kl=0, clamp=0, X=P16, ldo=4, out_trans=0,
                                                             **lists, **tail)),
        "dnmf_csr_resid_sqnorm": ("csr_resid_sqnorm", dict(csr, cols=9, Wp=P16, HTp=P16, k=4, **lists, sq=P16, **tail)),
        "dnmf_csr_masked_resid_sqnorm": ("csr_masked_resid_sqnorm", dict(csr, cols=9, Wp=P16, HTp=P16, k=4, **lists, sq=P16, **tail)),
    }


def _refused(lib, fn, who, good, rc=EINVAL, **bad):
    args = dict(good, **bad)
    assert set(args) == set(good), "unknown argument in %s" % (bad,)
    got = getattr(lib, fn)(*args.values())
    err = lib.dnmf_last_error()
    assert got == rc, "%s(%s) returned %d, expected %d (%s)" % (fn, bad, got, rc, err)
    assert (who + ":").encode() in err, "%s(%s): dnmf_last_error() does not name the entry point: %r" % (fn, bad, err)


def _kpad(k):
    return next(p for p in (16, 32, 64, 128, 256) if k <= p)


def _align256(x):
    return -(-x // 256) * 256


def _resid_ws(rows, cols, k, nseg):
    """the workspace of dnmf_csr_resid_sqnorm (include/dnmf.h): float64 Gram partials of both factors, one float64 per wave and segment"""
    nt = (-(-k // 16)) ** 2
    chunks = [max(1, min(-(-r // 512), max(8, 256 // nt))) for r in (rows, cols)]
    waves = min(-(-max(rows, 1) // 4) * 4, 8192)
    return sum(_align256(c * k * k * 8) for c in chunks) + _align256((waves + nseg) * 8)


def test_csr_shape_queries_without_gpu():
    from pydnmfk_amd._lib import lib
    assert [lib.dnmf_csr_kpad(k) for k in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256)] == [16, 16, 32, 32, 64, 64, 128, 128, 256, 256]
    assert lib.dnmf_csr_kpad(0) < 0 and lib.dnmf_csr_kpad(257) < 0 and lib.dnmf_csr_kpad(-1) < 0
    assert lib.dnmf_csr_seg() == 1024
    for fn in (lib.dnmf_csr_ws_bytes, lib.dnmf_csr_masked_ws_bytes):
        for bad in ((0, 10, 4, 0), (10, 0, 4, 0), (-1, 10, 4, 0), (10, 10, 0, 0), (10, 10, 257, 0), (10, 10, 4, -1)):
            assert fn(*bad) == 0, bad
        assert fn(10, 10, 4, 0) >= 256 and fn(10, 10, 256, 3) >= 256
    # the sizes the entry points ask for are the sizes the queries give
    for rows, cols, k, nseg in ((8, 9, 4, 0), (27, 3100, 129, 13), (16389, 70, 256, 0), (100000, 5, 17, 2)):
        assert lib.dnmf_csr_ws_bytes(rows, cols, k, nseg) == max(256, _align256(nseg * _kpad(k) * 4), _resid_ws(rows, cols, k, nseg))
        waves = min(-(-max(rows, cols) // 4) * 4, 8192)
        assert lib.dnmf_csr_masked_ws_bytes(rows, cols, k, nseg) == max(256, _align256(nseg * 2 * _kpad(k) * 4), _align256((waves + nseg) * 8))


def test_csr_argument_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    calls = _csr_calls()
    for fn, (who, good) in calls.items():
        ptrs = [a for a, v in good.items() if v == P16 and a not in ("col", "val", "ws")]
        for a in ptrs:                                                   # null operands (col / val may be null: a block without entries)
            _refused(lib, fn, who, good, **{a: None})
        for rows in (0, -3, 1 << 31):
            _refused(lib, fn, who, good, rows=rows)
        for k in (0, 257, -1):
            _refused(lib, fn, who, good, k=k)
        for a in ("Fp", "Lp", "Wp", "HTp"):                              # a packed image is read as float4
            if a in good:
                _refused(lib, fn, who, good, **{a: ODD})
        if "ldo" in good:                                                # k x rows output (out_trans) or rows x k
            _refused(lib, fn, who, good, ldo=3)
            _refused(lib, fn, who, good, ldo=7, out_trans=1)
            _refused(lib, fn, who, dict(good, k=256), ldo=255)
        if "cols" in good:
            _refused(lib, fn, who, good, cols=0)
            _refused(lib, fn, who, good, cols=1 << 31)
        # long-row lists
        long_ = dict(good, long_rows=P16, long_segptr=P16, n_long=2, nseg=5)
        _refused(lib, fn, who, long_, long_rows=None)
        _refused(lib, fn, who, long_, long_segptr=None)
        _refused(lib, fn, who, long_, nseg=1)
        _refused(lib, fn, who, long_, n_long=-1)
        _refused(lib, fn, who, good, nseg=-1)
        # workspace: one byte short, null, misaligned
        need = {"dnmf_csr_mm": 5 * 16 * 4, "dnmf_csr_kl_mm": 5 * 16 * 4, "dnmf_csr_masked_mm": 5 * 2 * 16 * 4,
                "dnmf_csr_masked_update": 5 * 2 * 16 * 4, "dnmf_csr_resid_sqnorm": _resid_ws(8, 9, 4, 5),
                "dnmf_csr_masked_resid_sqnorm": (8 + 5) * 8}[fn]
        _refused(lib, fn, who, long_, rc=EWS, ws_bytes=need - 1)
        _refused(lib, fn, who, long_, rc=EWS, ws=None)
        _refused(lib, fn, who, long_, rc=EWS, ws=ODD)
        assert str(need).encode() in lib.dnmf_last_error()
    for fn in ("dnmf_csr_resid_sqnorm", "dnmf_csr_masked_resid_sqnorm"):    # the residuals need their workspace without long rows too
        who, good = calls[fn]
        need = _resid_ws(8, 9, 4, 0) if fn == "dnmf_csr_resid_sqnorm" else 8 * 8
        _refused(lib, fn, who, good, rc=EWS, ws_bytes=need - 1)
        _refused(lib, fn, who, good, rc=EWS, ws=None)


def test_csr_pack_and_ratio_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    pack = dict(X=P16, rows=8, cols=4, ldx=4, transpose=0, P=P16, stream=None)
    for bad in (dict(X=None), dict(P=None), dict(P=ODD), dict(rows=0), dict(cols=0), dict(ldx=3), dict(cols=257, ldx=257),
                dict(transpose=1, rows=257), dict(transpose=1, rows=0), dict(transpose=1, cols=1 << 31, ldx=1 << 31)):
        _refused(lib, "dnmf_csr_pack", "csr_pack", pack, **bad)
    ratio = dict(X=P16, rows=8, cols=4, ldx=4, num=P16, den=P16, ldp=4, eps=1e-7, clamp=0, stream=None)
    for bad in (dict(X=None), dict(num=None), dict(den=None), dict(rows=0), dict(cols=0), dict(ldx=3), dict(ldp=3)):
        _refused(lib, "dnmf_csr_ratio_update", "csr_ratio_update", ratio, **bad)


# ---- the alignment of `ws` (include/dnmf.h: every workspace starts on a 16-byte boundary).  The float32, bf16x6, float64, whole-fit,
# BCD, HALS and grid-step entry points refuse any other address with DNMF_EWS as the FIRST of their checks -- every other argument below
# is made up (a pointer nothing may dereference, 8 for every integer), so a refusal that came later would be another one, or a fault.
# The CSR, masked dense and Itakura-Saito entry points check the alignment together with the size: test_csr_argument_validation_without_gpu
# above, tests/test_capi_masked.py, tests/test_capi_is.py.
WS_CHECKED_WITH_THE_SIZE = ("dnmf_csr_", "dnmf_masked_", "dnmf_is_")


def test_a_misaligned_workspace_is_refused_before_anything_else_without_gpu():
    from pydnmfk_amd import _lib
    lib = _lib.lib
    seen = []
    for name, args in _lib.SIGNATURES.items():
        if name.startswith("dnmf_comm_") or name.startswith(WS_CHECKED_WITH_THE_SIZE) or name == "dnmf_dense_plan":
            continue
        at = next((i for i in range(len(args) - 1) if args[i] is ctypes.c_void_p and args[i + 1] is ctypes.c_size_t), None)
        if at is None:
            continue
        call = [P16 if a is ctypes.c_void_p else 1 << 20 if a is ctypes.c_size_t else 1e-7 if a in (ctypes.c_float, ctypes.c_double) else 8
                for a in args]
        for odd in (ODD, P16 + 8, P16 + 1):
            call[at] = odd
            rc = getattr(lib, name)(*call)
            err = lib.dnmf_last_error()
            assert rc == EWS and b"16-byte boundary" in err, "%s with ws at %#x returned %d (%r)" % (name, odd, rc, err)
        seen.append(name)
    assert len(seen) == 52, (len(seen), seen)                    # 72 launching entry points take a workspace; 20 check it with the size
