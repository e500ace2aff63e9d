"""The two entry points of NMFk on a sparse block (csrc/dnmf_csr.hip: dnmf_csr_perturb_uniform, dnmf_csr_column_err): every bad
argument is refused by the host-side checks with a non-zero code, before any launch -- the pointers are made-up addresses that
nothing may dereference (the pattern of tests/test_capi.py)."""
from tests.test_capi import EWS, ODD, P16, _align256, _refused


def _gram_chunks(rows, k):
    nt = (-(-k // 16)) ** 2
    return max(1, min(-(-rows // 512), max(8, 256 // nt)))


def _colerr_ws(cols, k, masked, nseg):
    """include/dnmf.h: the Gram partials of W and their sum (zero meaning), one float64 pair per segment"""
    gram = 0 if masked else _align256(_gram_chunks(cols, k) * k * k * 8) + _align256(k * k * 8)
    return max(256, gram + _align256(nseg * 2 * 8))


def test_column_err_workspace_query_without_gpu():
    from pydnmfk_amd._lib import lib
    q = lib.dnmf_csr_column_err_ws_bytes
    for bad in ((0, 10, 4, 0, 0), (10, 0, 4, 0, 0), (-1, 10, 4, 0, 0), (10, 10, 0, 0, 0), (10, 10, 257, 1, 0), (10, 10, 4, 0, -1)):
        assert q(*bad) == 0, bad
    for rows, cols, k, nseg in ((9, 8, 4, 0), (27, 3100, 129, 13), (70, 16389, 256, 0), (5, 100000, 17, 2)):
        for masked in (0, 1):
            assert q(rows, cols, k, masked, nseg) == _colerr_ws(cols, k, masked, nseg), (rows, cols, k, masked, nseg)


def test_perturb_uniform_argument_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    good = dict(rowptr=P16, col=P16, val=P16, rows=8, ncols=9, transposed=0, noise_var=0.03, seed=1000, val_out=P16, stream=None)
    who = "csr_perturb_uniform"
    for bad in (dict(rowptr=None), dict(val_out=None), dict(rows=0), dict(rows=-3), dict(rows=1 << 31), dict(ncols=0), dict(ncols=-1),
                dict(ncols=1 << 31), dict(transposed=1), dict(transposed=1, rows=9, ncols=8), dict(noise_var=-0.5),
                dict(noise_var=float("nan")), dict(noise_var=float("inf"))):
        _refused(lib, "dnmf_csr_perturb_uniform", who, good, **bad)


def test_column_err_argument_validation_without_gpu():
    from pydnmfk_amd._lib import lib
    fn, who = "dnmf_csr_column_err", "csr_column_err"
    for masked in (0, 1):
        good = dict(rowptr=P16, col=P16, val=P16, rows=9, cols=8, Lp=P16, Fp=P16, k=4, masked=masked, long_rows=None, long_segptr=None,
                    n_long=0, nseg=0, num=P16, den=P16, ws=P16, ws_bytes=1 << 20, stream=None)
        for a in ("rowptr", "Lp", "Fp", "num", "den"):
            _refused(lib, fn, who, good, **{a: None})
        for rows in (0, -3, 1 << 31):
            _refused(lib, fn, who, good, rows=rows)
        for cols in (0, -1, 1 << 31):
            _refused(lib, fn, who, good, cols=cols)
        for k in (0, 257, -1):
            _refused(lib, fn, who, good, k=k)
        for a in ("Lp", "Fp"):                                           # a packed image is read as float4
            _refused(lib, fn, who, good, **{a: ODD})
        long_ = dict(good, long_rows=P16, long_segptr=P16, n_long=2, nseg=5)
        _refused(lib, fn, who, long_, long_rows=None)
        _refused(lib, fn, who, long_, long_segptr=None)
        _refused(lib, fn, who, long_, nseg=1)
        _refused(lib, fn, who, long_, n_long=-1)
        _refused(lib, fn, who, good, nseg=-1)
        need = 5 * 2 * 8 if masked else _colerr_ws(8, 4, 0, 5)
        _refused(lib, fn, who, long_, rc=EWS, ws_bytes=need - 1)
        _refused(lib, fn, who, long_, rc=EWS, ws=None)
        _refused(lib, fn, who, long_, rc=EWS, ws=ODD)
        assert str(need).encode() in lib.dnmf_last_error()
        if not masked:                                                   # the Gram matrix needs its workspace without long rows too
            need = _colerr_ws(8, 4, 0, 0)
            _refused(lib, fn, who, good, rc=EWS, ws_bytes=need - 1)
            _refused(lib, fn, who, good, rc=EWS, ws=None)
