"""The float64 kernels (csrc/dnmf_f64.hip, dnmf_f64_kl.h, dnmf_f64_tiny.hip) against the exact answer, element by element, on every
variant the dispatch can launch.  The shapes are the table of tests/_exact.py (F64_*): each case is named after the kernel variant it
reaches and asserts through dnmf_f64_plan, before it launches, that it does reach it; tests/test_f64_plan.py proves without a GPU that
the table covers every launchable instantiation and both sides of every host branch.

Every operand is a `Poisoned` view (NaN in the pitch padding, before the view and in a guard band after it), every output a view in a
sentinel-filled buffer, aligned (16-byte start, even pitch) and unaligned (8 bytes off, pitch cols + 3): the kernels load and store through
buffer descriptors with `nvalid` lane masks and out-of-range offsets, where a mask off by one reads padding (NaN) or drops a store (a
sentinel stays).  The reference is numpy float64 of the same operation on integer or dyadic operands, exact in every summation order
(tests/test_exact_cpu.py proves it for these shapes).

Ulp bounds per element, from the table at the top of tests/test_gpu_exact.py, in float64 spacing: products, Grams, sums, sqdiff, kl_quot and
the fused KL products equal (c = 0); MU updates c = 3; KL element-wise updates c = 2; scale_cols_div c = 1; scale_rows_mul by powers of
two and clamp_min exact; a fit with itr = 1 c = 6 through `_assert_normalized`.  Quotient references are formed in long double and
rounded once.

Not covered: pitches beyond the 2 GiB descriptor window (buf_ok false -- the `rt >>= 1` fallbacks and the refusals of the entry points):
they need operands of hundreds of GB.  The HALS float64 sweeps are held in tests/test_gpu_exact_hals.py."""
import functools

import numpy as np
import pytest

from tests import _exact as ex
from tests.test_gpu_exact import _assert_normalized, _outside_untouched

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E64 = 2.220446049250313e-16
D = torch.float64
ALIGN = (True, False)


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pydnmfk_amd import _lib, engine
    return engine, _lib


def _frozen(arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=8)
def _products(m, n, k):
    """ex.products in float64 with its exact answers: A, W, H, A H^T, W^T A, H H^T, W^T W (computed once per shape, read-only)"""
    A, W, H = ex.products(m, n, k, np.float64)
    return _frozen((A, W, H, A @ H.T, W.T @ A, H @ H.T, W.T @ W))


@functools.lru_cache(maxsize=8)
def _kl(m, n, k):
    """ex.kl in float64 with its exact answers: A, W, H, U, U H^T, W^T U"""
    A, W, H, U = ex.kl(m, n, k, np.float64)
    return _frozen((A, W, H, U, U @ H.T, W.T @ U))


def _P(x, aligned=True, ld=None):
    return ex.Poisoned(torch, np.array(x, dtype=np.float64), aligned=aligned, ld=ld)      # (a copy: the shared references are read-only)


def _out(rows, cols, aligned=True):
    return ex.Poisoned.out(torch, rows, cols, D, aligned)


def _vec(n, aligned=True):
    """a length-n output vector inside a sentinel-filled buffer"""
    o = _out(1, n, aligned)
    return o, o.view[0]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _quot(num, den):
    """num / den where den > 0, else 0: long double, rounded once to float64"""
    pos = den > 0
    return np.where(pos, (np.asarray(num, np.longdouble) / np.where(pos, den, 1).astype(np.longdouble)).astype(np.float64), 0.0)


def _reaches(lib_mod, op, m, n, k, ld, **want):
    p = lib_mod.f64_plan(op, m, n, k, ld)
    got = {f: p[f] for f in want}
    assert got == {f: v if isinstance(v, str) else int(v) for f, v in want.items()}, "%s %dx%d k=%d does not reach its variant: %s" % (op, m, n, k, p)
    return p


def _flag(name, on):
    return name if on else "no" + name


# ------------------------------------------------------------------------------------------------------------- aht, gram_hht
def _id_aht(c):
    m, n, k, rt, nt, vec, splits, v = c
    return "nt_kernel-RT%d-NT%d-%s-%dx%d-k%d%s" % (rt, nt, _flag("vec", vec), m, n, k, "-splits%d-V%d" % (splits, v) if splits > 1 else "")


@pytest.mark.parametrize("case", ex.F64_AHT, ids=_id_aht)
def test_aht_and_gram_hht(env, case):
    engine, L = env
    ops = engine.HIP_OPS_F64
    m, n, k, rt, nt, vec, splits, v = case
    A, W, H, AH, WtA, G, GW = _products(m, n, k)
    for aligned in ALIGN:
        Av, Hv = _P(A, aligned), _P(H, aligned)
        _reaches(L, "aht", m, n, k, [Av.ld, Hv.ld], family="nt", rt=rt, nt=nt, vec=vec, count=splits, v=v)
        o = _out(m, k, aligned)
        ops.aht(Av.view, Hv.view, o.view)
        ex.assert_ulp(o.check("aht"), AH, 0, "f64 aht aligned=%s" % aligned, tile=(16 * rt, 16))
        _reaches(L, "aht", k, n, k, [Hv.ld, Hv.ld], family="nt", rt=1, nt=nt, vec=vec, count=splits)
        o = _out(k, k, aligned)
        ops.gram_hht(Hv.view, o.view)
        ex.assert_ulp(o.check("gram_hht"), G, 0, "f64 gram_hht aligned=%s" % aligned)
        Av.check("A"); Hv.check("H")


# ------------------------------------------------------------------------------------------------------------- wta, gram_wtw
def _id_wta(c):
    m, n, k, nt, ct, vec, chunks, rpc, v = c
    return "tn_kernel-NT%d-%s-%dx%d-k%d-chunks%dx%d-V%d" % (nt, _flag("vec", vec), m, n, k, chunks, rpc, v)


@pytest.mark.parametrize("case", ex.F64_WTA, ids=_id_wta)
def test_wta_and_gram_wtw(env, case):
    engine, L = env
    ops = engine.HIP_OPS_F64
    m, n, k, nt, ct, vec, chunks, rpc, v = case
    A, W, H, AH, WtA, G, GW = _products(m, n, k)
    for aligned in ALIGN:
        Av, Wv = _P(A, aligned), _P(W, aligned)
        _reaches(L, "wta", m, n, k, [Av.ld, Wv.ld], family="tn", nt=nt, rt=ct, vec=vec, count=chunks, per=rpc, v=v)
        o = _out(k, n, aligned)
        ops.wta(Av.view, Wv.view, o.view)
        ex.assert_ulp(o.check("wta"), WtA, 0, "f64 wta aligned=%s" % aligned, tile=(16, 16 * ct))
        _reaches(L, "wta", m, k, k, [Wv.ld, Wv.ld], family="tn", nt=nt, rt=ct, count=chunks)
        o = _out(k, k, aligned)
        ops.gram_wtw(Wv.view, o.view)
        ex.assert_ulp(o.check("gram_wtw"), GW, 0, "f64 gram_wtw aligned=%s" % aligned)
        Av.check("A"); Wv.check("W")


# ------------------------------------------------------------------------------------------------------------- the fused KL products
def _id_uht(c):
    m, n, k, nt, rt, vec, full, splits, v = c
    return "kl_uht_kernel-NT%d-RT%d-%s-%s-%dx%d-k%d%s" % (nt, rt, _flag("vec", vec), _flag("full", full), m, n, k,
                                                         "-splits%d-V%d" % (splits, v) if splits > 1 else "")


@pytest.mark.parametrize("case", ex.F64_KL_UHT, ids=_id_uht)
def test_kl_uht(env, case):
    engine, L = env
    ops = engine.HIP_OPS_F64
    m, n, k, nt, rt, vec, full, splits, v = case
    A, W, H, U, UHt, WtU = _kl(m, n, k)
    for aligned in ALIGN:
        Av, Wv, Hv = _P(A, aligned), _P(W, aligned), _P(H, aligned)
        _reaches(L, "kl_uht", m, n, k, [Av.ld, Wv.ld, Hv.ld], family="kl_uht", nt=nt, rt=rt, vec=vec, full=full, count=splits, v=v)
        o = _out(m, k, aligned)
        ops.kl_uht(Av.view, Wv.view, Hv.view, E64, o.view)
        ex.assert_ulp(o.check("kl_uht"), UHt, 0, "f64 kl_uht aligned=%s" % aligned, tile=(16 * rt, 16))
        Av.check("A"); Wv.check("W"); Hv.check("H")


def _id_uht_big(c):
    m, n, k, nt, rt, splits, v = c
    return "kl_uht_kernel-NT%d-RT%d-vec-full-%dx%d-k%d-splits%d-V%d" % (nt, rt, m, n, k, splits, v)


@pytest.mark.parametrize("case", ex.F64_KL_UHT_BIG, ids=_id_uht_big)
def test_kl_uht_row_tiles_with_a_column_split(env, case):
    """RT = 2 and RT = 4 together with two column splits (m = 32768 and 65536 at n = 1024 -- the branch 65536 x 4096 takes): A of 0.27 and
    0.5 GB built on the device in a NaN-filled strided buffer, one product, the reference from torch float64 on the device (W has one
    power of two per row and H holds powers of two: W H is a single term, U = A / (W H) is A times a power of two, and U H^T sums
    multiples of 2^-4 below 2^15 -- exact in any order)"""
    engine, L = env
    ops = engine.HIP_OPS_F64
    m, n, k, nt, rt, splits, v = case
    lead, ld, guard = 8, n + 4, 67
    _reaches(L, "kl_uht", m, n, k, [ld, k + 4, n + 4], family="kl_uht", nt=nt, rt=rt, vec=True, full=True, count=splits, v=v)
    g = torch.Generator(device="cuda").manual_seed(m + k)
    buf = torch.full((lead + m * ld + guard,), float("nan"), dtype=D, device="cuda")
    try:
        A = buf.as_strided((m, n), (ld, 1), lead)
        A.copy_(torch.randint(0, 8, (m, n), device="cuda", generator=g, dtype=torch.int32))
        Wd = torch.zeros(m, k, dtype=D, device="cuda")
        Wd[torch.arange(m, device="cuda"), torch.randint(0, k, (m,), device="cuda", generator=g)] = \
            (2.0 ** torch.randint(0, 3, (m,), device="cuda", generator=g)).double()
        Hd = (2.0 ** torch.randint(1, 4, (k, n), device="cuda", generator=g)).double()
        wb = torch.full((lead + m * (k + 4) + guard,), float("nan"), dtype=D, device="cuda")
        hb = torch.full((lead + k * (n + 4) + guard,), float("nan"), dtype=D, device="cuda")
        Wv, Hv = wb.as_strided((m, k), (k + 4, 1), lead), hb.as_strided((k, n), (n + 4, 1), lead)
        Wv.copy_(Wd); Hv.copy_(Hd)
        ob = torch.full((lead + m * (k + 4) + guard,), ex.SENTINEL, dtype=D, device="cuda")
        out = ob.as_strided((m, k), (k + 4, 1), lead)
        ops.kl_uht(A, Wv, Hv, E64, out)
        _outside_untouched(ob, lead, k + 4, m, k, ex.SENTINEL, "kl_uht output")
        ref = (A / (Wd @ Hd)) @ Hd.T
        assert torch.equal(out, ref), "kl_uht: first bad row %d" % int((out != ref).any(1).nonzero()[0])
        _outside_untouched(buf, lead, ld, m, n, float("nan"), "A")
    finally:
        del buf
        torch.cuda.empty_cache()


def _id_wtu(c):
    m, n, k, nt, ct, vec, chunks, v = c
    return "kl_wtu_kernel-NT%d-CT%d-%s-%dx%d-k%d-chunks%d-V%d" % (nt, ct, _flag("vec", vec), m, n, k, chunks, v)


@pytest.mark.parametrize("case", ex.F64_KL_WTU, ids=_id_wtu)
def test_kl_wtu(env, case):
    engine, L = env
    ops = engine.HIP_OPS_F64
    m, n, k, nt, ct, vec, chunks, v = case
    A, W, H, U, UHt, WtU = _kl(m, n, k)
    for aligned in ALIGN:
        Av, Wv, Hv = _P(A, aligned), _P(W, aligned), _P(H, aligned)
        _reaches(L, "kl_wtu", m, n, k, [Av.ld, Wv.ld, Hv.ld], family="kl_wtu", nt=nt, rt=ct, vec=vec, count=chunks, v=v)
        o = _out(k, n, aligned)
        ops.kl_wtu(Av.view, Wv.view, Hv.view, E64, o.view)
        ex.assert_ulp(o.check("kl_wtu"), WtU, 0, "f64 kl_wtu aligned=%s" % aligned, tile=(16, 16 * ct))
        Av.check("A"); Wv.check("W"); Hv.check("H")


# ------------------------------------------------------------------------------------------------------------- the two images
def _id_img(c):
    m, n, k, ks, ct, vec, chunks = c
    return "nn_cols_kernel-KS%d-%s-%dx%d-k%d-chunks%d" % (ks, _flag("vec", vec), m, n, k, chunks)


def _image(engine, L, fn, Av, Wv, Hv, k, o, eps=None):
    """dnmf_f64_kl_quot / dnmf_f64_sqdiff straight into a sentinel-filled view"""
    m, n = Av.view.shape
    args = [Av.view.data_ptr(), m, n, Av.ld, Wv.view.data_ptr(), Wv.ld, Hv.view.data_ptr(), Hv.ld, k]
    args += [eps] if eps is not None else []
    L.check(fn(*args, o.view.data_ptr(), o.ld, engine._stream()))


@pytest.mark.parametrize("case", [c for c in ex.F64_IMAGE if c[0] < 10000], ids=_id_img)
def test_kl_quot(env, case):
    """dnmf_f64_kl_quot (f64_nn_cols_kernel<KS, NN_QUOT, VEC>) equals U; at k > 64 the KL products go through it and then the NT / TN forms"""
    engine, L = env
    ops = engine.HIP_OPS_F64
    m, n, k, ks, ct, vec, chunks = case
    A, W, H, U, UHt, WtU = _kl(m, n, k)
    for aligned in ALIGN:
        Av, Wv, Hv = _P(A, aligned), _P(W, aligned), _P(H, aligned)
        o = _out(m, n, aligned)
        _reaches(L, "kl_quot", m, n, k, [Av.ld, Wv.ld, Hv.ld, o.ld], family="nn_cols", nt=ks, rt=ct, vec=vec, count=chunks)
        _image(engine, L, L.lib.dnmf_f64_kl_quot, Av, Wv, Hv, k, o, E64)
        ex.assert_ulp(o.check("kl_quot"), U, 0, "f64 kl_quot aligned=%s" % aligned, tile=(16, 16 * ct))
        if k > 64:
            for op, shape, ref in (("kl_uht", (m, k), UHt), ("kl_wtu", (k, n), WtU)):
                _reaches(L, op, m, n, k, [Av.ld, Wv.ld, Hv.ld], family="image")
                s = _out(*shape, aligned)
                getattr(ops, op)(Av.view, Wv.view, Hv.view, E64, s.view)
                ex.assert_ulp(s.check(op), ref, 0, "f64 %s through the image, aligned=%s" % (op, aligned))
        Av.check("A"); Wv.check("W"); Hv.check("H")


@pytest.mark.parametrize("case", ex.F64_IMAGE, ids=_id_img)
def test_sqdiff_and_error_sums(env, case):
    """A = W H + (0..2): the squared-residual image, its sum (resid_sqnorm) and its column sums (column_err_sums) are small integers.
    m = 40: one row chunk of f64_colsum_partial_kernel; 130: three; 16400 x 132: 257, and nine trips of the sums' grid-stride loops"""
    engine, L = env
    ops = engine.HIP_OPS_F64
    m, n, k, ks, ct, vec, chunks = case
    _, W, H = _products(m, n, k)[:3]
    R = np.random.RandomState(m + k).randint(0, 3, size=(m, n)).astype(np.float64)
    A2 = W @ H + R
    assert L.f64_plan("colsum", m, n, 1)["count"] == {40: 1, 130: 3, 16400: 257}[m]
    assert (-(-m * n // (256 * L.f64_plan("sum", m, n, 1)["grid_x"])) > 8) == (m == 16400)
    for aligned in ALIGN if m < 10000 else (False,):
        Av, Wv, Hv = _P(A2, aligned), _P(W, aligned), _P(H, aligned)
        o = _out(m, n, aligned)
        _reaches(L, "sqdiff", m, n, k, [Av.ld, Wv.ld, Hv.ld, o.ld], family="nn_cols", nt=ks, rt=ct, vec=vec, count=chunks)
        _image(engine, L, L.lib.dnmf_f64_sqdiff, Av, Wv, Hv, k, o)
        ex.assert_ulp(o.check("sqdiff"), R ** 2, 0, "f64 sqdiff aligned=%s" % aligned, tile=(16, 16 * ct))
        got = float(ops.resid_sqnorm(Av.view, Wv.view, Hv.view).item())
        assert got == float((R ** 2).sum()), "f64 resid_sqnorm: %r, expected %r" % (got, float((R ** 2).sum()))
        assert float(ops.sqnorm(Av.view).item()) == float((A2 ** 2).sum()), "f64 sqnorm"
        num, den = ops.column_err_sums(Av.view, Wv.view, Hv.view)
        ex.assert_ulp(num.cpu().numpy(), (R ** 2).sum(0), 0, "f64 column_err_sums num")
        ex.assert_ulp(den.cpu().numpy(), (A2 ** 2).sum(0), 0, "f64 column_err_sums den")
        Av.check("A"); Wv.check("W"); Hv.check("H")


# ------------------------------------------------------------------------------------------------------------- MU updates
@pytest.mark.parametrize("case", ex.F64_MU, ids=lambda c: "nn_rows_kernel-upd_h_kernel-KS%d-%dx%d-k%d" % (c[3], c[0], c[1], c[2]))
def test_mu_updates(env, case):
    """mu_update_w (f64_nn_rows_kernel<KS, NN_UPD_W>) and mu_update_h (f64_upd_h_kernel<KS>), clamp off and on: c = 3; a zero row of W
    and a zero column of H stay exactly 0 (clamp off)"""
    engine, L = env
    ops = engine.HIP_OPS_F64
    m, n, k, ks = case
    A, W, H = (x.copy() for x in _products(m, n, k)[:3])
    W[[0, 17, m - 1]] = 0                                             # zero rows in the first, an inner and the ragged last tile
    H[:, [0, 33, n - 1]] = 0
    AH, WtA, G, GW = A @ H.T, W.T @ A, H @ H.T, W.T @ W                # integers: exact
    zr, zc = ~W.any(1), ~H.any(0)
    for d in (W @ G, GW @ H):
        assert np.all((d == 0) | ((d >= 2) & (d < 2.0 ** 51))), "a denominator that does not absorb eps"
    _reaches(L, "mu_update_w", m, n, k, [], family="nn_rows", nt=ks)
    _reaches(L, "mu_update_h", m, n, k, [], family="upd_h", nt=ks)
    Wq, Hq = _quot(W * AH, W @ G), _quot(H * WtA, GW @ H)
    for aligned in ALIGN:
        Wv = _P(W, aligned)
        ops.mu_update_w(Wv.view, _P(AH, aligned).view, _P(G, aligned).view, E64)
        w = Wv.check("mu_update_w")
        ex.assert_ulp(w, Wq, 3, "f64 mu_update_w aligned=%s" % aligned)
        assert not w[zr].any()
        for clamp in (False, True):
            Hv = _P(H, aligned)
            ops.mu_update_h(Hv.view, _P(WtA, aligned).view, _P(GW, aligned).view, E64, clamp)
            h = Hv.check("mu_update_h")
            ex.assert_ulp(h, np.maximum(Hq, E64) if clamp else Hq, 3, "f64 mu_update_h clamp=%s aligned=%s" % (clamp, aligned))
            assert clamp or not h[:, zc].any()


# ------------------------------------------------------------------------------------------------------------- element-wise, sums
@pytest.mark.parametrize("m,n,k", [(130, 70, 9), (600, 72, 20), (16400, 132, 20)], ids=["130x70-k9", "600x72-k20", "16400x132-grid-stride"])
def test_elementwise_and_sums(env, m, n, k):
    """dnmf_f64_ew ops 0-4, rowsum, colsum on padded views; ops 3 and 4 with S at a pitch of its own.  16400 x 132 is past 2^21 elements:
    the grid-stride loop of f64_ew_kernel takes a second trip (ops 0-2 on the m x n matrix)"""
    engine, L = env
    ops = engine.HIP_OPS_F64
    big = m * n > 1 << 21
    assert big == (m * n > 256 * L.f64_plan("ew", m, n, 1)["grid_x"])
    A = _products(m, n, k)[0]
    s = np.arange(1, n + 1, dtype=np.float64) * 3
    p2 = 2.0 ** (np.arange(m) % 24 - 12.0)
    for aligned in (False,) if big else ALIGN:
        X = _P(np.where(A > 2, A, 0), aligned)
        ops.clamp_min(X.view, E64)
        ex.assert_ulp(X.check("clamp_min"), np.where(A > 2, A, E64), 0, "f64 clamp_min (op 0)")
        X = _P(A, aligned)
        ops.scale_cols_div(X.view, _dev(s), E64)
        ex.assert_ulp(X.check("scale_cols_div"), _quot(A, np.broadcast_to(s, A.shape)), 1, "f64 scale_cols_div (op 1)")
        X = _P(A, aligned)
        ops.scale_rows_mul(X.view, _dev(p2))
        ex.assert_ulp(X.check("scale_rows_mul"), A * p2[:, None], 0, "f64 scale_rows_mul (op 2)")
        if big:
            continue
        Ak, W, H, U, UHt, WtU = _kl(m, n, k)
        rs, cs = H.sum(1), W.sum(0)                                  # rowsum(H) >= 2: eps absorbed; colsum(W) may be 0 or 1: one float64 addition
        Wv, Hv = _P(W, aligned), _P(H, aligned)
        xo, x = _vec(k, aligned)
        ops.rowsum(Hv.view, x)
        ex.assert_ulp(xo.check("rowsum")[0], rs, 0, "f64 rowsum")
        xo, x = _vec(k, aligned)
        ops.colsum(Wv.view, x)
        ex.assert_ulp(xo.check("colsum")[0], cs, 0, "f64 colsum")
        Wv.check("W"); Hv.check("H")
        S = _P(UHt, aligned, ld=ex.f64_pitch(k, aligned) + 6)
        assert S.ld != Wv.ld
        ops.kl_update_w(Wv.view, S.view, _dev(rs), E64)
        ex.assert_ulp(Wv.check("kl_update_w"), _quot(W * UHt, np.broadcast_to(rs + E64, W.shape)), 2, "f64 kl_update_w (op 4)")
        for clamp in (False, True):
            Hv = _P(H, aligned)
            S = _P(WtU, aligned, ld=ex.f64_pitch(n, aligned) + 6)
            assert S.ld != Hv.ld
            ops.kl_update_h(Hv.view, S.view, _dev(cs), E64, clamp)
            Hq = _quot(H * WtU, np.broadcast_to((cs + E64)[:, None], H.shape))
            ex.assert_ulp(Hv.check("kl_update_h"), np.maximum(Hq, E64) if clamp else Hq, 2, "f64 kl_update_h (op 3) clamp=%s" % clamp)
            S.check("S")


# ------------------------------------------------------------------------------------------------------------- whole fits, itr = 1
def _fit_id(method):
    return lambda c: "%s-%s-%dx%d-k%d" % (method, c[3], c[0], c[1], c[2])


def _fro_expected(m, n, k, seed=0):
    A, W, H, Wn, Hq = ex.fro_step(m, n, k, np.float64, seed=seed)
    return (A, W, H), np.maximum(Wn, E64), np.maximum(Hq, E64)


def _kl_expected(m, n, k, seed=0):
    """MU/KL with W fixed: H *= W^T U / (colsum(W) + eps), the divisor one float64 addition as the kernels form it; then the clamp"""
    A, W, H, U = ex.kl(m, n, k, np.float64, seed=seed)
    Hq = _quot(H * (W.T @ U), np.broadcast_to((W.sum(0) + E64)[:, None], H.shape))
    return (A, W, H), np.maximum(W, E64), np.maximum(Hq, E64)


@pytest.mark.parametrize("case", ex.F64_FIT_FRO, ids=_fit_id("mu-fro"))
def test_fit_mu_fro(env, case):
    """dnmf_f64_fit, itr = 1, on `fro_step` operands (the new W exact, the new H one rounding), the clamp after step 0 and
    normalize_features: c = 6.  The tiny kernel (asserted) and the chain of primitives"""
    engine, L = env
    m, n, k, fam = case
    assert L.lib.dnmf_f64_fit_tiny(m, n, k, 0) == int(fam == "fit_tiny") and L.f64_plan("fit", m, n, k, method=0)["family"] == fam
    ops, Wc, Hc = _fro_expected(m, n, k)
    for aligned in ALIGN:
        Ap, Wp, Hp = (_P(x, aligned) for x in ops)
        engine.HIP_OPS_F64.fit("mu", "fro", Ap.view, Wp.view, Hp.view, E64, True, 1)
        Ap.check("A")
        _assert_normalized(Wp.check("fit W"), Hp.check("fit H"), Wc, Hc, 6, "f64 mu-fro fit (%s) aligned=%s" % (fam, aligned), eps=E64)


@pytest.mark.parametrize("case", ex.F64_FIT_KL, ids=_fit_id("mu-kl-wfixed"))
def test_fit_mu_kl_w_fixed(env, case):
    engine, L = env
    m, n, k, fam = case
    assert L.lib.dnmf_f64_fit_tiny(m, n, k, 1) == int(fam == "fit_tiny") and L.f64_plan("fit", m, n, k, method=1)["family"] == fam
    ops, Wc, Hc = _kl_expected(m, n, k)
    for aligned in ALIGN:
        Ap, Wp, Hp = (_P(x, aligned) for x in ops)
        engine.HIP_OPS_F64.fit("mu", "kl", Ap.view, Wp.view, Hp.view, E64, False, 1)
        Ap.check("A")
        _assert_normalized(Wp.check("fit W"), Hp.check("fit H"), Wc, Hc, 6, "f64 mu-kl fit (%s) aligned=%s" % (fam, aligned), eps=E64)


@pytest.mark.parametrize("method", ["fro", "kl"])
def test_fit_stack_of_three(env, method):
    """HipOpsF64.fit on stacks [3][m][n] / [3][m][k] / [3][k][n] inside poisoned buffers: every member as the single fit"""
    engine, L = env
    m, n, k = ex.F64_FIT_STACK
    assert L.lib.dnmf_f64_fit_tiny(m, n, k, 0) == 1
    probs = [(_fro_expected if method == "fro" else _kl_expected)(m, n, k, seed=b) for b in range(3)]
    Ap, Wp, Hp = (ex.Poisoned(torch, np.stack([p[0][i] for p in probs])) for i in range(3))
    engine.HIP_OPS_F64.fit("mu", method, Ap.view, Wp.view, Hp.view, E64, method == "fro", 1)
    Ap.check("A")
    w3, h3 = Wp.check("fit W"), Hp.check("fit H")
    for b, (_, Wc, Hc) in enumerate(probs):
        _assert_normalized(w3[b], h3[b], Wc, Hc, 6, "f64 mu-%s fit [%d]" % (method, b), eps=E64)
