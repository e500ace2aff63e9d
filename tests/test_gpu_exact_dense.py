"""The fp32 dense kernels (csrc/dnmf.hip, csrc/dnmf_kl.hip, csrc/dnmf_kl16.hip and their headers) against the exact answer on the shapes that reach every variant
and every loop-trip class they have (tests/_exact.py: DENSE_REACH, DENSE_EW; tests/test_dense_plan.py proves the reach without a GPU).
Every case first asserts, through dnmf_dense_plan at the addresses and pitches of the very views it passes, that the launch is the one the
case is named after; then it runs the entry point through engine.HIP_OPS and compares with numpy float64 element by element.  Operands
are views in NaN-poisoned buffers, outputs views in sentinel-filled buffers (ex.Poisoned).

Bounds, from the table at the top of tests/test_gpu_exact.py: products and Grams c = 0; MU updates c = 3; the fused W phase on `fro_step`
operands exact; KL element-wise updates c = 2; scale_cols_div c = 1 (one IEEE division); the KL products on `kl` operands c = 0; the
residual, column-error and norm sums equal to the float64 integers."""
import numpy as np
import pytest

from tests import _exact as ex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
EPS32 = np.float32(EPS)


def _ids(cases):
    return [pytest.param(c, id=c[0]) for c in cases]


def _of(*ops):
    return _ids([c for c in ex.DENSE_REACH if c[1] in ops])


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pydnmfk_amd import engine
    from pydnmfk_amd import _lib
    return engine, _lib


def _view(x, name, aligned, bf16=False):
    a = ex.dense_is_aligned(aligned, name)
    if bf16:
        return ex.Poisoned(torch, x, dtype=torch.bfloat16, aligned=a, quantum=8)
    return ex.Poisoned(torch, x, aligned=a)


def _out(rows, cols, name, aligned):
    return ex.Poisoned.out(torch, rows, cols, torch.float32, ex.dense_is_aligned(aligned, name))


def _gram(engine, k, G=None):
    Gd = engine.new_gram(k, torch.device("cuda"))
    Gd.fill_(7.0)
    if G is not None:
        Gd.zero_()
        Gd[:k, :k] = torch.from_numpy(np.ascontiguousarray(G)).cuda().float()
    return Gd


def _check_gram(Gd, ref, k, what):
    g = Gd.cpu().numpy()
    ex.assert_ulp(g[:k, :k], ref, 0, what)
    assert not g[k:].any() and not g[:, k:].any(), "%s: the zero padding of the Gram was not written" % what


def _assert_plan(lib_mod, case, views):
    """the plan of the call about to be made, at the views' own pitches and addresses"""
    cid, op, m, n, k, aligned, bf16, want = case
    ld = [v.stride(-2) for v in views]
    off = [v.data_ptr() % 16 for v in views]
    p = lib_mod.dense_plan(op, max(m, 1), max(n, 1), k, ld, off, bf16a=bf16)
    got = {f: p[f] for f in want}
    assert got == {f: (v if isinstance(v, str) else int(v)) for f, v in want.items()}, (cid, p)
    return p


def _mu_ref(X, S, D, clamp=False):
    q = np.where(D > 0, X * S / np.where(D > 0, D, 1.0), 0.0)
    return np.maximum(q, EPS32) if clamp else q


# ------------------------------------------------------------------------------------------------------------- the NT form
@pytest.mark.parametrize("case", _of("aht", "aht_hblocks", "aht_update_w"))
def test_nt(env, case):
    """aht / aht_hblocks: exactly float64.  aht_update_w: c = 3 on integer operands, and exact on `fro_step` operands where the shape
    admits them (n >= k)"""
    engine, lib_mod = env
    ops = engine.HIP_OPS
    cid, op, m, n, k, aligned, bf16, want = case
    A, W, H, G = ex.dense_nt_operands(m, n, k)
    A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
    Av = _view(A, "A", aligned, bf16)
    if op == "aht_hblocks":
        nh = ex.DENSE_HBLK
        Hs = ex.Poisoned(torch, H.reshape(k, n // nh, nh).transpose(1, 0, 2), packed=True)
        o = _out(m, k, "AH", aligned)
        _assert_plan(lib_mod, case, [Av.view, Hs.view])
        ops.aht_hblocks(Av.view, Hs.view, o.view)
        ex.assert_ulp(o.check(cid), A64 @ H64.T, 0, cid)
        Hs.check("H blocks")
    elif op == "aht":
        Hv = _view(H, "H", aligned)
        o = _out(m, k, "AH", aligned)
        _assert_plan(lib_mod, case, [Av.view, Hv.view])
        ops.aht(Av.view, Hv.view, o.view)
        ex.assert_ulp(o.check(cid), A64 @ H64.T, 0, cid)
        Hv.check("H")
    else:
        Hv, Wv = _view(H, "H", aligned), _view(W, "W", aligned)
        _assert_plan(lib_mod, case, [Av.view, Hv.view, Wv.view])
        ops.aht_update_w(Av.view, Hv.view, _gram(engine, k, G), Wv.view, EPS)
        ex.assert_ulp(Wv.check(cid), _mu_ref(W64, A64 @ H64.T, W64 @ G), 3, cid)
        Hv.check("H")
        if n >= k:
            A2, W2, H2, Wn, _ = ex.fro_step(m, n, k)
            Av2, Hv2, Wv2 = _view(A2, "A", aligned, bf16), _view(H2, "H", aligned), _view(W2, "W", aligned)
            _assert_plan(lib_mod, case, [Av2.view, Hv2.view, Wv2.view])
            H264 = H2.astype(np.float64)
            ops.aht_update_w(Av2.view, Hv2.view, _gram(engine, k, H264 @ H264.T), Wv2.view, EPS)
            ex.assert_ulp(Wv2.check(cid), Wn, 0, cid + " (fro_step operands: exact)")
            Av2.check("A")
    Av.check("A")


@pytest.mark.parametrize("case", _of("gram_hht"))
def test_gram_hht(env, case):
    engine, lib_mod = env
    cid, op, m, n, k, aligned, bf16, want = case
    H = np.ascontiguousarray(ex.dense_tn_operands(n, 1, k)[1].T)
    Hv = _view(H, "H", aligned)
    Gd = _gram(engine, k)
    _assert_plan(lib_mod, case, [Hv.view])
    engine.HIP_OPS.gram_hht(Hv.view, Gd)
    H64 = H.astype(np.float64)
    _check_gram(Gd, H64 @ H64.T, k, cid)
    Hv.check("H")


# ------------------------------------------------------------------------------------------------------------- the TN form
@pytest.mark.parametrize("case", _of("wta", "wta_gram"))
def test_tn(env, case):
    """wta / wta_gram (tn_kernel, tn16_kernel with and without the riding Gram, every reduction): exactly float64"""
    engine, lib_mod = env
    ops = engine.HIP_OPS
    cid, op, m, n, k, aligned, bf16, want = case
    A, W = ex.dense_tn_operands(m, n, k)
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    Av, Wv = _view(A, "A", aligned, bf16), _view(W, "W", aligned)
    o = _out(k, n, "AtW", aligned)
    _assert_plan(lib_mod, case, [Av.view, Wv.view, o.view])
    if op == "wta":
        ops.wta(Av.view, Wv.view, o.view)
    else:
        Gd = _gram(engine, k)
        ops.wta_gram(Av.view, Wv.view, o.view, Gd)
        _check_gram(Gd, W64.T @ W64, k, cid + " Gram")
    ex.assert_ulp(o.check(cid), W64.T @ A64, 0, cid)
    Av.check("A")
    Wv.check("W")


@pytest.mark.parametrize("case", _of("gram_wtw"))
def test_gram_wtw(env, case):
    engine, lib_mod = env
    cid, op, m, n, k, aligned, bf16, want = case
    W = ex.dense_tn_operands(m, 1, k)[1]
    Wv = _view(W, "W", aligned)
    Gd = _gram(engine, k)
    _assert_plan(lib_mod, case, [Wv.view])
    engine.HIP_OPS.gram_wtw(Wv.view, Gd)
    W64 = W.astype(np.float64)
    _check_gram(Gd, W64.T @ W64, k, cid)
    Wv.check("W")


# ------------------------------------------------------------------------------------------------------------- the MU updates
@pytest.mark.parametrize("case", _of("mu_update_w"))
def test_mu_update_w(env, case):
    engine, lib_mod = env
    cid, op, m, n, k, aligned, bf16, want = case
    X, S, G = ex.dense_update_operands(m, k)
    Wv, Sv = _view(X, "W", aligned), _view(S, "AH", aligned)
    _assert_plan(lib_mod, case, [Wv.view, Sv.view])
    engine.HIP_OPS.mu_update_w(Wv.view, Sv.view, _gram(engine, k, G), EPS)
    X64 = X.astype(np.float64)
    ex.assert_ulp(Wv.check(cid), _mu_ref(X64, S.astype(np.float64), X64 @ G), 3, cid, tile=(16, 32))
    Sv.check("AH")


@pytest.mark.parametrize("case", _of("mu_update_h"))
def test_mu_update_h(env, case):
    engine, lib_mod = env
    cid, op, m, n, k, aligned, bf16, want = case
    X, S, G = ex.dense_update_operands(n, k)
    H, AtW = np.ascontiguousarray(X.T), np.ascontiguousarray(S.T)
    H64 = H.astype(np.float64)
    Sv = _view(AtW, "AtW", aligned)
    Gd = _gram(engine, k, G)
    for clamp in (False, True) if k * n < (1 << 22) else (False,):
        Hv = _view(H, "H", aligned)
        _assert_plan(lib_mod, case, [Hv.view, Sv.view])
        engine.HIP_OPS.mu_update_h(Hv.view, Sv.view, Gd, EPS, clamp)
        ex.assert_ulp(Hv.check(cid), _mu_ref(H64, AtW.astype(np.float64), G @ H64, clamp), 3, "%s clamp=%s" % (cid, clamp), tile=(32, 32))
    Sv.check("AtW")


# ------------------------------------------------------------------------------------------------------------- the element-wise passes
class _Plain:
    """a contiguous device copy with the `view` / `check` of ex.Poisoned"""

    def __init__(self, x):
        self.view = torch.from_numpy(x).cuda()

    def check(self, what=""):
        return self.view.cpu().numpy()


@pytest.mark.parametrize("case", _ids(ex.DENSE_EW))
def test_elementwise(env, case):
    engine, lib_mod = env
    ops = engine.HIP_OPS
    cid, op, rows, cols, aligned, want = case
    rs = np.random.RandomState(rows + cols)
    big = rows * cols >= (1 << 26)
    X = rs.randint(0, 8, size=(rows, cols)).astype(np.float32)
    al = aligned is not False
    if big:                                                          # 256 MiB: a plain contiguous tensor (a poisoned buffer's mask would be as large again)
        Xv = _Plain(X)
    else:
        Xv = ex.Poisoned(torch, X, aligned=al)
    nx = {"clamp_min": 0, "scale_cols_div": cols, "scale_rows_mul": rows, "kl_update_h": rows, "kl_update_w": cols}[op]
    xbuf = torch.zeros(nx + 4, device="cuda")
    xv = xbuf[3:3 + nx] if aligned == "x" else xbuf[:nx]
    Sv = ex.Poisoned(torch, rs.randint(0, 8, size=(rows, cols)).astype(np.float32), aligned=al) if op.startswith("kl_") else None
    p = lib_mod.dense_plan("ew", rows, cols, 1, [Xv.view.stride(0), Sv.view.stride(0) if Sv else 0, 0],
                           [Xv.view.data_ptr() % 16, Sv.view.data_ptr() % 16 if Sv else 0, xv.data_ptr() % 16], ew_op=op)
    assert {f: p[f] for f in want} == want, (cid, p)
    X64 = X.astype(np.float64)
    if op == "clamp_min":
        Xv.view.copy_(torch.from_numpy(np.where(X > 2, X, 0).astype(np.float32)))
        ops.clamp_min(Xv.view, EPS)
        ref, c = np.where(X > 2, X64, EPS32), 0
    elif op == "scale_cols_div":
        s = (np.arange(1, cols + 1) * 3).astype(np.float32)
        xv.copy_(torch.from_numpy(s))
        ops.scale_cols_div(Xv.view, xv, EPS)
        ref, c = X64 / (s.astype(np.float64) + EPS)[None, :], 1
    elif op == "scale_rows_mul":
        p2 = (2.0 ** (np.arange(rows) % 24 - 12.0)).astype(np.float32)
        xv.copy_(torch.from_numpy(p2))
        ops.scale_rows_mul(Xv.view, xv)
        ref, c = X64 * p2.astype(np.float64)[:, None], 0
    else:                                                            # x >= 2, an integer: eps is absorbed, one IEEE division and one product
        x = rs.randint(2, 100, size=nx).astype(np.float32)
        xv.copy_(torch.from_numpy(x))
        S64 = Sv.view.cpu().numpy().astype(np.float64)
        if op == "kl_update_h":
            ops.kl_update_h(Xv.view, Sv.view, xv, EPS, False)
            ref = X64 * S64 / x.astype(np.float64)[:, None]
        else:
            ops.kl_update_w(Xv.view, Sv.view, xv, EPS)
            ref = X64 * S64 / x.astype(np.float64)[None, :]
        c = 2
        Sv.check("S")
    ex.assert_ulp(Xv.check(cid), ref, c, cid)
    assert not xbuf[nx + (3 if aligned == "x" else 0):].any(), "the vector's buffer was written past its end"


# ------------------------------------------------------------------------------------------------------------- the KL products
def _ws_bytes(lib_mod, case):
    cid, op, m, n, k = case[:5]
    return lib_mod.lib.dnmf_ws_bytes_hblocks(m, n, k, ex.DENSE_HBLK) if op == "kl_uht_hblocks" else None


@pytest.mark.parametrize("case", _of("kl_uht", "kl_uht_hblocks", "kl_wtu"))
def test_kl_products(env, case):
    """kl_uht / kl_uht_hblocks (the pipelined kernel, kl_uht_kernel, both into one output, splits and their reduction, padded images)
    and kl_wtu: exactly float64 on operands with an exact quotient (ex.kl)"""
    engine, lib_mod = env
    ops = engine.HIP_OPS
    cid, op, m, n, k, aligned, bf16, want = case
    A, W, H, U = ex.kl(m, n, k)
    Av, Wv = _view(A, "A", aligned), _view(W, "W", aligned)
    if op == "kl_wtu":
        Hv, o = _view(H, "H", aligned), _out(k, n, "WTU", aligned)
        views, ref = [Av.view, Wv.view, Hv.view, o.view], W.astype(np.float64).T @ U
    else:
        o = _out(m, k, "UHT", aligned)
        ref = U @ H.astype(np.float64).T
        if op == "kl_uht_hblocks":
            nh = ex.DENSE_HBLK
            Hv = ex.Poisoned(torch, H.reshape(k, n // nh, nh).transpose(1, 0, 2), packed=True)
        else:
            Hv = _view(H, "H", aligned)
        views = [Av.view, Wv.view, Hv.view, o.view]
    ld = [v.stride(-2) for v in views]
    p = lib_mod.dense_plan(op, m, n, k, ld, [v.data_ptr() % 16 for v in views], ws_bytes=_ws_bytes(lib_mod, case))
    assert {f: p[f] for f in want} == want, (cid, p)
    getattr(ops, op)(Av.view, Wv.view, Hv.view, EPS, o.view)
    ex.assert_ulp(o.check(cid), ref, 0, cid, tile=(128, 32))
    for v, what in ((Av, "A"), (Wv, "W"), (Hv, "H")):
        v.check(what)


# ------------------------------------------------------------------------------------------------------------- residual, column error, norm
@pytest.mark.parametrize("case", _of("resid_sqnorm", "column_err"))
def test_residual_sums(env, case):
    """resid_sqnorm (resid_lds_kernel, resid_kernel) and column_err_sums: the float64 integers (ex.dense_resid_operands)"""
    engine, lib_mod = env
    ops = engine.HIP_OPS
    cid, op, m, n, k, aligned, bf16, want = case
    A, W, H, R = ex.dense_resid_operands(m, n, k, whole=op == "resid_sqnorm")
    Av, Wv, Hv = _view(A, "A", aligned, bf16), _view(W, "W", aligned), _view(H, "H", aligned)
    _assert_plan(lib_mod, case, [Av.view, Wv.view, Hv.view])
    if op == "resid_sqnorm":
        got = float(ops.resid_sqnorm(Av.view, Wv.view, Hv.view).item())
        assert got == float((R ** 2).sum()), "%s: %r, expected %r" % (cid, got, float((R ** 2).sum()))
    else:
        num, den = ops.column_err_sums(Av.view, Wv.view, Hv.view)
        ex.assert_ulp(num.cpu().numpy(), (R ** 2).sum(0), 0, cid + " num")
        ex.assert_ulp(den.cpu().numpy(), (A.astype(np.float64) ** 2).sum(0), 0, cid + " den")
    for v, what in ((Av, "A"), (Wv, "W"), (Hv, "H")):
        v.check(what)


@pytest.mark.parametrize("case", _of("sqnorm"))
def test_sqnorm(env, case):
    engine, lib_mod = env
    cid, op, m, n, k, aligned, bf16, want = case
    A = ex.dense_tn_operands(m, n, 1)[0]
    Av = _view(A, "A", aligned, bf16)
    _assert_plan(lib_mod, case, [Av.view])
    got = float(engine.HIP_OPS.sqnorm(Av.view).item())
    assert got == float((A.astype(np.float64) ** 2).sum()), cid
    Av.check("A")
