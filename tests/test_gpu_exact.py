"""Every kernel against the exact answer, element by element (tests/_exact.py): operands whose products are exact in fp32 in any
summation order, so a product must EQUAL float64 and an update must be within a stated number of ulps of the float64 quotient at every
element -- a dropped term in an edge tile, a ragged last slab or team member or a lane mask off by four columns fails here even where
the aggregate tolerances of test_gpu_kernels / test_gpu_fuzz / test_gpu_onepass cannot see it on a large matrix.  Every operand is a
view in a NaN-poisoned buffer (padding, the elements before the view, a guard band after it) and every output a view in a sentinel-
filled buffer: a kernel that reads padding gives NaN, one that writes outside its view changes a sentinel.

Ulp bounds per element (c: |x - q| <= c spacing(float32(q)), q the float64 quotient; zeros must be exactly zero, clamped values eps):
  products, Grams, row / column sums, the W phase of the MU step on `fro_step` operands     exact (c = 0)
  MU updates (mu_quot = s rcp(d), <= 1.5 ulp, dnmf_update.h; then times the factor)        c = 3
  KL element-wise updates (IEEE division, then times the factor, dnmf_stream.h)            c = 2
  the fused KL step's updates (rcp-based quotients)                                         c = 3
  float64 updates (div_pos64 or IEEE division, then the product; spacing of float64)       c = 3
  whole fits, itr = 1 (one step, clamp, normalize_features: W / (s + eps), H s with s the
  column sums of W -- within c of the interval the order-dependent eps terms of s span)    c = 6
Shapes are named after the dispatch boundary they sit on: k on both sides of 4, 16, 32, 64, 128 (the KP / tile boundaries of dnmf_kp and
the 16-wide kernels), n not a multiple of 4 / 32 / 64 / 512 (vector loads, column tiles, team members), ragged m at 16 / 32 / 128
(row tiles, slabs), unaligned starts (the generic paths)."""
import numpy as np
import pytest

from tests import _exact as ex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
EPS32 = np.float32(EPS)

# (m, n, k, aligned): every k of the KP and tile boundaries, with m ragged at 16 / 32 / 128 and n ragged at 4 / 32 / 64 / 512
PRIM = [
    pytest.param(129, 130, 1, True, id="k1-m%16-n%4"),
    pytest.param(1000, 515, 4, False, id="k4-unaligned-n%4"),
    pytest.param(4100, 2052, 5, True, id="k5-16wide-n%512"),
    pytest.param(257, 600, 15, False, id="k15-unaligned"),
    pytest.param(4100, 1024, 16, True, id="k16-16wide-m%128"),
    pytest.param(300, 2052, 17, True, id="k17-kp32-n%32"),
    pytest.param(1000, 515, 31, False, id="k31-unaligned-n%4"),
    pytest.param(2048, 1024, 32, True, id="k32-whole-tiles"),
    pytest.param(257, 4100, 33, True, id="k33-kp64-n%512"),
    pytest.param(1000, 600, 63, False, id="k63-unaligned"),
    pytest.param(2000, 1030, 64, True, id="k64-n%4"),
    pytest.param(513, 129, 65, True, id="k65-kp128"),
    pytest.param(700, 300, 127, False, id="k127-unaligned"),
    pytest.param(1024, 516, 128, True, id="k128-n%32"),
    pytest.param(300, 700, 129, True, id="k129-kp256"),
    pytest.param(260, 520, 192, False, id="k192-unaligned"),
    pytest.param(515, 333, 256, True, id="k256-n%4"),
]
SUB = [PRIM[i] for i in (0, 2, 5, 8, 10, 13, 16)]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pydnmfk_amd import engine
    from pydnmfk_amd._lib import lib
    return engine, lib


def _P(x, aligned=True, dtype=None):
    return ex.Poisoned(torch, x, dtype=dtype, aligned=aligned)


def _out(rows, cols, aligned=True, dtype=torch.float32):
    return ex.Poisoned.out(torch, rows, cols, dtype, aligned)


def _gram(engine, k, dtype=torch.float32):
    G = engine.new_gram(k, torch.device("cuda")).to(dtype)
    G.fill_(7.0)
    return G


def _check_gram(G, ref, k, what):
    g = G.cpu().numpy()
    ex.assert_ulp(g[:k, :k], ref, 0, what)
    assert not g[k:].any() and not g[:, k:].any(), "%s: the zero padding of the Gram was not written" % what


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().to(dtype)


# ------------------------------------------------------------------------------------------------------------- v_rcp_f32 at 2^p
def test_rcp_is_exact_at_powers_of_two(env):
    """the exact W phase of `fro_step` needs v_rcp_f32 (mu_quot) to be exact at powers of two: W one-hot with 1s, A H^T = 1, W G = 2^p"""
    engine, _ = env
    m, k = 96, 20
    rs = np.random.RandomState(5)
    jr = np.arange(m) % k
    W = np.zeros((m, k), np.float32)
    W[np.arange(m), jr] = 1
    p = rs.randint(1, 40, size=(k, k))
    G = _gram(engine, k)
    G.zero_()
    G[:k, :k] = _dev(2.0 ** p)
    Wv = _P(W)
    engine.HIP_OPS.mu_update_w(Wv.view, _dev(np.ones((m, k))), G, EPS)
    q = np.zeros((m, k))
    q[np.arange(m), jr] = 2.0 ** -p[jr, jr]
    ex.assert_ulp(Wv.check("rcp"), q, 0, "v_rcp_f32 at powers of two")


# ------------------------------------------------------------------------------------------------------------- products
@pytest.mark.parametrize("adt", ["f32", "bf16"])
@pytest.mark.parametrize("m,n,k,aligned", PRIM)
def test_products(env, m, n, k, aligned, adt):
    """gram_hht / gram_wtw, aht, wta, wta_gram (fp32 and bf16-stored A): exactly float64"""
    engine, _ = env
    ops = engine.HIP_OPS
    A, W, H = ex.products(m, n, k)
    A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
    Av = _P(A, aligned, torch.bfloat16 if adt == "bf16" else torch.float32)
    Wv, Hv = _P(W, aligned), _P(H, aligned)
    if adt == "f32":
        G = _gram(engine, k)
        ops.gram_hht(Hv.view, G)
        _check_gram(G, H64 @ H64.T, k, "gram_hht")
        ops.gram_wtw(Wv.view, G)
        _check_gram(G, W64.T @ W64, k, "gram_wtw")
    o = _out(m, k, aligned)
    ops.aht(Av.view, Hv.view, o.view)
    ex.assert_ulp(o.check("aht"), A64 @ H64.T, 0, "aht")
    o = _out(k, n, aligned)
    ops.wta(Av.view, Wv.view, o.view)
    ex.assert_ulp(o.check("wta"), W64.T @ A64, 0, "wta")
    o, G = _out(k, n, aligned), _gram(engine, k)
    ops.wta_gram(Av.view, Wv.view, o.view, G)
    ex.assert_ulp(o.check("wta_gram"), W64.T @ A64, 0, "wta_gram product")
    _check_gram(G, W64.T @ W64, k, "wta_gram Gram")
    for p, what in ((Av, "A"), (Wv, "W"), (Hv, "H")):
        p.check(what)


HB = [pytest.param(129, 64, 1, False, id="k1-unaligned"), pytest.param(300, 1024, 17, True, id="k17-m%16"),
      pytest.param(2048, 1024, 32, True, id="k32"), pytest.param(1000, 512, 64, False, id="k64-unaligned")]


@pytest.mark.parametrize("m,n,k,aligned", HB)
def test_hblocks(env, m, n, k, aligned):
    """aht_hblocks / kl_uht_hblocks: H as the stack of its 32-column blocks (what an allgather of the slices leaves)"""
    engine, _ = env
    ops = engine.HIP_OPS
    nh = 32
    A, W, H = ex.products(m, n, k)
    Hs = ex.Poisoned(torch, H.reshape(k, n // nh, nh).transpose(1, 0, 2), packed=True)   # contiguous, NaN before and after
    Av = _P(A, aligned)
    o = _out(m, k, aligned)
    ops.aht_hblocks(Av.view, Hs.view, o.view)
    ex.assert_ulp(o.check("aht_hblocks"), A.astype(np.float64) @ H.T.astype(np.float64), 0, "aht_hblocks")
    Hs.check("H blocks")
    Ak, Wk, Hk, U = ex.kl(m, n, k)
    Hs = ex.Poisoned(torch, Hk.reshape(k, n // nh, nh).transpose(1, 0, 2), packed=True)
    o = _out(m, k, aligned)
    ops.kl_uht_hblocks(_P(Ak, aligned).view, _P(Wk, aligned).view, Hs.view, EPS, o.view)
    ex.assert_ulp(o.check("kl_uht_hblocks"), U @ Hk.T.astype(np.float64), 0, "kl_uht_hblocks")
    Hs.check("H blocks")


# ------------------------------------------------------------------------------------------------------------- MU updates
def _mu_ref(X, S, D, clamp=False):
    q = np.where(D > 0, X * S / np.where(D > 0, D, 1.0), 0.0)
    return np.maximum(q, EPS32) if clamp else q


@pytest.mark.parametrize("m,n,k,aligned", PRIM)
def test_mu_updates(env, m, n, k, aligned):
    """mu_update_w, mu_update_h (clamp off and on), aht_update_w: c = 3 (s rcp(d), then the factor)"""
    engine, _ = env
    ops = engine.HIP_OPS
    A, W, H = ex.products(m, n, k)
    A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
    G, GW = H64 @ H64.T, W64.T @ W64
    AH, AtW = A64 @ H64.T, W64.T @ A64
    Gd, GWd = _gram(engine, k), _gram(engine, k)
    Gd.zero_(); GWd.zero_()
    Gd[:k, :k], GWd[:k, :k] = _dev(G), _dev(GW)
    Wref = _mu_ref(W64, AH, W64 @ G)
    Wv = _P(W, aligned)
    ops.mu_update_w(Wv.view, _P(AH.astype(np.float32), aligned).view, Gd, EPS)
    ex.assert_ulp(Wv.check("mu_update_w"), Wref, 3, "mu_update_w")
    for clamp in (False, True):
        Hv = _P(H, aligned)
        ops.mu_update_h(Hv.view, _P(AtW.astype(np.float32), aligned).view, GWd, EPS, clamp)
        ex.assert_ulp(Hv.check("mu_update_h"), _mu_ref(H64, AtW, GW @ H64, clamp), 3, "mu_update_h clamp=%s" % clamp)
    Wv = _P(W, aligned)
    ops.aht_update_w(_P(A, aligned).view, _P(H, aligned).view, Gd, Wv.view, EPS)
    ex.assert_ulp(Wv.check("aht_update_w"), Wref, 3, "aht_update_w")


# ------------------------------------------------------------------------------------------------------------- KL
@pytest.mark.parametrize("m,n,k,aligned", PRIM)
def test_kl(env, m, n, k, aligned):
    """kl_uht, kl_wtu, rowsum, colsum: exact; kl_update_w / kl_update_h: c = 2; mu_kl_step: W c = 3, H (from the kernel's new W,
    whose quotient U is no longer exact) 1e-5 of each element"""
    engine, _ = env
    ops = engine.HIP_OPS
    A, W, H, U = ex.kl(m, n, k)
    UHt, WtU, rs, cs, Wq, Hq = ex.kl_refs(A, W, H, U)
    Av, Wv, Hv = _P(A, aligned), _P(W, aligned), _P(H, aligned)
    o = _out(m, k, aligned)
    ops.kl_uht(Av.view, Wv.view, Hv.view, EPS, o.view)
    ex.assert_ulp(o.check("kl_uht"), UHt, 0, "kl_uht")
    o = _out(k, n, aligned)
    ops.kl_wtu(Av.view, Wv.view, Hv.view, EPS, o.view)
    ex.assert_ulp(o.check("kl_wtu"), WtU, 0, "kl_wtu")
    x = torch.full((k,), 7.0, device="cuda")
    ex.assert_ulp(ops.rowsum(Hv.view, x).cpu().numpy(), rs, 0, "rowsum")
    x = torch.full((k,), 7.0, device="cuda")
    ex.assert_ulp(ops.colsum(Wv.view, x).cpu().numpy(), cs, 0, "colsum")
    W2 = _P(W, aligned)
    ops.kl_update_w(W2.view, _P(UHt.astype(np.float32), aligned).view, _dev(rs), EPS)
    ex.assert_ulp(W2.check("kl_update_w"), Wq, 2, "kl_update_w")
    for clamp in (False, True):
        H2 = _P(H, aligned)
        ops.kl_update_h(H2.view, _P(WtU.astype(np.float32), aligned).view, _dev(cs), EPS, clamp)
        ex.assert_ulp(H2.check("kl_update_h"), np.maximum(Hq, EPS32) if clamp else Hq, 2, "kl_update_h clamp=%s" % clamp)
    # the fused step: H only (W fixed: the quotient stays exact), then W and H
    W3, H3 = _P(W, aligned), _P(H, aligned)
    ops.mu_kl_step(Av.view, W3.view, H3.view, EPS, False, False)
    ex.assert_ulp(H3.check("mu_kl_step H"), Hq, 3, "mu_kl_step (W fixed) H")
    ex.assert_ulp(W3.check("mu_kl_step W"), W.astype(np.float64), 0, "mu_kl_step (W fixed) W")
    W4, H4 = _P(W, aligned), _P(H, aligned)
    ops.mu_kl_step(Av.view, W4.view, H4.view, EPS, True, False)
    Wn = W4.check("mu_kl_step W")
    ex.assert_ulp(Wn, Wq, 3, "mu_kl_step W")
    Wn64 = Wn.astype(np.float64)
    Un = A.astype(np.float64) / (Wn64 @ H.astype(np.float64) + EPS)
    Hn = H.astype(np.float64) * (Wn64.T @ Un) / (Wn64.sum(0) + EPS)[:, None]
    h = H4.check("mu_kl_step H")
    assert np.all(np.abs(h - Hn) <= 1e-5 * np.abs(Hn)), "mu_kl_step H off by more than 1e-5 at %s" % (
        tuple(np.argwhere(~(np.abs(h - Hn) <= 1e-5 * np.abs(Hn)))[0]),)


# ------------------------------------------------------------------------------------------------------------- element-wise and norms
@pytest.mark.parametrize("m,n,k,aligned", SUB + [pytest.param(37, 1, 3, False, id="one-column-unaligned")])
def test_elementwise_and_norms(env, m, n, k, aligned):
    """clamp_min, scale_cols_div (c = 1: one IEEE division), scale_rows_mul (exact on powers of two), sqnorm / resid_sqnorm /
    column_err_sums (integers: exact), fp32 and bf16-stored A"""
    engine, _ = env
    ops = engine.HIP_OPS
    A, W, H = ex.products(m, n, k)
    A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
    X = _P(np.where(A > 2, A, 0).astype(np.float32), aligned)
    ops.clamp_min(X.view, EPS)
    ex.assert_ulp(X.check("clamp_min"), np.where(A > 2, A64, EPS32), 0, "clamp_min")
    s = np.arange(1, k + 1, dtype=np.float32) * 3
    Wv = _P(W, aligned)
    ops.scale_cols_div(Wv.view, _dev(s), EPS)
    ex.assert_ulp(Wv.check("scale_cols_div"), W64 / (s.astype(np.float64) + EPS)[None, :], 1, "scale_cols_div")
    p2 = 2.0 ** (np.arange(k) % 24 - 12.0)
    Hv = _P(H, aligned)
    ops.scale_rows_mul(Hv.view, _dev(p2))
    ex.assert_ulp(Hv.check("scale_rows_mul"), H64 * p2[:, None], 0, "scale_rows_mul")
    for adt in (torch.float32, torch.bfloat16):
        Av = _P(A, aligned, adt)
        assert float(ops.sqnorm(Av.view).item()) == float((A64 ** 2).sum()), "sqnorm %s" % adt
    # the residual norms square in fp32 before the float64 sums: A = W H + (0..2), so every residual square is at most 4 and the
    # fp32 partial sums stay exact (bf16 storage: where W H + 2 <= 256)
    rs = np.random.RandomState(m + k)
    A2 = W64 @ H64 + rs.randint(0, 3, size=(m, n))
    R = A2 - W64 @ H64
    for adt in (torch.float32, torch.bfloat16) if A2.max() <= 256 else (torch.float32,):
        Av = _P(A2.astype(np.float32), aligned, adt)
        got = float(ops.resid_sqnorm(Av.view, _P(W, aligned).view, _P(H, aligned).view).item())
        assert got == float((R ** 2).sum()), "resid_sqnorm %s: %r, expected %r" % (adt, got, float((R ** 2).sum()))
        num, den = ops.column_err_sums(Av.view, _P(W, aligned).view, _P(H, aligned).view)
        ex.assert_ulp(num.cpu().numpy(), (R ** 2).sum(0), 0, "column_err_sums num %s" % adt)
        ex.assert_ulp(den.cpu().numpy(), (A2 ** 2).sum(0), 0, "column_err_sums den %s" % adt)


# ------------------------------------------------------------------------------------------------------------- whole MU/FRO steps
FRO = [pytest.param(300, 130, 5, False, id="k5-unaligned"), pytest.param(1000, 515, 17, True, id="k17-n%4"),
       pytest.param(257, 600, 33, False, id="k33-unaligned"), pytest.param(2000, 1030, 64, True, id="k64-n%4"),
       pytest.param(700, 300, 128, True, id="k128"), pytest.param(515, 333, 256, True, id="k256-wide")]
# one-pass (the team kernel): whole teams, a ragged last slab, the 16-wide instantiation with teams of up to 16 members, a last
# member of one lane group (n % 512 == 4), n % 512 != 0 at k > 16
ONEPASS = [pytest.param(4096, 2048, 32, id="team-k32"), pytest.param(5000, 2052, 24, id="team-ragged-slab-last-member-4-cols"),
           pytest.param(4100, 3332, 12, id="team16-n%512"), pytest.param(4096, 8192, 16, id="team16-16-members"),
           pytest.param(5003, 3072, 9, id="team16-ragged-slab")]


def _fro_check(Wv, Hv, Wn, Hq, clamp, what):
    w, h = Wv.check(what + " W"), Hv.check(what + " H")
    if clamp:
        Wn, Hq = np.maximum(Wn, EPS32), np.maximum(Hq, EPS32)
    ex.assert_ulp(w, Wn, 0, what + " W (exact)")
    ex.assert_ulp(h, Hq, 3, what + " H")
    return w, h


def _fro_step(ops, A, W, H, clamp, aligned=True, adt=torch.float32):
    Av, Wv, Hv = _P(A, aligned, adt), _P(W, aligned), _P(H, aligned)
    ops.mu_fro_step(Av.view, Wv.view, Hv.view, EPS, True, clamp)
    Av.check("A")
    return Wv, Hv


@pytest.mark.parametrize("m,n,k,aligned", FRO)
def test_mu_fro_step_two_pass(env, m, n, k, aligned):
    """mu_fro_step on the two-pass route: the new W exact, the new H c = 3; fp32 and bf16-stored A, through HIP_OPS and through
    HIP_OPS_BF16X6 -- whose entry points forward every shape of FRO to the fp32 kernels (n % 128 != 0), so the second round covers the
    forwarding; the step on the split kernels: tests/test_gpu_exact_split.py::test_mu_fro_step"""
    engine, lib = env
    A, W, H, Wn, Hq = ex.fro_step(m, n, k)
    was = lib.dnmf_set_onepass(0)
    try:
        for ops in (engine.HIP_OPS, engine.HIP_OPS_BF16X6):
            for adt in (torch.float32, torch.bfloat16):
                for clamp in (False, True):
                    _fro_check(*_fro_step(ops, A, W, H, clamp, aligned, adt), Wn, Hq, clamp, "%s %s clamp=%s" % (ops.name, adt, clamp))
    finally:
        lib.dnmf_set_onepass(was)


@pytest.mark.parametrize("m,n,k", ONEPASS)
def test_mu_fro_step_one_pass(env, m, n, k):
    """the team kernel's in-kernel W_new^T A: forced one-pass (asserted taken), exact W, H c = 3, and the same bits as the two passes
    (W_new^T A and W_new^T W_new are exact either way, and the H update that consumes them is the same launch)"""
    engine, lib = env
    ops = engine.HIP_OPS
    A, W, H, Wn, Hq = ex.fro_step(m, n, k)
    for adt in (torch.float32, torch.bfloat16):
        for clamp in (False, True):
            got = {}
            for mode in (2, 0):
                was = lib.dnmf_set_onepass(mode)
                try:
                    if mode == 2:
                        assert lib.dnmf_mu_fro_onepass(m, n, k) == 1
                    got[mode] = _fro_check(*_fro_step(ops, A, W, H, clamp, True, adt), Wn, Hq, clamp, "pass %d %s clamp=%s" % (mode, adt, clamp))
                finally:
                    lib.dnmf_set_onepass(was)
            for x1, x0, what in zip(got[2], got[0], "WH"):
                assert np.array_equal(x1.view(np.uint32), x0.view(np.uint32)), \
                    "one-pass %s differs from the two passes (%s clamp=%s) first at %s" % (what, adt, clamp, tuple(np.argwhere(x1 != x0)[0]))
    ops.hals_check()


@pytest.mark.parametrize("m,n,k", [pytest.param(4096, 2048, 32, id="team-k32"), pytest.param(5000, 2052, 17, id="team-ragged"),
                                   pytest.param(4100, 3332, 12, id="team16-n%512")])
def test_team_w_quotient_is_correctly_rounded(env, m, n, k):
    """the team kernel's W update is div_pos(w (A H^T), W G + eps) (dnmf_team.h), which dnmf_common.h states gives the bits of the
    IEEE division wherever nothing under- or overflows.  On integer operands numerator and denominator are exact, so the new W must
    EQUAL the correctly rounded fp32 quotient numpy forms -- at every element, not only within an ulp"""
    engine, lib = env
    A, W, H = ex.products(m, n, k)
    A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
    num = (W64 * (A64 @ H64.T)).astype(np.float32)                         # exact: integers below 2^24
    den = (W64 @ (H64 @ H64.T)).astype(np.float32) + EPS32                 # exact integers >= 2: eps absorbed
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(W > 0, num / den, 0).astype(np.float32)              # IEEE fp32 division (a zero row of W stays 0)
    was = lib.dnmf_set_onepass(2)
    try:
        assert lib.dnmf_mu_fro_onepass(m, n, k) == 1
        Wv, Hv = _P(W), _P(H)
        engine.HIP_OPS.mu_fro_step(_P(A).view, Wv.view, Hv.view, EPS, True, False)
    finally:
        lib.dnmf_set_onepass(was)
    ex.assert_ulp(Wv.check("team W"), q.astype(np.float64), 0, "div_pos against the IEEE quotient")


def test_team_w_beyond_the_2gib_window(env):
    """W a column view of a 4096 x (2^21 + 2^17) buffer (rows 8.5 MiB apart; only the view is written): a team's 256 rows of W span
    more than the 2 GiB of the team kernel's W descriptor, so its last rows would read zeros and drop their stores -- the step must
    fall back to the two passes (dnmf_team.hip) and stay exact"""
    engine, lib = env
    ops = engine.HIP_OPS
    m, n, k = 4096, 8192, 16
    A, W, H, Wn, Hq = ex.fro_step(m, n, k)
    big = torch.empty(m, (1 << 21) + (1 << 17), dtype=torch.float32, device="cuda")
    try:
        Wv = big[:, :k]
        Wv.copy_(_dev(W))
        Hv = _P(H)
        was = lib.dnmf_set_onepass(2)
        try:
            assert lib.dnmf_mu_fro_onepass(m, n, k) == 1
            ops.mu_fro_step(_dev(A), Wv, Hv.view, EPS, True, False)
        finally:
            lib.dnmf_set_onepass(was)
        ex.assert_ulp(Wv.cpu().numpy(), Wn, 0, "W (ldw = 2^21 + 2^17)")
        ex.assert_ulp(Hv.check("H"), Hq, 3, "H (ldw = 2^21 + 2^17)")
    finally:
        del big
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- whole fits
FIT = [pytest.param(300, 130, 5, 1, id="small-k5"), pytest.param(1000, 260, 16, 1, id="small-k16-m%16"),
       pytest.param(257, 600, 32, 3, id="small-k32-batched"), pytest.param(1030, 515, 17, 2, id="small-k17-batched-n%4")]


def _assert_normalized(w, h, Wc, Hc, c, what, eps=EPS):
    """normalize_features on the clamped step: s = column sums of W, W / (s + eps), H s.  The clamped zeros of W add eps terms to
    s that an fp32 sum absorbs or keeps depending on its order, so s lies between the sum without them and the float64 sum with
    them; each element is held to c ulps of the interval that spans.  eps: the clamp of the operator set (float64: 2^-52, where the
    same holds for its float64 sums -- tests/test_gpu_exact_f64.py; there numpy's own float64 sum of Wc would absorb eps terms too,
    so the upper end is formed as s_lo + count eps: exact for the fp32 operands, within half an ulp of s for the float64 ones)"""
    clamped = Wc <= eps
    s_lo = np.where(clamped, 0, Wc).sum(0)
    s_hi = s_lo + clamped.sum(0) * eps
    ex.assert_ulp(w, Wc / (s_lo + eps)[None, :], c, what + " W", q_hi=Wc / (s_hi + eps)[None, :])
    ex.assert_ulp(h, Hc * s_lo[:, None], c, what + " H", q_hi=Hc * s_hi[:, None])


@pytest.mark.parametrize("m,n,k,B", FIT)
def test_fit_itr1(env, m, n, k, B):
    """HIP_OPS.fit with itr = 1 on the small whole-fit kernels (dnmf_mu_fit_persistent asserted): one step, the clamp after step 0,
    normalize_features -- c = 6 against the float64 of the same formulas on the exact step; mu-fro and mu-kl, single and batched"""
    engine, lib = env
    ops = engine.HIP_OPS
    assert lib.dnmf_mu_fit_persistent(m, n, k) == 1
    def stacks(probs):
        # [B][rows][cols] stacks with padded pitch inside NaN-poisoned buffers (members 16-byte apart, as stack_alloc lays them out)
        P = [ex.Poisoned(torch, np.stack([p[i] for p in probs])) for i in range(3)]
        return P, tuple(x.view if B > 1 else x.view[0] for x in P)

    probs = [ex.fro_step(m, n, k, seed=b) for b in range(B)]
    (Ap, Wp, Hp), args = stacks(probs)
    ops.fit("mu", "fro", *args, EPS, True, 1)
    Ap.check("A")
    w3, h3 = Wp.check("fit W"), Hp.check("fit H")
    for b, (A, W, H, Wn, Hq) in enumerate(probs):
        _assert_normalized(w3[b], h3[b], np.maximum(Wn, EPS32), np.maximum(Hq, EPS32), 6, "mu-fro fit [%d]" % b)
    # mu-kl, W fixed: the H quotient is exact; the clamp after step 0 and the normalisation as above
    probs = [ex.kl(m, n, k, seed=b) for b in range(B)]
    (Ap, Wp, Hp), args = stacks(probs)
    ops.fit("mu", "kl", *args, EPS, False, 1)
    Ap.check("A")
    w3, h3 = Wp.check("fit W"), Hp.check("fit H")
    for b, (A, W, H, U) in enumerate(probs):
        Hq = ex.kl_refs(A, W, H, U)[5]
        _assert_normalized(w3[b], h3[b], np.maximum(W.astype(np.float64), EPS32), np.maximum(Hq, EPS32), 6, "mu-kl fit [%d]" % b)


# ------------------------------------------------------------------------------------------------------------- bf16x6 and float64
@pytest.mark.parametrize("m,n,k,aligned", SUB)
def test_bf16x6_products(env, m, n, k, aligned):
    """the bf16x6 entry points on shapes WITHOUT a split kernel (no n of SUB is a multiple of 128: tests/test_bf16x6_plan.py asserts it):
    the forwarding to the fp32 kernels -- aht, wta, kl_uht, kl_wtu EQUAL float64, fp32 and bf16-stored A; aht_update_w c = 3.  The split
    kernels themselves (csrc/dnmf_split.h, dnmf_split_kl.h) are held to exact operands in tests/test_gpu_exact_split.py"""
    engine, _ = env
    ops = engine.HIP_OPS_BF16X6
    A, W, H = ex.products(m, n, k)
    A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
    for adt in (torch.float32, torch.bfloat16):
        Av = _P(A, aligned, adt)
        o = _out(m, k, aligned)
        ops.aht(Av.view, _P(H, aligned).view, o.view)
        ex.assert_ulp(o.check("bf16x6 aht"), A64 @ H64.T, 0, "bf16x6 aht %s" % adt)
        o = _out(k, n, aligned)
        ops.wta(Av.view, _P(W, aligned).view, o.view)
        ex.assert_ulp(o.check("bf16x6 wta"), W64.T @ A64, 0, "bf16x6 wta %s" % adt)
        G = _gram(engine, k)
        G.zero_()
        G[:k, :k] = _dev(H64 @ H64.T)
        Wv = _P(W, aligned)
        ops.aht_update_w(Av.view, _P(H, aligned).view, G, Wv.view, EPS)
        ex.assert_ulp(Wv.check("bf16x6 aht_update_w"), _mu_ref(W64, A64 @ H64.T, W64 @ (H64 @ H64.T)), 3, "bf16x6 aht_update_w %s" % adt)
    A, W, H, U = ex.kl(m, n, k)
    UHt, WtU, _, _, _, Hq = ex.kl_refs(A, W, H, U)
    Av, Wv, Hv = _P(A, aligned), _P(W, aligned), _P(H, aligned)
    o = _out(m, k, aligned)
    ops.kl_uht(Av.view, Wv.view, Hv.view, EPS, o.view)
    ex.assert_ulp(o.check("bf16x6 kl_uht"), UHt, 0, "bf16x6 kl_uht")
    o = _out(k, n, aligned)
    ops.kl_wtu(Av.view, Wv.view, Hv.view, EPS, o.view)
    ex.assert_ulp(o.check("bf16x6 kl_wtu"), WtU, 0, "bf16x6 kl_wtu")
    ops.mu_kl_step(Av.view, Wv.view, Hv.view, EPS, False, False)
    ex.assert_ulp(Hv.check("bf16x6 mu_kl_step"), Hq, 3, "bf16x6 mu_kl_step (W fixed) H")


F64 = [pytest.param(129, 130, 1, True, id="k1"), pytest.param(257, 600, 15, False, id="k15-unaligned"),
       pytest.param(300, 515, 17, True, id="k17-n%4"), pytest.param(1000, 600, 64, False, id="k64-unaligned"),
       pytest.param(513, 129, 65, True, id="k65")]


@pytest.mark.parametrize("m,n,k,aligned", F64)
def test_f64(env, m, n, k, aligned):
    """HIP_OPS_F64: Grams, aht, wta, kl_uht, kl_wtu exact; mu_update_w / mu_update_h c = 3 (float64 spacing)"""
    engine, _ = env
    ops = engine.HIP_OPS_F64
    d = torch.float64
    A, W, H = ex.products(m, n, k, np.float64)
    G, GW = H @ H.T, W.T @ W
    o = _out(k, k, aligned, d)
    ops.gram_hht(_P(H, aligned).view, o.view)
    ex.assert_ulp(o.check("f64 gram_hht"), G, 0, "f64 gram_hht")
    o = _out(k, k, aligned, d)
    ops.gram_wtw(_P(W, aligned).view, o.view)
    ex.assert_ulp(o.check("f64 gram_wtw"), GW, 0, "f64 gram_wtw")
    o = _out(m, k, aligned, d)
    ops.aht(_P(A, aligned).view, _P(H, aligned).view, o.view)
    ex.assert_ulp(o.check("f64 aht"), A @ H.T, 0, "f64 aht")
    o = _out(k, n, aligned, d)
    ops.wta(_P(A, aligned).view, _P(W, aligned).view, o.view)
    ex.assert_ulp(o.check("f64 wta"), W.T @ A, 0, "f64 wta")
    Wv = _P(W, aligned)
    ops.mu_update_w(Wv.view, _dev(A @ H.T, d), _dev(G, d), 2.220446049250313e-16)
    ex.assert_ulp(Wv.check("f64 mu_update_w"), _mu_ref(W, A @ H.T, W @ G), 3, "f64 mu_update_w")
    Hv = _P(H, aligned)
    ops.mu_update_h(Hv.view, _dev(W.T @ A, d), _dev(GW, d), 2.220446049250313e-16, False)
    ex.assert_ulp(Hv.check("f64 mu_update_h"), _mu_ref(H, W.T @ A, GW @ H), 3, "f64 mu_update_h")
    A, W, H, U = ex.kl(m, n, k, np.float64)
    o = _out(m, k, aligned, d)
    ops.kl_uht(_P(A, aligned).view, _P(W, aligned).view, _P(H, aligned).view, 2.220446049250313e-16, o.view)
    ex.assert_ulp(o.check("f64 kl_uht"), U @ H.T, 0, "f64 kl_uht")
    o = _out(k, n, aligned, d)
    ops.kl_wtu(_P(A, aligned).view, _P(W, aligned).view, _P(H, aligned).view, 2.220446049250313e-16, o.view)
    ex.assert_ulp(o.check("f64 kl_wtu"), W.T @ U, 0, "f64 kl_wtu")


@pytest.mark.parametrize("m,n,k", [(24, 20, 4), (40, 33, 5)])
def test_f64_tiny_fit(env, m, n, k):
    """dnmf_f64_fit on a tiny problem (f64_tiny_fit_kernel), itr = 1, mu-fro: W exact before the normalisation, c = 6 after"""
    engine, _ = env
    A, W, H, Wn, Hq = ex.fro_step(m, n, k, np.float64, tmax=2)
    Ap, Wp, Hp = _P(A), _P(W), _P(H)
    e64 = 2.220446049250313e-16
    engine.HIP_OPS_F64.fit("mu", "fro", Ap.view, Wp.view, Hp.view, e64, True, 1)
    Ap.check("A")
    s = np.maximum(Wn, e64).sum(0)
    ex.assert_ulp(Wp.check("f64 tiny fit W"), np.maximum(Wn, e64) / (s + e64)[None, :], 6, "f64 tiny fit W")
    ex.assert_ulp(Hp.check("f64 tiny fit H"), np.maximum(Hq, e64) * s[:, None], 6, "f64 tiny fit H")


# ------------------------------------------------------------------------------------------------------------- large A, windows
def _outside_untouched(buf, lead, ld, rows, cols, fill, what):
    """on the device: the lead, the pitch padding of every row and the guard of a buffer still hold `fill` (NaN or a sentinel)"""
    same = (lambda t: torch.isnan(t).all()) if fill != fill else (lambda t: (t == fill).all())
    pad = buf.as_strided((rows, ld - cols), (ld, 1), lead + cols) if ld > cols else buf[:0]
    assert bool(same(buf[:lead])) and bool(same(pad)) and bool(same(buf[lead + rows * ld:])), "%s: written outside its view" % what


def test_a_beyond_2_and_4_gib(env):
    """A of 140000 x 8192 fp32 with pitch 8196 (4.6 GB: descriptor windows past 2 GiB, a byte size past 4 GiB), binary, its padding
    NaN: aht and wta exactly float64 into sentinel-filled outputs, the reference on the device (integers: any order is exact)"""
    engine, _ = env
    ops = engine.HIP_OPS
    m, n, k = 140000, 8192, 16
    lead, ld, guard = 8, n + 4, 67
    g = torch.Generator(device="cuda").manual_seed(7)
    buf = torch.full((lead + m * ld + guard,), float("nan"), device="cuda")
    try:
        A = buf.as_strided((m, n), (ld, 1), lead)
        for r0 in range(0, m, 20000):
            A[r0:r0 + 20000] = torch.randint(0, 2, (min(20000, m - r0), n), device="cuda", generator=g, dtype=torch.int32).float()
        H = torch.randint(0, 4, (k, n), device="cuda", generator=g).float()
        W = torch.randint(0, 4, (m, k), device="cuda", generator=g).float()
        ob = torch.full((lead + m * (k + 4) + guard,), ex.SENTINEL, device="cuda")
        out = ob.as_strided((m, k), (k + 4, 1), lead)
        ops.aht(A, H, out)
        _outside_untouched(ob, lead, k + 4, m, k, ex.SENTINEL, "aht output")
        ref = torch.zeros(m, k, dtype=torch.float64, device="cuda")
        for r0 in range(0, m, 35000):
            ref[r0:r0 + 35000] = A[r0:r0 + 35000].double() @ H.double().T
        assert torch.equal(out.double(), ref), "aht: first bad row %d" % int((out.double() != ref).any(1).nonzero()[0])
        ob = torch.full((lead + k * (n + 4) + guard,), ex.SENTINEL, device="cuda")
        out = ob.as_strided((k, n), (n + 4, 1), lead)
        ops.wta(A, W, out)
        _outside_untouched(ob, lead, n + 4, k, n, ex.SENTINEL, "wta output")
        ref = torch.zeros(k, n, dtype=torch.float64, device="cuda")
        for r0 in range(0, m, 35000):
            ref += W[r0:r0 + 35000].double().T @ A[r0:r0 + 35000].double()
        assert torch.equal(out.double(), ref), "wta: first bad column %d" % int((out.double() != ref).any(0).nonzero()[0])
        _outside_untouched(buf, lead, ld, m, n, float("nan"), "A")
    finally:
        del buf
        torch.cuda.empty_cache()


def test_column_slice_leaves_the_window(env):
    """A = the first 1000 columns of a 4096 x 2^20 buffer (rows 4 MiB apart, so a row chunk's window is far past 2 GiB;
    dnmf_host.h, plan_kl_wtu: kl_wtu's row chunks are sized from n, so such a slice "takes the slower path, correctly"): kl_wtu, kl_uht,
    aht and wta exact; the rest of the buffer is NaN"""
    engine, _ = env
    ops = engine.HIP_OPS
    m, n, k = 4096, 1000, 16
    big = torch.full((m, 1 << 20), float("nan"), dtype=torch.float32, device="cuda")
    try:
        A, W, H = ex.products(m, n, k)
        Av = big[:, :n]
        Av.copy_(_dev(A))
        A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
        o = _out(m, k)
        ops.aht(Av, _dev(H), o.view)
        ex.assert_ulp(o.check("aht"), A64 @ H64.T, 0, "aht (lda = 2^20)")
        o = _out(k, n)
        ops.wta(Av, _dev(W), o.view)
        ex.assert_ulp(o.check("wta"), W64.T @ A64, 0, "wta (lda = 2^20)")
        Ak, Wk, Hk, U = ex.kl(m, n, k)
        Av.copy_(_dev(Ak))
        o = _out(m, k)
        ops.kl_uht(Av, _dev(Wk), _dev(Hk), EPS, o.view)
        ex.assert_ulp(o.check("kl_uht"), U @ Hk.T.astype(np.float64), 0, "kl_uht (lda = 2^20)")
        o = _out(k, n)
        ops.kl_wtu(Av, _dev(Wk), _dev(Hk), EPS, o.view)
        ex.assert_ulp(o.check("kl_wtu"), Wk.T.astype(np.float64) @ U, 0, "kl_wtu (lda = 2^20)")
        _outside_untouched(big.view(-1), 0, 1 << 20, m, n, float("nan"), "A")
    finally:
        del big
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- multi-rank
@pytest.mark.parametrize("exchange", [None, "native-hosted"], ids=["choreography", "native-hosted"])
@pytest.mark.parametrize("grid,shape", [pytest.param((2, 1), (1000, 300, 12), id="1d-2x1"),
                                        pytest.param((2, 2), (700, 520, 17), id="2d-2x2")])
def test_multirank_step(grid, shape, exchange):
    """one step on a 1D and a 2D grid (tests/_mp.py run_exact): every rank's block against the whole-matrix exact reference -- the new
    W equal, the new H within 3 ulps -- through the Python choreography and through the library-sequenced step"""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tests._mp import run_exact
    run_exact(grid, shape, exchange)


# ------------------------------------------------------------------------------------------------------------- workspace state
def _scratch_runs(engine, fn):
    """fn() after filling every scratch buffer with 0xFF bytes (NaN as fp32), then after zeroing them: the same bits
    (engine._scratch: no entry point keeps state in the shared scratch between calls)"""
    fn()                                                                   # sizes the scratch
    outs = []
    for byte in (0xFF, 0):
        for ws in engine._ws_cache.values():
            ws.fill_(byte)
        for img in engine.HipOpsF64._img.values():
            img.fill_(float("nan") if byte else 0.0)
        outs.append([t.clone() for t in fn()])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.uint8) if a.dtype != torch.bfloat16 else a, b.view(torch.uint8) if b.dtype != torch.bfloat16 else b) \
            and not torch.isnan(a).any(), "the result depends on what the scratch held before the call"


@pytest.mark.parametrize("m,n,k", [(1000, 515, 17), (4096, 2048, 32), (300, 130, 5), (257, 256, 40)])
def test_scratch_holds_no_state(env, m, n, k):
    """(257, 256, 40) is a split shape of the bf16x6 entry points (n % 128 == 0, k > 32: the images and partial sums of ntx, tnx,
    klx_uht and klx_wtu live in the scratch); at (4096, 2048, 32) only the KL ones are"""
    engine, lib = env
    ops, o6, f64 = engine.HIP_OPS, engine.HIP_OPS_BF16X6, engine.HIP_OPS_F64
    A, W, H = (_dev(x) for x in ex.products(m, n, k))
    Ak, Wk, Hk = (_dev(x) for x in ex.kl(m, n, k)[:3])
    Af, Wf, Hf, _, _ = (_dev(x) for x in ex.fro_step(m, n, k))

    def step(o, fro, onepass=0):
        def f():
            was = lib.dnmf_set_onepass(onepass)
            try:
                W1, H1 = (Wf.clone(), Hf.clone()) if fro else (Wk.clone(), Hk.clone())
                (o.mu_fro_step if fro else o.mu_kl_step)(Af if fro else Ak, W1, H1, EPS, True, False)
                return W1, H1
            finally:
                lib.dnmf_set_onepass(was)
        return f

    cases = [lambda: [ops.wta(A, W, torch.empty(k, n, device="cuda"))],
             lambda: [ops.wta_gram(A, W, torch.empty(k, n, device="cuda"), engine.new_gram(k, A.device))],
             lambda: [ops.gram_hht(H, engine.new_gram(k, A.device)), ops.gram_wtw(W, engine.new_gram(k, A.device))],
             lambda: [ops.kl_uht(Ak, Wk, Hk, EPS, torch.empty(m, k, device="cuda")), ops.kl_wtu(Ak, Wk, Hk, EPS, torch.empty(k, n, device="cuda"))],
             lambda: [ops.colsum(W, torch.empty(k, device="cuda")), ops.resid_sqnorm(A, W, H)],
             lambda: [o6.aht(A, H, torch.empty(m, k, device="cuda")), o6.wta(A, W, torch.empty(k, n, device="cuda"))],
             lambda: [o6.kl_uht(Ak, Wk, Hk, EPS, torch.empty(m, k, device="cuda"))],
             lambda: [o6.kl_wtu(Ak, Wk, Hk, EPS, torch.empty(k, n, device="cuda"))],
             step(ops, True), step(ops, False), step(o6, True), step(o6, False)]
    if lib.dnmf_mu_fro_onepass(m, n, k) or m >= 4096:
        cases.append(step(ops, True, 2))
    Ad, Wd, Hd = (x.double() for x in (A, W, H))
    cases.append(lambda: [f64.wta(Ad, Wd, torch.empty(k, n, dtype=torch.float64, device="cuda")),
                          f64.kl_uht(Ak.double(), Wk.double(), Hk.double(), 1e-16, torch.empty(m, k, dtype=torch.float64, device="cuda"))])
    if lib.dnmf_mu_fit_persistent(m, n, k):
        def fit():
            W1, H1 = Wf.clone(), Hf.clone()
            ops.fit("mu", "fro", Af, W1, H1, EPS, True, 1)
            return W1, H1
        cases.append(fit)
    for fn in cases:
        _scratch_runs(engine, fn)
