"""Ranks 128 < k <= 256 against the exact answer, element by element, on the shapes that reach every class of the composition
(tests/_exact.py: WIDE_REACH; tests/test_dense_plan.py proves the reach without a GPU, tests/test_exact_cpu.py the operands).  A wide rank
runs the tuned kernels twice -- the second call at r = k - 128 on sub-views whose pitches and offsets no other caller produces -- four
times for a Gram, and the plain kernels of csrc/dnmf_wide.hip for what contracts over k.  Every case first asserts, through
dnmf_dense_plan at the pitches and addresses of the very views it passes, the launches it is named after (ex.wide_panel_plans derives the
panel calls as the entry points issue them); then it runs the entry point through engine.HIP_OPS and compares with numpy float64 element
by element.  Operands are views in NaN-poisoned buffers, outputs views in sentinel-filled buffers (ex.Poisoned), and the library's
workspace is filled with NaN bit patterns before every call that keeps an intermediate there (the quotient image U of the KL products),
so a tile that is left out cannot be covered by what an earlier call left behind.

Bounds, from the table at the top of tests/test_gpu_exact.py: products, Grams (with the zero padding of all 256 rows and columns), the
KL products on `kl` operands and the residual / column-error integers c = 0; MU updates c = 3; mu_fro_step on `fro_step` operands W
exact, H c = 3; mu_kl_step as tests/test_gpu_exact.py::test_kl holds it.  Whole fits on fixed points of the step (`fro_fixed`,
`kl_fixed`, `kl_moved`): the step bit for bit, the closing normalisation to the bound of tests/test_gpu_small_exact.py (one IEEE division,
one product: 1 ulp, exact where colsum(W) is a power of two), the whole-fit call and the step loop torch.equal."""
import functools

import numpy as np
import pytest

from tests import _exact as ex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.test_gpu_exact_dense import EPS, EPS32, _check_gram, _gram, _ids, _mu_ref, _out, _view, env  # noqa: E402,F401  (env: the fixture)


def _of(*ops):
    return _ids([c for c in ex.WIDE_REACH if c[1] in ops])


def _ws(engine, m, n, k, poison=True):
    """the workspace the engine will pass for an m x n block at rank k (one cached buffer per device and stream, grown on demand): its
    size, for the plans; filled with 0xFF bytes (NaN as float32) so that nothing an earlier call left there can stand in for work"""
    ws = engine.workspace(max(m, 1), max(n, 1), k, torch.device("cuda"))
    if poison:
        ws.fill_(255)
    return ws.numel()


def _assert_plans(case, views, ws_bytes):
    """the plans of the call about to be made, at the views' own pitches and addresses and the engine's own workspace"""
    wide, plans = ex.wide_case_plans(case, ws_bytes, [v.stride(-2) for v in views], [v.data_ptr() % 16 for v in views])
    ex.wide_assert_plans(case, wide, plans)


# ------------------------------------------------------------------------------------------------------------- the products and the Grams
@pytest.mark.parametrize("case", _of("aht"))
def test_aht(env, case):
    engine, lib_mod = env
    cid, op, m, n, k, aligned, bf16, want = case
    A, W, H, G = ex.dense_nt_operands(m, n, k)
    Av, Hv, o = _view(A, "A", aligned, bf16), _view(H, "H", aligned), _out(m, k, "AH", aligned)
    _assert_plans(case, [Av.view, Hv.view], None)
    engine.HIP_OPS.aht(Av.view, Hv.view, o.view)
    ex.assert_ulp(o.check(cid), A.astype(np.float64) @ H.astype(np.float64).T, 0, cid, tile=(128, 128))
    Av.check("A")
    Hv.check("H")


@pytest.mark.parametrize("case", _of("wta", "wta_gram"))
def test_wta(env, case):
    engine, lib_mod = env
    ops = engine.HIP_OPS
    cid, op, m, n, k, aligned, bf16, want = case
    A, W = ex.dense_tn_operands(m, n, k)
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    Av, Wv, o = _view(A, "A", aligned, bf16), _view(W, "W", aligned), _out(k, n, "AtW", aligned)
    _assert_plans(case, [Av.view, Wv.view, o.view], _ws(engine, m, n, k))
    if op == "wta":
        ops.wta(Av.view, Wv.view, o.view)
    else:
        Gd = _gram(engine, k)
        ops.wta_gram(Av.view, Wv.view, o.view, Gd)
        _check_gram(Gd, W64.T @ W64, k, cid + " Gram")
    ex.assert_ulp(o.check(cid), W64.T @ A64, 0, cid, tile=(128, 128))
    Av.check("A")
    Wv.check("W")


@pytest.mark.parametrize("case", _of("gram_hht", "gram_wtw"))
def test_grams(env, case):
    """the four block calls into the 256-pitch buffer: every element of the k x k Gram, and zeros in all 256 rows and columns beyond"""
    engine, lib_mod = env
    cid, op, m, n, k, aligned, bf16, want = case
    Gd = _gram(engine, k)
    assert tuple(Gd.shape) == (256, 256)
    if op == "gram_hht":
        F = np.ascontiguousarray(ex.dense_tn_operands(n, 1, k)[1].T)
        Fv = _view(F, "H", aligned)
        _assert_plans(case, [Fv.view], _ws(engine, k, n, k))
        engine.HIP_OPS.gram_hht(Fv.view, Gd)
        ref = F.astype(np.float64) @ F.astype(np.float64).T
    else:
        F = ex.dense_tn_operands(m, 1, k)[1]
        Fv = _view(F, "W", aligned)
        _assert_plans(case, [Fv.view], _ws(engine, m, k, k))
        engine.HIP_OPS.gram_wtw(Fv.view, Gd)
        ref = F.astype(np.float64).T @ F.astype(np.float64)
    _check_gram(Gd, ref, k, cid)
    Fv.check(op)


# ------------------------------------------------------------------------------------------------------------- the KL products
@functools.lru_cache(maxsize=2)
def _kl_problem(m, n, k):
    return ex.kl(m, n, k)


@pytest.mark.parametrize("case", _of("kl_uht", "kl_wtu"))
def test_kl_products(env, case):
    """wide_nn_rows_kernel<W_QUOT> into the quotient image, then the two panels on it: exactly float64 on operands with an exact quotient"""
    engine, lib_mod = env
    cid, op, m, n, k, aligned, bf16, want = case
    A, W, H, U = _kl_problem(m, n, k)
    Av, Wv, Hv = _view(A, "A", aligned), _view(W, "W", aligned), _view(H, "H", aligned)
    if op == "kl_wtu":
        o, ref = _out(k, n, "WTU", aligned), W.astype(np.float64).T @ U
    else:
        o, ref = _out(m, k, "UHT", aligned), U @ H.astype(np.float64).T
    _assert_plans(case, [Av.view, Wv.view, Hv.view, o.view], _ws(engine, m, n, k))
    getattr(engine.HIP_OPS, op)(Av.view, Wv.view, Hv.view, EPS, o.view)
    ex.assert_ulp(o.check(cid), ref, 0, cid, tile=(16, 16))
    for v, what in ((Av, "A"), (Wv, "W"), (Hv, "H")):
        v.check(what)


# ------------------------------------------------------------------------------------------------------------- residual, column error
@pytest.mark.parametrize("case", _of("resid_sqnorm", "column_err"))
def test_residual_sums(env, case):
    """wide_nn_rows_kernel<W_SQSUM | W_COLERR>: the float64 integers.  column_err accumulates by contract (the caller zeroes, or keeps
    adding row blocks): the entry point is also started from nonzero integers in num / den and must return the sum"""
    engine, lib_mod = env
    ops = engine.HIP_OPS
    cid, op, m, n, k, aligned, bf16, want = case
    A, W, H, R = ex.dense_resid_operands(m, n, k, whole=op == "resid_sqnorm", sum_dtype=np.float64)
    Av, Wv, Hv = _view(A, "A", aligned), _view(W, "W", aligned), _view(H, "H", aligned)
    _assert_plans(case, [Av.view, Wv.view, Hv.view], _ws(engine, m, n, k))
    if op == "resid_sqnorm":
        got = float(ops.resid_sqnorm(Av.view, Wv.view, Hv.view).item())
        assert got == float((R ** 2).sum()), "%s: %r, expected %r" % (cid, got, float((R ** 2).sum()))
    else:
        rnum, rden = (R ** 2).sum(0), (A.astype(np.float64) ** 2).sum(0)
        num, den = ops.column_err_sums(Av.view, Wv.view, Hv.view)
        ex.assert_ulp(num.cpu().numpy(), rnum, 0, cid + " num", tile=(1, 16))
        ex.assert_ulp(den.cpu().numpy(), rden, 0, cid + " den", tile=(1, 16))
        n0, d0 = 3.0 + np.arange(n) % 7, 5.0 + np.arange(n) % 11
        acc = torch.full((2, n + 2), ex.SENTINEL, dtype=torch.float64, device="cuda")
        acc[0, :n], acc[1, :n] = torch.from_numpy(n0).cuda(), torch.from_numpy(d0).cuda()
        lib_mod.check(lib_mod.lib.dnmf_column_err(Av.view.data_ptr(), m, n, Av.view.stride(0), Wv.view.data_ptr(), Wv.view.stride(0),
                                                  Hv.view.data_ptr(), Hv.view.stride(0), k, acc[0].data_ptr(), acc[1].data_ptr(), engine._stream()))
        got = acc.cpu().numpy()
        ex.assert_ulp(got[0, :n], n0 + rnum, 0, cid + " num, accumulated", tile=(1, 16))
        ex.assert_ulp(got[1, :n], d0 + rden, 0, cid + " den, accumulated", tile=(1, 16))
        assert (got[:, n:] == ex.SENTINEL).all(), cid + ": written past the n columns"
    for v, what in ((Av, "A"), (Wv, "W"), (Hv, "H")):
        v.check(what)


# ------------------------------------------------------------------------------------------------------------- the MU updates
@pytest.mark.parametrize("case", _of("mu_update_w"))
def test_mu_update_w(env, case):
    engine, lib_mod = env
    cid, op, m, n, k, aligned, bf16, want = case
    X, S, G = ex.dense_update_operands(m, k)
    Wv, Sv = _view(X, "W", aligned), _view(S, "AH", aligned)
    _assert_plans(case, [Wv.view, Sv.view], None)
    engine.HIP_OPS.mu_update_w(Wv.view, Sv.view, _gram(engine, k, G), EPS)
    X64 = X.astype(np.float64)
    ex.assert_ulp(Wv.check(cid), _mu_ref(X64, S.astype(np.float64), X64 @ G), 3, cid, tile=(16, 16))
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
    for clamp in (False, True):
        Hv = _view(H, "H", aligned)
        _assert_plans(case, [Hv.view, Sv.view], None)
        engine.HIP_OPS.mu_update_h(Hv.view, Sv.view, Gd, EPS, clamp)
        ex.assert_ulp(Hv.check(cid), _mu_ref(H64, AtW.astype(np.float64), G @ H64, clamp), 3, "%s clamp=%s" % (cid, clamp), tile=(16, 16))
    Sv.check("AtW")


# ------------------------------------------------------------------------------------------------------------- whole steps
STEP_CASES = [(300, 320, 130, True), (300, 320, 144, True), (300, 320, 161, False), (300, 320, 255, False)]


@pytest.mark.parametrize("m,n,k,aligned", STEP_CASES, ids=lambda v: str(v))
def test_mu_fro_step(env, m, n, k, aligned):
    """mu_fro_step on `fro_step` operands (H H^T, A H^T, the wide W update, W^T W with W^T A, the wide H update, the clamp): the new W
    exact, the new H c = 3; fp32 and bf16-stored A, clamp off and on"""
    engine, lib_mod = env
    A, W, H, Wn, Hq = ex.fro_step(m, n, k)
    for bf16 in (False, True):
        for clamp in (False, True):
            what = "mu_fro_step k=%d %s clamp=%s" % (k, "bf16" if bf16 else "f32", clamp)
            Av, Wv, Hv = _view(A, "A", aligned, bf16), _view(W, "W", aligned), _view(H, "H", aligned)
            _ws(engine, m, n, k)
            engine.HIP_OPS.mu_fro_step(Av.view, Wv.view, Hv.view, EPS, True, clamp)
            ex.assert_ulp(Wv.check(what + " W"), np.maximum(Wn, EPS32) if clamp else Wn, 0, what + " W (exact)")
            ex.assert_ulp(Hv.check(what + " H"), np.maximum(Hq, EPS32) if clamp else Hq, 3, what + " H")
            Av.check("A")


@pytest.mark.parametrize("m,n,k,aligned", [(300, 256, 132, True), (261, 331, 131, False), (261, 331, 193, False), (300, 256, 255, True)],
                         ids=lambda v: str(v))
def test_mu_kl_step(env, m, n, k, aligned):
    """mu_kl_step as tests/test_gpu_exact.py::test_kl holds it: W fixed -- H c = 3, W untouched; W and H -- W c = 3, H (from the kernel's new
    W, whose quotient is no longer exact) 1e-5 of each element"""
    engine, lib_mod = env
    ops = engine.HIP_OPS
    A, W, H, U = _kl_problem(m, n, k)
    UHt, WtU, rs, cs, Wq, Hq = ex.kl_refs(A, W, H, U)
    Av = _view(A, "A", aligned)
    W3, H3 = _view(W, "W", aligned), _view(H, "H", aligned)
    _ws(engine, m, n, k)
    ops.mu_kl_step(Av.view, W3.view, H3.view, EPS, False, False)
    ex.assert_ulp(H3.check("mu_kl_step H"), Hq, 3, "mu_kl_step (W fixed) H")
    ex.assert_ulp(W3.check("mu_kl_step W"), W.astype(np.float64), 0, "mu_kl_step (W fixed) W")
    W4, H4 = _view(W, "W", aligned), _view(H, "H", aligned)
    _ws(engine, m, n, k)
    ops.mu_kl_step(Av.view, W4.view, H4.view, EPS, True, False)
    Wn = W4.check("mu_kl_step W")
    ex.assert_ulp(Wn, Wq, 3, "mu_kl_step W")
    Wn64 = Wn.astype(np.float64)
    Un = A.astype(np.float64) / (Wn64 @ H.astype(np.float64) + EPS)
    Hn = H.astype(np.float64) * (Wn64.T @ Un) / (Wn64.sum(0) + EPS)[:, None]
    h = H4.check("mu_kl_step H")
    ok = np.abs(h - Hn) <= 1e-5 * np.abs(Hn)
    assert ok.all(), "mu_kl_step H off by more than 1e-5 at %s" % (tuple(np.argwhere(~ok)[0]),)
    Av.check("A")


# ------------------------------------------------------------------------------------------------------------- whole fits on fixed points
FIT_GEN = {"fro": ex.fro_fixed, "kl": ex.kl_fixed, "kl_wfixed": ex.kl_moved}


@functools.lru_cache(maxsize=None)
def _fixed(family, k, seed):
    return FIT_GEN[family](*ex.WIDE_FIT_SHAPE, k, seed=seed)


def _check_fixed(family, k, prob, w, h, what, sq=None):
    """the fit returned normalize_features of the fixed point (tests/test_gpu_small_exact.py: W / s and H s within 1 ulp, exact where
    s = colsum(W) is a power of two), so every one of its steps returned its input bit for bit"""
    A64, W64, H64 = (x.astype(np.float64) for x in prob)
    if family == "kl_wfixed":
        H64 = 2 * H64                                               # step 0 doubles H, every later step keeps it
    s = W64.sum(0)
    pow2 = bool(np.all(np.frexp(s)[0] == 0.5))
    assert pow2 or family == "fro"
    c = 0 if pow2 else 1
    ex.assert_ulp(w, W64 / s[None, :], c, what + " W = W / colsum(W)")
    ex.assert_ulp(h, H64 * s[:, None], c, what + " H = H colsum(W)")
    if sq is not None:
        sa = float((A64 ** 2).sum())
        assert sq[1] == sa, "%s: sum A^2 is %r, expected %r" % (what, sq[1], sa)
        lim = 0.0 if pow2 else ((k + 4) * 2.0 ** -24) ** 2 * sa
        assert 0.0 <= sq[0] <= lim, "%s: sum (A - W H)^2 is %r, at most %r expected" % (what, sq[0], lim)


def _args(k, itr, norm, **kw):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.utils import parse
    comms = MPI_comm(None, 1, 1)
    args = parse()
    args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, 1, 1, k
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    args.itr, args.init, args.verbose, args.prune = itr, "rand", False, False
    args.norm, args.method, args.W_update = norm, "mu", True
    for key, v in kw.items():
        setattr(args, key, v)
    return args


@pytest.mark.parametrize("itr", ex.WIDE_FIT_STEPS)
@pytest.mark.parametrize("k", ex.WIDE_FIT_KS)
@pytest.mark.parametrize("family", sorted(FIT_GEN))
def test_whole_fits_stay_on_their_fixed_points(env, family, k, itr):
    """dnmf_mu_fro_fit / dnmf_mu_kl_fit (and the latter with W fixed on `kl_moved`) at a wide rank, for 1, 11 and 12 steps (clamps at
    steps 0 and 10): one problem and a batch of two different ones through the entry point on poisoned views, then through PyNMF with
    fit_loop = 'native' and 'python' and through PyNMF.fit_batch -- all held to the fixed point, the two loops and the batch bit-equal"""
    from pydnmfk_amd.pyDNMF import PyNMF
    engine, lib_mod = env
    ops = engine.HIP_OPS
    norm, wu = ("fro" if family == "fro" else "kl"), family != "kl_wfixed"
    probs = [_fixed(family, k, seed) for seed in (0, 1)]
    assert not np.array_equal(probs[0][1], probs[1][1])
    what = "%s k=%d itr=%d" % (family, k, itr)
    for B in (1, 2):                                                 # the entry point itself: matrices, then a stack of two
        P = [ex.Poisoned(torch, np.stack([p[i] for p in probs]) if B > 1 else probs[0][i]) for i in range(3)]
        sq = ops.fit("mu", norm, P[0].view, P[1].view, P[2].view, EPS, wu, itr).cpu().numpy()
        P[0].check(what + " A")
        w3, h3 = P[1].check(what + " W"), P[2].check(what + " H")
        if B == 1:
            w3, h3 = w3[None], h3[None]
        for b in range(B):
            _check_fixed(family, k, probs[b], w3[b], h3[b], "%s batch=%d [%d]" % (what, B, b), sq[b])
    dev = [tuple(torch.from_numpy(x).cuda() for x in p) for p in probs]
    res = {}
    for loop in ("native", "python"):
        f = PyNMF(dev[0][0], factors=[dev[0][1], dev[0][2]], params=_args(k, itr, norm, W_update=wu, fit_loop=loop))
        assert f._whole_fit_ok(f._ops()) == (loop == "native")
        res[loop] = f.fit()
        _check_fixed(family, k, probs[0], res[loop][0].cpu().numpy(), res[loop][1].cpu().numpy(), "%s PyNMF %s" % (what, loop))
    assert torch.equal(res["native"][0], res["python"][0]) and torch.equal(res["native"][1], res["python"][1]), what + ": the two loops differ"
    fits = [PyNMF(A, factors=[W0, H0], params=_args(k, itr, norm, W_update=wu)) for A, W0, H0 in dev]
    batched = PyNMF.fit_batch(fits)
    assert getattr(fits[0], "_stack", None) is not None and fits[0]._stack.shape[0] == 2      # it did run as ONE batch
    assert torch.equal(batched[0][0], res["native"][0]) and torch.equal(batched[0][1], res["native"][1]), what + ": the batch differs"
    for b in range(2):
        _check_fixed(family, k, probs[b], batched[b][0].cpu().numpy(), batched[b][1].cpu().numpy(), "%s fit_batch [%d]" % (what, b))
