"""Every entry point that takes `(ws, ws_bytes)` held to the workspace contract of include/dnmf.h -- size, state, bounds.

`engine._scratch` and `NativeComm._workspace` hand ONE cached buffer, with its whole length as `ws_bytes`, to every operator family in
turn: the buffer is as large as the biggest problem the process has seen and holds what the last call left.  Here each case runs under
tests/_ws.py::GuardedScratch instead: a view of EXACTLY the size the engine asked for between two sentinel bands, filled before every
request with 0xFF (NaN, all-ones tags), 0x00, 0x7F (3.39e38, a tag larger than any real one) or left as a call of ANOTHER family left
it, then once more four times as large (a buffer "left by a bigger problem") and, for the families whose entry points check
aligned16(ws), once at a base that is 16-byte but not 32-byte aligned.  Every run asserts
  (a) both bands are untouched;
  (b) the result meets the case's reference -- the exact generator and ulp table of the family's own exact test (tests/_exact.py,
      tests/_is.py, tests/_masked_dense.py, ...): no tolerance is new here;
  (c) all runs are bit-identical (uint8 views);
  (d) the recorder saw every C entry point the case names;
and that every run asked the same sequence of sizes (the queries of include/dnmf.h, asserted where the case names them).

The case table (CASES; tests/test_workspace_cpu.py holds it to _lib.SIGNATURES: no launching entry point is left out):
  dense-*        fp32 dense products, steps and their bf16-stored twins at (300, 130, 5), (1000, 515, 17), the first DENSE_KL entry
                 whose plan has mode == 1 (padded images in the workspace), the first DENSE_TN entry with a two-stage reduction and
                 the first DENSE_RESID entry that uses the workspace (no entry has reduce != "none": the first with mode == 1)
  hblocks        kl_uht_hblocks on its own query at the first hblocks entry of DENSE_KL
  wide-*         (300, 700, 129), (515, 333, 256): U at the END of the workspace
  onepass        the team step at the smallest one-pass shape, dnmf_set_onepass(2)
  x6             the eleven *_bf16x6 entry points at (257, 256, 40) on split operands
  hals-*         hals_update_w (the k sums of squares are read back FROM the workspace) on the first persistent and the first
                 column-launch entry of HALS_W_CASES; one whole step of the one-rank route
  fit-*          mu_fro / mu_kl / hals_fro fits and the bf16 twins, 12 steps: the first SMALL_REACH entry with two workgroups per
                 problem -- persistent, as a launch chain, as a batch of 3.  (The two squared norms a fit returns end in float64
                 atomics whose order is free: they are held to the reference in (b) and left out of (c).)
  bcd-*          bcd_update_w at BCD_COLSUM[0]; bcd_fro_fit at the smallest entry of FITS, single and batch 3 -- against the numpy
                 checker at the project's fit tolerances, W and H bit-identical over the runs
  f64-*          the float64 products, sums and the HALS column kernel at (257, 600, 15), (513, 129, 65); f64_fit tiny and chain
  csr-*          the LENS x LENS_N pattern at k = 3, 17, 256 on the block and the transposed block
  masked-*       masked dense pairs, fused updates (within an ulp of x * (num / (den + eps)) from the pair: the family's checker),
                 column error and a 12-step fit against the float64 statement
  is-*           Itakura-Saito pairs (exact), updates and divergence (1e-5 of float64: tests/test_gpu_is.py), the exact column
                 divergence and a 12-step fit
  grid-*         Position of tests/test_gpu_grid_workspace.py at 3x1, 1x3, 2x2-ragged, 2x3: fro, kl, hals, fro / hals with bf16 A.  No
                 exact answer exists for these (the recording collective is not an exchange): (b) is the bit-comparison with the run
                 on a zeroed workspace of exactly the query, which (c) contains.  The allgather of the stand-in gives every OTHER
                 member a fully written block (PeersPosition below): copying this member's block everywhere, as Position does, lets
                 a ragged grid read the pad of this rank's own send block, which no rank of a real exchange reads.

Measured on one MI355X, the whole file in one pytest run: 62 cases in 6.2 s; the slowest calls are dense-300x130-k5 (0.56 s, it loads the
library), csr-k3-A (0.51 s), the two csr-k256 cases (0.32 s each) and x6 (0.24 s); every other case takes 0.14 s or less."""
import ctypes
import functools

import numpy as np
import pytest

from tests import _exact as ex
from tests import _ws

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
EPS32 = np.float32(EPS)
E64 = 2.220446049250313e-16
RUNS = [(0xFF, 0, 512), (0x00, 0, 512), (0x7F, 0, 512), ("leftover", 0, 512), (0xFF, _ws.bigger, 512)]
ALIGN16 = (0xFF, 0, 512 + 16)


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pydnmfk_amd import engine
    from pydnmfk_amd._lib import lib
    torch.cuda.set_device(0)
    return engine, lib


class Case:
    """names: the C entry points the case must reach; make(engine, lib) -> Prob; align16: one more run at lead = 512 + 16; waits: the
    case runs kernels whose workgroups wait for each other (hals_check after every run); query(lib) -> the sizes the engine may ask"""

    def __init__(self, id, names, make, align16=False, waits=False, query=None):
        self.id, self.names, self.make, self.align16, self.waits, self.query = id, tuple(names), make, align16, waits, query


class Prob:
    """run() -> list of numpy arrays (fresh outputs every call); verify(arrays, what) asserts them against the reference; free: the
    indices of the outputs that are held to the reference only, not bit-compared over the runs"""

    def __init__(self, run, verify, close=None, free=()):
        self.run, self.verify, self.close, self.free = run, verify, close, frozenset(free)


def _P(x, aligned=True, dtype=None, **kw):
    return ex.Poisoned(torch, x, dtype=dtype, aligned=aligned, **kw)


def _out(rows, cols, aligned=True, dtype=torch.float32):
    return ex.Poisoned.out(torch, rows, cols, dtype, aligned)


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().to(dtype)


def _gram(engine, k, g=None, dtype=torch.float32):
    """a KP x KP Gram buffer: filled with 7 (an output) or holding g zero-padded (an operand)"""
    G = engine.new_gram(k, torch.device("cuda")).to(dtype)
    if g is None:
        G.fill_(7.0)
    else:
        G[:k, :k] = _dev(g, dtype)
    return G


def _check_gram(g, ref, k, what):
    ex.assert_ulp(g[:k, :k], ref, 0, what)
    assert not g[k:].any() and not g[:, k:].any(), "%s: the zero padding of the Gram was not written" % what


def _mu_ref(X, S, D, clamp=False):
    q = np.where(D > 0, X * S / np.where(D > 0, D, 1.0), 0.0)
    return np.maximum(q, EPS32) if clamp else q


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Steps:
    """a case as a list of (label, call() -> array or tuple of arrays, check(arrays..., what)): run() calls them in order"""

    def __init__(self):
        self.items = []

    def add(self, label, call, check):
        self.items.append((label, call, check))

    def prob(self, close=None):
        def run():
            out = []
            for _, call, _c in self.items:
                r = call()
                out.append(tuple(r) if isinstance(r, (tuple, list)) else (r,))
            return [a for r in out for a in r]

        def verify(arrays, what):
            arrays = list(arrays)
            for label, call, check in self.items:
                n = getattr(call, "nout", 1)
                check(*arrays[:n], "%s: %s" % (what, label))
                del arrays[:n]
            assert not arrays
        free, at = [], 0
        for _, call, _c in self.items:
            free += [at + i for i in getattr(call, "free", ())]
            at += getattr(call, "nout", 1)
        return Prob(run, verify, close, free)


def _nout(n):
    def deco(f):
        f.nout = n
        return f
    return deco


def _within_1e5(got, ref, what):
    bad = ~(np.abs(got - ref) <= 1e-5 * np.abs(ref))
    assert not bad.any(), "%s off by more than 1e-5 at %s" % (what, tuple(np.argwhere(bad)[0]))


# ------------------------------------------------------------------------------------------------------------- fp32 dense
def _dense_steps(engine, lib, ops, m, n, k, which, gen="products", bf16=True, onepass=None):
    """the steps of a dense case.  which: names of gram_hht gram_wtw wta wta_gram colsum kl kl_step fro_step resid.  gen: the generator of
    the product operands ("products", "tn": A and W only, "resid": dense_resid_operands for the residual).  Bounds: the table at the top
    of tests/test_gpu_exact.py"""
    S = Steps()
    adts = (torch.float32, torch.bfloat16) if bf16 else (torch.float32,)
    if {"gram_hht", "gram_wtw", "wta", "wta_gram", "colsum"} & set(which):
        if gen == "tn":
            A, W = ex.dense_tn_operands(m, n, k)
            H = None
        else:
            A, W, H = ex.products(m, n, k)
        A64, W64 = A.astype(np.float64), W.astype(np.float64)
        Wv = _P(W)
        Av = {adt: _P(A, True, adt) for adt in adts}
        if "gram_hht" in which:
            Hv, H64 = _P(H), H.astype(np.float64)
            S.add("gram_hht", lambda: ops.gram_hht(Hv.view, _gram(engine, k)).cpu().numpy(), lambda g, w: _check_gram(g, H64 @ H64.T, k, w))
        if "gram_wtw" in which:
            S.add("gram_wtw", lambda: ops.gram_wtw(Wv.view, _gram(engine, k)).cpu().numpy(), lambda g, w: _check_gram(g, W64.T @ W64, k, w))
        if "colsum" in which:
            S.add("colsum", lambda: ops.colsum(Wv.view, torch.full((k,), 7.0, device="cuda")).cpu().numpy(),
                  lambda x, w: ex.assert_ulp(x, W64.sum(0), 0, w))
        for adt in adts:
            if "wta" in which:
                def wta(adt=adt):
                    o = _out(k, n)
                    ops.wta(Av[adt].view, Wv.view, o.view)
                    return o.check("wta")
                S.add("wta %s" % adt, wta, lambda x, w: ex.assert_ulp(x, W64.T @ A64, 0, w))
            if "wta_gram" in which:
                @_nout(2)
                def wta_gram(adt=adt):
                    o, G = _out(k, n), _gram(engine, k)
                    ops.wta_gram(Av[adt].view, Wv.view, o.view, G)
                    return o.check("wta_gram"), G.cpu().numpy()

                def chk(x, g, w):
                    ex.assert_ulp(x, W64.T @ A64, 0, w + " product")
                    _check_gram(g, W64.T @ W64, k, w + " Gram")
                S.add("wta_gram %s" % adt, wta_gram, chk)
    if {"kl", "kl_step"} & set(which):
        Ak, Wk, Hk, U = ex.kl(m, n, k)
        UHt, WtU, _, _, Wq, Hq = ex.kl_refs(Ak, Wk, Hk, U)
        Akv, Wkv, Hkv = _P(Ak), _P(Wk), _P(Hk)
        if "kl" in which:
            def uht():
                o = _out(m, k)
                ops.kl_uht(Akv.view, Wkv.view, Hkv.view, EPS, o.view)
                return o.check("kl_uht")

            def wtu():
                o = _out(k, n)
                ops.kl_wtu(Akv.view, Wkv.view, Hkv.view, EPS, o.view)
                return o.check("kl_wtu")
            S.add("kl_uht", uht, lambda x, w: ex.assert_ulp(x, UHt, 0, w))
            S.add("kl_wtu", wtu, lambda x, w: ex.assert_ulp(x, WtU, 0, w))
        if "kl_step" in which:
            @_nout(2)
            def kl_step():
                W4, H4 = _P(Wk), _P(Hk)
                ops.mu_kl_step(Akv.view, W4.view, H4.view, EPS, True, False)
                return W4.check("mu_kl_step W"), H4.check("mu_kl_step H")

            def chk_kl(Wn, h, w):
                ex.assert_ulp(Wn, Wq, 3, w + " W")
                Wn64 = Wn.astype(np.float64)
                Un = Ak.astype(np.float64) / (Wn64 @ Hk.astype(np.float64) + EPS)
                _within_1e5(h, Hk.astype(np.float64) * (Wn64.T @ Un) / (Wn64.sum(0) + EPS)[:, None], w + " H")
            S.add("mu_kl_step", kl_step, chk_kl)
    if "fro_step" in which:
        Af, Wf, Hf, Wn, Hq2 = ex.fro_step(m, n, k)
        Afv = {adt: _P(Af, True, adt) for adt in adts}
        for adt in adts:
            @_nout(2)
            def fro(adt=adt):
                Wv2, Hv2 = _P(Wf), _P(Hf)
                was = lib.dnmf_set_onepass(onepass) if onepass is not None else None
                try:
                    if onepass == 2:
                        assert lib.dnmf_mu_fro_onepass(m, n, k) == 1
                    ops.mu_fro_step(Afv[adt].view, Wv2.view, Hv2.view, EPS, True, False)
                finally:
                    if was is not None:
                        lib.dnmf_set_onepass(was)
                return Wv2.check("mu_fro_step W"), Hv2.check("mu_fro_step H")

            def chk_fro(w_, h_, w):
                ex.assert_ulp(w_, Wn, 0, w + " W (exact)")
                ex.assert_ulp(h_, Hq2, 3, w + " H")
            S.add("mu_fro_step %s" % adt, fro, chk_fro)
    if "resid" in which:
        if gen == "resid":
            A2, Wr, Hr, R = ex.dense_resid_operands(m, n, k)
        else:
            _, Wr, Hr = ex.products(m, n, k)
            R = np.random.RandomState(m + k).randint(0, 3, size=(m, n)).astype(np.float64)
            A2 = (Wr.astype(np.float64) @ Hr.astype(np.float64) + R).astype(np.float32)
        want = float((R ** 2).sum())
        Wrv, Hrv = _P(Wr), _P(Hr)

        def chk_resid(x, w):
            assert float(x[0]) == want, "%s: %r, expected %r" % (w, float(x[0]), want)
        for adt in adts if A2.max() <= 256 else (torch.float32,):
            A2v = _P(A2, True, adt)
            S.add("resid_sqnorm %s" % adt, lambda A2v=A2v: ops.resid_sqnorm(A2v.view, Wrv.view, Hrv.view).cpu().numpy(), chk_resid)
    return S


DENSE_ALL = ("gram_hht", "gram_wtw", "wta", "wta_gram", "colsum", "kl", "kl_step", "fro_step", "resid")
DENSE_NAMES = {"gram_hht": ("dnmf_gram_hht",), "gram_wtw": ("dnmf_gram_wtw",), "wta": ("dnmf_wta", "dnmf_wta_bf16a"),
               "wta_gram": ("dnmf_wta_gram", "dnmf_wta_gram_bf16a"), "colsum": ("dnmf_colsum",), "kl": ("dnmf_kl_uht", "dnmf_kl_wtu"),
               "kl_step": ("dnmf_mu_kl_step",), "fro_step": ("dnmf_mu_fro_step", "dnmf_mu_fro_step_bf16a"),
               "resid": ("dnmf_resid_sqnorm_ws", "dnmf_resid_sqnorm_ws_bf16a")}


def _dense_query(m, n, k, which):
    def query(lib):
        q = set()
        if set(which) - {"gram_hht", "gram_wtw", "colsum"}:
            q.add(lib.dnmf_ws_bytes(m, n, k))
        if "gram_hht" in which:
            q.add(lib.dnmf_ws_bytes(k, n, k))
        if {"gram_wtw", "colsum"} & set(which):
            q.add(lib.dnmf_ws_bytes(m, k, k))
        return q
    return query


def dense(id, m, n, k, which, gen="products", bf16=True, onepass=None, waits=False):
    names = [x for w in which for x in DENSE_NAMES[w] if bf16 or not x.endswith("_bf16a")]
    return Case(id, names, lambda engine, lib: _dense_steps(engine, lib, engine.HIP_OPS, m, n, k, which, gen, bf16, onepass).prob(),
                waits=waits, query=_dense_query(m, n, k, which))


def _first(table, pred):
    """the first entry of a reach table of tests/_exact.py whose PLAN (dnmf_dense_plan on the views the table describes) meets pred"""
    from pydnmfk_amd import _lib
    for e in table:
        ld, off = ex.dense_plan_args(e[1], e[2], e[3], e[4], e[5], e[6])
        if pred(e, _lib.dense_plan(e[1], e[2], e[3], e[4], ld, off, bf16a=e[6])):
            return e
    return None


def _dense_cases():
    cases = [dense("dense-300x130-k5", 300, 130, 5, DENSE_ALL), dense("dense-1000x515-k17", 1000, 515, 17, DENSE_ALL)]
    e = _first(ex.DENSE_KL, lambda e, p: e[1] in ("kl_uht", "kl_wtu") and p["mode"] == 1)
    cases.append(dense("dense-kl-padded-images-%s" % e[0], e[2], e[3], e[4], ("kl", "kl_step"), bf16=False))
    e = _first(ex.DENSE_TN, lambda e, p: p["reduce"] == "two_stage")
    cases.append(dense("dense-tn-two-stage-%s" % e[0], e[2], e[3], e[4], ("wta", "wta_gram", "gram_wtw", "colsum"), gen="tn"))
    # (no entry of DENSE_RESID has a reduction: the residual ends in float64 atomics.  What it keeps in the workspace are the zero-padded
    # factor images of a ragged rank, mode == 1)
    e = _first(ex.DENSE_RESID, lambda e, p: p["reduce"] != "none") or _first(ex.DENSE_RESID, lambda e, p: e[1] == "resid_sqnorm" and p["mode"] == 1)
    cases.append(dense("dense-resid-%s" % e[0], e[2], e[3], e[4], ("resid",), gen="resid"))
    for m, n, k in ((300, 700, 129), (515, 333, 256)):
        cases.append(dense("wide-%dx%d-k%d" % (m, n, k), m, n, k, ("kl", "gram_wtw", "fro_step", "kl_step", "resid"), bf16=False))
    m, n, k = 4096, 2048, 32                               # the smallest one-pass case of tests/test_gpu_exact.py (ONEPASS)
    cases.append(dense("onepass-%dx%d-k%d" % (m, n, k), m, n, k, ("fro_step",), onepass=2, waits=True))
    return cases


def _hblocks_case():
    e = next(e for e in ex.DENSE_KL if e[1] == "kl_uht_hblocks")
    m, n, k, nh = e[2], e[3], e[4], ex.DENSE_HBLK

    def make(engine, lib):
        A, W, H, U = ex.kl(m, n, k)
        Hs = _P(H.reshape(k, n // nh, nh).transpose(1, 0, 2), packed=True)
        Av, Wv = _P(A), _P(W)
        S = Steps()

        def call():
            o = _out(m, k)
            engine.HIP_OPS.kl_uht_hblocks(Av.view, Wv.view, Hs.view, EPS, o.view)
            return o.check("kl_uht_hblocks")
        S.add("kl_uht_hblocks", call, lambda x, w: ex.assert_ulp(x, U @ H.T.astype(np.float64), 0, w))
        return S.prob()
    return Case("hblocks-%s" % e[0], ("dnmf_kl_uht_hblocks",), make, query=lambda lib: {lib.dnmf_ws_bytes_hblocks(m, n, k, nh)})


# ------------------------------------------------------------------------------------------------------------- bf16x6
X6_NAMES = ["dnmf_%s%s_bf16x6" % (op, a) for op in ("aht", "wta", "aht_update_w", "mu_fro_step") for a in ("", "_bf16a")] + \
           ["dnmf_kl_uht_bf16x6", "dnmf_kl_wtu_bf16x6", "dnmf_mu_kl_step_bf16x6"]


def _x6_case():
    m, n, k = 257, 256, 40

    def make(engine, lib):
        o6 = engine.HIP_OPS_BF16X6
        S = Steps()

        def _A(x, b):
            return ex.Poisoned(torch, x, dtype=torch.bfloat16 if b else torch.float32, quantum=8 if b else 4)
        rs = np.random.RandomState(m + n + k)
        G = ex._sym_gram(k, rs)
        Wi = rs.randint(1, 4, size=(m, k)).astype(np.float32)
        Wi[rs.rand(m) < 0.05] = 0
        Gd = _gram(engine, k, G)
        for b in (False, True):
            A, H = ex.pieces_product(m, n, k, "aht", bf16a=b)
            Av, Hv = _A(A, b), _P(H)
            plan = (ctypes.c_long * 12)()
            assert lib.dnmf_bf16x6_plan(m, n, k, Av.view.stride(0), int(b), int(Av.view.data_ptr() % 16 == 0), plan) == 0 and plan[0] == 1
            assert b or plan[1] == 1, "not a split shape of the KL kernels"

            def aht(Av=Av, Hv=Hv):
                o = _out(m, k)
                o6.aht(Av.view, Hv.view, o.view)
                return o.check("aht")
            S.add("aht bf16a=%d" % b, aht, lambda x, w, A=A, H=H: ex.assert_ulp(x, ex._mm(A, H, "aht"), 0, w, tile=(32, 32)))

            def fused(Av=Av, Hv=Hv):
                Wv = _P(Wi)
                o6.aht_update_w(Av.view, Hv.view, Gd, Wv.view, EPS)
                return Wv.check("aht_update_w")
            S.add("aht_update_w bf16a=%d" % b, fused,
                  lambda x, w, A=A, H=H: ex.assert_ulp(x, _mu_ref(Wi.astype(np.float64), ex._mm(A, H, "aht"), Wi.astype(np.float64) @ G), 3, w, tile=(32, 32)))
            A2, W2 = ex.pieces_product(m, n, k, "wta", bf16a=b)
            A2v, W2v = _A(A2, b), _P(W2)

            def wta(A2v=A2v, W2v=W2v):
                o = _out(k, n)
                o6.wta(A2v.view, W2v.view, o.view)
                return o.check("wta")
            S.add("wta bf16a=%d" % b, wta, lambda x, w, A2=A2, W2=W2: ex.assert_ulp(x, ex._mm(A2, W2, "wta"), 0, w, tile=(32, 32)))
        Af, Wf, Hf, Wn, Hq = ex.fro_step(m, n, k)
        for b in (False, True):
            Afv = _A(Af, b)

            @_nout(2)
            def fro(Afv=Afv):
                Wv, Hv = _P(Wf), _P(Hf)
                o6.mu_fro_step(Afv.view, Wv.view, Hv.view, EPS, True, False)
                return Wv.check("W"), Hv.check("H")

            def chk(w_, h_, w):
                ex.assert_ulp(w_, Wn, 0, w + " W (exact)", tile=(32, 32))
                ex.assert_ulp(h_, Hq, 3, w + " H", tile=(32, 32))
            S.add("mu_fro_step bf16a=%d" % b, fro, chk)
        Ak, Wk, Hk, U = ex.kl_pieces(m, n, k, "wh")
        Akv, Wkv, Hkv = _A(Ak, False), _P(Wk), _P(Hk)

        def uht():
            o = _out(m, k)
            o6.kl_uht(Akv.view, Wkv.view, Hkv.view, EPS, o.view)
            return o.check("kl_uht")

        def wtu():
            o = _out(k, n)
            o6.kl_wtu(Akv.view, Wkv.view, Hkv.view, EPS, o.view)
            return o.check("kl_wtu")
        S.add("kl_uht", uht, lambda x, w: ex.assert_ulp(x, U @ Hk.astype(np.float64).T, 0, w, tile=(32, 32)))
        S.add("kl_wtu", wtu, lambda x, w: ex.assert_ulp(x, Wk.astype(np.float64).T @ U, 0, w, tile=(32, 32)))
        Ai, Wi2, Hi, Ui = ex.kl(m, n, k)
        Hqi = ex.kl_refs(Ai, Wi2, Hi, Ui)[5]
        Aiv = _A(Ai, False)

        @_nout(2)
        def kl_step():
            Wv, Hv = _P(Wi2), _P(Hi)
            o6.mu_kl_step(Aiv.view, Wv.view, Hv.view, EPS, False, False)
            return Wv.check("W"), Hv.check("H")

        def chk_kl(w_, h_, w):
            ex.assert_ulp(h_, Hqi, 3, w + " (W fixed) H", tile=(32, 32))
            ex.assert_ulp(w_, Wi2.astype(np.float64), 0, w + " (W fixed) W", tile=(32, 32))
        S.add("mu_kl_step", kl_step, chk_kl)
        return S.prob()
    return Case("x6-%dx%d-k%d" % (m, n, k), X6_NAMES, make, query=lambda lib: {lib.dnmf_ws_bytes_bf16x6(m, n, k)})


# ------------------------------------------------------------------------------------------------------------- HALS
def _hals_w_case(entry):
    tag, m, k, aligned, plan = entry

    def make(engine, lib):
        from tests.test_gpu_exact_hals import _check_w
        ops = engine.HIP_OPS
        eps = ex.HALS_EPS_A
        P = ex.hals_w_problem(m, k, eps)
        G = _gram(engine, k, P["G"])
        AHv = _P(P["AH"].astype(np.float32), aligned)

        @_nout(2)
        def sweep():
            Wv = _P(P["W_old"].astype(np.float32), aligned)
            got = ops.hals_sweep_plan(Wv.view, AHv.view)
            assert got[:5] == plan, "plan %s, expected %s" % (got[:5], plan)
            ss2 = ops.hals_update_w(Wv.view, AHv.view, G, eps)           # (the k sums of squares: read back FROM the workspace)
            return Wv.check("W"), ss2.cpu().numpy()
        S = Steps()
        S.add("hals_update_w", sweep, lambda w_, ss2, w: _check_w(w_, ss2, P, w))
        return S.prob()
    return Case("hals-w-%s" % tag, ("dnmf_hals_sweep_w",), make, waits=True, query=lambda lib: {lib.dnmf_ws_bytes(m, k, k)})


def _hals_step_case():
    m, n, k = ex.HALS_STEP_BIG[0]

    def make(engine, lib):
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
        from pydnmfk_amd.utils import parse
        P = ex.hals_step_problem(m, n, k)
        comms = MPI_comm(None, 1, 1)
        p = parse()
        p.comm1, p.comm, p.p_r, p.p_c, p.k, p.m, p.n = comms.comm, comms, 1, 1, k, m, n
        p.row_comm, p.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
        p.norm, p.method, p.W_update, p.eps = "fro", "hals", True, ex.HALS_EPS_A

        @_nout(2)
        def step():
            Av, Wv, Hv = (ex.Poisoned(torch, P[x], packed=True) for x in ("A", "W_old", "H_old"))
            nmf_algorithms_1D(Av.view, Wv.view, Hv.view, params=p).update()
            Av.check("A")
            return Wv.check("W"), Hv.check("H")

        def chk(w_, h_, w):
            ex.assert_ulp(w_, P["W_new"], 0, w + ": W after one step", tile=(ex.HALS_ROWS, 4))
            assert np.isfinite(h_).all() and (h_ >= ex.HALS_EPS_A).all()
            bad = np.abs(h_ - P["H_new"]) > P["H_err"]                      # the derived bound of the H sweep (`hals_step_problem`)
            assert not bad.any(), "%s: H at %s is %r, expected %r" % (w, tuple(np.argwhere(bad)[0]), h_[tuple(np.argwhere(bad)[0])],
                                                                     P["H_new"][tuple(np.argwhere(bad)[0])])
        S = Steps()
        S.add("one HALS step", step, chk)
        return S.prob()
    return Case("hals-step-%dx%d-k%d" % (m, n, k), ("dnmf_hals_sweep_w",), make, waits=True,
                query=lambda lib: {lib.dnmf_ws_bytes(k, n, k), lib.dnmf_ws_bytes(m, k, k), lib.dnmf_ws_bytes(m, n, k)})


# ------------------------------------------------------------------------------------------------------------- whole fits
FIT_ITR = 12                                              # the tags of the waiting kernels wrap (a granule holds {value, step})
FIT_ENTRY = {"kl": "dnmf_mu_kl_fit", "fro": "dnmf_mu_fro_fit", "fro_bf16": "dnmf_mu_fro_fit_bf16a", "hals": "dnmf_hals_fro_fit",
             "hals_bf16": "dnmf_hals_fro_fit_bf16a"}


def _fit_case(family, mode):
    """the first SMALL_REACH entry of `family` with more than one workgroup per problem (the cross-workgroup exchange): mode "single",
    "chain" (dnmf_set_persistent(0): the launch chain) or "batch3".  MU: the fixed points of tests/test_gpu_small_exact.py, which return
    normalize_features of the input after any number of steps; HALS: the float64 checker at the tolerance of tests/test_gpu_fit.py"""
    _, m, n, k, plan = next(e for e in ex.SMALL_REACH if e[0] == family and e[4][4] > 1)
    B = 3 if mode == "batch3" else 1
    hals = family.startswith("hals")
    adt = torch.bfloat16 if family.endswith("bf16") else torch.float32

    def make(engine, lib):
        from tests import test_gpu_small_exact as sm
        ops = engine.HIP_OPS
        got_plan = sm._plan(lib, family, m, n, k)
        assert got_plan == plan and plan[4] > 1, got_plan
        if hals:
            from tests.test_gpu_fit import _checker_fit_f64, _close
            probs = [ex.hals_problem(m, n, k, seed) for seed in ex.HALS_SEEDS[:B]]
            refs = []
            for A, W, H in probs:
                Ad, Wd, Hd = (torch.from_numpy(x).cuda() for x in (A, W, H))
                refs.append(_checker_fit_f64(Ad.to(adt), Wd, Hd, FIT_ITR, True, "fro", "hals"))
        else:
            probs = [sm._problem(family, m, n, k, b) for b in range(B)]

        @_nout(3)
        def fit():
            (Ap, Wp, Hp), args = sm._stacks(probs, B, adt)
            was = lib.dnmf_set_persistent(0) if mode == "chain" else None
            try:
                sq = ops.fit("hals" if hals else "mu", "kl" if family == "kl" else "fro", *args, EPS, True, FIT_ITR)
                ops.hals_check()
            finally:
                if was is not None:
                    lib.dnmf_set_persistent(was)
            Ap.check("A")
            w3, h3 = Wp.check("W"), Hp.check("H")
            return (w3, h3, sq.cpu().numpy()) if B > 1 else (w3[None], h3[None], sq.cpu().numpy())

        def chk(w3, h3, sq, what):
            for b, (A, W, H) in enumerate(probs):
                if hals:
                    assert np.isfinite(w3[b]).all() and np.isfinite(h3[b]).all()
                    for X, Y, name in ((w3[b], refs[b][0], "W"), (h3[b], refs[b][1], "H")):
                        X = torch.from_numpy(np.ascontiguousarray(X)).cuda()
                        assert _close(X, Y, 1e-3), (what, b, name, float((X.double() - Y).abs().max()), float(Y.abs().max()))
                    continue
                A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
                s = W64.sum(0)
                pow2 = bool(np.all(np.frexp(s)[0] == 0.5))
                assert pow2 or family.startswith("fro")
                c = 0 if pow2 else 1
                ex.assert_ulp(w3[b], W64 / s[None, :], c, "%s [%d] W = W / colsum(W)" % (what, b))
                ex.assert_ulp(h3[b], H64 * s[:, None], c, "%s [%d] H = H colsum(W)" % (what, b))
                sa = float((A64 ** 2).sum())
                assert sq[b, 1] == sa, "%s [%d]: sum A^2 is %r, expected %r" % (what, b, sq[b, 1], sa)
                lim = 0.0 if pow2 else ((k + 4) * 2.0 ** -24) ** 2 * sa
                assert 0.0 <= sq[b, 0] <= lim, "%s [%d]: sum (A - W H)^2 is %r, at most %r expected" % (what, b, sq[b, 0], lim)
        fit.free = (2,)                                   # (the squared norms: float64 atomics, order free -- held in chk, not bit-compared)
        S = Steps()
        S.add("%s fit, %d steps, %s" % (family, FIT_ITR, mode), fit, chk)
        return S.prob()
    return Case("fit-%s-%dx%d-k%d-%s" % (family, m, n, k, mode), (FIT_ENTRY[family],), make, waits=True,
                query=lambda lib: {lib.dnmf_ws_bytes_fit(m, n, k, B)})


# ------------------------------------------------------------------------------------------------------------- BCD
def _bcd_w_case():
    R, k = ex.BCD_COLSUM[0]

    def make(engine, lib):
        from tests import test_gpu_exact_bcd as tb
        P = ex.bcd_pg_problem(R, k, seed=1, L=ex.BCD_L, side="w")
        assert P["pow2"]

        @_nout(2)
        def call():
            return tb._run_pg((engine, engine.HIP_OPS), P, "w", (True, False, R % 2 == 0), "bcd_update_w")

        def chk(out, s, w):
            ex.assert_ulp(out, P["expected"], 0, w, tile=(64, 16))
            tb._same_bits(s, P["s"], w + ": column sums")
        S = Steps()
        S.add("bcd_update_w", call, chk)
        return S.prob()
    return Case("bcd-update-w-%dx%d" % (R, k), ("dnmf_bcd_update_w",), make, query=lambda lib: {lib.dnmf_bcd_ws_bytes_w(R, k)})


def _bcd_fit_case(B):
    from tests.test_gpu_exact_bcd import FITS
    m, n, k, itr, _ = min(FITS, key=lambda f: f[0] * f[1])

    def make(engine, lib):
        from pydnmfk_amd.pyDNMF import PyNMF
        from tests._bcd import BcdOracleOps, check_tolerances
        from tests._golden import rel_fro
        from tests.test_gpu_bcd import _args
        probs, refs = [], []
        for b in range(B):
            rs = np.random.RandomState(m + n + k + b)
            A = (rs.rand(m, 5) @ rs.rand(5, n) + 0.01 * rs.rand(m, n)).astype(np.float32)
            W0, H0 = rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)
            probs.append((A, W0, H0))
            refs.append(PyNMF(A, factors=[W0, H0], params=_args(k, itr), ops=BcdOracleOps()).fit())      # the numpy checker, on the CPU

        @_nout(3)
        def fit():
            if B == 1:
                A, W, H = (_dev(x) for x in probs[0])
            else:
                A, W, H = (engine.stack_alloc(B, *probs[0][i].shape, torch.float32, torch.device("cuda")) for i in range(3))
                for b in range(B):
                    for t, x in zip((A, W, H), probs[b]):
                        t[b].copy_(_dev(x))
            sq = engine.HIP_OPS.fit("bcd", "fro", A, W, H, EPS, True, itr)
            w3, h3 = W.cpu().numpy(), H.cpu().numpy()
            return (w3, h3, sq.cpu().numpy()) if B > 1 else (w3[None], h3[None], sq.cpu().numpy())

        def chk(w3, h3, sq, what):
            for b, (Wc, Hc, ec) in enumerate(refs):
                assert np.isfinite(w3[b]).all() and np.isfinite(h3[b]).all()
                err = float(np.sqrt(sq[b, 0] / sq[b, 1]))
                check_tolerances("%s [%d]" % (what, b), {0: {"fit%d" % itr: (rel_fro(w3[b], Wc), rel_fro(h3[b], Hc), abs(err - ec))}})
        fit.free = (2,)
        S = Steps()
        S.add("bcd fit, %d iterations, batch %d" % (itr, B), fit, chk)
        return S.prob()
    return Case("bcd-fit-%dx%d-k%d-%s" % (m, n, k, "batch3" if B > 1 else "single"), ("dnmf_bcd_fro_fit",), make,
                query=lambda lib: {lib.dnmf_bcd_ws_bytes_fit(m, n, k, B)})


# ------------------------------------------------------------------------------------------------------------- float64
F64_NAMES = ("dnmf_f64_aht", "dnmf_f64_wta", "dnmf_f64_kl_uht", "dnmf_f64_kl_wtu", "dnmf_f64_sum", "dnmf_f64_colsum", "dnmf_f64_hals_w_col")


def _f64_case(m, n, k):
    D = torch.float64

    def make(engine, lib):
        from tests.test_gpu_exact_hals import _check_w
        ops = engine.HIP_OPS_F64
        S = Steps()
        A, W, H = ex.products(m, n, k, np.float64)
        Av, Wv, Hv = _P(A), _P(W), _P(H)

        def aht():
            o = _out(m, k, True, D)
            ops.aht(Av.view, Hv.view, o.view)
            return o.check("aht")

        def wta():
            o = _out(k, n, True, D)
            ops.wta(Av.view, Wv.view, o.view)
            return o.check("wta")
        S.add("f64 aht", aht, lambda x, w: ex.assert_ulp(x, A @ H.T, 0, w))
        S.add("f64 wta", wta, lambda x, w: ex.assert_ulp(x, W.T @ A, 0, w))
        Ak, Wk, Hk, U = ex.kl(m, n, k, np.float64)
        Akv, Wkv, Hkv = _P(Ak), _P(Wk), _P(Hk)

        def uht():
            o = _out(m, k, True, D)
            ops.kl_uht(Akv.view, Wkv.view, Hkv.view, E64, o.view)
            return o.check("kl_uht")

        def wtu():
            o = _out(k, n, True, D)
            ops.kl_wtu(Akv.view, Wkv.view, Hkv.view, E64, o.view)
            return o.check("kl_wtu")
        S.add("f64 kl_uht", uht, lambda x, w: ex.assert_ulp(x, U @ Hk.T, 0, w))
        S.add("f64 kl_wtu", wtu, lambda x, w: ex.assert_ulp(x, Wk.T @ U, 0, w))
        # the sums: A = W H + (0..2), small integers (tests/test_gpu_exact_f64.py::test_sqdiff_and_error_sums)
        R = np.random.RandomState(m + k).randint(0, 3, size=(m, n)).astype(np.float64)
        A2 = W @ H + R
        A2v = _P(A2)

        @_nout(5)
        def sums():
            sq, rsq = ops.sqnorm(A2v.view), ops.resid_sqnorm(A2v.view, Wv.view, Hv.view)
            num, den = ops.column_err_sums(A2v.view, Wv.view, Hv.view)
            cs = ops.colsum(Wv.view, torch.full((k,), 7.0, dtype=D, device="cuda"))
            return [t.cpu().numpy() for t in (sq, rsq, num, den, cs)]

        def chk_sums(sq, rsq, num, den, cs, w):
            assert float(sq[0]) == float((A2 ** 2).sum()) and float(rsq[0]) == float((R ** 2).sum()), (w, float(sq[0]), float(rsq[0]))
            ex.assert_ulp(num, (R ** 2).sum(0), 0, w + " column_err_sums num")
            ex.assert_ulp(den, (A2 ** 2).sum(0), 0, w + " column_err_sums den")
            ex.assert_ulp(cs, W.sum(0), 0, w + " colsum")
        S.add("f64 sums", sums, chk_sums)
        Ph = ex.hals_w_problem(m, k, ex.HALS_EPS_A, dtype=np.float64)
        G = _gram(engine, k, Ph["G"], D)
        AHv = _P(Ph["AH"].astype(np.float64))

        @_nout(2)
        def hals():
            Wh = _P(Ph["W_old"].astype(np.float64))
            ss2 = ops.hals_update_w(Wh.view, AHv.view, G, ex.HALS_EPS_A)
            return Wh.check("W"), ss2.cpu().numpy()
        S.add("f64 hals_update_w", hals, lambda w_, ss2, w: _check_w(w_, ss2, Ph, w))
        return S.prob()
    return Case("f64-%dx%d-k%d" % (m, n, k), F64_NAMES, make,
                query=lambda lib: {lib.dnmf_f64_ws_bytes(m, n, k), lib.dnmf_f64_ws_bytes(m, k, k), lib.dnmf_f64_ws_bytes(m, n, 1)})


def _f64_fit_case(fam):
    m, n, k, _ = next(c for c in ex.F64_FIT_FRO if c[3] == fam)

    def make(engine, lib):
        from pydnmfk_amd import _lib
        from tests.test_gpu_exact import _assert_normalized
        assert _lib.f64_plan("fit", m, n, k, method=0)["family"] == fam
        A, W, H, Wn, Hq = ex.fro_step(m, n, k, np.float64)

        @_nout(2)
        def fit():
            Ap, Wp, Hp = _P(A), _P(W), _P(H)
            engine.HIP_OPS_F64.fit("mu", "fro", Ap.view, Wp.view, Hp.view, E64, True, 1)
            Ap.check("A")
            return Wp.check("fit W"), Hp.check("fit H")
        S = Steps()
        S.add("f64 fit (%s)" % fam, fit, lambda w_, h_, w: _assert_normalized(w_, h_, np.maximum(Wn, E64), np.maximum(Hq, E64), 6, w, eps=E64))
        return S.prob()
    return Case("f64-fit-%s-%dx%d-k%d" % (fam, m, n, k), ("dnmf_f64_fit",), make, query=lambda lib: {lib.dnmf_f64_ws_bytes_fit(m, n, k)})


# ------------------------------------------------------------------------------------------------------------- CSR
CSR_NAMES = ("dnmf_csr_mm", "dnmf_csr_kl_mm", "dnmf_csr_resid_sqnorm", "dnmf_csr_masked_mm", "dnmf_csr_masked_update",
             "dnmf_csr_masked_resid_sqnorm", "dnmf_csr_column_err")


@functools.lru_cache(maxsize=1)
def _pattern():
    return ex.lens_pattern()


def _csr_case(k, side):
    def make(engine, lib):
        from tests import test_gpu_exact_sparse as ts
        from tests.test_gpu_sparse_nmfk import _colerr_ref
        ops = engine.HIP_CSR_OPS
        S = Steps()
        pattern = _pattern()
        # the products and the residual of a block whose unstored entries are zeros
        A, mask, W, H, blk = ts._oriented(side, *ts._problem(ex.sparse_products, pattern, k))
        m, n = mask.shape
        ref = ex.sparse_exact(A, mask, W, H)
        Wv, Hv = ts._P(W, True), ts._P(H, True)

        @_nout(5)
        def products():
            o1, o2 = ts._out(m, k, True), ts._out(k, n, True)
            ops.aht(blk, Hv.view, o1.view)
            ops.wta(blk, Wv.view, o2.view)
            r = ops.resid_sqnorm(blk, Wv.view, Hv.view)
            num, den = ops.column_err_sums(blk, Wv.view, Hv.view)
            return o1.check("aht"), o2.check("wta"), r.cpu().numpy(), num.cpu().numpy(), den.cpu().numpy()
        cn, cd = _colerr_ref(A, mask, W, H, False)

        def chk_products(aht, wta, r, num, den, w):
            ex.assert_ulp(aht, ref["aht"], 0, w + " aht")
            ex.assert_ulp(wta, ref["wta"], 0, w + " wta")
            assert float(r[0]) == ref["resid"], (w, float(r[0]), ref["resid"])
            assert np.array_equal(num, cn) and np.array_equal(den, cd), w + " column_err_sums"
        S.add("csr products", products, chk_products)
        Ak, maskk, Wk, Hk, blkk = ts._oriented(side, *ts._problem(ex.sparse_kl, pattern, k))
        refk = ex.sparse_exact(Ak, maskk, Wk, Hk, kl=True)
        Wkv, Hkv = ts._P(Wk, True), ts._P(Hk, True)

        @_nout(2)
        def klp():
            o1, o2 = ts._out(m, k, True), ts._out(k, n, True)
            ops.kl_uht(blkk, Wkv.view, Hkv.view, EPS, o1.view)
            ops.kl_wtu(blkk, Wkv.view, Hkv.view, EPS, o2.view)
            return o1.check("kl_uht"), o2.check("kl_wtu")

        def chk_kl(uht, wtu, w):
            ex.assert_ulp(uht, refk["uht"], 0, w + " kl_uht")
            ex.assert_ulp(wtu, refk["wtu"], 0, w + " kl_wtu")
        S.add("csr kl products", klp, chk_kl)
        # ... and of a block whose unstored entries are missing
        for norm in ("fro", "kl"):
            Am, maskm, Wm, Hm, blkm = ts._oriented(side, *ts._masked_problem(norm, pattern, k), missing="unstored")
            rm = ex.sparse_exact(Am, maskm, Wm, Hm, kl=norm == "kl")
            nw, dw, nh, dh = ts._pairs(rm, norm)
            Wmv, Hmv = ts._P(Wm, True), ts._P(Hm, True)

            @_nout(6)
            def masked(blkm=blkm, Wmv=Wmv, Hmv=Hmv, Wm=Wm, Hm=Hm, norm=norm):
                out = []
                for fn, rows, cols in ((ops.masked_aht_pair, m, k), (ops.masked_wta_pair, k, n)):
                    pair = ex.Poisoned(torch, np.full((2 * rows, cols), ex.SENTINEL, np.float32), fill=ex.SENTINEL, packed=True)
                    fn(blkm, Wmv.view, Hmv.view, EPS, norm, pair.view.reshape(-1))
                    out.append(pair.check(fn.__name__))
                W1, H1 = ts._P(Wm, True), ts._P(Hm, True)
                ops.masked_update_w(blkm, W1.view, Hmv.view, EPS, norm)
                ops.masked_update_h(blkm, Wmv.view, H1.view, EPS, norm, clamp=True)
                r = ops.resid_sqnorm(blkm, Wmv.view, Hmv.view)
                cn_, cd_ = ops.column_err_sums(blkm, Wmv.view, Hmv.view)
                return out[0], out[1], W1.check("masked_update_w"), H1.check("masked_update_h"), r.cpu().numpy(), torch.stack((cn_, cd_)).cpu().numpy()
            mn, md = _colerr_ref(Am, maskm, Wm, Hm, True)

            def chk_masked(pw, ph, w1, h1, r, ce, w, nw=nw, dw=dw, nh=nh, dh=dh, Wm=Wm, Hm=Hm, rm=rm, mn=mn, md=md, norm=norm):
                ex.assert_ulp(pw[:m], nw, 0, w + " W numerator")
                ex.assert_ulp(pw[m:], dw, 0, w + " W denominator")
                ex.assert_ulp(ph[:k], nh, 0, w + " H numerator")
                ex.assert_ulp(ph[k:], dh, 0, w + " H denominator")
                ts._assert_ratio(w1, ts._ratio_ref(Wm, nw, dw, False), False, w + " masked_update_w")
                ts._assert_ratio(h1, ts._ratio_ref(Hm, nh, dh, True), True, w + " masked_update_h clamp=1")
                if norm == "fro":
                    assert float(r[0]) == rm["resid_masked"], (w, float(r[0]), rm["resid_masked"])
                    assert np.array_equal(ce[0], mn) and np.array_equal(ce[1], md), w + " masked column_err_sums"
            S.add("csr masked %s" % norm, masked, chk_masked)
        return S.prob()
    def query(lib):
        m, n = (len(ex.LENS), ex.LENS_N) if side == "A" else (ex.LENS_N, len(ex.LENS))
        nseg = int(sum(-(-x // 1024) for x in ex.LENS if x > 1024))                # the segments of the long rows: on the row image (A) or the transpose's (At)
        t_nseg = nseg if side == "At" else 0
        return {lib.dnmf_csr_ws_bytes(m, n, k, nseg), lib.dnmf_csr_masked_ws_bytes(m, n, k, nseg),
                lib.dnmf_csr_column_err_ws_bytes(n, m, k, 0, t_nseg), lib.dnmf_csr_column_err_ws_bytes(n, m, k, 1, t_nseg)}
    return Case("csr-k%d-%s" % (k, side), CSR_NAMES, make, align16=True, query=query)


# ------------------------------------------------------------------------------------------------------------- masked dense
MASKED_NAMES = ("dnmf_masked_aht_pair", "dnmf_masked_wta_pair", "dnmf_masked_update_w", "dnmf_masked_update_h")


def _masked_case(shape, k):
    m, n = shape

    def make(engine, lib):
        from tests import _masked_dense as D
        from tests import test_gpu_masked_dense as tm
        ops = engine.HIP_MASKED_OPS
        A, mask, W, H, ref = D.exact_problem(m, n, k) if shape in D.EXACT_SHAPES else D.loop_problem(m, n, k)
        e = np.float32(EPS)

        @_nout(14)
        def call():
            # the pairs of both objectives with the checks of tests/test_gpu_masked_dense.py (exact `fro` pairs and `kl` denominators,
            # the `kl` numerators per element where a sum is one term), then the fused endings on the same views
            Ap, Wp, Hp, blk, got = tm._exact_pair_checks(A, mask, W, H, ref)
            out = []
            for norm in ("fro", "kl"):
                W1, H1, H2 = _P(W), _P(H), _P(H)
                ops.masked_update_w(blk, W1.view, Hp.view, EPS, norm)
                ops.masked_update_h(blk, Wp.view, H1.view, EPS, norm)
                ops.masked_update_h(blk, Wp.view, H2.view, EPS, norm, clamp=True)
                out += list(got[norm]) + [W1.check("fused W"), H1.check("fused H"), H2.check("fused H, clamped")]
            return out

        def chk(*args):
            w = args[-1]
            for i, norm in enumerate(("fro", "kl")):
                nw, dw, nh, dh, w1, h1, h2 = args[7 * i:7 * i + 7]
                expW, expH = W * (nw / (dw + e)), H * (nh / (dh + e))
                tm._assert_within_an_ulp(w1, expW, "%s %s fused W" % (w, norm))
                tm._assert_within_an_ulp(h1, expH, "%s %s fused H" % (w, norm))
                tm._assert_within_an_ulp(h2, np.maximum(expH, e), "%s %s fused H, clamped" % (w, norm))
        S = Steps()
        S.add("masked pairs and fused endings", call, chk)
        return S.prob()
    return Case("masked-%dx%d-k%d" % (m, n, k), MASKED_NAMES, make, align16=True, query=lambda lib: {lib.dnmf_masked_ws_bytes(m, n, k)})


def _masked_colerr_case(k):
    from tests import _masked_nmfk as N
    m, n = N.COLERR_LOOP_CASES[0]["shape"]

    def make(engine, lib):
        from pydnmfk_amd.masked import MaskedDenseBlock
        from tests import _masked_dense as D
        A, mask, W, H = N.colerr_case(m, n, k)
        rn, rd = N.colerr_ref(A, mask, W, H)
        Ap, Wp, Hp = _P(D.nan_marked(A, mask)), _P(W), _P(H)
        blk = MaskedDenseBlock(Ap.view)

        @_nout(2)
        def call():
            num, den = engine.HIP_MASKED_OPS.column_err_sums(blk, Wp.view, Hp.view)
            return num.cpu().numpy(), den.cpu().numpy()
        def chk(num, den, w):
            assert np.array_equal(num, rn) and np.array_equal(den, rd), "%s: the sums are not the float64 integers" % w
        S = Steps()
        S.add("masked column_err_sums", call, chk)
        return S.prob()
    return Case("masked-colerr-%dx%d-k%d" % (m, n, k), ("dnmf_masked_column_err",), make, align16=True,
                query=lambda lib: {lib.dnmf_masked_column_err_ws_bytes(m, n, k)})


def _masked_fit_case(norm):
    def make(engine, lib):
        from pydnmfk_amd.masked import MaskedDenseBlock
        from tests import _masked as M
        from tests import _masked_dense as D
        from tests._golden import rel_fro
        A, mask, W0, H0, k = M.small_problem()
        An = D.nan_marked(A, mask)
        Wr, Hr, err_r = M.fit(D.coo_of_dense(An), A.shape, W0, H0, FIT_ITR, norm)

        @_nout(3)
        def fit():
            blk = MaskedDenseBlock(_dev(An))
            W, H = _dev(W0), _dev(H0)
            sq = engine.HIP_MASKED_OPS.fit("mu", norm, blk, W, H, EPS, True, FIT_ITR)
            return W.cpu().numpy(), H.cpu().numpy(), sq.cpu().numpy()

        def chk(w_, h_, sq, w):
            err = float(np.sqrt(sq[0, 0] / sq[0, 1]))
            dw, dh, de = rel_fro(w_, Wr), rel_fro(h_, Hr), abs(err - err_r) / err_r
            assert dw <= 1e-4 and dh <= 1e-4 and de <= 1e-5, (w, dw, dh, de)     # (tests/test_gpu_masked_dense.py: the one-rank fit against float64)
        fit.free = (2,)
        S = Steps()
        S.add("masked %s fit, %d steps" % (norm, FIT_ITR), fit, chk)
        return S.prob()
    return Case("masked-fit-%s" % norm, ("dnmf_masked_mu_fit",), make, align16=True, query=lambda lib: {lib.dnmf_masked_ws_bytes_fit(24, 12, 3)})


# ------------------------------------------------------------------------------------------------------------- Itakura-Saito
IS_NAMES = ("dnmf_is_aht_pair", "dnmf_is_wta_pair", "dnmf_is_update_w", "dnmf_is_update_h", "dnmf_is_divergence", "dnmf_is_column_div")


def _is_case(shape, k):
    m, n = shape

    def make(engine, lib):
        from tests import _is as I
        from tests import _is_nmfk as K
        from tests import test_gpu_is as ti
        ops = engine.HIP_OPS
        A, W, H, ref = I.exact_problem(m, n, k)
        exp = ti._expected(A, W, H)
        Ap, Wp, Hp = _P(A), _P(W), _P(H)
        Ac, Wc, Hc, count = K.coldiv_case(m, n, k)
        Acp, Wcp, Hcp = _P(Ac), _P(Wc), _P(Hc)

        @_nout(9)
        def call():
            out = []
            for side, (r, c) in (("w", (m, k)), ("h", (k, n))):
                num, den = _out(r, c), _out(r, c)
                ops.is_pair_into(side, Ap.view, Wp.view, Hp.view, EPS, num.view, den.view)
                out += [num.check("is %s num" % side), den.check("is %s den" % side)]
            W1, H1, H2 = _P(W), _P(H), _P(H)
            ops.is_update_w(Ap.view, W1.view, Hp.view, EPS)
            ops.is_update_h(Ap.view, Wp.view, H1.view, EPS)
            ops.is_update_h(Ap.view, Wp.view, H2.view, EPS, clamp=True)
            div = ops.is_divergence(Ap.view, Wp.view, Hp.view, EPS)
            cdiv = ops.is_column_div(Acp.view, Wcp.view, Hcp.view, EPS)
            return out + [W1.check("W1"), H1.check("H1"), H2.check("H2"), div.cpu().numpy(), cdiv.cpu().numpy()]

        def chk(nw, dw, nh, dh, w1, h1, h2, div, cdiv, w):
            for g, r_, name in zip((nw, dw, nh, dh), ref["w"] + ref["h"], ("num_w", "den_w", "num_h", "den_h")):
                assert np.array_equal(g.astype(np.float64), r_), "%s %s: %d elements differ from the exact answer" % (w, name, int((g != r_).sum()))
            du = [ti._rel(w1, exp["W"]), ti._rel(h1, exp["H"]), ti._rel(h2, np.maximum(exp["H"], EPS))]
            dd = abs(float(div[0]) - exp["div"]) / exp["div"]
            assert max(du) <= ti.BOUND and dd <= ti.BOUND, (w, du, dd)
            # the column divergence on the planted problem (tests/test_gpu_is_nmfk.py): count[c] * u bit for bit, u a float32 near 1 - ln 2
            assert not cdiv[count == 0].any()
            u = cdiv[0] / count[0]
            assert np.array_equal(cdiv, count * u) and float(np.float64(np.float32(u))) == u and abs(u - (1.0 - np.log(2.0))) <= 2.0 ** -21, (w, u)
        S = Steps()
        S.add("is", call, chk)
        return S.prob()
    return Case("is-%dx%d-k%d" % (m, n, k), IS_NAMES, make, align16=True,
                query=lambda lib: {lib.dnmf_is_ws_bytes(m, n, k), lib.dnmf_is_column_div_ws_bytes(m, n, k)})


def _is_fit_case():
    def make(engine, lib):
        from tests import _is as I
        from tests import test_gpu_is as ti
        from tests._golden import rel_fro
        A, W0, H0, k = ti._fit_problem()
        Wr, Hr, err_r = I.fit(A, W0, H0, FIT_ITR)

        @_nout(3)
        def fit():
            Ad, W, H = _dev(A), _dev(W0), _dev(H0)
            sq = engine.HIP_OPS.fit("mu", "is", Ad, W, H, EPS, True, FIT_ITR)
            return W.cpu().numpy(), H.cpu().numpy(), sq.cpu().numpy()

        def chk(w_, h_, sq, w):
            err = float(np.sqrt(sq[0, 0] / sq[0, 1]))
            dw, dh, de = rel_fro(w_, Wr), rel_fro(h_, Hr), abs(err - err_r) / err_r
            assert dw <= ti.FIT_BOUND and dh <= ti.FIT_BOUND and de <= ti.ERR_BOUND, (w, dw, dh, de)
        fit.free = (2,)
        S = Steps()
        S.add("is fit, %d steps" % FIT_ITR, fit, chk)
        return S.prob()
    return Case("is-fit", ("dnmf_is_mu_fit",), make, align16=True, query=lambda lib: {lib.dnmf_is_ws_bytes_fit(200, 136, 5)})


# ------------------------------------------------------------------------------------------------------------- grid steps
def _grid_case(name):
    from tests.test_gpu_grid_workspace import _GRIDS
    grid, shape = _GRIDS[name]
    two_d = grid[0] > 1 and grid[1] > 1
    d = "2d" if two_d else "1d"
    names = ["dnmf_mu_fro_step_" + d, "dnmf_mu_kl_step_" + d, "dnmf_hals_fro_step_" + d, "dnmf_mu_fro_step_%s_bf16a" % d, "dnmf_hals_fro_step_%s_bf16a" % d]

    def make(engine, lib):
        from tests.test_gpu_grid_workspace import ALLGATHER, Position

        class PeersPosition(Position):
            """Position whose allgather puts a fully written block of 0.25 in every OTHER member's place (its own block in its own).
            The recording collective of Position copies this member's block everywhere; on a ragged grid the library then reads a
            larger member's block at that member's width and so reaches the pad of this rank's send block -- floats no kernel wrote and
            no rank of a real exchange ever reads (a peer's block is written to its own width).  What the workspace held would show
            in the result through the stand-in, not through the library."""

            def _collective(self, op, group, send, recv, count, stream):
                if op != ALLGATHER:
                    return super()._collective(op, group, send, recv, count, stream)
                members, me = (self.p_r * self.p_c, self.p_r, self.p_c)[group], (self.rank, self.i, self.j)[group]
                self.trace.append((op, group, self._where(send), self._where(recv), count, 4))
                torch.cuda.synchronize()
                peer = torch.full((count,), 0.25, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                for q in range(members):
                    if self.hip.hipMemcpy(recv + q * count * 4, send if q == me else peer.data_ptr(), count * 4, 3):
                        return 1
                return 0
        pos = [PeersPosition(grid, rank, shape) for rank in range(grid[0] * grid[1])]

        def run():
            out = []
            for p in pos:
                for family, bf16 in (("fro", False), ("kl", False), ("hals", False), ("fro", True), ("hals", True)):
                    assert p.step(family, w_update=True, bf16=bf16), "a step of more than one rank exchanges something"
                    out += [p.W.cpu().numpy(), p.H.cpu().numpy()]
            return out

        def verify(arrays, what):
            # no exact answer: the bits of the run on a zeroed workspace of exactly the query (the driver's (c)); here: finite numbers
            assert all(np.isfinite(a).all() for a in arrays), what

        def close():
            for p in pos:
                p.close()
        return Prob(run, verify, close)

    def query(lib):
        from tests.test_gpu_grid_workspace import part
        q = set()
        for rank in range(grid[0] * grid[1]):
            m_l, n_l = part(shape[0], grid[0], rank // grid[1]), part(shape[1], grid[1], rank % grid[1])
            q.add(lib.dnmf_ws_bytes_2d(m_l, n_l, shape[2], *grid) if two_d else lib.dnmf_ws_bytes_1d(m_l, n_l, shape[2]))
        return q
    return Case("grid-%s" % name, names, make, waits=True, query=query)


def _cases():
    from tests import _is as I
    from tests import _masked_dense as D
    cases = _dense_cases() + [_hblocks_case(), _x6_case()]
    cases += [_hals_w_case(next(c for c in ex.HALS_W_CASES if c[4][0] == 1)), _hals_w_case(next(c for c in ex.HALS_W_CASES if c[4][0] == 0)),
              _hals_step_case()]
    cases += [_fit_case(f, mode) for f in ("fro", "kl", "hals", "fro_bf16", "hals_bf16") for mode in ("single", "chain", "batch3")]
    cases += [_bcd_w_case(), _bcd_fit_case(1), _bcd_fit_case(3)]
    cases += [_f64_case(257, 600, 15), _f64_case(513, 129, 65), _f64_fit_case("fit_tiny"), _f64_fit_case("fit_chain")]
    cases += [_csr_case(k, side) for k in (3, 17, 256) for side in ("A", "At")]
    cases += [_masked_case(s, k) for s in ((130, 97),) + tuple(c["shape"] for c in D.EXACT_LOOP_CASES[:2]) for k in (3, 128)]
    cases += [_masked_colerr_case(k) for k in (3, 128)] + [_masked_fit_case("fro"), _masked_fit_case("kl")]
    cases += [_is_case(s, k) for s in (I.EXACT_SHAPES[0],) + tuple(c["shape"] for c in I.EXACT_LOOP_CASES[:2]) for k in (3, 128)] + [_is_fit_case()]
    cases += [_grid_case(name) for name in ("3x1", "1x3", "2x2-ragged", "2x3")]
    return cases


CASES = _cases()


# ------------------------------------------------------------------------------------------------------------- the driver
def _foreign(engine, waits):
    """one call of ANOTHER family under the same guard: what it leaves in the workspace is the 'leftover' state.  A case of waiting
    kernels follows a KL product at a wide rank (U at the end of the workspace, finite fp32 everywhere); every other case follows a
    persistent HALS sweep (the slot slab with its tags, the k sums of squares behind it)"""
    g = torch.Generator(device="cuda").manual_seed(5)
    if waits:
        A, W, H = (torch.rand(s, device="cuda", generator=g) + 0.05 for s in ((64, 96), (64, 129), (129, 96)))
        engine.HIP_OPS.kl_uht(A, W, H, EPS, torch.empty(64, 129, device="cuda"))
    else:
        W, AH = torch.rand(700, 5, device="cuda", generator=g), torch.rand(700, 5, device="cuda", generator=g)
        G = engine.new_gram(5, W.device)
        G[:5, :5] = torch.eye(5, device="cuda") * 3 + 1
        engine.HIP_OPS.hals_update_w(W, AH, G, EPS)
        engine.HIP_OPS.hals_check()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_workspace_contract(env, case):
    engine, lib = env
    prob = case.make(engine, lib)
    results, asked_all = [], []
    runs = RUNS + ([ALIGN16] if case.align16 else [])
    try:
        with _ws.Recorder(lib, case.names) as rec:
            for state, extra, lead in runs:
                what = "%s [ws %s%s%s]" % (case.id, state if isinstance(state, str) else "0x%02X" % state,
                                          ", four times the query" if extra else "", ", 16-byte base" if lead != 512 else "")
                with _ws.guarded(engine, state, extra, lead) as g:
                    if state == "leftover":
                        _foreign(engine, case.waits)
                    first = len(g.sizes)
                    got = prob.run()
                    torch.cuda.synchronize()
                    g.check(what)                                                   # (a)
                    asked = g.sizes[first:]
                assert asked, "%s: the engine asked for no workspace" % what
                if case.waits:
                    engine.HIP_OPS.hals_check()
                prob.verify(got, what)                                              # (b)
                results.append((what, got))
                asked_all.append(asked)
        assert not rec.missing(), "%s never reached %s" % (case.id, rec.missing())  # (d)
    finally:
        if prob.close is not None:
            prob.close()
    free = prob.free
    what0, first = results[0]
    for what, got in results[1:]:                                                   # (c)
        assert len(got) == len(first)
        for i, (a, b) in enumerate(zip(first, got)):
            if i in free:
                continue
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bytes(a), _bytes(b)), \
                "%s: output %d differs in bits from %s -- the result depends on what the workspace held or on its size" % (what, i, what0)
    for what_asked in asked_all[1:]:
        assert what_asked == asked_all[0], "%s: the sizes asked for differ between runs: %s / %s" % (case.id, asked_all[0], what_asked)
    if case.query is not None:
        assert set(asked_all[0]) == {int(q) for q in case.query(lib)}, "%s asked %s, include/dnmf.h names %s" % (
            case.id, sorted(set(asked_all[0])), sorted(case.query(lib)))
    print("%s: sizes asked %s" % (case.id, asked_all[0]))
