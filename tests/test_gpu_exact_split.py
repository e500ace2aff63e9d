"""The six bf16x6 kernels (csrc/dnmf_split.h: split3_rows, split3_cols, ntx, tnx; csrc/dnmf_split_kl.h: klx_wtu, klx_uht) against the
exact answer, element by element, on shapes that REACH them: n a multiple of 128, 16-byte aligned rows of A.  Every case first asserts
through dnmf_bf16x6_plan that the split kernel is the one taken, with the instantiation and the loop trip counts its name says
(tests/test_bf16x6_plan.py checks the same table without a GPU).  tests/test_gpu_exact.py runs its bf16x6 cases on n = 130, 2052, ...:
the forwarding to the fp32 kernels.

Two kinds of operands (tests/_exact.py; proofs: tests/test_exact_cpu.py):
  * the integer families of the fp32 suite -- every indexing error shows, but x2 = x3 = 0: five of the six piece products are zero;
  * `pieces_product` / `kl_pieces`: second and third pieces of both signs, the three dropped terms zero by construction, every sum of
    piece products exact in fp32 in any order.  The numpy model of the kernels' arithmetic with one term deleted, two planes swapped
    or a plane zeroed differs from float64 in every 32 x 32 tile of the output, so a kernel with that defect fails here in that tile.
Bounds: products EQUAL float64; the fused W update and the H of a step within 3 ulps (s rcp(d), then times the factor); the W of a
`fro_step` step exact; KL as tests/test_gpu_exact.py::test_kl.  Operands are views in NaN buffers, outputs views in sentinel buffers.

Measured on one MI355X: the 48 tests take 5.2 s of pytest time together; the comment above each test has its cases."""
import numpy as np
import pytest

from tests import _exact as ex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
EPS32 = np.float32(EPS)
FRO, KL, KT, NSET, TNX_CHUNKS, TNX_ROWS, WTUX_CHUNKS, WTUX_BLOCKS, UHTX_SPLITS, UHTX_COLS, NTX_STREAMED, TNX_STREAMED = range(12)

F32_CASES = [pytest.param(c, False, id="f32-" + c[0]) for c in ex.X6_F32]
BF16_CASES = [pytest.param(c, True, id="bf16-" + c[0]) for c in ex.X6_BF16]
KL_CASES = [pytest.param(c, id=c[0]) for c in ex.X6_KL]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pydnmfk_amd import engine
    from pydnmfk_amd._lib import lib
    return engine, lib


def _A(x, bf16=False, lda=0):
    """A as a view with 16-byte aligned rows: lead 8 elements, pitch a multiple of 16 bytes (lda = 0: n + 4 floats / n + 8 bf16)"""
    return ex.Poisoned(torch, x, dtype=torch.bfloat16 if bf16 else torch.float32, quantum=8 if bf16 else 4, ld=lda or None)


def _P(x, aligned=True):
    return ex.Poisoned(torch, x, aligned=aligned)


def _out(rows, cols, aligned=True):
    return ex.Poisoned.out(torch, rows, cols, torch.float32, aligned)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().float()


def _gram(engine, G):
    k = G.shape[0]
    Gd = engine.new_gram(k, torch.device("cuda"))
    Gd.zero_()
    Gd[:k, :k] = _dev(G)
    return Gd


def _plan(lib, Av, k):
    """the plan of the call that gets this view of A"""
    import ctypes
    out = (ctypes.c_long * 12)()
    bf16 = Av.dtype == torch.bfloat16
    m, n = Av.view.shape
    assert lib.dnmf_bf16x6_plan(m, n, k, Av.view.stride(0), int(bf16), int(Av.view.data_ptr() % 16 == 0), out) == 0
    return list(out)


def _assert_fro_plan(lib, Av, k, want):
    p = _plan(lib, Av, k)
    assert p[FRO] == 1, "not a split shape: the fp32 kernels would run"
    assert (p[KT], p[NSET], p[TNX_CHUNKS], p[TNX_ROWS]) == want, p
    return p


def _mu_ref(X, S, D, clamp=False):
    q = np.where(D > 0, X * S / np.where(D > 0, D, 1.0), 0.0)
    return np.maximum(q, EPS32) if clamp else q


T32 = (32, 32)


# ------------------------------------------------------------------------------------------------------------- A H^T, W^T A, fused W
# MI355X: 0.01 - 0.16 s per case (0.5 s for the first, which loads the library); the generators and comparisons on the host are most of it
@pytest.mark.parametrize("case,bf16", F32_CASES + BF16_CASES)
def test_frobenius_products(env, case, bf16):
    """aht, wta EQUAL float64 and aht_update_w within 3 ulps, fp32 and bf16-stored A: split3_rows / ntx (every KT, the interior and the
    edge instantiation, wfast on and off), split3_cols / tnx (every KT, one to four row chunks, a ragged last one) -- the integer
    family, then the pieces families"""
    engine, lib = env
    o6 = engine.HIP_OPS_BF16X6
    _, m, n, k, lda, fal, want = case

    def run_aht(A, H, what):
        Av, Hv, o = _A(A, bf16, lda), _P(H, fal), _out(m, k, fal)
        _assert_fro_plan(lib, Av, k, want)
        o6.aht(Av.view, Hv.view, o.view)
        ex.assert_ulp(o.check(what), ex._mm(A, H, "aht"), 0, what, tile=T32)
        Av.check("A"); Hv.check("H")

    def run_wta(A, W, what):
        Av, Wv, o = _A(A, bf16, lda), _P(W, fal), _out(k, n, fal)
        _assert_fro_plan(lib, Av, k, want)
        o6.wta(Av.view, Wv.view, o.view)
        ex.assert_ulp(o.check(what), ex._mm(A, W, "wta"), 0, what, tile=T32)
        Av.check("A"); Wv.check("W")

    def run_fused(A, H, W, G, what):
        Av, Hv, Wv = _A(A, bf16, lda), _P(H, fal), _P(W, fal)
        p = _assert_fro_plan(lib, Av, k, want)
        o6.aht_update_w(Av.view, Hv.view, _gram(engine, G), Wv.view, EPS)
        W64 = W.astype(np.float64)
        ex.assert_ulp(Wv.check(what), _mu_ref(W64, ex._mm(A, H, "aht"), W64 @ G), 3, what, tile=T32)
        Av.check("A"); Hv.check("H")
        return p

    A, W, H = ex.products(m, n, k)
    run_aht(A, H, "aht (integers)")
    run_wta(A, W, "wta (integers)")
    H64 = H.astype(np.float64)
    run_fused(A, H, W, H64 @ H64.T, "aht_update_w (integers)")
    rs = np.random.RandomState(m + n + k)
    G = ex._sym_gram(k, rs)                                          # W G: integers >= 2 below 2^22, eps is absorbed
    Wi = rs.randint(1, 4, size=(m, k)).astype(np.float32)
    Wi[rs.rand(m) < 0.05] = 0
    for rot in ex.x6_rots(n):
        A, H = ex.pieces_product(m, n, k, "aht", bf16a=bf16, rot=rot)
        run_aht(A, H, "aht (pieces, rot %d)" % rot)
        run_fused(A, H, Wi, G, "aht_update_w (pieces, rot %d)" % rot)
    for rot in ex.x6_rots(m):
        A, W = ex.pieces_product(m, n, k, "wta", bf16a=bf16, rot=rot)
        run_wta(A, W, "wta (pieces, rot %d)" % rot)


# MI355X: 0.06 s and less per case
@pytest.mark.parametrize("case", [pytest.param(c, id=c[0]) for c in ex.X6_FALLBACK])
def test_ranks_below_the_kernels_give_the_bits_of_the_fp32_route(env, case):
    """k = 32 with fp32 A and k = 16 with bf16-stored A: the plan reports the fp32 route, and aht, wta, aht_update_w give the bits of
    HIP_OPS on random data (where any other arithmetic would differ)"""
    engine, lib = env
    ops, o6 = engine.HIP_OPS, engine.HIP_OPS_BF16X6
    _, m, n, k, bf16 = case
    rs = np.random.RandomState(k)
    A, W, H = (rs.rand(*s).astype(np.float32) for s in ((m, n), (m, k), (k, n)))
    Av = _A(A, bf16)
    assert _plan(lib, Av, k)[FRO] == 0
    H64 = H.astype(np.float64)
    got = {}
    for o in (ops, o6):
        Hv, Wv, W2 = _P(H), _P(W), _P(W)
        o1, o2 = _out(m, k), _out(k, n)
        o.aht(Av.view, Hv.view, o1.view)
        o.wta(Av.view, Wv.view, o2.view)
        o.aht_update_w(Av.view, Hv.view, _gram(engine, H64 @ H64.T), W2.view, EPS)
        got[o.name] = (o1.check("aht"), o2.check("wta"), W2.check("aht_update_w"))
    for a, b, what in zip(got[ops.name], got[o6.name], ("aht", "wta", "aht_update_w")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: bf16x6 differs from the fp32 entry point on a shape without a split kernel" % what
    Av.check("A")


# ------------------------------------------------------------------------------------------------------------- whole MU/FRO steps
# MI355X: 0.02 s and less per case
@pytest.mark.parametrize("case,bf16", F32_CASES + BF16_CASES)
def test_mu_fro_step(env, case, bf16):
    """mu_fro_step_bf16x6 on `fro_step` operands, clamp off and on: the new W exact, the new H within 3 ulps"""
    engine, lib = env
    _, m, n, k, lda, fal, want = case
    A, W, H, Wn, Hq = ex.fro_step(m, n, k)
    for clamp in (False, True):
        Av, Wv, Hv = _A(A, bf16, lda), _P(W, fal), _P(H, fal)
        _assert_fro_plan(lib, Av, k, want)
        engine.HIP_OPS_BF16X6.mu_fro_step(Av.view, Wv.view, Hv.view, EPS, True, clamp)
        Av.check("A")
        w, h = Wv.check("W"), Hv.check("H")
        Wr, Hr = (np.maximum(Wn, EPS32), np.maximum(Hq, EPS32)) if clamp else (Wn, Hq)
        ex.assert_ulp(w, Wr, 0, "mu_fro_step clamp=%s W (exact)" % clamp, tile=T32)
        ex.assert_ulp(h, Hr, 3, "mu_fro_step clamp=%s H" % clamp, tile=T32)


# ------------------------------------------------------------------------------------------------------------- KL
def _assert_kl_plan(lib, Av, k, want):
    p = _plan(lib, Av, k)
    assert p[KL] == 1, "not a split shape: the fp32 kernels would run"
    assert (p[KT], p[WTUX_CHUNKS], p[WTUX_BLOCKS], p[UHTX_SPLITS], p[UHTX_COLS]) == want, p


# MI355X: 0.01 - 0.15 s per case
@pytest.mark.parametrize("case", KL_CASES)
def test_kl_products(env, case):
    """kl_uht (one, two and three column splits; the direct store of k columns) and kl_wtu (one to eight row chunks, a workgroup with
    one live wave) EQUAL float64: the integer family `kl`, then every kind of `kl_pieces`"""
    engine, lib = env
    o6 = engine.HIP_OPS_BF16X6
    _, m, n, k, lda, fal, want = case
    probs = [("integers",) + ex.kl(m, n, k)]
    probs += [("pieces %s rot %d" % (kind, rot),) + ex.kl_pieces(m, n, k, kind, rot=rot) for kind in ex.KLX_KINDS for rot in ex.klx_rots(m)]
    for what, A, W, H, U in probs:
        Av, Wv, Hv = _A(A, False, lda), _P(W, fal), _P(H, fal)
        _assert_kl_plan(lib, Av, k, want)
        o = _out(m, k, fal)
        o6.kl_uht(Av.view, Wv.view, Hv.view, EPS, o.view)
        ex.assert_ulp(o.check("kl_uht"), U @ H.astype(np.float64).T, 0, "kl_uht (%s)" % what, tile=T32)
        o = _out(k, n, fal)
        o6.kl_wtu(Av.view, Wv.view, Hv.view, EPS, o.view)
        ex.assert_ulp(o.check("kl_wtu"), W.astype(np.float64).T @ U, 0, "kl_wtu (%s)" % what, tile=T32)
        for v, name in ((Av, "A"), (Wv, "W"), (Hv, "H")):
            v.check(name)


# MI355X: 0.02 s and less per case
@pytest.mark.parametrize("case", KL_CASES)
def test_mu_kl_step(env, case):
    """mu_kl_step_bf16x6 on `kl` operands.  W fixed: the quotient U stays exact, H within 3 ulps, W untouched.  W moving: W within 3
    ulps; H comes from the kernel's new W, whose quotient is no longer exact: 1e-5 of each element (as test_gpu_exact.py::test_kl)"""
    engine, lib = env
    o6 = engine.HIP_OPS_BF16X6
    _, m, n, k, lda, fal, want = case
    A, W, H, U = ex.kl(m, n, k)
    _, _, _, _, Wq, Hq = ex.kl_refs(A, W, H, U)
    Av, Wv, Hv = _A(A, False, lda), _P(W, fal), _P(H, fal)
    _assert_kl_plan(lib, Av, k, want)
    o6.mu_kl_step(Av.view, Wv.view, Hv.view, EPS, False, False)
    ex.assert_ulp(Hv.check("H"), Hq, 3, "mu_kl_step (W fixed) H", tile=T32)
    ex.assert_ulp(Wv.check("W"), W.astype(np.float64), 0, "mu_kl_step (W fixed) W", tile=T32)
    Wv, Hv = _P(W, fal), _P(H, fal)
    o6.mu_kl_step(Av.view, Wv.view, Hv.view, EPS, True, False)
    Wn = Wv.check("W")
    ex.assert_ulp(Wn, Wq, 3, "mu_kl_step W", tile=T32)
    Wn64 = Wn.astype(np.float64)
    Un = A.astype(np.float64) / (Wn64 @ H.astype(np.float64) + EPS)
    Hn = H.astype(np.float64) * (Wn64.T @ Un) / (Wn64.sum(0) + EPS)[:, None]
    h = Hv.check("H")
    bad = ~(np.abs(h - Hn) <= 1e-5 * np.abs(Hn))
    assert not bad.any(), "mu_kl_step H off by more than 1e-5 at %s" % (tuple(np.argwhere(bad)[0]),)
    Av.check("A")


# ------------------------------------------------------------------------------------------------------------- A past the caches
# MI355X: 0.74 s (fp32, 32768 x 2048) and 1.18 s (bf16, 65536 x 2048), generators included: the default tier
STREAMED_CASES = [pytest.param(c, id=c[0]) for c in ex.X6_STREAMED]


@pytest.mark.parametrize("case", STREAMED_CASES)
def test_streamed_products(env, case):
    """A of exactly 256 MiB: ntx and tnx in the instantiations that stream A past the caches (AUX = 2, asserted through the plan).  aht
    and wta EQUAL float64 -- integers made and multiplied in float64 on the device, then the pieces family"""
    engine, lib = env
    o6 = engine.HIP_OPS_BF16X6
    _, m, n, k, bf16, want = case
    g = torch.Generator(device="cuda").manual_seed(11)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, device="cuda", generator=g, dtype=torch.int32).float()
    A, H, W = ri(0, 8, (m, n)), ri(1, 4, (k, n)), ri(1, 4, (m, k))        # sums below 65536 * 7 * 3 < 2^24
    if bf16:
        A = A.to(torch.bfloat16)
    try:
        class V:
            view, dtype = A, A.dtype
        p = _assert_fro_plan(lib, V, k, want)
        assert (p[NTX_STREAMED], p[TNX_STREAMED]) == (1, 1)
        o = _out(m, k)
        o6.aht(A, H, o.view)
        o.check("aht")
        assert torch.equal(o.view.double(), A.double() @ H.double().T), "aht (integers)"
        o = _out(k, n)
        o6.wta(A, W, o.view)
        o.check("wta")
        assert torch.equal(o.view.double(), W.double().T @ A.double()), "wta (integers)"
        del A
        for side, rows, cols in (("aht", m, k), ("wta", k, n)):
            An, F = ex.pieces_product(m, n, k, side, bf16a=bf16)
            A = torch.from_numpy(An).cuda()
            A = A.to(torch.bfloat16) if bf16 else A
            Fv, o = _P(F), _out(rows, cols)
            (o6.aht if side == "aht" else o6.wta)(A, Fv.view, o.view)
            ex.assert_ulp(o.check(side), ex._mm(An, F, side), 0, "%s (pieces)" % side, tile=T32)
            del A
    finally:
        A = None
        torch.cuda.empty_cache()
