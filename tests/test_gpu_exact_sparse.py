"""The sparse (CSR) kernels against the exact answer, element by element (csrc/dnmf_csr.h through engine.HipCsrOps): the operands of
tests/_exact.py (`sparse_products`, `sparse_kl`; tests/test_exact_cpu.py proves them) make every sum these kernels form exact in
fp32 in any order, and the residuals exact in float64, so every output element must EQUAL the float64 answer.  One dropped stored
entry, one lane group folded twice, one column written at k instead of k - 1 fails here; the relative Frobenius norms of
test_gpu_sparse / test_gpu_masked cannot see any of them.  The fused endings are held to a reference built from the exact float64
pair, never from the library's own pair.

The stored pattern is `_exact.LENS` x 3100: rows of NG - 1 / NG / NG + 1 entries for every lane-group count NG = 256 / KPAD, of 63 / 64 /
65 (the pairs a wave reads per step), of 1023 / 1024 / 1025 and 2047 / 2048 / 2049 (the segments of a long row), empty rows, two empty
columns.  Every case runs on the block of A and on the block of A^T with the factor roles swapped, so the prescribed lengths pass
through the row image (out_trans = 0) and through the transposed image (out_trans = 1), and each factor is once the lane-dense side
of the KL dot product.  The tests assert that the blocks really have long rows where they are meant to.  k sits on both sides of every
KPAD boundary; the views alternate between 16-byte aligned ones with a padded pitch and odd starts with an odd pitch.  Every factor
is a view in a NaN-poisoned buffer and every output a view in a sentinel-filled buffer (`_exact.Poisoned`).

Ulp bounds per element (c: |x - q| <= c spacing(float32(q)), q the float64 reference; a zero must be exactly zero):
  aht, wta, wta_gram, kl_uht, kl_wtu, both halves of masked_aht_pair / masked_wta_pair ('fro', 'kl')      exact (c = 0)
  resid_sqnorm, dense meaning and missing='unstored'                                                     == the float64 integer
  masked_update_w, masked_update_h, ratio_update                                                         c = 2
The last line: the kernels evaluate x * (num / (den + eps)) (csr_ratio1).  num and den are exact on these operands and den + eps is
one correctly rounded fp32 addition, which the reference reproduces: q = x num / float32(den + eps).  What is left is one IEEE
division (the library is built without fast-math: hipcc's fp32 division is correctly rounded, relative error <= 2^-24) and one
multiplication (another 2^-24): a relative error below 2^-23 + 2^-48, and one ulp of the result is at least 2^-24 of it, so the
result is within 2 ulps -- the bound tests/test_gpu_exact.py uses for the same sequence in the KL element-wise updates.  A row or
column without a stored entry, or a zero factor element, gives exactly 0 (exactly eps with the clamp: an element below eps gives eps)."""
import numpy as np
import pytest

from tests import _exact as ex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
EPS32 = np.float32(EPS)
SEG = 1024

# k on both sides of every KPAD boundary (16 / 32 / 64 / 128 / 256), aligned and unaligned views in turn
KS = [1, 3, 4, 5, 16, 17, 32, 33, 64, 65, 128, 129, 256]
CASES = [pytest.param(k, i % 2 == 0, id="k%d-%s" % (k, "aligned" if i % 2 == 0 else "unaligned")) for i, k in enumerate(KS)]
SIDES = ["A", "At"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pydnmfk_amd.engine import HIP_CSR_OPS
    return HIP_CSR_OPS


@pytest.fixture(scope="module")
def pattern():
    return ex.lens_pattern()


def _P(x, aligned):
    return ex.Poisoned(torch, np.asarray(x, dtype=np.float32), aligned=aligned)


def _out(rows, cols, aligned):
    return ex.Poisoned.out(torch, rows, cols, torch.float32, aligned)


def _block(A, mask, missing=None):
    """the block whose stored positions are exactly `mask` (observed zeros stay stored under missing='unstored')"""
    from pydnmfk_amd.sparse import SparseBlock
    r, c = np.nonzero(mask)
    blk = SparseBlock.from_coo(torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(np.ascontiguousarray(A[r, c])).cuda(),
                               mask.shape, keep_zeros=missing is not None, missing=missing)
    assert blk.nnz == int(mask.sum()), "the block dropped stored entries"
    assert np.array_equal((blk.crow[1:] - blk.crow[:-1]).cpu().numpy(), mask.sum(1))
    assert np.array_equal((blk.t_crow[1:] - blk.t_crow[:-1]).cpu().numpy(), mask.sum(0))
    return blk


def _segments(lengths):
    lengths = np.asarray(lengths)
    long_ = lengths[lengths > SEG]
    return len(long_), int(np.sum(-(-long_ // SEG)))


def _oriented(side, A, mask, W, H, missing=None):
    """the problem on the block of A or of A^T (factor roles swapped), and the precondition: the long rows go through the segment
    kernels of the row image on A and of the transposed image on A^T"""
    if side == "At":
        A, mask, W, H = ex.transposed(A, mask, W, H)
    blk = _block(A, mask, missing)
    n_long, nseg = _segments(ex.LENS)
    assert n_long >= 5 and nseg == 13
    row_side = (blk.n_long, blk.nseg, blk.t_n_long, blk.t_nseg)
    assert row_side == ((n_long, nseg, 0, 0) if side == "A" else (0, 0, n_long, nseg)), row_side
    return A, mask, W, H, blk


def _checked(views):
    for v, what in views:
        v.check(what)


def _problem(gen, mask, k, **kw):
    """(side-independent) A, mask, W, H of a generator"""
    A, W, H = gen(mask, k, **kw)
    return A, mask, W, H


# ------------------------------------------------------------------------------------------------------------- products
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("k,aligned", CASES)
def test_products(ops, pattern, k, aligned, side):
    """aht, wta, wta_gram on `sparse_products`, kl_uht, kl_wtu on `sparse_kl`: exactly float64"""
    from pydnmfk_amd import engine
    A, mask, W, H, blk = _oriented(side, *_problem(ex.sparse_products, pattern, k))
    m, n = mask.shape
    ref = ex.sparse_exact(A, mask, W, H)
    Wv, Hv = _P(W, aligned), _P(H, aligned)
    o = _out(m, k, aligned)
    ops.aht(blk, Hv.view, o.view)
    ex.assert_ulp(o.check("aht"), ref["aht"], 0, "aht")
    o = _out(k, n, aligned)
    ops.wta(blk, Wv.view, o.view)
    ex.assert_ulp(o.check("wta"), ref["wta"], 0, "wta")
    o = _out(k, n, aligned)
    G = engine.new_gram(k, torch.device("cuda"))
    G.fill_(7.0)
    ops.wta_gram(blk, Wv.view, o.view, G)
    ex.assert_ulp(o.check("wta_gram"), ref["wta"], 0, "wta_gram product")
    g = G.cpu().numpy()
    ex.assert_ulp(g[:k, :k], ref["gram_w"], 0, "wta_gram Gram")
    assert not g[k:].any() and not g[:, k:].any(), "wta_gram: the zero padding of the Gram was not written"
    _checked(((Wv, "W"), (Hv, "H")))

    A, mask, W, H, blk = _oriented(side, *_problem(ex.sparse_kl, pattern, k))
    ref = ex.sparse_exact(A, mask, W, H, kl=True)
    Wv, Hv = _P(W, aligned), _P(H, aligned)
    o = _out(m, k, aligned)
    ops.kl_uht(blk, Wv.view, Hv.view, EPS, o.view)
    ex.assert_ulp(o.check("kl_uht"), ref["uht"], 0, "kl_uht")
    o = _out(k, n, aligned)
    ops.kl_wtu(blk, Wv.view, Hv.view, EPS, o.view)
    ex.assert_ulp(o.check("kl_wtu"), ref["wtu"], 0, "kl_wtu")
    _checked(((Wv, "W"), (Hv, "H")))


# ------------------------------------------------------------------------------------------------------------- masked passes
def _masked_problem(norm, pattern, k):
    return _problem(ex.sparse_kl if norm == "kl" else ex.sparse_products, pattern, k, stored_zeros=True)


def _pairs(ref, norm):
    """the exact float64 pairs (num_w, den_w, num_h, den_h) of a norm"""
    return (ref["aht"], ref["den_w"], ref["wta"], ref["den_h"]) if norm == "fro" else (ref["uht"], ref["klden_w"], ref["wtu"], ref["klden_h"])


@pytest.mark.parametrize("norm", ["fro", "kl"])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("k,aligned", CASES)
def test_masked_pairs(ops, pattern, k, aligned, side, norm):
    """masked_aht_pair, masked_wta_pair with observed zeros: numerator and denominator exactly float64"""
    A, mask, W, H, blk = _oriented(side, *_masked_problem(norm, pattern, k), missing="unstored")
    assert ((A == 0) & mask).sum() >= 3
    m, n = mask.shape
    nw, dw, nh, dh = _pairs(ex.sparse_exact(A, mask, W, H, kl=norm == "kl"), norm)
    Wv, Hv = _P(W, aligned), _P(H, aligned)
    for fn, rows, cols, num, den in ((ops.masked_aht_pair, m, k, nw, dw), (ops.masked_wta_pair, k, n, nh, dh)):
        pair = ex.Poisoned(torch, np.full((2 * rows, cols), ex.SENTINEL, np.float32), fill=ex.SENTINEL, aligned=aligned, packed=True)
        gn, gd = fn(blk, Wv.view, Hv.view, EPS, norm, pair.view.reshape(-1))      # ONE contiguous [num | den]
        assert gn.data_ptr() == pair.view.data_ptr() and gd.data_ptr() == gn.data_ptr() + 4 * rows * cols
        got = pair.check(fn.__name__)
        ex.assert_ulp(got[:rows], num, 0, "%s %s numerator" % (fn.__name__, norm))
        ex.assert_ulp(got[rows:], den, 0, "%s %s denominator" % (fn.__name__, norm))
    _checked(((Wv, "W"), (Hv, "H")))


def _ratio_ref(X, num, den, clamp=False):
    """x num / float32(den + eps), the addition rounded to fp32 as the kernel rounds it; float64 otherwise"""
    d32 = (den + np.float64(EPS32)).astype(np.float32).astype(np.float64)
    q = X.astype(np.float64) * num / d32
    return np.maximum(q, np.float64(EPS32)) if clamp else q


def _assert_ratio(got, q, clamp, what):
    ex.assert_ulp(got, q, 2, what)
    if clamp:                                                               # what the clamp raised is eps itself, not near it
        low = q <= np.float64(EPS32)
        assert low.any() and np.all(got[low] == EPS32), "%s: a clamped element is not eps" % what
    else:
        assert (q == 0).any()


@pytest.mark.parametrize("norm", ["fro", "kl"])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("k,aligned", CASES)
def test_masked_updates(ops, pattern, k, aligned, side, norm):
    """the fused endings and ratio_update on pitched factors, against x num / float32(den + eps) from the EXACT pair: c = 2"""
    A, mask, W, H, blk = _oriented(side, *_masked_problem(norm, pattern, k), missing="unstored")
    nw, dw, nh, dh = _pairs(ex.sparse_exact(A, mask, W, H, kl=norm == "kl"), norm)
    empty_r, empty_c = mask.sum(1) == 0, mask.sum(0) == 0
    assert empty_r.any() and empty_c.any()
    for clamp in (False, True):
        qw, qh = _ratio_ref(W, nw, dw, clamp), _ratio_ref(H, nh, dh, clamp)
        Wv, Hv = _P(W, aligned), _P(H, aligned)
        if not clamp:                                                       # (masked_update_w has no clamp)
            ops.masked_update_w(blk, Wv.view, Hv.view, EPS, norm)
            got = Wv.check("masked_update_w")
            _assert_ratio(got, qw, False, "masked_update_w %s" % norm)
            assert not got[empty_r].any(), "masked_update_w: a row without a stored entry is not zero"
            Hv.check("H")
            Wv = _P(W, aligned)
        ops.masked_update_h(blk, Wv.view, Hv.view, EPS, norm, clamp=clamp)
        got = Hv.check("masked_update_h")
        _assert_ratio(got, qh, clamp, "masked_update_h %s clamp=%d" % (norm, clamp))
        assert np.all(got[:, empty_c] == (EPS32 if clamp else 0)), "masked_update_h: a column without a stored entry"
        Wv.check("W")
        # the element-wise pass that follows an allreduce of the pair: V = 4 on aligned views with cols % 4 == 0, else V = 1
        for X, num, den, q, what in ((W, nw, dw, qw, "W"), (H, nh, dh, qh, "H")):
            Xv, Nv, Dv = _P(X, aligned), _P(num, aligned), _P(den, aligned)
            ops.ratio_update(Xv.view, Nv.view, Dv.view, EPS, clamp=clamp)
            _assert_ratio(Xv.check("ratio_update"), q, clamp, "ratio_update %s %s clamp=%d" % (what, norm, clamp))
            _checked(((Nv, "num"), (Dv, "den")))


@pytest.mark.parametrize("aligned", [True, False], ids=["V4", "V1"])
def test_ratio_update_paths(ops, pattern, aligned):
    """ratio_update once on 16-byte aligned views with a pitch and a width that are multiples of 4 (csr_ratio_kernel<4>) and once on
    odd starts with an odd pitch (csr_ratio_kernel<1>), clamp off and on"""
    k = 64
    A, mask, W, H = _masked_problem("fro", pattern, k)
    nw, dw, nh, dh = _pairs(ex.sparse_exact(A, mask, W, H), "fro")
    for X, num, den in ((W, nw, dw), (H, nh, dh)):
        for clamp in (False, True):
            Xv, Nv, Dv = _P(X, aligned), _P(num, aligned), _P(den, aligned)
            vec = all(v.view.data_ptr() % 16 == 0 and v.ld % 4 == 0 for v in (Xv, Nv, Dv)) and X.shape[1] % 4 == 0
            assert vec == aligned
            ops.ratio_update(Xv.view, Nv.view, Dv.view, EPS, clamp=clamp)
            _assert_ratio(Xv.check("ratio_update"), _ratio_ref(X, num, den, clamp), clamp, "ratio_update V=%d clamp=%d" % (4 if vec else 1, clamp))
            _checked(((Nv, "num"), (Dv, "den")))


# ------------------------------------------------------------------------------------------------------------- residuals
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("k,aligned", CASES)
def test_resid_sqnorm(ops, pattern, k, aligned, side):
    """||A - W H||^2 (closed form: Gram term plus a pass over the stored entries) and its restriction to the stored positions: the
    float64 integer itself"""
    for missing, key in ((None, "resid"), ("unstored", "resid_masked")):
        A, mask, W, H, blk = _oriented(side, *_problem(ex.sparse_products, pattern, k, stored_zeros=missing is not None), missing=missing)
        ref = ex.sparse_exact(A, mask, W, H)[key]
        assert ref > 0 and ref == float(int(ref))
        Wv, Hv = _P(W, aligned), _P(H, aligned)
        got = float(ops.resid_sqnorm(blk, Wv.view, Hv.view).cpu())
        assert got == ref, "resid_sqnorm (missing=%r): got %r, expected %r (off by %g)" % (missing, got, ref, got - ref)
        _checked(((Wv, "W"), (Hv, "H")))


@pytest.fixture(scope="module")
def many_rows():
    """2 * 8192 + 5 rows of 0..5 entries: the residual's row pass has 8192 waves, so each takes three rows (two for the last ones)"""
    lengths = np.random.RandomState(11).randint(0, 6, size=2 * 8192 + 5)
    return ex.sparse_pattern(lengths, 70, seed=1)


@pytest.mark.parametrize("k", [3, 17, 256])
def test_resid_sqnorm_many_rows(ops, many_rows, k):
    """more rows than waves (CSR_RESID_WAVES = 8192): every wave loops over its rows; the Gram chunks (497 rows at k = 3, 17) are no
    multiple of the Gram kernel's 64-row slab"""
    m, n = many_rows.shape
    assert m == 2 * 8192 + 5 and m > 2 * 8192 and -(-m // 33) == 497
    for missing, key in ((None, "resid"), ("unstored", "resid_masked")):
        A, W, H = ex.sparse_products(many_rows, k, stored_zeros=missing is not None)
        blk = _block(A, many_rows, missing)
        assert blk.n_long == 0 and blk.t_n_long == 0                       # (the row pass alone: no segment kernels here)
        ref = ex.sparse_exact(A, many_rows, W, H)[key]
        assert ref > 0 and ref == float(int(ref))
        Wv, Hv = _P(W, k != 17), _P(H, k != 17)
        got = float(ops.resid_sqnorm(blk, Wv.view, Hv.view).cpu())
        assert got == ref, "resid_sqnorm (missing=%r): got %r, expected %r (off by %g)" % (missing, got, ref, got - ref)
        _checked(((Wv, "W"), (Hv, "H")))
