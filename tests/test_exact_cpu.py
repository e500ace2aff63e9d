"""The exact-operand generators of tests/_exact.py keep their promise: on their operands every product and every partial sum is
exact in fp32, so a float32 evaluation in any order -- numpy's BLAS matmul with its own blocking, a sequential sum from either
end -- equals float64 bit for bit.  This proves the generators, not the kernels (tests/test_gpu_exact.py holds those to it)."""
import numpy as np
import pytest

from tests import _exact as ex

SHAPES = [(33, 47, 1), (64, 129, 5), (130, 72, 17), (257, 131, 33), (96, 515, 65), (40, 300, 129), (48, 520, 256)]


def _seq(X, Y, reverse=False):
    """X @ Y in float32 as one sequential sum over the contraction index, from the front or from the back"""
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    acc = np.zeros((X.shape[0], Y.shape[1]), dtype=np.float32)
    order = range(X.shape[1] - 1, -1, -1) if reverse else range(X.shape[1])
    for t in order:
        acc += np.outer(X[:, t], Y[t])
    return acc


def _all_orders(X, Y, what):
    ref = X.astype(np.float64) @ Y.astype(np.float64)
    for got, how in ((X.astype(np.float32) @ Y.astype(np.float32), "BLAS"), (_seq(X, Y), "forward"), (_seq(X, Y, True), "reversed")):
        assert np.array_equal(got.astype(np.float64), ref), "%s (%s) is not exact in float32" % (what, how)
    return ref


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_products_are_exact(m, n, k):
    A, W, H = ex.products(m, n, k)
    _all_orders(A, H.T, "A H^T")
    _all_orders(W.T, A, "W^T A")
    G = _all_orders(H, H.T, "H H^T")
    GW = _all_orders(W.T, W, "W^T W")
    eps = np.float32(np.finfo(np.float32).eps)
    for d, what in ((_all_orders(W, G, "W G"), "W G"), (_all_orders(GW, H, "G H"), "G H")):
        d32 = d.astype(np.float32)
        assert np.array_equal(d32[d > 0] + eps, d32[d > 0]), "%s + eps is not absorbed" % what
    for x in (A, W, H):                                                    # bf16 storage and the bf16x6 split are exact too
        assert np.array_equal(x, x.astype(np.float32).view(np.uint32).__and__(0xFFFF0000).view(np.float32))
    A64, _, _ = ex.products(m, n, k, np.float64)
    assert np.array_equal(A64, A.astype(np.float64))


@pytest.mark.parametrize("m,n,k", [(64, 129, 5), (130, 72, 17), (257, 600, 16), (1000, 2052, 32), (4096, 8192, 16), (40, 300, 33)])
def test_fro_step_is_exact(m, n, k):
    """the W phase of one MU/Frobenius step is exact in float32 in every order; the H phase's numerator and denominator are"""
    A, W, H, Wn, Hq = ex.fro_step(m, n, k)
    small = m * n * k <= 4e6
    G = _all_orders(H, H.T, "H H^T") if small else H.astype(np.float64) @ H.T
    AH = _all_orders(A, H.T, "A H^T") if small else A.astype(np.float64) @ H.T
    WG = W.astype(np.float32) @ G.astype(np.float32)
    assert np.array_equal(WG.astype(np.float64), W.astype(np.float64) @ G)
    eps = np.float32(np.finfo(np.float32).eps)
    Wn32 = W * (AH.astype(np.float32) * (np.float32(1) / (WG + eps)))     # s rcp(d), then w: exact on these operands
    assert np.array_equal(Wn32.astype(np.float64), Wn)
    num = Wn32.T @ A
    den = (Wn32.T @ Wn32) @ H
    assert np.array_equal(num.astype(np.float64), Wn.T @ A.astype(np.float64))
    assert np.array_equal(den.astype(np.float64), (Wn.T @ Wn) @ H.astype(np.float64))
    assert np.array_equal(den[den > 0] + eps, den[den > 0])
    ex.assert_ulp(H * (num * (np.float32(1) / (den + eps))), Hq, 3, "H phase in float32")


@pytest.mark.parametrize("m,n,k", [(64, 129, 5), (130, 72, 17), (257, 600, 33), (33, 515, 64), (40, 300, 129)])
def test_kl_quotient_is_exact(m, n, k):
    A, W, H, U = ex.kl(m, n, k)
    WH = _all_orders(W, H, "W H")
    eps = np.float32(np.finfo(np.float32).eps)
    U32 = A / (WH.astype(np.float32) + eps)
    assert np.array_equal(U32.astype(np.float64), U)
    _all_orders(U32, H.T, "U H^T")
    _all_orders(W.T, U32, "W^T U")
    assert np.array_equal(H.sum(1, dtype=np.float32).astype(np.float64), H.astype(np.float64).sum(1))


def test_ulp_comparator_reports_the_first_bad_element():
    q = np.arange(1, 1 + 40 * 70, dtype=np.float64).reshape(40, 70) / 3.0
    x = q.astype(np.float32)
    ex.assert_ulp(x, q, 1)
    with pytest.raises(AssertionError):
        ex.assert_ulp(x, q, 0)                                             # 1/3 is not exact
    y = x.copy()
    y[37, 65] = np.nextafter(np.nextafter(y[37, 65], np.float32(np.inf)), np.float32(np.inf))
    with pytest.raises(AssertionError, match=r"\(37, 65\) in tile \(2, 2\) of \(3, 3\) \[last row tile\] \[last column tile\]"):
        ex.assert_ulp(y, q, 1)
    z = x.copy()
    z[0, 0], q2 = 1e-30, q.copy()
    q2[0, 0] = 0.0
    with pytest.raises(AssertionError, match=r"first at \(0, 0\)"):
        ex.assert_ulp(z, q2, 3)                                             # a zero must be exactly zero


# ---------------------------------------------------------------------------------------------------------- sparse (CSR) blocks
SPARSE_KS = (1, 17, 64, 129, 256)
SEG = 1024                                                                  # entries of one segment of a long row (csrc/dnmf_csr.h)


def _kpad(k):
    return next(p for p in (16, 32, 64, 128, 256) if k <= p)


def _gather_orders(mask, coef, F, ng, dtype=np.float32):
    """out[r] = sum over the stored c of row r of coef[r][c] F[c], in `dtype`, three ways: the stored entries front to back, back to
    front, and as the kernels do it -- entry j of a segment of SEG entries goes to lane group j % ng, every group sums its entries in
    order, the groups are folded by an xor butterfly (neighbours first), the segments are added in order.  coef is zero off the mask,
    and adding an exact zero changes nothing, so the dense loop over c IS the sparse sum."""
    m, n = mask.shape
    k = F.shape[1]
    coef, F = coef.astype(dtype), F.astype(dtype)
    rank = np.where(mask, np.cumsum(mask, 1) - 1, 0)
    nseg = int(rank.max(initial=0)) // SEG + 1
    fwd, rev = np.zeros((m, k), dtype), np.zeros((m, k), dtype)
    parts = np.zeros((nseg, ng, m, k), dtype)
    rows = np.arange(m)
    for c in range(n):
        t = coef[:, c, None] * F[c]
        fwd += t
        parts[rank[:, c] // SEG, rank[:, c] % ng, rows] += t
    for c in range(n - 1, -1, -1):
        rev += coef[:, c, None] * F[c]
    while parts.shape[1] > 1:
        parts = parts[:, 0::2] + parts[:, 1::2]
    ker = np.zeros((m, k), dtype)
    for s in range(nseg):
        ker += parts[s, 0]
    return fwd, rev, ker


def _exact_in_all_orders(mask, coef, F, ng, ref, what, dtype=np.float32):
    for got, how in zip(_gather_orders(mask, coef, F, ng, dtype), ("forward", "reversed", "lane groups")):
        assert np.array_equal(got.astype(np.float64), ref), "%s (%s, %d lane groups) is not exact in %s" % (what, how, ng, np.dtype(dtype))


@pytest.fixture(scope="module")
def lens_mask():
    return ex.lens_pattern()


def test_sparse_pattern_has_the_prescribed_rows(lens_mask):
    assert lens_mask.shape == (27, 3100) and lens_mask.dtype == bool
    assert lens_mask.sum(1).tolist() == ex.LENS
    assert np.array_equal(lens_mask, ex.lens_pattern())                                # the same pattern every time
    assert lens_mask.sum(0).max() <= 27 and (lens_mask.sum(0) == 0).any()              # the transpose has short and empty rows
    many = ex.sparse_pattern(np.arange(2 * 8192 + 5) % 6, 70, seed=1)
    assert np.array_equal(many.sum(1), np.arange(2 * 8192 + 5) % 6)


@pytest.mark.parametrize("k", SPARSE_KS)
def test_sparse_products_are_exact(lens_mask, k):
    """every pass of the Frobenius side on `sparse_products` operands, on the block and on its transpose, in every order"""
    eps = np.float32(np.finfo(np.float32).eps)
    ng = 256 // _kpad(k)
    prob = ex.sparse_products(lens_mask, k, stored_zeros=True)
    assert ((prob[0] == 0) & lens_mask).sum() >= 3                                     # observed zeros
    assert (prob[1].sum(1) == 0).any() and (prob[2].sum(0) == 0).any()                 # a zero row of W, a zero column of H
    for A, mask, W, H in ((prob[0], lens_mask) + prob[1:], ex.transposed(prob[0], lens_mask, *prob[1:])):
        ref = ex.sparse_exact(A, mask, W, H)
        D = _all_orders(W, H, "W H")
        PD = np.where(mask, D, 0.0)
        _exact_in_all_orders(mask, A, H.T, ng, ref["aht"], "A H^T")
        _exact_in_all_orders(mask, PD, H.T, ng, ref["den_w"], "P(W H) H^T")
        _exact_in_all_orders(mask.T, A.T, W, ng, ref["wta"].T, "W^T A")
        _exact_in_all_orders(mask.T, PD.T, W, ng, ref["den_h"].T, "W^T P(W H)")
        _all_orders(W.T, W, "W^T W")
        for den in (ref["den_w"], ref["den_h"]):                                       # what the fused ending divides by is one rounding
            d32 = den.astype(np.float32)
            assert np.array_equal(d32.astype(np.float64), den) and np.all(np.isfinite(prob[0].max() * d32.max() / eps))
        # the residuals: float64 sums of integers, against integer arithmetic
        Ai, Di = A.astype(np.int64), W.astype(np.int64) @ H.astype(np.int64)
        Mi = mask.astype(np.int64)
        gram = int(np.sum((W.astype(np.int64).T @ W.astype(np.int64)) * (H.astype(np.int64) @ H.astype(np.int64).T)))
        cross, sq = Ai * (Ai - 2 * Di), Mi * (Ai - Di) ** 2
        assert gram + int(cross.sum()) == int(((Ai - Di) ** 2).sum()) == int(ref["resid"]) and float(int(ref["resid"])) == ref["resid"]
        assert int(sq.sum()) == int(ref["resid_masked"]) and float(int(ref["resid_masked"])) == ref["resid_masked"]
        one = np.ones((mask.shape[1], 1))
        _exact_in_all_orders(mask, cross, one, ng, cross.sum(1, keepdims=True).astype(np.float64), "sum a (a - 2 d)", np.float64)
        _exact_in_all_orders(mask, sq, one, ng, sq.sum(1, keepdims=True).astype(np.float64), "sum (a - d)^2", np.float64)
        assert abs(cross).sum() < 2 ** 53 and gram < 2 ** 53


@pytest.mark.parametrize("k", SPARSE_KS)
def test_sparse_kl_is_exact(lens_mask, k):
    """the KL passes on `sparse_kl` operands: the fused quotient is exact, and so are both products and both denominators"""
    eps = np.float32(np.finfo(np.float32).eps)
    ng = 256 // _kpad(k)
    prob = ex.sparse_kl(lens_mask, k, stored_zeros=True)
    assert ((prob[0] == 0) & lens_mask).sum() >= 3
    for A, mask, W, H in ((prob[0], lens_mask) + prob[1:], ex.transposed(prob[0], lens_mask, *prob[1:])):
        ref = ex.sparse_exact(A, mask, W, H, kl=True)
        D = _all_orders(W, H, "W H").astype(np.float32)
        assert np.array_equal(D + eps, D)                                               # eps is absorbed
        U32 = np.where(mask, A / (D + eps), np.float32(0))
        assert U32.dtype == np.float32 and np.array_equal(U32.astype(np.float64), ref["U"])
        Mf = mask.astype(np.float32)
        _exact_in_all_orders(mask, U32, H.T, ng, ref["uht"], "U H^T")
        _exact_in_all_orders(mask, Mf, H.T, ng, ref["klden_w"], "stored-position sums of H rows")
        _exact_in_all_orders(mask.T, U32.T, W, ng, ref["wtu"].T, "W^T U")
        _exact_in_all_orders(mask.T, Mf.T, W, ng, ref["klden_h"].T, "stored-position sums of W columns")
