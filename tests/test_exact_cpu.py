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
