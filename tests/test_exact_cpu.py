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


# ---------------------------------------------------------------------------------------------------------- fixed points of a whole MU step
F32_EPS = np.float32(np.finfo(np.float32).eps)
ORDERS = ("forward", "reversed", 11, 12)                                    # (a number: that seed's random permutation of the terms)


def _mm(X, Y, order):
    """X @ Y in float32, one term of the contraction after the other in the given order (every partial sum rounds to float32)"""
    assert X.dtype == np.float32 and Y.dtype == np.float32
    L = X.shape[1]
    idx = {"forward": np.arange(L), "reversed": np.arange(L)[::-1]}.get(order)
    if idx is None:
        idx = np.random.RandomState(order).permutation(L)
    acc = np.zeros((X.shape[0], Y.shape[1]), dtype=np.float32)
    for t in idx:
        acc += np.outer(X[:, t], Y[t])
    return acc


def _rcp(d):
    """v_rcp_f32 where it is exact: at powers of two (asserted)"""
    d = (d + F32_EPS).astype(np.float32)
    man, _ = np.frexp(d)
    assert np.all(man == 0.5) and np.all(d >= 2), "a divisor is not a power of two >= 2 after + eps"
    return (np.float32(1) / d).astype(np.float32)


def _ones(L):
    return np.ones((L, 1), dtype=np.float32)


def _kl_step32(A, W, H, order, w_update, clamp):
    """dist_nmf.py:806-849 in float32 as the small kernels evaluate it: quotients as products with the reciprocal"""
    if w_update:
        U = A * _rcp(_mm(W, H, order))
        W = W * (_mm(U, H.T.copy(), order) * _rcp(_mm(H, _ones(H.shape[1]), order)).T)
    U = A * _rcp(_mm(W, H, order))
    H = H * (_mm(W.T.copy(), U, order) * _rcp(_mm(W.T.copy(), _ones(W.shape[0]), order)))
    return (np.maximum(W, F32_EPS), np.maximum(H, F32_EPS)) if clamp else (W, H)


def _fro_step32(A, W, H, order, clamp):
    """dist_nmf.py:716-751 in float32, the same way"""
    G = _mm(H, H.T.copy(), order)
    W = W * (_mm(A, H.T.copy(), order) * _rcp(_mm(W, G, order)))
    GW = _mm(W.T.copy(), W, order)
    H = H * (_mm(W.T.copy(), A, order) * _rcp(_mm(GW, H, order)))
    return (np.maximum(W, F32_EPS), np.maximum(H, F32_EPS)) if clamp else (W, H)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("family,m,n,k", [e[:4] for e in ex.SMALL_REACH if not e[0].startswith("hals")],
                         ids=["%s-%dx%d-k%d" % e[:4] for e in ex.SMALL_REACH if not e[0].startswith("hals")])
def test_fixed_points_return_their_input(family, m, n, k):
    """`kl_fixed`, `fro_fixed` and `kl_moved` at every shape of the reach table that runs them: three steps in float32 with the terms of
    every sum forward, reversed and in two random orders, with and without the clamp -- the input comes back bit for bit (`kl_moved`:
    2 H after step 0, then that)"""
    for seed in (0, 1):
        A, W, H = {"kl": ex.kl_fixed, "kl_wfixed": ex.kl_moved}.get(family, ex.fro_fixed)(m, n, k, seed=seed)
        assert A.dtype == W.dtype == H.dtype == np.float32 and A.shape == (m, n) and W.shape == (m, k) and H.shape == (k, n)
        for x in (A, W, H):                                                 # positive powers of two: the clamp is a no-op, bf16 storage exact
            assert np.all(x >= 1) and np.all(np.frexp(x)[0] == 0.5)
            assert np.array_equal(x, (_bits(x) & 0xFFFF0000).view(np.float32))
        Hend = 2 * H if family == "kl_wfixed" else H
        for order in ORDERS:
            for clamp in (False, True):
                Wt, Ht = W, H
                for it in range(3):
                    if family.startswith("fro"):
                        Wt, Ht = _fro_step32(A, Wt, Ht, order, clamp)
                    else:
                        Wt, Ht = _kl_step32(A, Wt, Ht, order, family == "kl", clamp)
                    assert Wt.dtype == Ht.dtype == np.float32
                    assert np.array_equal(_bits(Wt), _bits(W)) and np.array_equal(_bits(Ht), _bits(Hend)), (family, order, clamp, it)
        # the closing normalisation divides by colsum(W): a power of two on the KL operands (exact), an integer >= 2 on the Frobenius ones
        s = _mm(W.T.copy(), _ones(m), "reversed")[:, 0]
        assert np.array_equal(s.astype(np.float64), W.astype(np.float64).sum(0)) and np.array_equal(s + F32_EPS, s) and np.all(s >= 2)
        if not family.startswith("fro"):
            assert np.all(np.frexp(s)[0] == 0.5)
    assert not np.array_equal(ex.kl_fixed(m, n, k, seed=0)[1], ex.kl_fixed(m, n, k, seed=1)[1]) or m * k == 1     # the seeds differ


def test_fro_fixed_refuses_a_length_divisible_by_three():
    for m, n in ((129, 37), (130, 36)):
        with pytest.raises(AssertionError, match="divisible by 3"):
            ex.fro_fixed(m, n, 5)


def _hals_fp32_gap(m, n, k, seed, rank_k):
    """the checker's 11-step HALS loop run in numpy float32 against its float64 run, in units of the largest entry: what ANY fp32
    evaluation of that loop may differ by on this data"""
    from oracle import nmf_oracle as orc
    A, W, H = ex.hals_problem(m, n, k, seed, rank_k)
    run = lambda a, w, h: orc.fit_single(a, w, h, 11, norm="fro", W_update=True, method="hals", eps=float(F32_EPS))[:2]
    Wr, Hr = run(*(x.astype(np.float64) for x in (A, W, H)))
    W32, H32 = run(A, W, H)
    assert W32.dtype == np.float32
    return max(np.abs(W32 - Wr).max() / Wr.max(), np.abs(H32 - Hr).max() / Hr.max())


HALS_SHAPES = sorted({e[1:4] for e in ex.SMALL_REACH if e[0].startswith("hals")})


@pytest.mark.parametrize("m,n,k", HALS_SHAPES, ids=lambda v: str(v))
def test_hals_reach_data_is_well_conditioned(m, n, k):
    """the float64 loop the HALS rows are held to at 1e-3 must be one an fp32 evaluation CAN follow: the checker's own loop in numpy
    float32 stays within half of that on the data used, at every seed used -- the suite's random data at all shapes but four, where
    it does not (shown), and rank-k data there"""
    for seed in ex.HALS_SEEDS:
        assert _hals_fp32_gap(m, n, k, seed, None) <= 5e-4, (m, n, k, seed)
    if (m, n, k) in ex.HALS_RANK_K:
        assert max(_hals_fp32_gap(m, n, k, seed, False) for seed in ex.HALS_SEEDS) > 1e-3, "random data is well-conditioned here: use it"


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
