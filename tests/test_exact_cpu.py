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


# ---------------------------------------------------------------------------------------------------------- the float64 shapes
# The shapes of tests/test_gpu_exact_f64.py are far larger than the fp32 ones (65500 rows): the generators' bounds follow the dtype, and
# the claims are proved here in float64 arithmetic against exact integers (int64 holds every sum: the totals are below 2^53).
F64_EPS = 2.220446049250313e-16


def _orders64(X, Y, scale, what):
    """X @ Y in float64 in four orders -- BLAS, the contraction index reversed, sequential slabs of 48 and of 1000 terms added in slab
    order -- all equal to the exact product of the integers X scale[0], Y scale[1]; returns that product over the scales, as float64"""
    Xi, Yi = np.rint(X * scale[0]).astype(np.int64), np.rint(Y * scale[1]).astype(np.int64)
    assert np.array_equal(Xi / scale[0], X) and np.array_equal(Yi / scale[1], Y), "%s: the operands are not multiples of the stated units" % what
    exact = Xi @ Yi
    assert np.abs(exact).max() < 2 ** 53
    ref = exact.astype(np.float64) / (scale[0] * scale[1])
    L = X.shape[1]
    got = {"BLAS": X @ Y, "reversed": X[:, ::-1] @ Y[::-1]}
    for step in (48, 1000):
        acc = np.zeros_like(ref)
        for t in range(0, L, step):
            acc += X[:, t:t + step] @ Y[t:t + step]
        got["slabs of %d" % step] = acc
    for how, g in got.items():
        assert np.array_equal(g, ref), "%s (%s) is not exact in float64" % (what, how)
    return ref


F64_PRODUCT_PROOF = sorted({c[:3] for c in ex.F64_AHT if c[0] >= 8200 and c[1] == 70} | {c[:3] for c in ex.F64_AHT if c[6] > 1}
                           | {c[:3] for c in ex.F64_WTA if c[0] == 600 and c[1] == 71} | {c[:3] for c in ex.F64_MU} | {ex.F64_IMAGE[-1][:3]})
F64_KL_PROOF = sorted({c[:3] for c in ex.F64_KL_UHT if c[1] == 70 or c[7] > 1} | {c[:3] for c in ex.F64_KL_WTU if c[0] == 600}
                      | {c[:3] for c in ex.F64_IMAGE_K})


@pytest.mark.parametrize("m,n,k", F64_PRODUCT_PROOF, ids=str)
def test_float64_products_are_exact(m, n, k):
    """`products` in float64: the four products and the two MU denominators are integers, equal in every order; a positive
    denominator is in [2, 2^51) and absorbs eps = 2^-52"""
    A, W, H = ex.products(m, n, k, np.float64)
    assert A.dtype == W.dtype == H.dtype == np.float64
    one = (1, 1)
    _orders64(A, H.T, one, "A H^T")
    _orders64(W.T, A, one, "W^T A")
    G, GW = _orders64(H, H.T, one, "H H^T"), _orders64(W.T, W, one, "W^T W")
    for d, what in ((_orders64(W, G, one, "W G"), "W G"), (_orders64(GW, H, one, "G H"), "G H")):
        assert np.all((d == 0) | ((d >= 2) & (d < 2.0 ** 51))), what
        assert np.array_equal(d[d > 0] + F64_EPS, d[d > 0]), "%s + eps is not absorbed in float64" % what
    S = _orders64(W, H, one, "W H")                                            # the residual operands of sqdiff: A = W H + (0..2)
    assert (S.max() + 2) ** 2 * m * n < 2 ** 53                                # (so is the sum of the squares of A, whatever its order)


@pytest.mark.parametrize("m,n,k", F64_KL_PROOF, ids=str)
def test_float64_kl_quotient_is_exact(m, n, k):
    """`kl` in float64: W H is a power of two >= 2 that absorbs eps, U = A / (W H + eps) is A times a power of two (exactly), and
    U H^T, W^T U (multiples of 2^-5), rowsum(H), colsum(W) are equal in every order"""
    A, W, H, U = ex.kl(m, n, k, np.float64)
    assert A.dtype == W.dtype == H.dtype == np.float64
    WH = _orders64(W, H, (1, 1), "W H")
    assert np.array_equal(WH + F64_EPS, WH), "W H + eps is not absorbed in float64"
    U64 = A / (WH + F64_EPS)
    assert np.array_equal(U64, U)
    e = np.log2(WH)
    assert np.array_equal(e, np.round(e)) and e.min() >= 1 and np.array_equal(U * WH, A) and np.array_equal(np.ldexp(A, -e.astype(int)), U)
    _orders64(U, H.T, (32, 1), "U H^T")
    _orders64(W.T, U, (1, 32), "W^T U")
    ones = np.ones((1, n)), np.ones((m, 1))
    assert np.array_equal(_orders64(ones[0], H.T, (1, 1), "rowsum(H)")[0], H.sum(1))
    assert np.array_equal(_orders64(W.T, ones[1], (1, 1), "colsum(W)")[:, 0], W.sum(0))


@pytest.mark.parametrize("m,n,k", sorted({c[:3] for c in ex.F64_FIT_FRO} | {ex.F64_FIT_STACK}), ids=str)
def test_float64_fro_step_is_exact(m, n, k):
    """`fro_step` in float64: the W phase is exact (W G a power of two >= 2), the H phase has exact numerators and denominators >= 2"""
    A, W, H, Wn, Hq = ex.fro_step(m, n, k, np.float64)
    G, AH = H @ H.T, A @ H.T
    WG = W @ G
    assert np.array_equal(np.log2(WG), np.round(np.log2(WG))) and WG.min() >= 2
    assert np.array_equal(W * (AH / (WG + F64_EPS)), Wn)
    num, den = Wn.T @ A, (Wn.T @ Wn) @ H
    assert np.array_equal(num, Wn[::-1].T @ A[::-1]) and np.array_equal(den, (Wn[::-1].T @ Wn[::-1]) @ H)
    assert np.all((den == 0) | (den >= 2)) and np.array_equal(den[den > 0] + F64_EPS, den[den > 0])
    ex.assert_ulp(H * (num / (den + F64_EPS)), Hq, 1, "H phase in float64")


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


# ---------------------------------------------------------------------------------------------------------- one exact HALS sweep
# `hals_w_problem` / `hals_h_problem`: the sweeps of csrc/dnmf_hals.h evaluated in numpy float32 in the forms the kernels use, each with
# its sums taken forward, reversed and in one random order, end at the constructed answer bit for bit -- with eps = 2^-3 (every sum
# exact) and with the library's eps = 2^-23 (the clamped terms absorbed by the single rounding of each fmaf).
F32 = np.float32


def _fma(a, b, c):
    """fmaf on float32 arrays: the float64 product and sum are exact on these operands (`hals_w_problem` asserts the range), so
    rounding them once is the fused operation"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def _orders(n, seed=0):
    return (("forward", np.arange(n)), ("reversed", np.arange(n)[::-1]), ("random", np.random.RandomState(seed + n).permutation(n)))


def _ss2(u, rows):
    """sum of squares in float64, one row after the other in the order `rows`"""
    u = u.astype(np.float64)[rows]
    return float(np.cumsum(u * u)[-1])


def _w_persistent(W, AH, G, eps, order, rows, lagged):
    """the two-launch form: T[i][j] = AH[i][j] - sum_{l > j} W[i][l] G[l][j] (the products summed in `order`, then one subtraction: the
    MFMA pass), then per column u, ss2 in float64, w = u / (float)sqrt(ss2) and t[j] = fmaf(-w, G[kk][j], t[j]) for j > kk -- at once, or
    lagged as hals_col_step does it: j = kk + 1 first, the others at the start of the next column's turn"""
    m, k = W.shape
    acc = np.zeros((m, k), dtype=F32)
    for l in order:
        acc[:, :l] = _fma(W[:, l:l + 1], G[l:l + 1, :l], acc[:, :l])
    t = AH - acc
    T0 = t.copy()
    ss2 = np.zeros(k)
    for kk in range(k):
        if lagged and kk > 0:
            t[:, kk + 1:] = _fma(-t[:, kk - 1:kk], G[kk - 1:kk, kk + 1:], t[:, kk + 1:])
        u = np.maximum(t[:, kk], F32(eps))
        ss2[kk] = _ss2(u, rows)
        ss = F32(np.sqrt(ss2[kk]))
        t[:, kk] = u / ss if ss > 0 else u
        hi = kk + 2 if lagged else k
        t[:, kk + 1:hi] = _fma(-t[:, kk:kk + 1], G[kk:kk + 1, kk + 1:hi], t[:, kk + 1:hi])
    return T0, t, ss2


def _w_columns(W, AH, G, eps, order, rows):
    """hals_w_col_kernel: the pending normalisation of column kk - 1, dot = sum_j fmaf(row[j], g[j], dot) over ALL j, t = row[kk] g[kk] +
    AH - dot; then hals_w_scale_kernel on the last column"""
    W = W.copy()
    m, k = W.shape
    ss2 = np.zeros(k)
    for kk in range(k):
        if kk > 0:
            den = F32(np.sqrt(ss2[kk - 1]))
            if den > 0:
                W[:, kk - 1] = W[:, kk - 1] / den
        dot = np.zeros(m, dtype=F32)
        for j in order:
            dot = _fma(W[:, j], G[j, kk], dot)
        t = (W[:, kk] * G[kk, kk] + AH[:, kk]) - dot
        W[:, kk] = np.maximum(t, F32(eps))
        ss2[kk] = _ss2(W[:, kk], rows)
    den = F32(np.sqrt(ss2[k - 1]))
    if den > 0:
        W[:, k - 1] = W[:, k - 1] / den
    return W, ss2


def _check_w(got, ss2, P, how):
    assert got.dtype == F32 and np.array_equal(got.astype(np.float64), P["W_new"]), "W sweep, %s: not the constructed answer" % how
    assert np.all(np.abs(ss2 - P["ss2"]) <= P["ss2_tol"]), "W sweep, %s: ss2 off by %g" % (how, np.max(np.abs(ss2 - P["ss2"]) - P["ss2_tol"]))
    assert np.array_equal(np.sqrt(ss2).astype(F32), 2.0 ** P["p"])


HALS_W_PROOF = sorted({(m, k) for _, m, k, _, _ in ex.HALS_W_CASES} | set(ex.HALS_W_F64)
                      | {(ex._slots(c + over), ex.HALS_POLL_K) for c in ex.HALS_CAPS for over in (0, 1)})


@pytest.mark.parametrize("eps", [ex.HALS_EPS_A, ex.HALS_EPS_B], ids=["eps2^-3", "eps2^-23"])
@pytest.mark.parametrize("m,k", HALS_W_PROOF)
def test_hals_w_problem_is_exact_in_every_form(m, k, eps):
    P = ex.hals_w_problem(m, k, eps)
    W, AH, G = P["W_old"], P["AH"], P["G"]
    T0_exact = AH.astype(np.float64) - W.astype(np.float64) @ np.tril(G.astype(np.float64), -1)
    for (how, order), (_, rows) in zip(_orders(k), _orders(m, 1)):
        for lagged in (False, True):
            T0, got, ss2 = _w_persistent(W, AH, G, eps, order, rows, lagged)
            assert np.array_equal(T0.astype(np.float64), T0_exact), "the transform pass is not exact (%s)" % how
            _check_w(got, ss2, P, "persistent form%s, %s" % (", lagged" if lagged else "", how))
        got, ss2 = _w_columns(W, AH, G, eps, order, rows)
        _check_w(got, ss2, P, "column form, %s" % how)
    if eps == ex.HALS_EPS_A:
        assert not P["ss2_tol"].any() and np.array_equal(P["ss2"], 4.0 ** P["p"])
    if m >= 130:
        c = P["clamped"]
        assert c.any(0).all() and (~c).any(0).all() and c[m - 1].any() and c[ex.HALS_ROWS * ((m - 1) // ex.HALS_ROWS):].any()
        assert np.all(P["G"][~np.eye(k, dtype=bool)] > 0)


def test_hals_w_problem_is_free_of_the_row_count_modulo_three():
    """entries of 3 (9 = 0 mod 3) lift the condition pure powers of four would put on m"""
    for m in (130, 131, 132, 513, 514, 515):
        for eps in (ex.HALS_EPS_A, ex.HALS_EPS_B):
            ex.hals_w_problem(m, 4, eps)


@pytest.mark.parametrize("eps", [ex.HALS_EPS_A, ex.HALS_EPS_B], ids=["eps2^-3", "eps2^-23"])
@pytest.mark.parametrize("k,n", sorted(set(ex.HALS_H_CASES) | set(ex.HALS_H_F64)))
def test_hals_h_problem_is_exact_in_every_order(k, n, eps):
    H0, AtW, G2, Hn = ex.hals_h_problem(k, n, eps)
    for how, order in _orders(k):
        H = H0.copy()
        for kk in range(k):
            dot = np.zeros(n, dtype=F32)
            for j in order:
                dot = _fma(G2[kk, j], H[j], dot)
            H[kk] = np.maximum((H[kk] + AtW[kk]) - dot, F32(eps))
        assert H.dtype == F32 and np.array_equal(H.astype(np.float64), Hn), "H sweep, %s: not the constructed answer" % how
    clamped = Hn == eps
    if k > 1 and n > k:
        assert clamped.any(1).all() and (~clamped).any(1).all(), "a row without both kinds of column"


HALS_STEP_PROOF = [e[1:4] for e in ex.SMALL_REACH if e[0] == "hals"] + ex.HALS_STEP_BIG
HALS_STEP_BF16 = [e[1:4] for e in ex.SMALL_REACH if e[0] == "hals_bf16"]


def test_hals_step_bf16_rows_left_out_stay_few():
    """at most 3 bf16-A rows may be left to the old checks, each must really be out of the generator's reach, every other row has a
    problem whose A is bf16 in every entry"""
    left = set(ex.HALS_STEP_BF16_LEFT)
    assert len(left) <= 3 and left <= set(HALS_STEP_BF16)
    for m, n, k in HALS_STEP_BF16:
        if (m, n, k) in left:
            with pytest.raises(AssertionError):
                ex.hals_step_problem(m, n, k, bf16=True)
        else:
            for seed in range(3):
                P = ex.hals_step_problem(m, n, k, seed, bf16=True)
                assert ex.is_bf16(P["A"]).all() and P["A"].min() >= 0


@pytest.mark.parametrize("m,n,k,bf16", [s + (False,) for s in HALS_STEP_PROOF] + [s + (True,) for s in HALS_STEP_BF16 if s not in ex.HALS_STEP_BF16_LEFT])
def test_hals_step_problem_has_an_exact_w_phase(m, n, k, bf16):
    """A H^T and H H^T in every order, then the W sweep in every form: the constructed W_new bit for bit; A >= 0"""
    for seed in range(3 if m * n * k < 1e6 else 1):
        P = ex.hals_step_problem(m, n, k, seed, bf16)
        A, W, H = P["A"], P["W_old"], P["H_old"]
        assert A.min() >= 0 and P["clamped"].any(0).all() and P["clamped"][m - 1].any()
        small = m * n * k <= 4e6
        AH = _all_orders(A, H.T, "A H^T") if small else A.astype(np.float64) @ H.astype(np.float64).T
        G = _all_orders(H, H.T, "H H^T")
        assert np.array_equal(AH, P["AH"]) and np.array_equal(G, P["G"]) and np.all(G[~np.eye(k, dtype=bool)] >= 1)
        assert P["clamped"].any(0).all() and (~P["clamped"]).any(0).all()
        AH32, G32 = AH.astype(F32), G.astype(F32)
        for (how, order), (_, rows) in zip(_orders(k), _orders(m, 1)):
            for lagged in (False, True):
                _, got, ss2 = _w_persistent(W, AH32, G32, ex.HALS_EPS_A, order, rows, lagged)
                assert np.array_equal(got.astype(np.float64), P["W_new"]) and np.all(np.log2(ss2) % 2 == 0), how
            got, ss2 = _w_columns(W, AH32, G32, ex.HALS_EPS_A, order, rows)
            assert np.array_equal(got.astype(np.float64), P["W_new"]) and np.all(np.log2(ss2) % 2 == 0), how
            # the small whole-fit kernel sums the squares in float32: exact too (multiples of 2^-6 below 2^18 of them)
            u = np.maximum(P["W_new"] * np.sqrt(ss2)[None, :], 0).astype(F32)
            assert np.array_equal(np.cumsum((u * u)[rows], axis=0, dtype=F32)[-1].astype(np.float64), ss2)
        Wc = np.maximum(P["W_new"], ex.HALS_EPS_A)
        s = Wc.sum(0)
        for order in (np.arange(m), np.arange(m)[::-1]):
            assert np.array_equal(np.cumsum(Wc.astype(F32)[order], axis=0, dtype=F32)[-1].astype(np.float64), s), "colsum(W) is not exact"
        assert np.array_equal((s + ex.HALS_EPS_A).astype(F32).astype(np.float64), s + ex.HALS_EPS_A)


@pytest.mark.parametrize("m,k", ex.HALS_W_F64_B)
def test_hals_w_problem_float64_with_the_library_eps_stays_within_its_bound(m, k):
    """float64, eps = 2^-23: the column form in numpy float64 (fma replaced by two roundings: within the (k + 2) R M the bound allows), its
    sums forward, reversed and in a random order, ends within W_rel of the exact answer and within ss2_tol of the exact sums of squares"""
    P = ex.hals_w_problem(m, k, ex.HALS_EPS_B, dtype=np.float64)
    assert P["AH"].dtype == np.float64 and P["W_rel"].max() < 1e-8 and P["W_rel"][0] < 1e-14
    for (how, order), (_, rows) in zip(_orders(k), _orders(m, 1)):
        W = P["W_old"].copy()
        ss2 = np.zeros(k)
        for kk in range(k):
            if kk > 0:
                W[:, kk - 1] /= np.sqrt(ss2[kk - 1])
            dot = np.zeros(m)
            for j in order:
                dot = dot + W[:, j] * P["G"][j, kk]
            W[:, kk] = np.maximum((W[:, kk] * P["G"][kk, kk] + P["AH"][:, kk]) - dot, ex.HALS_EPS_B)
            ss2[kk] = np.cumsum((W[:, kk] ** 2)[rows])[-1]
        W[:, k - 1] /= np.sqrt(ss2[k - 1])
        assert np.all(np.abs(W - P["W_new"]) <= P["W_rel"][None, :] * P["W_new"]), how
        assert np.all(np.abs(ss2 - P["ss2"]) <= P["ss2_tol"]), how


@pytest.mark.parametrize("m,n,k,bf16", [s + (False,) for s in HALS_STEP_PROOF] + [s + (True,) for s in HALS_STEP_BF16 if s not in ex.HALS_STEP_BF16_LEFT])
def test_hals_step_problem_h_bound_holds_in_float32(m, n, k, bf16):
    """the H phase of the step in numpy float32 -- W^T A and W^T W through BLAS and as sequential sums from either end, the sweep's dot
    products forward, reversed and in a random order -- stays within the derived bound H_err of the float64 sweep"""
    P = ex.hals_step_problem(m, n, k, bf16=bf16)
    A, H0, Wn = P["A"], P["H_old"], P["W_new"].astype(F32)
    small = m * n * k <= 4e6
    prods = [(Wn.T @ A, Wn.T @ Wn)] + ([(_seq(Wn.T, A, r), _seq(Wn.T, Wn, r)) for r in (False, True)] if small else [])
    for (AtW, G2), (how, order) in zip(prods * 3, _orders(k)):
        H = H0.copy()
        for kk in range(k):
            dot = np.zeros(n, dtype=F32)
            for j in order:
                dot = dot + G2[kk, j] * H[j]
            H[kk] = np.maximum((H[kk] + AtW[kk]) - dot, F32(ex.HALS_EPS_A))
        assert H.dtype == F32 and np.all(np.abs(H - P["H_new"]) <= P["H_err"]), how
    if k == 1 and not bf16:
        assert np.max(P["H_err"] / np.abs(P["H_new"])) < 1e-5


# ---------------------------------------------------------------------------------------------------------- the BCD projected-gradient step
# `bcd_pg_problem`: out = max(0, Xm - (S - P) / L) evaluated in numpy float32 with the terms of S forward, reversed and in a random
# order, each with fused and with separately rounded multiply-adds, on both sides, ends at the constructed answer bit for bit -- with
# L = 2^6 (the float64 answer) and with L = float32(||G||_F) (the float32 expression); the checker of tests/_bcd.py gives the same bits.
def _pg32(P, side, order, fused):
    Xm, G = P["Xm"], P["G"]
    X, Y = (Xm, G) if side == "w" else (G, Xm)
    acc = np.zeros(Xm.shape, dtype=F32)
    for t in order:
        acc = _fma(X[:, t:t + 1], Y[t:t + 1], acc) if fused else acc + X[:, t:t + 1] * Y[t:t + 1]
    assert acc.dtype == F32
    y = Xm - (acc - P["P"]) / F32(P["L"])
    return np.where(y < 0, F32(0), y)


def _butterfly(v):
    """the xor butterfly of a 64-lane wave over axis 0 in float32: every lane ends with the total"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    assert v.dtype == F32 and np.array_equal(v[0], v[63])
    return v[0]


@pytest.mark.parametrize("L", [ex.BCD_L, None], ids=["L2^6", "Lnorm"])
@pytest.mark.parametrize("R,k", ex.BCD_PG_PROOF + ex.BCD_COLSUM)
def test_bcd_pg_problem_is_exact_in_every_order(R, k, L):
    import torch
    from tests._bcd import LH, LW, BcdOracleOps
    for side in ("w", "h"):
        P = ex.bcd_pg_problem(R, k, seed=1, L=L, side=side)
        assert P["Xm"].dtype == P["P"].dtype == P["G"].dtype == F32 and P["L"] == float(F32(P["L"]))
        assert k == 1 or not np.array_equal(P["G"], P["G"].T)
        sh = P["shares"]
        assert sh["clamped"] >= 0.1 and sh["zero"] >= 0.1 and sh["positive"] >= 0.3, sh
        if L is None:
            assert P["L"] == float(F32(np.linalg.norm(P["G"].astype(np.float64)))) and np.frexp(P["L"])[0] != 0.5 or k == 1
        else:                                                    # the float64 answer, from the operands alone
            X64, P64, G64 = (P[x].astype(np.float64) for x in ("Xm", "P", "G"))
            S = X64 @ G64 if side == "w" else G64 @ X64
            assert np.array_equal(np.maximum(0, X64 - (S - P64) / L), P["expected"])
        for how, order in _orders(k):
            for fused in (True, False):
                got = _pg32(P, side, order, fused)
                assert got.dtype == F32 and np.array_equal(got.astype(np.float64), P["expected"]), (side, how, fused)
        st = torch.zeros(16, dtype=torch.float64)
        st[LW if side == "w" else LH] = P["L"]
        out = torch.full(P["Xm"].shape, -1.0)
        t = {x: torch.from_numpy(P[x]) for x in ("Xm", "P", "G")}
        if side == "w":
            s = torch.full((k,), -1.0)
            BcdOracleOps().bcd_update_w(t["Xm"], t["P"], t["G"], st, out, s)
            assert np.array_equal(_bits(s.numpy()), _bits(P["s"]))
        else:
            BcdOracleOps().bcd_update_h(t["Xm"], t["P"], t["G"], st, out)
        assert np.array_equal(_bits(out.numpy()), _bits(P["expected"].astype(F32))), "the checker disagrees (%s side)" % side


@pytest.mark.parametrize("R,k", ex.BCD_PG_PROOF + ex.BCD_COLSUM)
def test_bcd_pg_problem_column_sums_round_once(R, k):
    """L = 2^6, W side: the partial of every 64-row workgroup is exact in float32 in the butterfly order and as a sequential sum from either
    end; the float64 sum of the partials is exact in any order; so s is float32(exact sum) -- one rounding"""
    P = ex.bcd_pg_problem(R, k, seed=1, side="w")
    y = P["expected"].astype(F32)
    nb = -(-R // 64)
    y = np.concatenate([y, np.zeros((nb * 64 - R, k), dtype=F32)]).reshape(nb, 64, k).transpose(1, 0, 2)      # [lane][workgroup][column]
    exact = y.astype(np.float64).sum(0)
    for got, how in ((_butterfly(y), "butterfly"), (np.cumsum(y, axis=0, dtype=F32)[-1], "forward"),
                     (np.cumsum(y[::-1], axis=0, dtype=F32)[-1], "reversed")):
        assert got.dtype == F32 and np.array_equal(got.astype(np.float64), exact), how
    total = int(np.rint(exact * 64).astype(np.int64).sum(0).max())
    assert np.array_equal(exact * 64, np.rint(exact * 64)) and total < 2 ** 53
    for order in (np.arange(nb), np.arange(nb)[::-1], np.random.RandomState(nb).permutation(nb)):
        tot = np.cumsum(exact[order], axis=0)[-1]
        assert np.array_equal(tot, P["expected"].sum(0)) and np.array_equal(_bits(tot.astype(F32)), _bits(P["s"]))
    if R > 2 ** 14:
        assert nb > 256 and np.any(exact[256:].sum(0) > 0), "no partial beyond the first 256 carries weight"
        assert not np.array_equal(exact[:256].sum(0).astype(F32), P["s"])


# ---------------------------------------------------------------------------------------------------------- exact operands on a grid
GRID_SHAPES = sorted({shape for e in ex.GRID_EXACT for shape in e[2]})


def _part(total, p):
    """the partition rule (utils.py:36-41): the first total % p members hold one item more"""
    return [total // p + (1 if q < total % p else 0) for q in range(p)]


def _sum32(terms, order):
    """the float32 sum of a list of equally shaped float32 arrays, one after the other in the given order"""
    idx = {"forward": np.arange(len(terms)), "reversed": np.arange(len(terms))[::-1]}.get(order)
    if idx is None:
        idx = np.random.RandomState(order).permutation(len(terms))
    acc = np.zeros_like(terms[0])
    for t in idx:
        acc = (acc + terms[t]).astype(np.float32)
    return acc


@pytest.mark.parametrize("m,n,k", GRID_SHAPES)
def test_hals_h_step_problem_is_exact_in_any_order(m, n, k):
    """`hals_h_step_problem` at every shape of the grid tier: W^T A and W^T W summed in float32 as p partial sums over row blocks (p = 1..4,
    the partition rule), the partials and the terms of every row update forward, reversed and in two random orders -- every evaluation
    equals the float64 sweep bit for bit"""
    A, W, H_old, Hn = ex.hals_h_step_problem(m, n, k)
    eps = np.float32(ex.HALS_EPS_A)
    assert A.dtype == W.dtype == H_old.dtype == np.float32 and A.min() >= 0 and W.min() >= 0 and H_old.min() >= 0
    assert np.array_equal(ex.hals_h_exact(H_old, W.T.astype(np.float64) @ A, W.T.astype(np.float64) @ W, ex.HALS_EPS_A), Hn)
    for p in (1, 2, 3, 4):
        cuts = np.cumsum([0] + _part(m, p))
        for order in ORDERS:
            AtW = _sum32([_mm(W[a:b].T.copy(), A[a:b], order) for a, b in zip(cuts[:-1], cuts[1:])], order)
            G2 = _sum32([_mm(W[a:b].T.copy(), W[a:b], order) for a, b in zip(cuts[:-1], cuts[1:])], order)
            H = H_old.copy()
            for kk in range(k):
                t = _sum32([H[kk], AtW[kk]] + [(-G2[kk, j] * H[j]).astype(np.float32) for j in range(k)], order)
                H[kk] = np.maximum(t, eps)
            assert np.array_equal(H.astype(np.float64), Hn), "p = %d, order %s: the float32 H phase is not the float64 sweep" % (p, order)


class _Rank:
    def __init__(self, rank):
        self.rank, self.size = rank, 1


def _grid_branches(grid, shape, extra=None):
    """per rank of the grid: what the choreography of pydnmfk_amd/dist_nmf.py decides for the shape -- its own objects, built on empty blocks"""
    import torch
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D, nmf_algorithms_2D
    from pydnmfk_amd.utils import determine_block_params, parse
    from tests._ops_double import OracleOps
    (p_r, p_c), (m, n, k) = grid, shape
    out = []
    for rank in range(p_r * p_c):
        s, e = determine_block_params(rank, (p_r, p_c), (m, n)).determine_block_index_range_asymm()
        m_l, n_l = e[0] + 1 - s[0], e[1] + 1 - s[1]
        p = parse()
        p.m, p.n, p.p_r, p.p_c, p.k, p.eps, p.W_update, p.norm, p.method = m, n, p_r, p_c, k, 1e-7, True, "fro", "mu"
        p.comm1 = p.row_comm = p.col_comm = p.comm = _Rank(rank)
        for key, val in (extra or {}).items():
            setattr(p, key, val)
        A = torch.empty(m_l, n_l)
        if p_r > 1 and p_c > 1:
            alg = nmf_algorithms_2D(A, torch.empty(1, k), torch.empty(k, 1), params=p, ops=OracleOps())
            hc, wc = alg.h_counts, alg.w_counts
            assert hc == _part(n_l, p_r) and wc == _part(m_l, p_c)
            blockable = alg._h_blockable("aht_hblocks") and alg._h_blockable("kl_uht_hblocks")
            sliceable = len(set(hc)) == 1 and hc[0] % 4 == 0                # (_product_scattered_to_H, the fp32 operator set)
            out.append(dict(m_l=m_l, n_l=n_l, h=hc, w=wc, blockable=blockable, sliceable=sliceable, w_equal=len(set(wc)) == 1))
        else:
            alg = nmf_algorithms_1D(A, torch.empty(m_l if p_c == 1 else m, k), torch.empty(k, n_l if p_r == 1 else n), params=p, ops=OracleOps())
            nch = alg._overlap_chunks(n_l)
            cw = -(-(-(-n_l // nch)) // 64) * 64
            out.append(dict(m_l=m_l, n_l=n_l, nch=nch, chunks=[min(cw, n_l - c0) for c0 in range(0, n_l, cw)] if nch > 1 else [n_l]))
    return out


def test_grid_shapes_reach_their_branches():
    """every (grid, shape) of GRID_EXACT takes the branch of the choreography it is named after: the stacked [p_r][k][n_h] blocks with
    the KL re-blocking copies, the sliced products without the stack, the transposing route; equal and ragged row counts of gather_W;
    the chunk widths of the overlapped H phase"""
    from tests._mp import EXACT_MODES
    table = {e[0]: e for e in ex.GRID_EXACT}
    b = _grid_branches((2, 2), (512, 256, 16))
    assert all(r["blockable"] and r["sliceable"] and r["w_equal"] and r["h"] == [64, 64] for r in b)
    b = _grid_branches((2, 2), (515, 272, 33))
    assert all(r["sliceable"] and not r["blockable"] and r["h"] == [68, 68] for r in b) and not all(r["w_equal"] for r in b)
    b = _grid_branches((2, 2), (515, 263, 33))
    assert not any(r["sliceable"] or r["blockable"] for r in b) and sorted(r["h"] for r in b) == [[66, 65], [66, 65], [66, 66], [66, 66]]
    b = _grid_branches((2, 3), (241, 199, 33))
    assert not any(r["sliceable"] for r in b) and [67, 66, 66] == [b[j]["n_l"] for j in range(3)] and {tuple(r["w"]) for r in b} == {(41, 40, 40), (40, 40, 40)}
    assert {tuple(r["h"]) for r in b} == {(34, 33), (33, 33)}
    for gid in ("3x2", "4x2"):
        _, grid, (shape,), _, _ = table[gid]
        b = _grid_branches(grid, shape)
        assert not any(r["sliceable"] for r in b) and any(len(set(r["h"])) > 1 for r in b) and any(not r["w_equal"] for r in b)
    # row grids: 101, 100, 100 rows; with overlap_chunks = 4 from 64 columns on, n = 262 goes out as chunks of 128, 128 and 6 columns
    b = _grid_branches((3, 1), (301, 262, 5), EXACT_MODES["overlap4"])
    assert [r["m_l"] for r in b] == [101, 100, 100] and all(r["nch"] == 4 and r["chunks"] == [128, 128, 6] for r in b)
    assert all(r["chunks"] == [262] for r in _grid_branches((3, 1), (301, 262, 5)))           # the default: one packed exchange
    b = _grid_branches((4, 1), (1024, 520, 64))
    assert [r["m_l"] for r in b] == [256] * 4 and all(r["chunks"] == [520] for r in b)
    b = _grid_branches((1, 3), (301, 262, 17))
    assert [r["n_l"] for r in b] == [88, 87, 87] and all(r["chunks"] == [r["n_l"]] for r in b)
    # every kind of every grid has its modes, the overlapped H phase only where it exists
    for e in ex.GRID_EXACT:
        cases = ex.grid_exact_cases(e)
        assert len(cases) == len(e[2]) * len(ex.GRID_KINDS) and e[1][0] * e[1][1] <= 8
        for kind, shape, modes in cases:
            assert modes and all(mo in EXACT_MODES for mo in modes)
            assert any(mo.startswith("overlap4") for mo in modes) == (e[1][1] == 1 and e[0] != "4x1" and kind in ex.GRID_OVERLAP_KINDS)


# ---------------------------------------------------------------------------------------------------------- bf16x6: operands with pieces
X6_CASES = [pytest.param(c, False, id="f32-" + c[0]) for c in ex.X6_F32] + [pytest.param(c, True, id="bf16-" + c[0]) for c in ex.X6_BF16]


def test_cut3_is_the_split_of_the_header():
    """x1 = rne_bf16(x), x2 = rne_bf16(x - x1), x3 = rne_bf16(x - x1 - x2): ties go to even, the pieces are bf16 numbers, their sum is
    x, and the example of the design -- 1 + 3 2^-9 cuts to 1 + 2^-7 and -2^-9"""
    x = np.float32([1 + 3 * 2.0 ** -9, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 257 * 2.0 ** -17, 1 + 767 * 2.0 ** -17, 3.0, 0.0, -1 - 2.0 ** -8])
    p = ex.cut3(x)
    assert all(ex.is_bf16(q).all() for q in p)
    assert [float(q[0]) for q in p] == [1 + 2.0 ** -7, -2.0 ** -9, 0.0]
    assert [float(q[1]) for q in p] == [1.0, 2.0 ** -8, 0.0] and [float(q[2]) for q in p] == [1 + 2.0 ** -6, -2.0 ** -8, 0.0]
    assert [float(q[3]) for q in p] == [1.0, 2.0 ** -9, 2.0 ** -17] and [float(q[4]) for q in p] == [1 + 2.0 ** -7, -2.0 ** -9, -2.0 ** -17]
    assert [float(q[7]) for q in p] == [-1.0, -2.0 ** -8, 0.0]
    rs = np.random.RandomState(3)
    y = (rs.rand(4096).astype(np.float32) + np.float32(0.5)) * np.float32(2.0) ** rs.randint(-20, 20, size=4096)
    q = ex.cut3(y)                                                          # (asserts x1 + x2 + x3 == x)
    assert np.all(np.abs(q[1]) <= 2.0 ** -8 * np.abs(y)) and np.all(np.abs(q[2]) <= 2.0 ** -16 * np.abs(y))
    for i, pool in enumerate(ex.X6_POOLS):
        assert np.all(ex.npieces(pool) == i + 1) and np.all(pool > 0)


def _x6_mutations(bf16):
    """(name, keyword arguments of x6_model): each kept term deleted, a piece plane zeroed, the second and third planes swapped (bf16-
    stored A: all three terms are kept, so a swap of the factor's planes is the same sum and only deletions can show)"""
    terms = ex.X3_TERMS if bf16 else ex.X6_TERMS
    muts = [("without x%d y%d" % t, dict(terms=tuple(u for u in terms if u != t))) for t in terms]
    muts += [("plane %d of the factor zero" % (i + 1), dict(terms=terms, f_planes=tuple(0 if j == i else j + 1 for j in range(3)))) for i in range(3)]
    if not bf16:
        muts += [("plane %d of A zero" % (i + 1), dict(terms=terms, a_planes=tuple(0 if j == i else j + 1 for j in range(3)))) for i in range(3)]
        muts += [("planes 2 and 3 of the factor swapped", dict(terms=terms, f_planes=(1, 3, 2))),
                 ("planes 2 and 3 of A swapped", dict(terms=terms, a_planes=(1, 3, 2)))]
    return terms, muts


def _f32_any_order(T, terms, seed):
    """the kept piece products added in float32, term by term in a random order"""
    acc = np.zeros_like(T[(1, 1)], dtype=np.float32)
    for i in np.random.RandomState(seed).permutation(len(terms)):
        acc = acc + T[terms[i]].astype(np.float32)
    return acc.astype(np.float64)


@pytest.mark.parametrize("side", ["aht", "wta"])
@pytest.mark.parametrize("case,bf16", X6_CASES)
def test_pieces_products_are_exact_and_every_term_counts(case, bf16, side):
    """on `pieces_product` operands the model of the kernels' arithmetic EQUALS the float64 product, in float32 too, and the model with
    any one kept term deleted, a plane zeroed or two planes swapped differs from it in every 32 x 32 tile of the output: the GPU
    assertion can fail.  (A contraction of fewer than three indices holds one type of pair per call: the three rotations between them.)"""
    _, m, n, k = case[:4]
    terms, muts = _x6_mutations(bf16)
    seen = {}
    for rot in ex.x6_rots(n if side == "aht" else m):
        A, F = ex.pieces_product(m, n, k, side, bf16a=bf16, rot=rot)
        ref = ex._mm(A, F, side)
        T = ex.x6_pieces_products(A, F, side)
        assert np.array_equal(ex.x6_model(A, F, side, terms, T=T), ref), "the model is not the float64 product"
        assert np.array_equal(_f32_any_order(T, terms, rot), ref)
        assert all(np.array_equal(T[t].astype(np.float32), T[t]) for t in terms), "a sum of piece products is no float32 number"
        assert not any(T[t].any() for t in ex.X6_DROPPED)
        for name, kw in muts:
            seen[name] = seen.get(name, False) | ex.tiles_differ(ex.x6_model(A, F, side, T=T, **kw), ref)
    for name, d in seen.items():
        assert d.all(), "%s: the model equals float64 in tile %s of %s" % (name, tuple(np.argwhere(~d)[0]), d.shape)


@pytest.mark.parametrize("case", [pytest.param(c, id=c[0]) for c in ex.X6_KL])
def test_kl_pieces_are_exact_and_every_term_counts(case):
    """`kl_pieces`: the model of klx_uht_kernel / klx_wtu_kernel equals the float64 U H^T and W^T U for every kind; a term deleted
    from S = W H, or from the second product, changes every 32 x 32 output tile in at least one of the kinds (k >= 4: every kept
    term of both products; k = 1: W and H are single powers of two, only the pieces of U take part)"""
    _, m, n, k = case[:4]
    s_need = ex.X6_TERMS if k >= 4 else ((1, 1),)
    p_need = ex.X6_TERMS if k >= 4 else ((1, 1), (2, 1), (3, 1))
    for which in ("uht", "wtu"):
        seen = {}
        for kind in ex.KLX_KINDS:
            for rot in ex.klx_rots(m):
                A, W, H, U = ex.kl_pieces(m, n, k, kind, rot=rot)
                W64, H64 = W.astype(np.float64), H.astype(np.float64)
                ref = U @ H64.T if which == "uht" else W64.T @ U
                assert np.array_equal(ex.klx_model(A, W, H, which), ref), "%s, kind %s: the model is not the float64 product" % (which, kind)
                assert np.array_equal(ref.astype(np.float32), ref)
                for t in s_need:
                    d = ex.tiles_differ(ex.klx_model(A, W, H, which, s_terms=tuple(u for u in ex.X6_TERMS if u != t)), ref)
                    seen[("S", t)] = seen.get(("S", t), False) | d
                for t in p_need:
                    d = ex.tiles_differ(ex.klx_model(A, W, H, which, p_terms=tuple(u for u in ex.X6_TERMS if u != t)), ref)
                    seen[(which, t)] = seen.get((which, t), False) | d
        for key, d in seen.items():
            assert d.all(), "%s without x%d y%d: the model equals float64 in tile %s of %s" % (key[0], key[1][0], key[1][1], tuple(np.argwhere(~d)[0]), d.shape)


@pytest.mark.parametrize("case", [pytest.param(c, id=c[0]) for c in ex.X6_STREAMED])
def test_pieces_products_fit_the_streamed_shapes(case):
    """the 256 MiB shapes: the generator's own assertions -- the dropped terms are zero for every pair, every piece product is a multiple of
    2^-17, the magnitudes along every line stay below 2^24 units -- which with x = x1 + x2 + x3 (cut3 asserts it) make the kept terms
    add up to the product exactly; every output tile holds every kept term.  (The model itself and the mutations: the smaller shapes.)"""
    _, m, n, k, bf16, _ = case
    terms = ex.X3_TERMS if bf16 else ex.X6_TERMS
    for side in ("aht", "wta"):
        A, F = ex.pieces_product(m, n, k, side, bf16a=bf16)
        import scipy.sparse as sp
        rows, cols = np.nonzero(A)
        Vp, Fp = ex.cut3(A[rows, cols]), [x.astype(np.float64) for x in ex.cut3(F)]
        for a, b in terms:
            X = sp.csr_matrix((Vp[a - 1].astype(np.float64), (rows, cols)), shape=A.shape)
            T = X @ Fp[b - 1].T if side == "aht" else (X.T @ Fp[b - 1]).T
            assert ex.tiles_differ(T, 0.0).all(), "x%d y%d is zero in a whole output tile" % (a, b)


# ---------------------------------------------------------------------------------------------------------- the fp32 dense reach table
# The operands of tests/test_gpu_exact_dense.py at the shapes of ex.DENSE_REACH: exact in fp32 in forward, reversed and tile-rotated
# order, and able to see what the tier is for -- every unit of work a loop iteration owns (a 32-column k-tile of a 128-row block, an
# 8-row batch of a row chunk, a partial slab, a slice of 32 slabs, a 16-row tile of an update trip) contributes a nonzero term to its
# output tile, so deleting or doubling it changes the float64 answer there.
def _rotated_sums(X, Yt, tile, rows, shift):
    """X[rows] @ Yt.T in float32, k-tile by k-tile from tile `shift` on (wrapping), then the same from the back"""
    X, Yt = X[rows].astype(np.float32), Yt.astype(np.float32)
    nk = -(-X.shape[1] // tile)
    out = []
    for order in ([(shift + t) % nk for t in range(nk)], [(shift - t) % nk for t in range(nk)]):
        acc = np.zeros((X.shape[0], Yt.shape[0]), dtype=np.float32)
        for t in order:
            for c in range(t * tile, min((t + 1) * tile, X.shape[1])):
                acc += np.outer(X[:, c], Yt[:, c])
        out.append(acc)
    return out


def _nt_proof(A, H, tile, cid):
    m, n = A.shape
    A64, H64 = A.astype(np.float64), H.astype(np.float64)
    ref = A64 @ H64.T
    nk = -(-n // tile)
    blocks = sorted({0, min(1, (m - 1) // 128), (m - 1) // 128, max(0, m // 128 - 1)})
    for b in blocks:
        rows = slice(128 * b, min(128 * b + 32, m))                                  # the first wave's rows of the block
        for got in _rotated_sums(A, H, tile, rows, b * 37 % nk) + _rotated_sums(A, H, tile, rows, 0):
            assert np.array_equal(got.astype(np.float64), ref[rows]), "%s: A H^T is not exact in float32 (block %d)" % (cid, b)
    nblk = -(-m // 128)
    pad = np.zeros((nblk * 128 - m, H.shape[0]))
    for t in range(nk):
        P = A64[:, t * tile:(t + 1) * tile] @ H64[:, t * tile:(t + 1) * tile].T       # what k-tile t adds, every block at once
        per_block = np.abs(np.vstack([P, pad])).reshape(nblk, -1).max(1)
        assert per_block.min() > 0, "%s: k-tile %d adds nothing to row block %d" % (cid, t, int(per_block.argmin()))


@pytest.mark.parametrize("case", [c for c in ex.DENSE_REACH if c[1] in ("aht", "aht_hblocks", "aht_update_w")], ids=lambda c: c[0])
def test_dense_nt_operands_are_exact_and_see_every_tile(case):
    cid, op, m, n, k, aligned, bf16, _ = case
    tile = 64 if bf16 else 32
    A, W, H, G = ex.dense_nt_operands(m, n, k)
    _nt_proof(A, H, tile, cid)
    for x in (A, W, H):                                                              # bf16 storage is exact
        assert ex.is_bf16(x).all()
    if op == "aht_update_w":
        d = W.astype(np.float32) @ G.astype(np.float32)
        assert np.array_equal(d.astype(np.float64), W.astype(np.float64) @ G)
        eps = np.float32(np.finfo(np.float32).eps)
        assert np.array_equal(d[d > 0] + eps, d[d > 0]), "W G + eps is not absorbed"
        if n >= k:
            A2, W2, H2, Wn, _ = ex.fro_step(m, n, k)
            _nt_proof(A2, H2, tile, cid + " (fro_step)")
            assert ex.is_bf16(A2).all() and ex.tiles_differ(Wn, W2.astype(np.float64), 32).all()


def _col_blocks(P, width=32):
    """per block of `width` columns: does P hold a nonzero there?"""
    pad = np.zeros((P.shape[0], -P.shape[1] % width))
    return np.abs(np.hstack([P, pad])).reshape(P.shape[0], -1, width).max(axis=(0, 2)) > 0


def _chunk_batches(m, rpc, batch):
    """(first row, end row) of every `batch`-row step of every row chunk"""
    return [(r, min(r + batch, e)) for b in range(0, m, rpc) for e in (min(b + rpc, m),) for r in range(b, e, batch)]


@pytest.mark.parametrize("case", [c for c in ex.DENSE_REACH if c[1] in ("wta", "wta_gram", "gram_wtw", "gram_hht")], ids=lambda c: c[0])
def test_dense_tn_operands_are_exact_and_see_every_batch(case):
    cid, op, m, n, k, aligned, bf16, want = case
    count, per = ex.DENSE_CHUNKS[cid]
    if op == "gram_hht":                                                             # H H^T in column splits of `per` columns
        H = np.ascontiguousarray(ex.dense_tn_operands(n, 1, k)[1].T)
        ref = _all_orders(H, H.T, "H H^T") if n * k * k <= 4e6 else H.astype(np.float64) @ H.astype(np.float64).T
        slabs = [H[:, c:c + per].astype(np.float64) for c in range(0, n, per)]
        parts = [s @ s.T for s in slabs]
        for s in slabs:
            for t in range(0, s.shape[1], 32):
                assert (s[:, t:t + 32] @ s[:, t:t + 32].T).any(), "%s: a k-tile of a split adds nothing" % cid
    else:
        A, W = ex.dense_tn_operands(m, n, k)
        Y = W if op == "gram_wtw" else A
        assert ex.is_bf16(A).all() and ex.is_bf16(W).all()
        W64, Y64 = W.astype(np.float64), Y.astype(np.float64)
        ref = W64.T @ Y64
        if m * k * Y.shape[1] <= 4e6:
            _all_orders(W.T, Y, "W^T Y")
        batch = 16 if want["family"].startswith("tn16") else 8
        for r0, r1 in _chunk_batches(m, per, batch):                                 # in every 32-column block of the output: every wave's tile
            assert _col_blocks(W64[r0:r1].T @ Y64[r0:r1]).all(), "%s: the batch of rows %d..%d adds nothing to a column block" % (cid, r0, r1)
            if op == "wta_gram":
                assert (W64[r0:r1].T @ W64[r0:r1]).any()
        parts = [W64[b:b + per].T @ Y64[b:b + per] for b in range(0, m, per)]
    assert len(parts) == count and np.array_equal(sum(parts), ref)
    acc32 = np.zeros(ref.shape, dtype=np.float32)
    for q in reversed(parts):                                                        # the slabs summed in fp32, last first
        acc32 += q.astype(np.float32)
    assert np.array_equal(acc32.astype(np.float64), ref)
    assert all(_col_blocks(q).all() for q in parts), "%s: a partial slab with an all-zero column block" % cid
    if want.get("reduce") == "two_stage":
        assert all(_col_blocks(sum(parts[s:s + 32])).all() for s in range(0, len(parts), 32))


@pytest.mark.parametrize("case", [c for c in ex.DENSE_REACH if c[1] in ("mu_update_w", "mu_update_h")], ids=lambda c: c[0])
def test_dense_update_operands_are_exact_and_see_every_tile(case):
    cid, op, m, n, k, aligned, bf16, _ = case
    rows = m if op == "mu_update_w" else n
    X, S, G = ex.dense_update_operands(rows, k)
    X64 = X.astype(np.float64)
    d = X64 @ G
    d32 = X.astype(np.float32) @ G.astype(np.float32)
    assert np.array_equal(d32.astype(np.float64), d)
    if rows * k * k <= 4e6:
        _all_orders(X, G, "X G")
    eps = np.float32(np.finfo(np.float32).eps)
    assert np.array_equal(d32[d32 > 0] + eps, d32[d32 > 0]), "X G + eps is not absorbed"
    q = np.where(d > 0, X64 * S / np.where(d > 0, d, 1.0), 0.0)
    far = np.abs(q - X64) > 4 * np.spacing(np.maximum(np.abs(q), np.abs(X64)).astype(np.float32))      # a skipped tile is not within c = 3
    pad = np.zeros((-rows % 16, k), dtype=bool)
    assert np.vstack([far, pad]).reshape(-1, 16 * k).any(1).all(), "%s: a 16-row tile the update leaves as it was" % cid


@pytest.mark.parametrize("case", ex.DENSE_KL + ex.DENSE_KL16, ids=lambda c: c[0])
def test_dense_kl_operands_are_exact_and_see_every_tile(case):
    """ex.kl at the shapes of the KL cases: both products exact in float32, every 32-column k-tile of every 128-row tile adds a nonzero
    term to U H^T, every 32-row block adds one to every 32-column block of W^T U, and so does every chunk slab and slice"""
    cid, op, m, n, k, aligned, bf16, want = case
    A, W, H, U = ex.kl(m, n, k)
    W64, H64 = W.astype(np.float64), H.astype(np.float64)
    U32 = (A / (W @ H + np.float32(np.finfo(np.float32).eps))).astype(np.float32)
    assert np.array_equal(U32.astype(np.float64), U), "the quotient is not exact in float32"
    if op == "kl_wtu":
        ref = W64.T @ U
        assert np.array_equal((W.T @ U32).astype(np.float64), ref)
        count, per = ex.DENSE_CHUNKS[cid]
        rb = 16 if want["family"] == "kl16_wtu" else 32                              # the rows a loop iteration owns
        for r0 in range(0, m, rb):
            assert _col_blocks(W64[r0:r0 + rb].T @ U[r0:r0 + rb]).all(), "%s: row block %d adds nothing to a column block" % (cid, r0 // rb)
        parts = [W64[b:b + per].T @ U[b:b + per] for b in range(0, m, per)]
        assert len(parts) == count and np.array_equal(sum(parts), ref)
        if want.get("reduce") == "two_stage":
            assert all(_col_blocks(sum(parts[s:s + 32])).all() for s in range(0, len(parts), 32))
    else:
        ref = U @ H64.T
        assert np.array_equal((U32 @ H.T).astype(np.float64), ref)
        nblk = -(-m // 128)
        pad = np.zeros((nblk * 128 - m, k))
        for t in range(0, n, 32):
            P = U[:, t:t + 32] @ H64[:, t:t + 32].T
            assert np.abs(np.vstack([P, pad])).reshape(nblk, -1).max(1).min() > 0, "%s: k-tile %d adds nothing to a row tile" % (cid, t // 32)


@pytest.mark.parametrize("case", [c for c in ex.DENSE_RESID if c[1] != "sqnorm"], ids=lambda c: c[0])
def test_dense_resid_operands_are_exact_and_see_every_block(case):
    cid, op, m, n, k, aligned, bf16, want = case
    A, W, H, R = ex.dense_resid_operands(m, n, k, whole=op == "resid_sqnorm")
    assert ex.is_bf16(A).all()
    WH = W @ H                                                                       # float32
    assert np.array_equal(WH.astype(np.float64), W.astype(np.float64) @ H.astype(np.float64))
    assert np.array_equal(((A - WH) ** 2).astype(np.float64), R ** 2)
    padr, padc = -m % 32, -n % 128
    blocks = np.pad(R, ((0, padr), (0, padc))).reshape((m + padr) // 32, 32, (n + padc) // 128, 128).max(axis=(1, 3))
    assert (blocks > 0).all(), "%s: a 32-row block of a 128-column block without a residual" % cid


# ---------------------------------------------------------------------------------------------------------- ranks 128 < k <= 256
# The operands of tests/test_gpu_exact_wide.py at the shapes of ex.WIDE_REACH: exact in fp32 forward and reversed, and every unit of work
# a loop iteration of the wide path owns -- a 16 x 16 tile of a row strip of wide_nn_rows_kernel, a 16-row tile of k of wide_upd_h_kernel, a
# panel of the composition -- adds a nonzero term to its output (all terms are non-negative), so dropping or doubling it changes the
# float64 answer there.
def _both_ways(X, Y, what):
    """X @ Y exact in float32 from the front and from the back: term by term where that is affordable, else BLAS on the operands and on
    the operands with the contraction index reversed"""
    if X.shape[0] * X.shape[1] * Y.shape[1] <= 5e7:
        return _all_orders(X, Y, what)
    ref = X.astype(np.float64) @ Y.astype(np.float64)
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    for got, how in ((X32 @ Y32, "BLAS"), (np.ascontiguousarray(X32[:, ::-1]) @ np.ascontiguousarray(Y32[::-1]), "BLAS, reversed")):
        assert np.array_equal(got.astype(np.float64), ref), "%s (%s) is not exact in float32" % (what, how)
    return ref


def _tiles16(X):
    """per 16 x 16 tile of X (ragged edge tiles included): does it hold a nonzero?"""
    r, c = X.shape
    P = np.pad(np.abs(X), ((0, -r % 16), (0, -c % 16)))
    return P.reshape(P.shape[0] // 16, 16, P.shape[1] // 16, 16).max(axis=(1, 3)) > 0


def _panels(ref, axis, per=128):
    """the blocks a wide entry point writes, one per panel call, along `axis` (2: both -- the four blocks of a Gram)"""
    cut = lambda X, ax: [X[:per], X[per:]] if ax == 0 else [X[:, :per], X[:, per:]]
    return [b for half in cut(ref, 0) for b in cut(half, 1)] if axis == 2 else cut(ref, axis)


@pytest.mark.parametrize("case", [c for c in ex.WIDE_REACH if c[1] in ("aht", "wta", "wta_gram", "gram_hht", "gram_wtw")], ids=lambda c: c[0])
def test_wide_product_operands_are_exact_and_every_panel_counts(case):
    cid, op, m, n, k, aligned, bf16, _ = case
    if op == "aht":
        A, W, H, G = ex.dense_nt_operands(m, n, k)
        blocks = _panels(_both_ways(A, H.T, "A H^T"), 1)
        assert ex.is_bf16(A).all()
    elif op == "gram_hht":
        H = np.ascontiguousarray(ex.dense_tn_operands(n, 1, k)[1].T)
        blocks = _panels(_both_ways(H, H.T, "H H^T"), 2)
    else:
        A, W = ex.dense_tn_operands(m, max(n, 1), k)
        assert ex.is_bf16(A).all()
        blocks = _panels(_both_ways(W.T, A, "W^T A"), 0) if op != "gram_wtw" else []
        if op != "wta":
            blocks += _panels(_both_ways(W.T, W, "W^T W"), 2)
    assert len(blocks) == {"aht": 2, "wta": 2, "wta_gram": 6, "gram_hht": 4, "gram_wtw": 4}[op]
    for b in blocks:
        assert b.size and _tiles16(b).all(), "%s: a panel's block with an all-zero 16 x 16 tile" % cid


@pytest.mark.parametrize("case", [c for c in ex.WIDE_REACH if c[1] in ("kl_uht", "kl_wtu")], ids=lambda c: c[0])
def test_wide_kl_operands_are_exact_and_every_tile_counts(case):
    cid, op, m, n, k, aligned, bf16, _ = case
    A, W, H, U = ex.kl(m, n, k)
    U32 = (A / (W @ H + np.float32(np.finfo(np.float32).eps))).astype(np.float32)
    assert np.array_equal(U32.astype(np.float64), U), "the quotient is not exact in float32"
    _both_ways(W, H, "W H")
    # a tile of the quotient image that wide_nn_rows_kernel<W_QUOT> leaves out: H > 0 and every row of W has one nonzero, so a nonzero
    # U[r][c] is a term of row r of U H^T and of column c of W^T U
    assert _tiles16(U).all(), "%s: a 16 x 16 tile of U without a nonzero" % cid
    assert (H > 0).all() and ((W > 0).sum(1) == 1).all()
    ref = _both_ways(U32, H.T, "U H^T") if op == "kl_uht" else _both_ways(W.T, U32, "W^T U")
    for b in _panels(ref, 1 if op == "kl_uht" else 0):
        assert b.any(), "%s: a panel that adds nothing" % cid


@pytest.mark.parametrize("case", [c for c in ex.WIDE_REACH if c[1] in ("resid_sqnorm", "column_err")], ids=lambda c: c[0])
def test_wide_resid_operands_are_exact_and_every_tile_counts(case):
    cid, op, m, n, k, aligned, bf16, _ = case
    A, W, H, R = ex.dense_resid_operands(m, n, k, whole=op == "resid_sqnorm", sum_dtype=np.float64)
    WH = _both_ways(W, H, "W H")
    d = A - (W @ H)                                                                    # float32, as the kernel forms it
    assert np.array_equal(d.astype(np.float64), R) and np.array_equal(A.astype(np.float64) - WH, R)
    assert float((R ** 2).sum()) < 2.0 ** 53 and float((A.astype(np.float64) ** 2).sum()) < 2.0 ** 53
    assert _tiles16(R).all(), "%s: a 16 x 16 tile without a residual" % cid
    if op == "column_err":                                                             # every column of every strip's tile: num and den
        P = np.pad(R, ((0, -m % 16), (0, 0))).reshape(-1, 16, n)
        assert (np.abs(P).max(1) > 0).mean() > 0.99 and _tiles16(A).all()


@pytest.mark.parametrize("case", [c for c in ex.WIDE_REACH if c[1] in ("mu_update_w", "mu_update_h")], ids=lambda c: c[0])
def test_wide_update_operands_are_exact_and_every_tile_counts(case):
    """X G exact and absorbing eps; the update moves an element by more than the c = 3 of the comparison in every 16 x 16 tile of W (a
    trip of the column loop of wide_nn_rows_kernel<W_UPD_W>) and of H (a 16-row tile of k of a wave's 16 columns in wide_upd_h_kernel)"""
    cid, op, m, n, k, aligned, bf16, _ = case
    rows = m if op == "mu_update_w" else n
    X, S, G = ex.dense_update_operands(rows, k)
    X64 = X.astype(np.float64)
    d = _both_ways(X, G, "X G")
    d32 = d.astype(np.float32)
    eps = np.float32(np.finfo(np.float32).eps)
    assert np.array_equal(d32[d32 > 0] + eps, d32[d32 > 0]), "X G + eps is not absorbed"
    q = np.where(d > 0, X64 * S / np.where(d > 0, d, 1.0), 0.0)
    far = np.abs(q - X64) > 4 * np.spacing(np.maximum(np.abs(q), np.abs(X64)).astype(np.float32))
    assert _tiles16(far if op == "mu_update_w" else far.T).all(), "%s: a 16 x 16 tile the update leaves as it was" % cid


@pytest.mark.parametrize("k", ex.WIDE_FIT_KS)
def test_wide_fit_operands_are_fixed_points(k):
    """`fro_fixed`, `kl_fixed` and `kl_moved` accept the wide ranks at the shape of the whole-fit cases, and one step of the float32 model
    (any order of the sums) returns its input"""
    m, n = ex.WIDE_FIT_SHAPE
    for seed in (0, 1):
        for order in ("forward", "reversed"):
            A, W, H = ex.fro_fixed(m, n, k, seed=seed)
            W1, H1 = _fro_step32(A, W, H, order, True)
            assert np.array_equal(_bits(W1), _bits(W)) and np.array_equal(_bits(H1), _bits(H))
            A, W, H = ex.kl_fixed(m, n, k, seed=seed)
            W1, H1 = _kl_step32(A, W, H, order, True, True)
            assert np.array_equal(_bits(W1), _bits(W)) and np.array_equal(_bits(H1), _bits(H))
            A, W, H = ex.kl_moved(m, n, k, seed=seed)
            W1, H1 = _kl_step32(A, W, H, order, False, True)
            assert np.array_equal(_bits(W1), _bits(W)) and np.array_equal(_bits(H1), _bits(2 * H))
            W2, H2 = _kl_step32(A, W1, H1, order, False, False)
            assert np.array_equal(_bits(H2), _bits(H1))
