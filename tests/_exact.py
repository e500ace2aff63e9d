"""Exact-by-construction operands for the kernel tests (tests/test_exact_cpu.py proves them, tests/test_gpu_exact.py uses them).

Every product the kernels form on these operands is exact in fp32 -- small non-negative integers, or dyadic rationals with few
significant bits -- so the sums come out the same in every summation order, split-K plan and MFMA shape, and a product is compared
with float64 bit for bit.  Where a kernel divides, the numerator and the denominator are still exact and each element is held to
an ulp bound against the float64 quotient (`assert_ulp`).  Every generator asserts its own range bound: all terms are non-negative
multiples of a common power of two, so a total below 2^24 of those units bounds every partial sum as well.

`Poisoned` places an operand inside a larger buffer whose padding, the elements before the view and a guard band after it hold
NaN (a legal PyTorch view); outputs sit in a buffer filled with a sentinel.  `check()` asserts that nothing outside the view changed.
"""
import numpy as np

MANT = {np.float32: 24, np.float64: 53}


def _bound(total, unit, dtype, what):
    """all terms non-negative multiples of `unit`: every partial sum is exact when the total is below 2^mantissa units"""
    top = float(np.max(total)) if np.size(total) else 0.0
    lim = float(unit) * 2.0 ** MANT[np.dtype(dtype).type]
    assert top < lim, "%s: total %g reaches 2^%d units of %g -- the shape is too large for exact operands" % (what, top, MANT[np.dtype(dtype).type], unit)


def products(m, n, k, dtype=np.float32, seed=0):
    """A in 0..7, W and H in 1..3 with some zero rows / columns: A H^T, W^T A, the Grams, and the MU denominators W (H H^T),
    (W^T W) H are integers.  The denominators are 0 (a zero row of W / column of H: that factor element stays 0) or >= 2 and
    below 2^22, so eps is absorbed in every order (an integer below 2^22 is an even number of its own ulps).  float64: below 2^51,
    where an integer >= 2 absorbs eps = 2^-52 the same way (it is at most half an ulp, and at 2 and 3, where it is exactly half, the
    integer's last bit is even)."""
    rs = np.random.RandomState(seed + 1009 * m + 17 * n + k)
    A = rs.randint(0, 8, size=(m, n)).astype(dtype)
    A[rs.rand(m, n) < 0.2] = 0
    W = rs.randint(1, 4, size=(m, k)).astype(dtype)
    H = rs.randint(1, 4, size=(k, n)).astype(dtype)
    W[rs.rand(m) < 0.05] = 0
    H[:, rs.rand(n) < 0.05] = 0
    A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
    G, GW = H64 @ H64.T, W64.T @ W64
    dw, dh = W64 @ G, GW @ H64
    for tot, what in ((A64 @ H64.T, "A H^T"), (W64.T @ A64, "W^T A"), (G, "H H^T"), (GW, "W^T W")):
        _bound(tot, 1.0, dtype, what)
    for d, what in ((dw, "W HH^T"), (dh, "W^TW H")):
        _bound(d, 0.25, dtype, what)                # below 2^22 (float64: 2^51 -- an integer in [2, 2^51) absorbs 2^-52 as well)
        assert np.all((d == 0) | (d >= 2)), what
    return A, W, H


def _groups(n, k, tmax):
    """k power-of-two group widths 2^t (t <= tmax) that tile the first columns of n; the columns after the last group stay zero in H"""
    t = [0] * k
    used = k
    while used < n:
        j = min(range(k), key=lambda i: t[i])
        if t[j] >= tmax or used + (1 << t[j]) > n:
            break
        used += 1 << t[j]
        t[j] += 1
    assert used <= n, (n, k)
    return t


def fro_step(m, n, k, dtype=np.float32, seed=0, tmax=6):
    """One MU/Frobenius step with an exact W phase: H has one nonzero per column, 2^-t_j in the 2^t_j columns of group j (G = H H^T
    is diag(2^-t_j)); W[r][j] = 2^(t_j + 1 + s), s in 0..2 (W G = 2^(1 + s) >= 2); A in {0, 2^a}.  The new W is then 2^a times the
    count of nonzeros of A's row in group j, exactly.  The H phase has exact numerators 2^2a sum_r cnt A/2^a and single-term
    denominators 2^2a (cnt^T cnt)[j][g] 2^-t_g >= 2 (a chosen for that), below 2^22 units, so only its quotient rounds.
    Returns A, W, H and the expected new W (exact) and the float64 quotient of the new H."""
    assert n >= k
    rs = np.random.RandomState(seed + 31 * m + 7 * n + k)
    t = _groups(n, k, tmax)
    a = (max(t) + 2) // 2
    H = np.zeros((k, n), dtype=np.float64)
    grp = np.full(n, -1)
    c = 0
    for j in range(k):
        w = 1 << t[j]
        H[j, c:c + w] = 2.0 ** -t[j]
        grp[c:c + w] = j
        c += w
    p = min(0.5, max(0.05, 40.0 / max(m, 1) ** 0.5 / 2 ** (max(t) / 2)))
    A = np.where(rs.rand(m, n) < p, 2.0 ** a, 0.0)
    W = np.stack([2.0 ** (t[j] + 1 + rs.randint(0, 3, size=m)) for j in range(k)], axis=1)
    G = H @ H.T
    assert np.array_equal(G, np.diag(np.diag(G)))
    AH = A @ H.T
    Wn = W * AH / (W @ G)
    cnt = AH / 2.0 ** a * 2.0 ** np.array(t)                     # nonzeros of A per row and group
    assert np.array_equal(Wn, 2.0 ** a * cnt)
    num, den = Wn.T @ A, (Wn.T @ Wn) @ H
    _bound(cnt.T @ cnt, 0.25, dtype, "H-phase denominators")                      # below 2^22 (float64: 2^51) units of 2^(2a - t_g) >= 2
    _bound(num, 2.0 ** (2 * a), dtype, "W_new^T A")
    assert np.all((den == 0) | (den >= 2)), "an H-phase denominator in (0, 2): raise a"
    Hq = np.where(den > 0, H * num / np.where(den > 0, den, 1.0), 0.0)
    return A.astype(dtype), W.astype(dtype), H.astype(dtype), Wn, Hq


def kl(m, n, k, dtype=np.float32, seed=0, qmax=3):
    """KL operands with an exact quotient U = A / (W H + eps): W has one nonzero per row, a power of two 2^(0..2) in column j(r);
    H[j][c] = 2^q, q in 1..qmax.  (W H)[r][c] = W[r][j(r)] H[j(r)][c] is a power of two >= 2, so eps is absorbed and U is A times a
    power of two; U H^T and W^T U are sums of multiples of 2^-(2 + qmax), A in 0..7.  rowsum(H) >= 2 and colsum(W) are integers
    (a colsum of 0 or 1 does not absorb eps: the reference of the KL H update rounds colsum + eps to float32 as the kernel does)."""
    rs = np.random.RandomState(seed + 13 * m + 5 * n + 3 * k)
    A = rs.randint(0, 8, size=(m, n)).astype(np.float64)
    A[rs.rand(m, n) < 0.2] = 0
    jr = rs.randint(0, k, size=m)
    W = np.zeros((m, k))
    W[np.arange(m), jr] = 2.0 ** rs.randint(0, 3, size=m)
    H = 2.0 ** rs.randint(1, qmax + 1, size=(k, n))
    WH = W @ H
    assert np.all(WH >= 2) and np.array_equal(np.log2(WH), np.round(np.log2(WH)))
    U = A / WH
    unit = 2.0 ** -(2 + qmax)
    _bound(U @ H.T, unit, dtype, "U H^T")
    _bound(W.T @ U, unit, dtype, "W^T U")
    _bound(H.sum(1), 1.0, np.float32, "rowsum(H)")
    return A.astype(dtype), W.astype(dtype), H.astype(dtype), U


# ---------------------------------------------------------------------------------------------------------- fixed points of a whole MU step
# Operands at which ONE whole MU step -- both phases, the clamp, any number of times -- returns its input bit for bit in fp32 (the small
# whole-fit kernels of csrc/dnmf_small.h over several steps: tests/test_gpu_small_exact.py; proofs: tests/test_exact_cpu.py).
#   W[r][j] = 2^a_r g_j,  H[j][c] = h_j 2^q_c,  g_j, h_j and g_j h_j powers of two with sum_j g_j h_j = 2^s,  A = W H = 2^(a_r + q_c + s).
# Every sum a step forms has terms that are multiples of one power of two with fewer than 2^24 of them in total (exact in any order), and
# every divisor is a power of two >= 2 (eps is absorbed; the kernels divide by multiplying with v_rcp_f32, which is exact there:
# test_rcp_is_exact_at_powers_of_two).  All entries are positive powers of two: the clamp is a no-op, bf16 storage is exact.
def _rank_split(k, rs):
    """g, h (k powers of two each, g >= 2, h >= 1) with sum g h a power of two: 2^S ones (2^S >= 4 k) merged pairwise, two equal values
    into their sum, until k values are left -- the sum stays 2^S --, each value split at random between g and h; g doubled"""
    S = max(0, int(np.ceil(np.log2(k)))) + 2
    vals = [0] * (1 << S)                                       # exponents
    while len(vals) > k:
        dup = [v for v in set(vals) if vals.count(v) >= 2]      # (distinct powers of two never add up to a power of two: there is one)
        v = dup[rs.randint(len(dup))]
        vals.remove(v); vals.remove(v); vals.append(v + 1)
    e = np.array(vals)[rs.permutation(k)]
    u = np.array([rs.randint(0, x + 1) for x in e])
    g, h = 2.0 ** (u + 1), 2.0 ** (e - u)
    assert np.sum(g * h) == 2.0 ** (S + 1)
    return g, h, S + 1


def _pow2_total(L, base, rs):
    """L exponents in {0, 1}, at random places, with sum base^e a power of two (base 2: a total in [L, 2 L]; base 4: one in [L, 4 L],
    which exists when 3 does not divide L, since 4^e = 1 mod 3 and the powers of two alternate between 1 and 2 mod 3)"""
    assert base in (2, 4)
    if base == 4:
        assert L % 3 != 0, "no set of %d powers of four sums to a power of two: a Frobenius fixed point needs m and n not divisible by 3" % L
    for p in range(0, 64):
        t, rem = divmod(2 ** p - L, base - 1)                   # t entries of `base`, L - t of 1
        if 2 ** p >= L and rem == 0 and t <= L:
            break
    e = np.zeros(L, dtype=np.int64)
    e[rs.permutation(L)[:t]] = 1
    tot = float(np.sum(float(base) ** e))
    assert tot == 2.0 ** p
    return e


def _fixed(m, n, k, base, qlo, seed):
    rs = np.random.RandomState(seed + 1013 * m + 19 * n + 7 * k + base)
    g, h, s = _rank_split(k, rs)
    a, q = _pow2_total(m, base, rs), _pow2_total(n, base, rs) + qlo
    W = 2.0 ** a[:, None] * g[None, :]
    H = h[:, None] * 2.0 ** q[None, :]
    A = W @ H
    assert np.array_equal(A, 2.0 ** (a[:, None] + q[None, :] + s))
    # the terms of a sum over j are multiples of the smallest one, min g h >= 2 times the common factor, and add up to 2^s of it
    _bound(2.0 ** s / np.min(g * h), 1.0, np.float32, "a sum over the rank")
    return A, W, H, g, h, a, q


def kl_fixed(m, n, k, dtype=np.float32, seed=0):
    """A fixed point of the MU/KL step: q_c in {1, 2} with sum_c 2^q_c a power of two, a_r in {0, 1} with sum_r 2^a_r one.  W H is a
    power of two >= 2, so U = A / (W H + eps) = 1; U H^T = rowsum(H) = h_j sum 2^q and W^T U = colsum(W) = g_j sum 2^a are what the
    updates divide by, powers of two >= 2: both factors stay; the closing normalisation divides by colsum(W), a power of two."""
    A, W, H, g, h, a, q = _fixed(m, n, k, 2, 1, seed)
    _bound(np.sum(2.0 ** q), 2.0, np.float32, "rowsum(H) = U H^T in units of 2 h_j")
    _bound(np.sum(2.0 ** a), 1.0, np.float32, "colsum(W) = W^T U in units of g_j")
    for d, what in ((A, "W H"), (H.sum(1), "rowsum(H)"), (W.sum(0), "colsum(W)")):
        assert np.all(d >= 2) and np.array_equal(np.log2(d), np.round(np.log2(d))), "%s is not a power of two >= 2" % what
    return A.astype(dtype), W.astype(dtype), H.astype(dtype)


def kl_moved(m, n, k, dtype=np.float32, seed=0):
    """`kl_fixed` with A doubled, for fits with W FIXED: U = 2, so step 0 gives exactly 2 H, where W (2 H) = A: a fixed point from
    step 1 on.  The H of step 1 is the first that is not the caller's array -- a workgroup that reads the caller's H instead of the
    published one doubles it again.  Returns A, W, H; the fit must end at H_out = 2 H."""
    A, W, H = kl_fixed(m, n, k, dtype, seed)
    return (2 * A).astype(dtype), W, H


def fro_fixed(m, n, k, dtype=np.float32, seed=0):
    """A fixed point of the MU/Frobenius step: q_c, a_r in {0, 1} with sum_c 4^q_c and sum_r 4^a_r powers of two (m, n not divisible
    by 3).  A H^T = W (H H^T) and W^T A = (W^T W) H term for term -- 2^(a_r + s) h_j sum 4^q and g_j 2^(q_c + s) sum 4^a --, powers of
    two >= 2 with every partial sum exact.  colsum(W) = g_j sum 2^a_r is an integer >= 2, in general not a power of two: the
    normalisation rounds once per element (the step itself does not)."""
    A, W, H, g, h, a, q = _fixed(m, n, k, 4, 0, seed)
    G, GW = H @ H.T, W.T @ W
    _bound(np.sum(4.0 ** q), 1.0, np.float32, "A H^T in units of 2^(a_r + s) h_j, H H^T in units of h_j h_l")
    _bound(np.sum(4.0 ** a), 1.0, np.float32, "W^T A in units of g_j 2^(q_c + s), W^T W in units of g_j g_l")
    _bound(W.sum(0) / g, 0.25, np.float32, "colsum(W) in units of g_j")                             # below 2^22: s + eps rounds to s
    for d, what in ((W @ G, "W (H H^T)"), (GW @ H, "(W^T W) H")):
        assert np.all(d >= 2) and np.array_equal(np.log2(d), np.round(np.log2(d))), "%s is not a power of two >= 2" % what
    assert np.array_equal(A @ H.T, W @ G) and np.array_equal(W.T @ A, GW @ H) and np.all(W.sum(0) >= 2)
    return A.astype(dtype), W.astype(dtype), H.astype(dtype)


# The reach table of the small whole-fit kernels (csrc/dnmf_small.h; the dispatch of csrc/dnmf_fit.hip): one shape, about the smallest there
# is, for every instantiation the plans can choose, with the plan dnmf_small_fit_plan must report for it -- {route, KP, NW, ALDS, P, ns,
# cw, bf16_resident}; route 1: the barrier kernel, 2: the W-fixed MU/KL kernel, 3: the HALS kernel.  tests/test_capi_small.py asserts every
# entry without a GPU; tests/test_gpu_small_exact.py runs every one.  The Frobenius shapes have m and n not divisible by 3 (`fro_fixed`).
# Between them the barrier-kernel entries of every family hold a single slab (P = 1, NW = 4), the maximum P = 64, a ragged last slab,
# n % 16 != 0 and k = 1, 16, 17, 32; n = 353, 497, ... give the W phase whole groups of four column tiles and a tail, n = 37 a tail alone.
SMALL_FAMILIES = {"kl": (1, 0, 1), "fro": (0, 0, 1), "fro_bf16": (0, 1, 1), "kl_wfixed": (1, 0, 0), "hals": (2, 0, 1), "hals_bf16": (2, 1, 1)}   # method, bf16, w_update
SMALL_REACH = [
    ("kl", 130, 37, 5, (1, 16, 8, 1, 2, 48, 0, 0)),
    ("kl", 100, 20, 16, (1, 16, 6, 1, 2, 32, 0, 0)),
    ("kl", 130, 353, 1, (1, 16, 8, 0, 2, 368, 0, 0)),
    ("kl", 17, 5, 1, (1, 16, 4, 1, 1, 16, 0, 0)),
    ("kl", 50, 497, 7, (1, 16, 4, 0, 1, 512, 0, 0)),
    ("kl", 130, 37, 17, (1, 32, 8, 1, 2, 48, 0, 0)),
    ("kl", 100, 20, 32, (1, 32, 6, 1, 2, 32, 0, 0)),
    ("kl", 130, 305, 20, (1, 32, 8, 0, 2, 320, 0, 0)),
    ("kl", 40, 50, 31, (1, 32, 4, 1, 1, 64, 0, 0)),
    ("kl", 50, 401, 17, (1, 32, 4, 0, 1, 416, 0, 0)),
    ("kl", 8191, 20, 3, (1, 16, 8, 1, 64, 32, 0, 0)),
    ("fro", 130, 37, 5, (1, 16, 8, 1, 2, 48, 0, 0)),
    ("fro", 100, 20, 16, (1, 16, 6, 1, 2, 32, 0, 0)),
    ("fro", 130, 353, 1, (1, 16, 8, 0, 2, 368, 0, 0)),
    ("fro", 17, 5, 1, (1, 16, 4, 1, 1, 16, 0, 0)),
    ("fro", 50, 497, 7, (1, 16, 4, 0, 1, 512, 0, 0)),
    ("fro", 130, 37, 17, (1, 32, 8, 1, 2, 48, 0, 0)),
    ("fro", 100, 20, 32, (1, 32, 6, 1, 2, 32, 0, 0)),
    ("fro", 130, 305, 20, (1, 32, 8, 0, 2, 320, 0, 0)),
    ("fro", 40, 50, 31, (1, 32, 4, 1, 1, 64, 0, 0)),
    ("fro", 50, 401, 17, (1, 32, 4, 0, 1, 416, 0, 0)),
    ("fro", 8191, 20, 3, (1, 16, 8, 1, 64, 32, 0, 0)),
    ("fro_bf16", 130, 37, 5, (1, 16, 8, 1, 2, 48, 0, 0)),
    ("fro_bf16", 130, 497, 5, (1, 16, 8, 0, 2, 512, 0, 0)),
    ("fro_bf16", 17, 5, 1, (1, 16, 4, 1, 1, 16, 0, 0)),
    ("fro_bf16", 50, 833, 7, (1, 16, 4, 0, 1, 848, 0, 0)),
    ("fro_bf16", 130, 37, 17, (1, 32, 8, 1, 2, 48, 0, 0)),
    ("fro_bf16", 130, 370, 20, (1, 32, 8, 0, 2, 384, 0, 0)),
    ("fro_bf16", 40, 50, 31, (1, 32, 4, 1, 1, 64, 0, 0)),
    ("fro_bf16", 50, 593, 17, (1, 32, 4, 0, 1, 608, 0, 0)),
    ("fro_bf16", 8191, 20, 3, (1, 16, 8, 1, 64, 32, 0, 0)),
    ("fro_bf16", 100, 20, 16, (1, 16, 4, 1, 2, 32, 0, 0)),
    ("fro_bf16", 100, 20, 32, (1, 32, 4, 1, 2, 32, 0, 0)),
    ("kl_wfixed", 530, 21, 5, (2, 16, 8, 0, 2, 32, 0, 0)),
    ("kl_wfixed", 530, 21, 17, (2, 32, 8, 0, 2, 32, 0, 0)),
    ("kl_wfixed", 2270, 20, 5, (1, 16, 8, 1, 18, 32, 0, 0)),
    ("kl_wfixed", 1102, 20, 17, (1, 32, 8, 1, 9, 32, 0, 0)),
    ("hals", 50, 37, 5, (3, 16, 4, 0, 1, 48, 48, 0)),
    ("hals", 130, 37, 5, (3, 16, 8, 0, 2, 48, 24, 0)),
    ("hals", 50, 37, 17, (3, 32, 4, 0, 1, 48, 48, 0)),
    ("hals", 130, 37, 17, (3, 32, 8, 0, 2, 48, 24, 0)),
    ("hals", 8191, 20, 3, (3, 16, 8, 0, 64, 32, 1, 0)),
    ("hals", 17, 5, 1, (3, 16, 4, 0, 1, 16, 16, 0)),
    ("hals", 100, 20, 16, (3, 16, 4, 0, 2, 32, 16, 0)),
    ("hals", 40, 50, 32, (3, 32, 4, 0, 1, 64, 64, 0)),
    ("hals_bf16", 50, 37, 5, (3, 16, 4, 1, 1, 48, 48, 1)),
    ("hals_bf16", 130, 37, 5, (3, 16, 8, 1, 2, 48, 24, 1)),
    ("hals_bf16", 50, 37, 17, (3, 32, 4, 1, 1, 48, 48, 1)),
    ("hals_bf16", 130, 37, 17, (3, 32, 8, 1, 2, 48, 24, 1)),
    ("hals_bf16", 50, 610, 5, (3, 16, 4, 0, 1, 624, 624, 0)),
    ("hals_bf16", 130, 417, 5, (3, 16, 8, 0, 2, 432, 216, 0)),
    ("hals_bf16", 50, 370, 17, (3, 32, 4, 0, 1, 384, 384, 0)),
    ("hals_bf16", 130, 290, 17, (3, 32, 8, 0, 2, 304, 152, 0)),
    ("hals_bf16", 8191, 20, 3, (3, 16, 8, 1, 64, 32, 1, 1)),
    ("hals_bf16", 17, 5, 1, (3, 16, 4, 1, 1, 16, 16, 1)),
    ("hals_bf16", 100, 20, 16, (3, 16, 4, 1, 2, 32, 16, 1)),
    ("hals_bf16", 40, 50, 32, (3, 32, 4, 1, 1, 64, 64, 1)),
]


# The data of the HALS rows of the table (tests/test_gpu_small_exact.py compares with the float64 loop of the checker): the random data of
# tests/test_gpu_fit.py -- A uniform in [0.01, 1.01) with every seventh column zero at odd seeds, factors uniform in [0, 1) -- wherever
# that loop is well-conditioned.  At the four shapes below it is not: with k close to n or above m / 3 on full-rank data components die
# at the clamp or survive depending on the last bits, and the checker's OWN loop run in numpy float32 ends 0.6 to 1.2 of the largest
# entry away from its float64 run after 11 steps (tests/test_exact_cpu.py asserts that, and that it stays within 5e-4 on the data used
# here at every shape and seed); there the data has rank k plus 1 % noise.
HALS_RANK_K = {(50, 37, 17), (40, 50, 32), (50, 370, 17), (100, 20, 16)}
HALS_SEEDS = (10, 11, 12)


def hals_problem(m, n, k, seed, rank_k=None):
    rs = np.random.RandomState(seed + m + 7 * n + k)
    if (m, n, k) in HALS_RANK_K if rank_k is None else rank_k:
        A = (rs.rand(m, k) + 0.1) @ (rs.rand(k, n) + 0.1) + 0.01 * rs.rand(m, n)
    else:
        A = rs.rand(m, n) + 0.01
        if seed % 2:
            A[:, ::7] = 0.0
    return A.astype(np.float32), rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- one exact HALS sweep
# HALS has no exact fixed point, but ONE sweep from a chosen state is exact: the generators below work backwards from the answer
# (tests/test_exact_cpu.py proves them in every order, tests/test_gpu_exact_hals.py holds the kernels of csrc/dnmf_hals.h to them).
# Two values of the clamp go through the entry points' `eps` argument:
#   HALS_EPS_A = 2^-3   a clamped entry is an ordinary dyadic number: every sum of the sweep is exact in fp32 in any order;
#   HALS_EPS_B = 2^-23  the library's eps.  A clamped w = eps / 2^p reaches a later t[j] as a term below a quarter ulp of its integer value
#                       (|t| >= 1), which the single rounding of each fmaf absorbs -- the generator keeps the sum of those terms along
#                       every row below 2^-25 --, so the fp32 results are the integers of the construction again.
HALS_EPS_A = 2.0 ** -3
HALS_EPS_B = 2.0 ** -23
HALS_ROWS = 512                                                   # rows per workgroup of the persistent sweep (HALS_WG, csrc/dnmf_common.h)


def _sym_gram(k, rs):
    """symmetric, off-diagonals in {1, 2} (no zero a mutation could hide behind), diagonal in 2..5"""
    G = np.triu(rs.randint(1, 3, size=(k, k)), 1)
    return (G + G.T + np.diag(rs.randint(2, 6, size=k))).astype(np.float64)


def _squares_to(total, n, rs):
    """n values in {1, 2, 3}, at random places, whose squares add up to `total`: n + 3 a + 8 b = total with a twos and b threes (the
    threes are what frees n from any condition modulo 3).  None if there is no such split."""
    X = total - n
    if X < 0:
        return None
    b = np.arange(0, min(n, X // 8) + 1)
    a3 = X - 8 * b
    ok = (a3 % 3 == 0) & (a3 // 3 + b <= n)
    if not ok.any():
        return None
    b = int(rs.choice(b[ok]))
    a = (X - 8 * b) // 3
    v = np.ones(n)
    v[:a] = 2
    v[a:a + b] = 3
    return v[rs.permutation(n)]


def hals_w_exact(W_old, AH, G, eps, dtype=np.float32):
    """The W sweep in exact arithmetic, each value rounded ONCE to `dtype`: for every column kk, t = AH[:, kk] - sum_{l > kk} W_old[:, l]
    G[l][kk] - sum_{l < kk} W_new[:, l] G[l][kk]; u = max(t, eps); ss2 = sum u^2; W_new[:, kk] = u / dtype(sqrt(ss2)).  The float64 sums
    here are exact on the generators' operands (multiples of 2^-(23 + p) below 2^12: `hals_w_problem` asserts the range).  Returns the
    pre-clamp values t, W_new and ss2 (float64)."""
    W_old, AH, G = (np.asarray(x, dtype=np.float64) for x in (W_old, AH, G))
    m, k = W_old.shape
    T, Wn, ss2 = np.zeros((m, k)), np.zeros((m, k)), np.zeros(k)
    for kk in range(k):
        t = AH[:, kk] - W_old[:, kk + 1:] @ G[kk + 1:k, kk] - Wn[:, :kk] @ G[:kk, kk]
        T[:, kk] = t.astype(dtype)
        u = np.maximum(T[:, kk], eps)
        ss2[kk] = np.sum(u * u)
        ss = float(dtype(np.sqrt(ss2[kk])))
        Wn[:, kk] = (u / ss).astype(dtype) if ss > 0 else u
    return T, Wn, ss2


def hals_w_problem(m, k, eps, seed=0, dtype=np.float32):
    """One exact W sweep (csrc/dnmf_hals.h), built backwards from the answer.  Returns a dict: W_old, AH (m x k), G (k x k), the
    expected pre-clamp values T_final (column kk at its own turn), W_new, ss2 (k float64), p (ss2 = 4^p up to the eps terms), ss2_tol
    (0 for HALS_EPS_A) and `clamped` (m x k bool).

    G: `_sym_gram`.  W_old in 0..3.  Column kk of the clamped pre-normalisation U: eps in its clamped rows, values of {1, 2, 3} elsewhere
    with sum U^2 = 4^p_kk exactly (`_squares_to`; with eps = 2^-3 the 64 clamped rows add 64 eps^2 = 1 to it, with eps = 2^-23 their
    2^-46 each vanish in float(sqrt(ss2)) and ss2 is held to ss2_tol = the eps terms plus one float64 rounding per addition).  So
    (float)sqrt(ss2) = 2^p_kk and W_new = U / 2^p_kk is exact.  The pre-clamp target is U where not clamped and an integer in -3..-1
    where clamped; AH[i][kk] = target + sum_{l > kk} W_old[i][l] G[l][kk] + sum_{l < kk} W_new[i][l] G[l][kk] (eps = 2^-23: without the
    clamped W_new terms, so AH is an integer and the exact sweep ends a hair below the target, rounded once: the target).
    Clamped rows: the last row in even columns, the first row of the last workgroup in odd ones (eps = 2^-23: in columns 0 and 1 only),
    the others at random (eps = 2^-3: 64 per column, m >= 130; eps = 2^-23: two per column, dealt round so that no row clamps often,
    m >= 16).  Smaller m: no row clamps (m = 1 cannot have both kinds).

    ss2_tol, eps = 2^-23: the integer squares and all their partial sums are exact in float64; only a partial sum that carries one of the
    n_c terms of 2^-46 can round, by at most half a spacing of 4^p, and along its way to the total it does so where it merges with
    another such partial or crosses a binade (at most 2 p + 2 of them; between those it stays on the grid it was rounded to, the
    integers added to it are multiples of that grid).  So |ss2 - 4^p| <= n_c (2^-46 + (2 p + 5) spacing(4^p) / 2).

    dtype = float64 with eps = 2^-23: float64 does NOT absorb the clamped terms, so AH carries them (exact: multiples of 2^-(23 + p)
    below 2^12) and the pre-clamp values are the integers again, exactly; ss2 = 4^p + n_c 2^-46 is then no float64 number, its square root
    rounds and every later column sees a W_new that is off in the last bits.  `W_rel` bounds that per column (R = 2^-53, M the largest
    sum of magnitudes of a row): tau_j = sum_{l < j} G[l][j] 3 / 2^p_l c_l + (k + 2) R M bounds the error of t (|t| >= 1 where it does not
    clamp, <= -1 + tau where it does: no clamp flips while tau < 1/2), the sum of squares is within 2 tau_j + 2200 R of its value,
    relatively (at most 2200 additions on any path to the total: two trips, the trees, a chain of 2048 workgroups), its root within half
    of that plus ss2_tol / (2 4^p) + R, and c_j = 1.01 (tau_j + that + R) bounds |w - W_new| / W_new in column j (column 0: exact inputs,
    only ss2_tol and the two roundings)."""
    assert eps in (HALS_EPS_A, HALS_EPS_B), "the construction is proved for eps = 2^-3 and 2^-23"
    mode_a = eps == HALS_EPS_A
    rs = np.random.RandomState(seed + 1013 * m + 7 * k + (0 if mode_a else 3))
    G = _sym_gram(k, rs)
    W_old = rs.randint(0, 4, size=(m, k)).astype(np.float64)
    last, wg0 = m - 1, HALS_ROWS * ((m - 1) // HALS_ROWS)
    clamped = np.zeros((m, k), dtype=bool)
    deal = rs.permutation(m)
    for kk in range(k):
        if mode_a and m >= 130:
            forced = last if kk % 2 == 0 else wg0
            rest = np.setdiff1d(np.arange(m), [forced])
            clamped[rs.choice(rest, size=63, replace=False), kk] = True
            clamped[forced, kk] = True
        elif not mode_a and m >= 16:
            clamped[deal[[(2 * kk) % m, (2 * kk + 1) % m]], kk] = True
            if kk < 2:
                clamped[last if kk == 0 else wg0, kk] = True
    U = np.zeros((m, k))
    p = np.zeros(k, dtype=np.int64)
    for kk in range(k):
        free = np.flatnonzero(~clamped[:, kk])
        nc = m - free.size
        for pk in range(0, 16):
            v = _squares_to(4 ** pk - (nc // 64 if mode_a else 0), free.size, rs)
            if v is not None:
                break
        assert v is not None, "no column of %d values in {1, 2, 3} has a power of four as its sum of squares" % free.size
        U[free, kk], U[clamped[:, kk], kk], p[kk] = v, eps, pk
    Wn = U / 2.0 ** p[None, :]
    target = np.where(clamped, -rs.randint(1, 4, size=(m, k)).astype(np.float64), U)
    f64b = not mode_a and np.dtype(dtype) == np.float64
    Wn_seen = Wn if mode_a or f64b else np.where(clamped, 0.0, Wn)
    AH = target + W_old @ np.tril(G, -1) + Wn_seen @ np.triu(G, 1)
    # range: every value of the sweep is a multiple of `unit`; the sum of the magnitudes of all terms of a row bounds every partial sum
    unit = (eps if mode_a else 1.0) / 2.0 ** p.max()
    top = np.max(np.abs(AH) + 3 + (W_old + Wn) @ G + W_old * np.diag(G)[None, :])
    assert top < unit * 2.0 ** 24 if mode_a else top * 2.0 ** (23 + p.max()) < 2.0 ** 52, "m = %d, k = %d: the sweep leaves the exact range" % (m, k)
    if not mode_a:                                                  # the clamped terms a row collects stay below a quarter ulp of 1
        tiny = np.where(clamped, eps / 2.0 ** p[None, :], 0.0) @ np.triu(G, 1)
        assert tiny.max(initial=0.0) < 2.0 ** -25, "m = %d, k = %d: a row clamps too often for eps = 2^-23" % (m, k)
    nc = clamped.sum(0)
    ss2_tol = np.zeros(k) if mode_a else nc * (eps * eps + (2 * p + 5) * np.spacing(4.0 ** p) / 2)
    W_rel = np.zeros(k)
    if f64b:                                                        # the exact sweep with the exact W_new: the integers, and 4^p + n_c eps^2
        T = AH - W_old @ np.tril(G, -1) - Wn @ np.triu(G, 1)
        W_new, ss2 = Wn, 4.0 ** p + nc * eps * eps
        R = 2.0 ** -53
        for j in range(k):
            tau = (G[:j, j] * 3 / 2.0 ** p[:j]) @ W_rel[:j] + (k + 2) * R * top if j else 0.0
            root = ((2 * tau + 2200 * R) / 2 if j else 0.0) + ss2_tol[j] / (2 * 4.0 ** p[j]) + R
            W_rel[j] = 1.01 * (tau + root + R)
            assert tau < 0.5, "m = %d, k = %d: the float64 bound with eps = 2^-23 reaches a clamp decision at column %d" % (m, k, j)
            ss2_tol[j] += (2 * tau + 2200 * R) * 4.0 ** p[j] if j else 0.0
    else:
        T, W_new, ss2 = hals_w_exact(W_old, AH, G, eps)
    assert np.array_equal(T, target) and np.array_equal(W_new, Wn), "the exact sweep does not end at the constructed answer"
    if mode_a:
        assert np.array_equal(ss2, 4.0 ** p)
    for s in (ss2 - ss2_tol, ss2 + ss2_tol):
        assert np.array_equal(np.sqrt(s).astype(np.float32), 2.0 ** p)
    if not f64b:
        assert np.all(np.abs(ss2 - 4.0 ** p) <= ss2_tol)
    if m >= (130 if mode_a else 16):
        assert clamped.any(0).all() and (~clamped).any(0).all() and clamped[last].any() and clamped[wg0:].any()
    cast = lambda x: x.astype(dtype)
    for x in (W_old, AH, G, W_new):
        assert np.array_equal(cast(x).astype(np.float64), x)
    return dict(W_old=cast(W_old), AH=cast(AH), G=cast(G), T_final=target, W_new=W_new, ss2=ss2, p=p, ss2_tol=ss2_tol, W_rel=W_rel, clamped=clamped)


def hals_h_exact(H_old, AtW, G2, eps, dtype=np.float32):
    """The H sweep in exact arithmetic, each row rounded once: H[kk] = max(H[kk] + AtW[kk] - G2[kk] . H, eps) with the rows above kk
    already updated (float64 sums, exact on the generator's operands)."""
    H = np.array(H_old, dtype=np.float64)
    AtW, G2 = np.asarray(AtW, dtype=np.float64), np.asarray(G2, dtype=np.float64)
    for kk in range(H.shape[0]):
        H[kk] = np.maximum((H[kk] + AtW[kk] - G2[kk] @ H).astype(dtype), eps)
    return H


def hals_h_problem(k, n, eps, seed=0):
    """One exact H sweep: H_old in 0..3, G2 = `_sym_gram`, the new H chosen first -- eps where it clamps (from a pre-clamp integer in
    -3..-1), 1..3 elsewhere -- and AtW solved for: AtW[kk] = pre-clamp - H_old[kk] + sum_{j >= kk} G2[kk][j] H_old[j] + sum_{j < kk}
    G2[kk][j] H_new[j].  eps = 2^-3: any entry may clamp (each with probability 0.3); every value is a multiple of 2^-3 below 2^21.
    eps = 2^-23: a clamped eps is not absorbed by the integers it meets, so the clamped rows of a column are its LAST ones, from a row
    s_c that runs over 0..k with c: the rows above them never see an eps and those below clamp whatever it does to their pre-clamp
    value (<= -1 + k 2^-21); AtW leaves the eps terms out.  Every row (k > 1) has clamped and unclamped columns for n >= k + 1.
    Returns H_old, AtW, G2 and the expected new H (float64)."""
    assert eps in (HALS_EPS_A, HALS_EPS_B)
    mode_a = eps == HALS_EPS_A
    rs = np.random.RandomState(seed + 101 * k + 3 * n + (0 if mode_a else 1))
    G2 = _sym_gram(k, rs)
    H_old = rs.randint(0, 4, size=(k, n)).astype(np.float64)
    if mode_a:
        clamped = rs.rand(k, n) < 0.3
        clamped[rs.randint(k, size=n), np.arange(n)] |= n > 1       # (and at least one per column)
    else:
        clamped = np.arange(k)[:, None] >= ((np.arange(n) + 1) % (k + 1))[None, :]
    Hn = np.where(clamped, eps, rs.randint(1, 4, size=(k, n)).astype(np.float64))
    pre = np.where(clamped, -rs.randint(1, 4, size=(k, n)).astype(np.float64), Hn)
    seen = Hn if mode_a else np.where(clamped, 0.0, Hn)
    AtW = pre - H_old + np.triu(G2) @ H_old + np.tril(G2, -1) @ seen
    _bound(np.abs(AtW) + 3 + G2 @ (H_old + Hn) + H_old, eps if mode_a else 2.0 ** -3, np.float32, "the H sweep")
    assert np.array_equal(hals_h_exact(H_old, AtW, G2, eps), Hn), "the exact H sweep does not end at the constructed answer"
    f32 = lambda x: x.astype(np.float32)
    for x in (H_old, AtW, G2, Hn):
        assert np.array_equal(f32(x).astype(np.float64), x)
    return f32(H_old), f32(AtW), f32(G2), Hn


def hals_h_step_problem(m, n, k, seed=0):
    """The H phase of ONE HALS step with W FIXED, exact from a real A and W (eps = 2^-3): where `hals_h_problem` hands the sweep kernel
    a made-up AtW and G2, here they are W^T A and W^T W of small integers, so on a grid they are what crosses the ranks.  Most rows of
    W hold one entry in {1, 2}, about 15 % a second entry, a 1, in another column (the off-diagonals of G2), about 3 % are zero;
    Ht in 0..3; A = W Ht + (a 0/1 noise at 10 %) with 5 % of the entries zeroed; H_old = max(Ht + {-1, 0, 1}, 0) (-1 at 10 %, 0 and 1 at 45 %
    each) with 5 % zero columns.
    W^T A and W^T W are non-negative integers, H_old is one, and every row of H[kk] = max(H[kk] + AtW[kk] - G2[kk] . H, eps) is a sum of
    multiples of 2^-3 whose magnitudes add up to less than 2^21 (asserted): exact in float32 in any order, however AtW and G2 were
    summed over the ranks.  Asserted as well, so that a shape the design cannot serve raises: every row of the new H has at least
    10 % unclamped entries, at least 10 % of all entries clamp, every operand is a float32 number, G2 has a nonzero off-diagonal (k >= 2).
    Returns A, W, H_old (float32) and the expected new H (float64, `hals_h_exact`)."""
    eps = HALS_EPS_A
    rs = np.random.RandomState(seed + 31 * m + 7 * n + k + 11)
    W = np.zeros((m, k))
    j1 = rs.randint(0, k, size=m)
    W[np.arange(m), j1] = rs.randint(1, 3, size=m)
    if k >= 2:
        second = np.flatnonzero(rs.rand(m) < 0.15)
        W[second, (j1[second] + 1 + rs.randint(0, k - 1, size=second.size)) % k] = 1
    W[rs.rand(m) < 0.03] = 0
    Ht = rs.randint(0, 4, size=(k, n)).astype(np.float64)
    A = W @ Ht + (rs.rand(m, n) < 0.1)
    A[rs.rand(m, n) < 0.05] = 0
    # (an entry that starts BELOW Ht gains about G2[kk][kk] and every later row coupled to it loses G2[kk][j] times that in the same column:
    #  with -1 as likely as 0 and +1 whole rows clamp at m / k of 30 and more, so -1 is the rare offset)
    H_old = np.maximum(Ht + rs.choice([-1, 0, 1], size=(k, n), p=[0.1, 0.45, 0.45]), 0.0)
    H_old[:, rs.rand(n) < 0.05] = 0
    AtW, G2 = W.T @ A, W.T @ W
    Hn = hals_h_exact(H_old, AtW, G2, eps)
    # every value of a row update is a multiple of eps; the sum of the magnitudes of its terms, with the largest |H| the sweep holds
    Hmax = np.maximum(H_old, Hn)
    _bound(Hmax + AtW + G2 @ Hmax, eps, np.float32, "the H phase of a W-fixed HALS step")
    _bound(A.sum(0)[None, :] * W.max(), 1.0, np.float32, "W^T A")
    clamped = Hn == eps                                             # (the rows below a clamped entry hold multiples of eps, not integers)
    assert np.array_equal(Hn / eps, np.rint(Hn / eps)) and Hn.min() >= eps
    assert (1 - clamped.mean(1)).min() >= 0.1, "%d x %d, k = %d: a row of the new H has fewer than 10 %% unclamped entries" % (m, n, k)
    assert clamped.mean() >= 0.1, "%d x %d, k = %d: fewer than 10 %% of the new H clamp" % (m, n, k)
    assert k < 2 or G2[~np.eye(k, dtype=bool)].any(), "%d x %d, k = %d: W^T W is diagonal" % (m, n, k)
    f32 = lambda x: x.astype(np.float32)
    for x in (A, W, H_old, AtW, G2, Hn):
        assert np.array_equal(f32(x).astype(np.float64), x)
    return f32(A), f32(W), f32(H_old), Hn


def kl_refs(A, W, H, U):
    """float64 answers of one MU/KL step on `kl` operands: U H^T, W^T U, rowsum(H), colsum(W), and the quotients of the new W and of
    the new H with W fixed (the divisors as the kernels form them: one fp32 addition of eps)"""
    W64, H64 = W.astype(np.float64), H.astype(np.float64)
    eps32 = np.float32(np.finfo(np.float32).eps)
    UHt, WtU = U @ H64.T, W64.T @ U
    rs, cs = H64.sum(1), W64.sum(0)
    dw = (rs.astype(np.float32) + eps32).astype(np.float64)             # one fp32 addition, as the kernels do
    dh = (cs.astype(np.float32) + eps32).astype(np.float64)
    return UHt, WtU, rs, cs, W64 * UHt / dw[None, :], H64 * WtU / dh[:, None]


def is_bf16(x):
    """element-wise: the float32 value has no bits below bfloat16's 8-bit significand"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & 0xFFFF) == 0


def _column_mix(m):
    """(p, n1, n2, n3, a, b): a column of m rows -- n1 ones, n2 twos, n3 threes, a entries of 1/2, b of 1/4, the rest eps = 1/8 -- whose
    squares add up to 4^p: m + 3 b + 15 a + 63 n1 + 255 n2 + 575 n3 = 64 4^p (n3 = 2 (1 - m) mod 3 leaves a multiple of 3 for a and b)"""
    n3 = (2 * (1 - m)) % 3
    for p in range(0, 12):
        r = 64 * 4 ** p - m - 575 * n3
        if r < 0:
            continue
        n2 = min(r // 255, 40)
        r -= 255 * n2
        n1 = min(r // 63, 6)
        r -= 63 * n1
        a, b = (r // 3) // 5, (r // 3) % 5
        if r % 3 == 0 and a <= 6 and 1 <= n1 + n2 + n3 and n1 + n2 + n3 + a + b <= m - 2:
            return p, n1, n2, n3, a, b
    raise AssertionError("no column of %d rows with these values has a power of four as its sum of squares" % m)


def _step_design_bf16(m, n, k, rs):
    """The W phase of `hals_step_problem` with every entry of A representable in bfloat16 (8 significant bits).  What costs bits in
    AH = pre-clamp + sum_{l > kk} W_old G + sum_{l < kk} W_new G is the last sum, so: ONE p for all columns (`_column_mix`: a few rows of
    1/4, 1/2, 1, 2, 3, all others clamped), every off-diagonal of G equal to g = 2^(3 + p) (H2: one column of 2^((3 + p) / 2), or two of
    2^((2 + p) / 2)), so W_new g = 8 U is 1 for a clamped entry and 2, 4, 8, 16, 24 for the others; W_old one-hot with a 1 (or a zero
    row).  AH is then a small integer (plus 1/4 or 1/2 in a row that takes a fraction: those go to the rows with the smallest sums),
    the unclamped values of a column go to the rows that carry least so far.  The columns of A that meet zeros of H_old are free (0..7)."""
    eps = HALS_EPS_A
    nh = n - k
    assert nh >= 2, "the bf16 construction needs n >= k + 2"
    p, n1, n2, n3, a, b = _column_mix(m)
    g = 2.0 ** (3 + p)
    H2 = np.zeros((k, nh))
    nz = 1 if p % 2 else 2
    H2[:, :nz] = 2.0 ** ((3 + p) // 2 if p % 2 else (2 + p) // 2)
    D = 2.0 ** rs.randint(0, 2, size=k)
    H_old = np.hstack([np.diag(D), H2])
    G = H_old @ H_old.T
    assert np.all(G[~np.eye(k, dtype=bool)] == g)
    W_old = np.zeros((m, k))
    hot = rs.randint(0, k + 1, size=m)                              # (k: a zero row)
    W_old[np.arange(m)[hot < k], hot[hot < k]] = 1
    U, clamped, S, load = np.full((m, k), eps), np.ones((m, k), dtype=bool), np.zeros((m, k)), np.zeros(m)
    vals = np.concatenate([np.full(b, 0.25), np.full(a, 0.5), np.full(n1, 1.0), np.full(n2, 2.0), np.full(n3, 3.0)])
    for kk in range(k):
        S[:, kk] = W_old[:, kk + 1:] @ G[kk + 1:, kk] + (U[:, :kk] / 2.0 ** p) @ G[:kk, kk]
        forced = m - 1 if kk % 2 == 0 else 0
        order = np.argsort(S[:, kk] + load + rs.rand(m), kind="stable")
        order = order[order != forced][:vals.size]
        U[order, kk], clamped[order, kk] = vals, False
        load[order] += 8 * vals
    target = np.where(clamped, -np.minimum(rs.randint(0, 4, size=(m, k)), np.floor(S)), U)
    AH = target + S
    A2 = np.zeros((m, nh))
    A2[:, nz:] = rs.randint(0, 8, size=(m, nh - nz))
    A2[:, 0] = rs.rand(m) < 0.5
    A2[((AH - A2 @ H2.T) < 0).any(1), 0] = 0
    A = np.hstack([(AH - A2 @ H2.T) / D[None, :], A2])
    return A, W_old, H_old, G, U, clamped, np.full(k, p), target, AH


def hals_step_problem(m, n, k, seed=0, bf16=False):
    """ONE whole HALS step (W sweep, then the H sweep on the new W) with an exact W phase, eps = 2^-3.  H_old = [D | H2]: D a k x k
    diagonal of 1s and 2s, H2 0/1 with a first column of ones, so G = H_old H_old^T = D^2 + H2 H2^T has off-diagonals >= 1.  The W
    phase is built as in `hals_w_problem` for that G, for any m >= 11: per column 4 clamped rows (the last row in even columns, row 0
    in odd ones), 3 rows of 1/4 and 3 of 1/2 -- together 4/64 + 3/16 + 3/4 = 1 -- and values of {1, 2, 3} whose squares add up to
    4^p - 1.  A clamped pre-clamp value is 0, -1, -2 or -3, as low as A >= 0 allows (with every sum exact nothing can flip a clamp).
    A = [A1 | A2]: A2 0/1, sparse, kept in the rows where A1 = (AH - A2 H2^T) D^-1 stays >= 0, so A H_old^T = AH term for term,
    non-negative multiples of 2^-(3 + p) below 2^24 of them.
    The H phase is NOT exact and cannot be made so: every entry of the new W is >= eps / 2^p > 0, so G2 = W^T W has off-diagonals of
    many bits, each row of the H sweep multiplies them with the rows above it and the bits add up row by row; W^T A itself leaves 24
    bits from m of about a hundred on.  A forward error bound is no substitute: the columns of this W are far from orthogonal (G2
    off-diagonals up to 0.8), the bound of row kk carries those of the rows above it with these weights and passes the values
    themselves from k = 16 on.  It is derived and asserted all the same -- it holds a few 1e-6 of the entries at k = 1, a few per cent
    at k = 5 and k = 12 -- and the H sweep kernels have `hals_h_problem` for every element.  H_err, with u = 2^-24 and g(c) = c u / (1 - c u):
    W^T A and W^T W are sums of m exact non-negative products, within g(m) of their values in any order; row kk of the sweep forms k
    products, their sum and two more additions, in any order within g(2 k + 2) of the sum of the magnitudes, and carries the errors E_j
    of the rows above it with weights G2[kk][j]; the clamp is 1-Lipschitz; magnitudes are enlarged by their own bounds.
    bf16=True: the construction of `_step_design_bf16` instead, every entry of A a bfloat16 number (asserted; a shape it cannot serve
    raises AssertionError and belongs in HALS_STEP_BF16_LEFT).
    Returns a dict: A, W_old, H_old (float32), W_new (the exact new W, float64), H_new (the float64 sweep), H_err, AH, G and `clamped`."""
    eps = HALS_EPS_A
    nh = n - k
    assert nh >= 1 and m >= 11, "the construction needs n > k and m >= 11"
    rs = np.random.RandomState(seed + 31 * m + 7 * n + k + (5 if bf16 else 0))
    if bf16:
        A, W_old, H_old, G, U, clamped, p, target, AH = _step_design_bf16(m, n, k, rs)
        assert is_bf16(A).all(), "%d x %d, k = %d: an entry of A needs more than 8 significant bits" % (m, n, k)
        return _step_finish(m, n, k, eps, A, W_old, H_old, G, U, clamped, p, target, AH)
    D = 2.0 ** rs.randint(0, 2, size=k)
    H2 = (rs.rand(k, nh) < 0.3).astype(np.float64)
    H2[:, 0] = 1
    H_old = np.hstack([np.diag(D), H2])
    G = H_old @ H_old.T
    W_old = rs.randint(0, 4, size=(m, k)).astype(np.float64)
    U, clamped, p = np.zeros((m, k)), np.zeros((m, k), dtype=bool), np.zeros(k, dtype=np.int64)
    for kk in range(k):
        forced = m - 1 if kk % 2 == 0 else 0
        rows = np.concatenate([[forced], rs.permutation(np.setdiff1d(np.arange(m), [forced]))])
        for pk in range(0, 16):
            v = _squares_to(4 ** pk - 1, m - 10, rs)
            if v is not None:
                break
        assert v is not None
        U[rows[:4], kk], U[rows[4:7], kk], U[rows[7:10], kk], U[rows[10:], kk] = eps, 0.25, 0.5, v
        clamped[rows[:4], kk], p[kk] = True, pk
    Wn = U / 2.0 ** p[None, :]
    S = W_old @ np.tril(G, -1) + Wn @ np.triu(G, 1)
    target = np.where(clamped, -np.minimum(rs.randint(0, 4, size=(m, k)), np.floor(S)), U)
    AH = target + S
    A2 = (rs.rand(m, nh) < 0.15).astype(np.float64)
    A2[((AH - A2 @ H2.T) < 0).any(1)] = 0
    A = np.hstack([(AH - A2 @ H2.T) / D[None, :], A2])
    return _step_finish(m, n, k, eps, A, W_old, H_old, G, U, clamped, p, target, AH)


def _step_finish(m, n, k, eps, A, W_old, H_old, G, U, clamped, p, target, AH):
    """the checks of `hals_step_problem` and the float64 H sweep with its bound"""
    Wn = U / 2.0 ** p[None, :]
    unit = eps / 2.0 ** p.max()
    assert A.min() >= 0 and np.array_equal(A @ H_old.T, AH)
    _bound(AH + 3 + (W_old + Wn) @ G + W_old * np.diag(G)[None, :], unit, np.float32, "the W phase of the step")
    _bound(G, 1.0, np.float32, "H H^T")
    T, W_new, ss2 = hals_w_exact(W_old, AH, G, eps)
    assert np.array_equal(T, target) and np.array_equal(W_new, Wn) and np.array_equal(ss2, 4.0 ** p)
    u = 2.0 ** -24
    g = lambda cnt: cnt * u / (1 - cnt * u)
    AtW, G2 = Wn.T @ A, Wn.T @ Wn
    eA, eG = g(m) * AtW, g(m) * G2
    H, E = H_old.copy(), np.zeros((k, n))
    for kk in range(k):
        Hm = np.abs(H) + E
        mag = Hm[kk] + AtW[kk] + eA[kk] + (G2[kk] + eG[kk]) @ Hm
        E[kk] = (eA[kk] + eG[kk] @ Hm + G2[kk] @ E + g(2 * k + 2) * mag) * (1 + 2.0 ** -20)      # (and the float64 evaluation of this reference)
        H[kk] = np.maximum(H[kk] + AtW[kk] - G2[kk] @ H, eps)
    f32 = lambda x: x.astype(np.float32)
    for x in (A, W_old, H_old):
        assert np.array_equal(f32(x).astype(np.float64), x)
    return dict(A=f32(A), W_old=f32(W_old), H_old=f32(H_old), W_new=Wn, H_new=H, H_err=E, AH=AH, G=G, clamped=clamped)


# bf16-A rows of the reach table that `hals_step_problem(bf16=True)` cannot serve (they keep the checks of test_hals_reach only)
HALS_STEP_BF16_LEFT = []


# one step on the big path (no small whole-fit kernel applies): the one-rank route of nmf_algorithms_1D
HALS_STEP_BIG = [(3000, 300, 12), (2100, 260, 40)]


# The shapes of tests/test_gpu_exact_hals.py with what dnmf_hals_sweep_plan must report for each -- (route, KP, grid, transform, vec):
# route 1 = the persistent sweep (grid = ceil(m / 512)), 0 = column launches (grid = min(ceil(m / 256), 2048)); transform 0 = whole
# tiles, 1 = 16-byte rows with guards, 2 = scalar rows.  aligned: 16-byte aligned starts and pitches (`Poisoned`), else odd ones.
def _slots(nwg):
    """m whose last workgroup (of nwg) holds ONE live row"""
    return HALS_ROWS * nwg - (HALS_ROWS - 1)


HALS_W_CASES = [
    # KP = 32
    ("700x5", 700, 5, True, (1, 32, 2, 2, 0)),
    ("1024x32-full-tiles", 1024, 32, True, (1, 32, 2, 0, 0)),
    ("1000x12-guarded", 1000, 12, True, (1, 32, 2, 1, 0)),
    ("1000x12-odd", 1000, 12, False, (1, 32, 2, 2, 0)),
    ("1x1", 1, 1, True, (1, 32, 1, 2, 0)),
    ("513x1", 513, 1, True, (1, 32, 2, 2, 0)),
    # KP = 64
    ("900x33", 900, 33, True, (1, 64, 2, 2, 0)),
    ("1024x64-vec-full", 1024, 64, True, (1, 64, 2, 0, 1)),
    ("1030x36-vec-guarded", 1030, 36, True, (1, 64, 3, 1, 1)),
    ("1030x36-odd", 1030, 36, False, (1, 64, 3, 2, 0)),
    # KP = 128
    ("1500x65", 1500, 65, True, (1, 128, 3, 2, 0)),
    ("1536x128-full-tiles", 1536, 128, True, (1, 128, 3, 0, 0)),
    ("1100x100-guarded", 1100, 100, True, (1, 128, 3, 1, 0)),
    # wide ranks: column launches only
    ("600x129-wide", 600, 129, True, (0, 256, 3, -1, 0)),
    ("300x256-wide", 300, 256, False, (0, 256, 2, -1, 0)),
    # the column kernels' grid-stride loop: a second trip of the 2048 x 256 grid (and more workgroups than the slot slab holds)
    ("524588x2-stride", 524588, 2, True, (0, 32, 2048, -1, 0)),
    # slot polling (hals_poll<NQ> per polling wave of 256 slots), the last workgroup holding one live row
    ("poll-kp128-129wg", _slots(129), 65, True, (1, 128, 129, 2, 0)),
] + [("poll-%dwg" % nwg, _slots(nwg), 3, True, (1, 32, nwg, 2, 0)) for nwg in (64, 65, 128, 129, 256, 257, 330, 400)]
HALS_CAPS = (512, 1024)                                           # resident workgroups of the KP = 32 sweep the proofs cover (an MI355X holds 512)
HALS_POLL_K = 3                                                   # the rank of the two cases at nwg = cap and cap + 1 (read from the plan)
HALS_W_F64 = [(300, 7), (1000, 33), (513, 128)]
HALS_W_F64_B = HALS_W_F64[:2]                                     # eps = 2^-23 in float64: the derived bound W_rel grows like 1.4^k and means nothing at k = 128
HALS_H_CASES = ([(k, n) for k in (1, 5, 32, 33, 64) for n in (1, 255, 256, 257, 600)]          # hals_h_kernel<32>, <64>: 256 columns per workgroup
                + [(k, n) for k in (65, 100, 128) for n in (1, 63, 64, 65, 200)]                # hals_h_kernel_lds: 64 columns per workgroup
                + [(k, n) for k in (129, 192, 256) for n in (70, 300)])                         # the wide kernel
HALS_H_F64 = [(7, 200), (64, 257), (128, 65)]


# ---------------------------------------------------------------------------------------------------------- sparse (CSR) blocks
# Row lengths on both sides of every structural boundary of csrc/dnmf_csr.h: the lane-group counts NG = 256 / KPAD = 16, 8, 4, 2, 1,
# the 64 (col, val) pairs a wave reads per step, and the segment length 1024 of a long row (one, two and three segments, a ragged
# fourth).  27 rows (not a multiple of a workgroup's 4 waves), an empty row right after the longest one, a short last row.
LENS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 0, 2]
LENS_N = 3100


def sparse_pattern(lengths, n, seed=0, empty_cols=0):
    """A boolean len(lengths) x n mask: row r holds exactly lengths[r] stored positions, at random columns; `empty_cols` random
    columns hold none (rows of the transposed image without a stored entry)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.min(initial=0) >= 0 and lengths.max(initial=0) <= n - empty_cols, "a row cannot hold that many entries"
    rs = np.random.RandomState(seed + 7 * len(lengths) + n)
    score = rs.rand(len(lengths), n)
    score[:, rs.choice(n, size=empty_cols, replace=False)] = 2.0               # ranked last in every row
    mask = score.argsort(1).argsort(1) < lengths[:, None]
    assert np.array_equal(mask.sum(1), lengths) and (mask.sum(0) == 0).sum() >= empty_cols
    return mask


def lens_pattern(seed=0):
    """the standard pattern: LENS x LENS_N with two empty columns"""
    return sparse_pattern(LENS, LENS_N, seed, empty_cols=2)


def sparse_exact(A, mask, W, H, kl=False):
    """float64 answers of every pass over a block whose stored positions are `mask` (A is zero elsewhere), D = W H:
    aht = A H^T, wta = W^T A; Frobenius pairs (aht, P(D) H^T), (wta, W^T P(D)); resid = ||A - D||^2, resid_masked = sum over the
    mask of (a - d)^2.  kl=True: U = P(A / D) (the generators make D a power of two >= 2 there: eps is absorbed), uht = U H^T,
    wtu = W^T U, and the KL denominators P(1) H^T (stored-position sums of H rows), W^T P(1) (of W columns)."""
    A64, W64, H64, M = A.astype(np.float64), W.astype(np.float64), H.astype(np.float64), mask.astype(np.float64)
    D = W64 @ H64
    PD = M * D
    out = {"aht": A64 @ H64.T, "wta": W64.T @ A64, "den_w": PD @ H64.T, "den_h": W64.T @ PD, "gram_w": W64.T @ W64,
           "resid": float(np.sum((A64 - D) ** 2)), "resid_masked": float(np.sum(M * (A64 - D) ** 2))}
    if kl:
        U = np.where(mask, A64 / np.where(mask, D, 1.0), 0.0)
        out.update(U=U, uht=U @ H64.T, wtu=W64.T @ U, klden_w=M @ H64.T, klden_h=W64.T @ M)
    return out


def sparse_products(mask, k, seed=0, stored_zeros=False):
    """A in 1..7 on the mask (with `stored_zeros` a few observed positions hold 0: `keep_zeros` / missing='unstored'), W and H in
    1..3 with some zero rows of W / columns of H.  Integers below 2^24, exact in fp32 in any order: A H^T, W^T A, W^T W, every
    <W_r, H_c> (<= 9 k), and the masked pairs' denominators P(W H) H^T, W^T P(W H).  Integers below 2^53, exact in float64: the
    stored-entry sum of squares, <W^T W, H H^T>, the cross term sum v d, sum over the mask of (a - d)^2."""
    m, n = mask.shape
    rs = np.random.RandomState(seed + 1009 * m + 17 * n + k)
    A = np.where(mask, rs.randint(1, 8, size=(m, n)), 0).astype(np.float32)
    if stored_zeros:
        r, c = np.nonzero(mask)
        z = rs.choice(r.size, size=max(3, r.size // 50), replace=False)
        A[r[z], c[z]] = 0
    W = rs.randint(1, 4, size=(m, k)).astype(np.float32)
    H = rs.randint(1, 4, size=(k, n)).astype(np.float32)
    W[rs.rand(m) < 0.05] = 0
    W[rs.randint(m)] = 0                                        # (a small block has a zero row / column too)
    H[:, rs.rand(n) < 0.05] = 0
    H[:, rs.randint(n)] = 0
    ref = sparse_exact(A, mask, W, H)
    W64, H64, A64 = W.astype(np.float64), H.astype(np.float64), A.astype(np.float64)
    for what in ("aht", "wta", "den_w", "den_h", "gram_w"):
        _bound(ref[what], 1.0, np.float32, what)
    _bound(H64 @ H64.T, 1.0, np.float32, "H H^T")
    _bound(9.0 * k, 1.0, np.float32, "<W_r, H_c>")
    cross = float(np.sum(A64 * (W64 @ H64)))
    for tot, what in ((np.sum(A64 * A64), "sum a^2"), (np.sum(ref["gram_w"] * (H64 @ H64.T)), "<W^T W, H H^T>"), (2.0 * cross, "2 sum a d"),
                      (np.sum(A64 * A64) + 2.0 * cross, "sum |a (a - 2 d)|"), (ref["resid_masked"], "sum (a - d)^2")):
        _bound(tot, 1.0, np.float64, what)
    return A, W, H


def sparse_kl(mask, k, seed=0, stored_zeros=False, qmax=3):
    """The structure of `kl` on a stored pattern: W one-hot per row with 2^(0..2), H = 2^(1..qmax), A in 1..7 on the mask (a few
    observed zeros with `stored_zeros`).  <W_r, H_c> is a power of two >= 2 (one non-zero product, so the dot is exact whichever
    side is the lane-dense one; eps is absorbed) and val / (d + eps) is exact; U H^T and W^T U are sums of multiples of
    2^-(2 + qmax); the stored-position sums of H rows and of W columns are integers."""
    m, n = mask.shape
    rs = np.random.RandomState(seed + 13 * m + 5 * n + 3 * k)
    A = np.where(mask, rs.randint(1, 8, size=(m, n)), 0).astype(np.float32)
    if stored_zeros:
        r, c = np.nonzero(mask)
        z = rs.choice(r.size, size=max(3, r.size // 50), replace=False)
        A[r[z], c[z]] = 0
    W = np.zeros((m, k), dtype=np.float32)
    W[np.arange(m), rs.randint(0, k, size=m)] = 2.0 ** rs.randint(0, 3, size=m)
    H = (2.0 ** rs.randint(1, qmax + 1, size=(k, n))).astype(np.float32)
    WH = W.astype(np.float64) @ H.astype(np.float64)
    assert np.all(WH >= 2) and np.array_equal(np.log2(WH), np.round(np.log2(WH)))
    ref = sparse_exact(A, mask, W, H, kl=True)
    unit = 2.0 ** -(2 + qmax)
    _bound(ref["uht"], unit, np.float32, "U H^T")
    _bound(ref["wtu"], unit, np.float32, "W^T U")
    _bound(ref["klden_w"], 1.0, np.float32, "stored-position sums of H rows")
    _bound(ref["klden_h"], 1.0, np.float32, "stored-position sums of W columns")
    return A, W, H


def transposed(A, mask, W, H):
    """the same problem seen from A^T: (A^T, mask^T) with the factor roles swapped to (H^T, W^T)"""
    return tuple(np.ascontiguousarray(x) for x in (A.T, mask.T, H.T, W.T))


# ---------------------------------------------------------------------------------------------------------- the BCD projected-gradient step
# out = max(0, Xm - (S - P) / L), S = Xm G on the W side (Xm, P, out [R x k]) and G Xm on the H side ([k x R]); csrc/dnmf_bcd.h.  Proofs:
# tests/test_exact_cpu.py; the kernels: tests/test_gpu_exact_bcd.py.
BCD_L = 64.0                                                      # the power-of-two step bound of the exact family
BCD_PG_PROOF = [(131, 1), (131, 17), (203, 33), (16500, 3), (520, 256), (300, 100)]      # (R, k) proved in every order, both sides
BCD_PG_R = (1, 63, 64, 65, 131)                                   # rows of a workgroup: 64 (BCD_ROWS)
BCD_PG_K = (1, 2, 15, 16, 17, 32, 33, 63, 64, 65, 100, 128, 129, 255, 256)
BCD_COLSUM = [(19137, 17), (40001, 4)]                            # 300 and 626 workgroup partials: two and three trips of bcd_colsum_kernel


def bcd_pg_problem(R, k, seed=0, L=BCD_L, side="w", shift=True):
    """Operands of one projected-gradient step whose result is known exactly.  Xm holds integers 0..3 and G integers 0..2 (not
    symmetric for k > 1, G[0][0] >= 1), so every term of S is a non-negative integer and S <= 6 k <= 1536: exact in float32 in any
    order, fused or not.  P = max(0, S + u), u an integer in [-200, 200]: gr = S - P is an integer with |gr| <= 200 (the elements `shift`
    forces below zero: up to 6 ceil(L), and they end at 0).

    L = 2^p (the default 2^6): gr / L is a multiple of 1 / L with few bits, y = Xm - gr / L <= 3 + 200 / 64 = 6.125 is exact, and so
    is the clamp -- the float32 result IS the float64 one (`expected`, compared with assert_ulp(..., 0)).  The column sums (W side):
    a workgroup's partial adds 64 values <= 6.125 that are multiples of 2^-6, at most 64 * 6.125 * 2^6 < 2^15 units: exact in float32
    in any butterfly order; the float64 sum of the partials is exact (below 2^53 units); the one rounding left is the final
    conversion, so s == float32(exact sum) (`s`).
    L = None: L = float32(||G||_F), what a fit would hold.  S and gr are exact as before; the quotient, the subtraction and the clamp
    are one IEEE float32 operation each, so the result must equal the numpy float32 evaluation bit for bit (`expected` is that
    evaluation, held in float64); s depends on the summation order here and keeps a relative bound.

    shift: the random design alone clamps 11-26 % of the elements and none at k = 1, so every seventh element (in storage order) is
    forced below zero -- P = S - ceil(L) (Xm + c), c in 1..3: y <= -c -- and every seventh is an exact zero: P = S - L Xm where L is a
    power of two (y = Xm - Xm), and Xm = 0, P = S elsewhere (y = 0 - 0 / L).  P is negative at some of those.  The shares of clamped,
    exactly-zero and positive elements are in `shares`; callers assert them.
    Returns a dict: Xm, P, G (float32), L (a float that is a float32), expected (float64), s (float32 column sums, W side), shares."""
    assert side in ("w", "h")
    rs = np.random.RandomState(seed + 7919 * R + 31 * k + (side == "h"))
    shape = (R, k) if side == "w" else (k, R)
    Xm = rs.randint(0, 4, size=shape).astype(np.float64)
    G = rs.randint(0, 3, size=(k, k)).astype(np.float64)
    G[0, 0] = max(G[0, 0], 1.0)
    if k > 1 and np.array_equal(G, G.T):
        G[0, 1], G[1, 0] = 2.0, 0.0
    pow2 = L is not None
    Lf = np.float32(L if pow2 else np.sqrt((G * G).sum()))
    if pow2:
        assert np.frexp(Lf)[0] == 0.5 and Lf >= 1, "L must be a power of two >= 1 (or None)"
    flat = np.arange(Xm.size).reshape(shape)
    forced_neg, forced_zero = (flat % 7 == 2) & shift, (flat % 7 == 5) & shift
    if R * k < 7 and shift:                                      # (too few elements for all three kinds: keep what fits, in this order)
        forced_neg, forced_zero = flat == 1, flat == 2
    if not pow2:
        Xm[forced_zero] = 0.0
    S = Xm @ G if side == "w" else G @ Xm
    _bound(S, 1.0, np.float32, "Xm G")
    P = np.maximum(0.0, np.rint(S + rs.randint(-200, 201, size=shape)))
    P[forced_neg] = (S - np.ceil(float(Lf)) * (Xm + rs.randint(1, 4, size=shape)))[forced_neg]
    P[forced_zero] = (S - float(Lf) * Xm)[forced_zero] if pow2 else S[forced_zero]
    gr = S - P
    assert np.abs(P).max() < 2 ** 22 and np.abs(gr).max() < 2 ** 22
    if pow2:
        y = Xm - gr / float(Lf)
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y) and (Lf < 64 or y.max() <= 6.125)
        assert np.array_equal(y * float(Lf), np.rint(y * float(Lf))), "y is not a multiple of 1 / L"
        _bound(64 * max(y.max(), 0.0), 1.0 / float(Lf), np.float32, "a workgroup's column-sum partial")
    else:
        y = (Xm.astype(np.float32) - gr.astype(np.float32) / Lf).astype(np.float64)
    assert (y[forced_neg] < 0).all() and (y[forced_zero] == 0).all()
    out = np.where(y < 0, 0.0, y)
    shares = {"clamped": float((y < 0).mean()), "zero": float((y == 0).mean()), "positive": float((y > 0).mean())}
    s = out.sum(0).astype(np.float32) if side == "w" else None
    return {"Xm": Xm.astype(np.float32), "P": P.astype(np.float32), "G": G.astype(np.float32), "L": float(Lf), "expected": out, "s": s,
            "shares": shares, "pow2": pow2}


# ---------------------------------------------------------------------------------------------------------- exact operands on a grid
# One update() of nmf_algorithms_1D / _2D per kind on more than one rank (tests/_mp.py run_exact_cases; tests/test_exact_grid_cpu.py with
# the checker back end, tests/test_gpu_exact_grid.py with the HIP kernels).  GRID_EXACT: (id, grid, shapes, modes, long tier) -- every
# kind at every shape in every mode, the overlapped H phase for the MU/Frobenius kinds only.  The branch of dist_nmf.py each shape is
# named after is asserted by tests/test_exact_cpu.py::test_grid_shapes_reach_their_branches.
GRID_KINDS = ("fro", "fro_bf16", "kl_wfixed", "kl_w", "kl_fixed", "hals", "hals_bf16", "hals_wfixed")
GRID_OVERLAP_KINDS = ("fro", "fro_bf16")
_ROW = ("choreography", "overlap4", "native-hosted", "overlap4-native", "direct")
_COL = ("choreography", "native-hosted", "direct")
_2D = ("choreography", "native-hosted")
GRID_EXACT = [
    ("3x1", (3, 1), [(301, 262, 5), (301, 262, 17)], _ROW, False),          # row blocks 101, 100, 100; chunks of 128, 128, 6 columns
    ("1x3", (1, 3), [(301, 262, 5), (301, 262, 17)], _COL, False),          # column blocks 88, 87, 87
    ("2x2-blockable", (2, 2), [(512, 256, 16)], _2D, False),                # h = 64, 64: the [p_r][k][n_h] stack as it is; equal w
    ("2x2-sliceable", (2, 2), [(515, 272, 33)], _2D, False),                # h = 68, 68: sliced products, no stack; ragged w
    ("2x2-ragged", (2, 2), [(515, 263, 33)], _2D, False),                   # h = 66, 66 | 66, 65: the transposing route
    ("2x3", (2, 3), [(241, 199, 33)], _2D, False),                          # ragged, three-member row groups
    ("3x2", (3, 2), [(301, 197, 5)], _2D, True),
    ("4x2", (4, 2), [(203, 259, 64)], _2D, True),                           # eight ranks
    ("4x1", (4, 1), [(1024, 520, 64)], _COL, True),                         # the default overlap settings (one packed exchange at n = 520) and direct
]
GRID_CPU_MODES = ("choreography", "overlap4")                               # the modes that need no library


def grid_exact_cases(entry, cpu=False, kinds=GRID_KINDS):
    """[(kind, shape, modes), ...] of an entry of GRID_EXACT; cpu: the modes of the checker back end only"""
    _, grid, shapes, modes, _ = entry
    out = []
    for shape in shapes:
        for kind in kinds:
            ms = tuple(mo for mo in modes if (kind in GRID_OVERLAP_KINDS or not mo.startswith("overlap4")) and (not cpu or mo in GRID_CPU_MODES))
            out.append((kind, shape, ms))
    return out


# ---------------------------------------------------------------------------------------------------------- bf16x6: operands with pieces
# The arithmetic of csrc/dnmf_split.h as its header states it, in numpy, and operands on which it is EXACT although second and third
# pieces are not zero (tests/test_exact_cpu.py proves the families and that a model with a term deleted, two pieces swapped or a piece
# plane zeroed differs in every 32 x 32 output tile; tests/test_gpu_exact_split.py holds the six kernels to them).  The integer
# families above have at most 3 significant bits: x2 = x3 = 0, and five of the six piece products are multiplied by zero.
#   cut3(x): x1 = rne_bf16(x), x2 = rne_bf16(x - x1), x3 = rne_bf16(x - x1 - x2)
#   fp32 A:        x y ~ x1 y1 + (x1 y2 + x2 y1) + (x1 y3 + x2 y2 + x3 y1)     (X6_TERMS; dropped: x2 y3, x3 y2, x3 y3)
#   bf16-stored A: x y = x y1 + x y2 + x y3                                    (X3_TERMS)
# Values: one piece {1, 2}; two pieces 1 + i 2^-8, i odd (x2 = +-2^-8); three pieces 1 + a 2^-17 with a residual of nine bits
# after x1 (a = 257: x2 = 2^-9, x3 = 2^-17; a = 767: x1 = 1 + 2^-7, x2 = -2^-9, x3 = -2^-17), all positive, pieces of both signs.  A multiplied pair is two x two pieces, three x
# one or one x three, so the dropped terms are zero and every piece product is a multiple of 2^-17 (2^-8 2^-8, 2^-17 1); a contraction
# line may hold 2^24 of those units = 128 in magnitudes, i.e. about 60 products of values near 1 and 2: A is sparse.
X6_TERMS = ((1, 1), (1, 2), (2, 1), (1, 3), (2, 2), (3, 1))
X6_DROPPED = ((2, 3), (3, 2), (3, 3))
X3_TERMS = ((1, 1), (1, 2), (1, 3))                              # (piece of A, piece of the fp32 factor)
X6_UNIT = 2.0 ** -17


def bf16_rne(x):
    """float32 -> the nearest bfloat16, ties to even, as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(np.float32)


def cut3(x, check=True):
    """the three bf16 pieces of float32 values (float32 arrays; both subtractions are exact in fp32, asserted through the sum)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x1 = bf16_rne(x)
    r1 = x - x1
    x2 = bf16_rne(r1)
    r2 = r1 - x2
    x3 = bf16_rne(r2)
    assert not check or np.array_equal(x1.astype(np.float64) + x2 + x3, x.astype(np.float64)), "a value needs more than three bf16 pieces"
    return [x1, x2, x3]


def npieces(x):
    """how many of the three pieces are nonzero (1 for zero itself)"""
    p = cut3(x)
    return 1 + (p[1] != 0) + (p[2] != 0)


X6_P1 = np.array([1.0, 2.0])
X6_P2 = np.array([1 + i * 2.0 ** -8 for i in (1, 3, 5, 7)])
X6_P3 = np.array([1 + a * 2.0 ** -17 for a in (257, 259, 261, 763, 765, 767)])      # (x2, x3) 2^17 = (256, 1), (260, -1), ..., (-256, -1)
X6_POOLS = (X6_P1, X6_P2, X6_P3)
assert np.all(npieces(X6_P3) == 3) and np.all(npieces(X6_P2) == 2) and np.all(npieces(X6_P1) == 1)


def _mm(X, Y, side):
    """float64 X Y^T ('aht': X m x n, Y k x n) or Y^T X ('wta': X m x n, Y m x k) of float32 operands (a large X: as a sparse matrix;
    on the operands here every float64 sum is exact, so the order does not matter)"""
    Y = Y.astype(np.float64)
    if X.size > 1 << 22:
        import scipy.sparse as sp
        Xs = sp.csr_matrix(X).astype(np.float64)
        return np.asarray(Xs @ Y.T) if side == "aht" else np.ascontiguousarray(np.asarray(Xs.T @ Y).T)
    X = X.astype(np.float64)
    return X @ Y.T if side == "aht" else Y.T @ X


def x6_pieces_products(A, F, side):
    """T[(a, b)] = (piece a of A)(piece b of the factor) for all nine pairs, float64"""
    Ap, Fp = cut3(A), cut3(F)
    return {(a, b): _mm(Ap[a - 1], Fp[b - 1], side) for a in (1, 2, 3) for b in (1, 2, 3)}


def x6_model(A, F, side, terms=X6_TERMS, a_planes=(1, 2, 3), f_planes=(1, 2, 3), T=None):
    """the product as the kernels form it: sum over `terms` (a, b) of (plane a of A) (plane b of the factor), in float64 (exact on
    the families here).  side 'aht': A F^T with F = H (k x n); 'wta': F^T A with F = W (m x k).  a_planes / f_planes: which cut lies
    in which plane of the operand (0: that plane is zero), to model swapped or lost planes.  T: x6_pieces_products, if at hand."""
    T = x6_pieces_products(A, F, side) if T is None else T
    out = np.zeros_like(T[(1, 1)])
    for a, b in terms:
        if a_planes[a - 1] and f_planes[b - 1]:
            out = out + T[(a_planes[a - 1], f_planes[b - 1])]
    return out


def _signs_both(pieces, what, third=True):
    for s in (1, 2) if third else (1,):
        v = np.concatenate([p[s].ravel() for p in pieces])
        assert (v > 0).any() and (v < 0).any(), "%s: piece %d has one sign only" % (what, s + 1)


def pieces_product(m, n, k, side, bf16a=False, seed=0, rot=0, nnz=20):
    """A (m x n, sparse) and the factor F -- side 'aht': F = H (k x n), the product A H^T contracts over the columns of A; 'wta':
    F = W (m x k), W^T A contracts over its rows.  Contraction index i has type (i + rot) % 3:
      0  A two pieces,   F two pieces      x1 y1, x1 y2, x2 y1, x2 y2
      1  A three pieces, F one piece       x1 y1, x2 y1, x3 y1
      2  A one piece,    F three pieces    x1 y1, x1 y2, x1 y3
    (rot: with a contraction of fewer than three indices one call cannot hold every type; the callers run rot = 0, 1, 2.)
    bf16a: every A one piece (a bf16 number), F two and three pieces: the three-term path.  About `nnz` nonzeros of A per
    contraction line.  Asserted: the three dropped terms are zero for every multiplied pair, second and third pieces of both signs
    occur, every piece is a multiple of the unit that makes all piece products multiples of 2^-17, and the sum of the magnitudes of
    the piece products along every contraction line is below 2^24 of those units: exact in fp32 in any order."""
    assert side in ("aht", "wta")
    rs = np.random.RandomState(seed + 7919 * m + 31 * n + 3 * k + 101 * rot + (1 if side == "wta" else 0) + (2 if bf16a else 0))
    L = n if side == "aht" else m
    typ = (np.arange(L) + rot) % 3
    ta = np.zeros(L, dtype=int) if bf16a else np.array([1, 2, 0])[typ]                       # index into X6_POOLS
    tf = (1 + rs.randint(0, 2, size=L)) if bf16a else np.array([1, 0, 2])[typ]
    draw = lambda t: np.choose(t, [P[rs.randint(0, len(P), size=t.shape)] for P in X6_POOLS])
    F = draw(np.broadcast_to(tf[None, :], (k, n)) if side == "aht" else np.broadcast_to(tf[:, None], (m, k))).astype(np.float32)
    flat = np.unique(rs.randint(0, m * n, size=int(round(min(0.5, nnz / L) * m * n))))       # the nonzeros of A
    rows, cols = flat // n, flat % n
    line = cols if side == "aht" else rows                            # their contraction index
    vals = draw(ta[line]).astype(np.float32)
    A = np.zeros((m, n), dtype=np.float32)
    A[rows, cols] = vals
    Vp, Fp = cut3(vals), cut3(F)                                      # (the pieces of A, at its nonzeros only)
    a_on = [np.bincount(line[P != 0], minlength=L) > 0 for P in Vp]   # per contraction index
    f_on = [(P != 0).any(axis=0 if side == "aht" else 1) for P in Fp]
    for a, b in X6_DROPPED:
        assert not (a_on[a - 1] & f_on[b - 1]).any(), "a multiplied pair has a nonzero dropped term x%d y%d" % (a, b)
    if bf16a:
        assert is_bf16(vals).all()
    if L >= 3:                                                        # (a shorter contraction does not hold every type)
        _signs_both([Fp] if bf16a else [Vp, Fp], "pieces_product")
    ua = np.array([1.0, 2.0 ** -8, 2.0 ** -17])
    for q in Vp:                                                      # every piece a multiple of the unit of its type
        v = q / ua[ta[line]]
        assert np.array_equal(v, np.rint(v)), "a piece of A is no multiple of its unit"
    for q in Fp:
        v = q / (ua[tf][None, :] if side == "aht" else ua[tf][:, None])
        assert np.array_equal(v, np.rint(v)), "a piece of the factor is no multiple of its unit"
    import scipy.sparse as sp
    Am = sp.csr_matrix((sum(np.abs(P.astype(np.float64)) for P in Vp), (rows, cols)), shape=(m, n))
    Fm = sum(np.abs(P.astype(np.float64)) for P in Fp)
    mag = Am @ Fm.T if side == "aht" else Am.T @ Fm                   # >= the magnitudes of the kept terms
    _bound(mag, X6_UNIT, np.float32, "bf16x6 piece products along a contraction line (%s, %d x %d, k = %d)" % (side, m, n, k))
    return A, F


def _pow2(x):
    with np.errstate(divide="ignore"):
        return np.array_equal(np.log2(x), np.round(np.log2(x)))


KLX_KINDS = ("w", "h", "wh")


def kl_pieces(m, n, k, kind, seed=0, rot=0, nnz=20):
    """KL operands for the bf16x6 kernels (csrc/dnmf_split_kl.h): S = W H is a power of two >= 4 -- so eps is absorbed and U = A / (S + eps)
    is exact -- but a sum in which second and third pieces take part and cancel.  A row of W is nonzero in a window of 2 ('w', 'h') or
    4 ('wh') consecutive rank columns that starts anywhere (m < 32: in up to 32 adjacent windows, so that few rows still reach every
    column; the magnitudes of S keep an 18-bit value to 64 columns):
      'w'   W[r][j] = 2^p (1 +- d) alternating along the window, H[j][c] = 2^q for every j: S = 2^(p + q) times the width.  d by row type
            (r + rot) % 3: 0: 1 + d has three pieces, U of that row one piece; 1: d an odd multiple of 2^-8 of either sign (two
            pieces and one), U two pieces; 2: d = 0, U three pieces.  W^T U sees every kept term, S = W H the terms x1 y1, x2 y1, x3 y1.
      'h'   the mirror image: W[r][j] = 2^p in the window, H[j][c] = 2^q (1 + (-1)^j d_c), d and the pieces of U by COLUMN type:
            U H^T sees every kept term, S the terms x1 y1, x1 y2, x1 y3.
      'wh'  W[r][j] = 2^p (1 + (-1)^j a_r), H[j][c] = 2^q (1 + s_j b_c) with s = + + - - along j, a and b odd multiples of 2^-8 of
            either sign: over four consecutive j the sums of (-1)^j, s_j and (-1)^j s_j vanish, S = 2^(p + q + 2) with x2 y2 among
            its terms; U one and two pieces.
    k below the window (k = 1; k < 4 for 'wh'): W and H are powers of two, U one to three pieces.  U = A / S is sparse (about `nnz` per
    row and column).  Asserted: S, the dropped terms of all three products, both signs, and the magnitudes of the piece products of
    S (per line, in units of 2^(p + q - 17)), U H^T (unit 2^-16: q >= 1) and W^T U (unit 2^-17) below 2^24 units.
    Returns A, W, H (float32), U (float64)."""
    assert kind in KLX_KINDS
    rs = np.random.RandomState(seed + 4099 * m + 37 * n + 5 * k + 11 * rot + KLX_KINDS.index(kind))
    gs = 4 if kind == "wh" else 2
    p, q = rs.randint(0, 2, size=m), rs.randint(1, 3, size=n)
    tr, tc = (np.arange(m) + rot) % 3, (np.arange(n) + rot) % 3
    d3, d2 = X6_P3 - 1.0, X6_P2 - 1.0
    sgn = lambda size: rs.choice([-1.0, 1.0], size=size)
    j = np.arange(k)
    alt = (-1.0) ** j
    W = np.zeros((m, k))
    H = np.ones((k, 1)) * 2.0 ** q[None, :]
    upool = np.zeros((m, n), dtype=int)                               # index into X6_POOLS of U's entries
    if k < gs:
        W[:, 0] = 2.0 ** p
        upool[:] = (tr[:, None] + tc[None, :]) % 3
        width = 1
    else:
        nw = 1
        while m < 32 and nw < 32 and 2 * nw * gs <= k:
            nw *= 2
        width = nw * gs
        o = rs.randint(0, k - width + 1, size=m)
        inwin = (j[None, :] >= o[:, None]) & (j[None, :] < o[:, None] + width)
        if kind == "w":
            d = np.choose(tr, [d3[rs.randint(0, len(d3), size=m)], sgn(m) * d2[rs.randint(0, len(d2), size=m)], np.zeros(m)])
            W = np.where(inwin, 2.0 ** p[:, None] * (1 + alt[None, :] * d[:, None]), 0.0)
            upool[:] = np.array([0, 1, 2])[tr][:, None]
        elif kind == "h":
            d = np.choose(tc, [d3[rs.randint(0, len(d3), size=n)], sgn(n) * d2[rs.randint(0, len(d2), size=n)], np.zeros(n)])
            H = 2.0 ** q[None, :] * (1 + alt[:, None] * d[None, :])
            W = np.where(inwin, 2.0 ** p[:, None] * np.ones((1, k)), 0.0)
            upool[:] = np.array([0, 1, 2])[tc][None, :]
        else:
            a = sgn(m) * d2[rs.randint(0, len(d2), size=m)]
            b = sgn(n) * d2[rs.randint(0, len(d2), size=n)]
            s4 = np.array([1.0, 1.0, -1.0, -1.0])[j % 4]
            W = np.where(inwin, 2.0 ** p[:, None] * (1 + alt[None, :] * a[:, None]), 0.0)
            H = 2.0 ** q[None, :] * (1 + s4[:, None] * b[None, :])
            upool[:] = rs.randint(0, 2, size=(m, n))
    S = W @ H
    assert np.array_equal(S, width * 2.0 ** (p[:, None] + q[None, :])) and S.min() >= 2 and _pow2(S), "W H is not the power of two of the design"
    Uv = np.choose(upool, [P[rs.randint(0, len(P), size=(m, n))] for P in X6_POOLS])
    U = np.where(rs.rand(m, n) < min(0.5, nnz / n, nnz / m), Uv, 0.0)
    A = U * S
    f32 = lambda x: x.astype(np.float32)
    for x in (A, W, H, U):
        assert np.array_equal(f32(x).astype(np.float64), x)
    Wp, Hp, Up = cut3(W), cut3(H), cut3(U)
    nz = lambda P: P != 0
    for a, b in X6_DROPPED:
        # S: W[r][j] meets H[j][c] for every r, c with W[r][j] != 0; U H^T: U[r][c] meets H[j][c] for every j; W^T U: W[r][j] meets U[r][c]
        assert not (nz(Wp[a - 1]).any(0) & nz(Hp[b - 1]).any(1)).any(), "S = W H has a nonzero dropped term"
        assert not (nz(Up[a - 1]).any(0) & nz(Hp[b - 1]).any(0)).any(), "U H^T has a nonzero dropped term"
        assert not (nz(Up[a - 1]).any(1) & nz(Wp[b - 1]).any(1)).any(), "W^T U has a nonzero dropped term"
    if k >= gs and min(m, n) >= 3:
        _signs_both([Wp, Up] if kind == "w" else [Hp, Up] if kind == "h" else [Wp, Hp, Up], "kl_pieces", third=kind != "wh")
    absum = lambda P: sum(np.abs(x.astype(np.float64)) for x in P)
    _bound(absum(Up) @ absum(Hp).T, 2.0 ** -16, np.float32, "U H^T piece products along a row")
    _bound(absum(Wp).T @ absum(Up), 2.0 ** -17, np.float32, "W^T U piece products along a column")
    _bound((absum(Wp) / 2.0 ** p[:, None]) @ (absum(Hp) / 2.0 ** q[None, :]), 2.0 ** (-16 if kind == "wh" else -17), np.float32, "W H piece products")
    return f32(A), f32(W), f32(H), U


def klx_model(A, W, H, which, s_terms=X6_TERMS, p_terms=X6_TERMS, eps=float(np.finfo(np.float32).eps)):
    """the KL products as the kernels form them: S = sum over s_terms (a, b) of (piece a of W)(piece b of H); U = A / (S + eps) in fp32;
    `which` 'uht': sum over p_terms (a, b) of (piece a of U)(piece b of H)^T, 'wtu': (piece b of W)^T (piece a of U).  float64 sums."""
    Wp, Hp = ([x.astype(np.float64) for x in cut3(X)] for X in (W, H))
    S = sum(Wp[a - 1] @ Hp[b - 1] for a, b in s_terms)
    with np.errstate(divide="ignore", invalid="ignore"):
        U = (A.astype(np.float32) / (S.astype(np.float32) + np.float32(eps))).astype(np.float32)
    U = np.where(np.isfinite(U), U, 0).astype(np.float32)
    Up = [x.astype(np.float64) for x in cut3(U, check=False)]          # (with a term of S deleted U is no value of the design)
    if which == "uht":
        return sum(Up[a - 1] @ Hp[b - 1].T for a, b in p_terms)
    return sum(Wp[b - 1].T @ Up[a - 1] for a, b in p_terms)


def x6_rots(L):
    """the rotations of the pair types a caller of `pieces_product` runs: all three where the contraction is shorter than three"""
    return (0, 1, 2) if L < 3 else (0,)


def klx_rots(m):
    """... of `kl_pieces`: kind 'w' types the ROWS, and a last 32-row tile of one or two rows holds one or two types per call
    (and fewer than 32 rows leave some tile of W^T U without an entry of the type a term needs: three independent draws)"""
    return (0, 1, 2) if m % 32 in (1, 2) or m < 32 else (0,)


def tiles_differ(X, Y, tile=32):
    """per 32 x 32 tile of two equal-shaped matrices: does any element differ (a boolean matrix over the tiles, ragged last tiles kept)"""
    D = ~(np.asarray(X) == np.asarray(Y))
    r, c = -(-D.shape[0] // tile), -(-D.shape[1] // tile)
    P = np.zeros((r * tile, c * tile), dtype=bool)
    P[:D.shape[0], :D.shape[1]] = D
    return P.reshape(r, tile, c, tile).any(axis=(1, 3))


# The shapes of tests/test_gpu_exact_split.py, named after the boundary they sit on, with the plan dnmf_bf16x6_plan must report
# (tests/test_bf16x6_plan.py, without a GPU): (id, m, n, k, lda, factors aligned, (KT, tiles in flight, tnx chunks, rows per chunk)).
# lda = 0: the pitch Poisoned gives an aligned view (n + 4 for fp32, n + 8 for bf16).  tnx: cdiv(m, 256) chunks of cdiv(m, chunks) rows
# rounded up to 64.
X6_F32 = [
    ("k33-kmin-m1-edge-only-n128-one-trip", 1, 128, 33, 0, True, (2, 4, 1, 64)),
    ("k40-below-kp-m31-edge-only-n256", 31, 256, 40, 0, True, (2, 4, 1, 64)),
    ("k63-m100-edge-only-n384-odd-multiple-unaligned", 100, 384, 63, 0, False, (2, 4, 1, 128)),
    ("k64-nset4-m128-interior-only-n128-lda2n", 128, 128, 64, 256, True, (2, 4, 1, 128)),
    ("k65-kt4-m129-both-n256-unaligned", 129, 256, 65, 0, False, (4, 2, 1, 192)),
    ("k64-nset4-m257-both-two-chunks-n1152-rotation", 257, 1152, 64, 0, True, (2, 4, 2, 192)),
    ("k128-m640-three-chunks-n384-lda4n", 640, 384, 128, 1536, True, (4, 2, 3, 256)),
    ("k97-kt4-m1000-ragged-chunk-n1152-rotation-unaligned", 1000, 1152, 97, 0, False, (4, 2, 4, 256)),
    ("k40-m129-n128-lda4n-unaligned", 129, 128, 40, 512, False, (2, 4, 1, 192)),
]
X6_BF16 = [
    ("k17-kmin-kt1-m1-n128-two-tiles", 1, 128, 17, 0, True, (1, 2, 1, 64)),
    ("k20-kt1-m100-n256-unaligned", 100, 256, 20, 0, False, (1, 2, 1, 128)),
    ("k32-kt1-m129-both-n384", 129, 384, 32, 0, True, (1, 2, 1, 192)),
    ("k48-kt2-m257-n1152-rotation-unaligned", 257, 1152, 48, 0, False, (2, 2, 2, 192)),
    ("k100-kt4-m1000-ragged-chunk-n128", 1000, 128, 100, 0, True, (4, 2, 4, 256)),
    ("k64-kt2-m640-n256-lda4n", 640, 256, 64, 1024, True, (2, 2, 3, 256)),
]
X6_FALLBACK = [("k32-f32", 129, 256, 32, False), ("k16-bf16", 129, 256, 16, True)]       # (id, m, n, k, bf16-stored A): the fp32 route
# KL: (id, m, n, k, lda, factors aligned, (KT, wtux chunks, 32-row blocks per chunk, uhtx splits, columns per split))
X6_KL = [
    ("k1-n128-one-split-m100", 100, 128, 1, 0, True, (1, 1, 4, 1, 128)),
    ("k5-n128-m640-five-chunks-one-live-wave-unaligned", 640, 128, 5, 0, False, (1, 5, 4, 1, 128)),
    ("k32-n512-two-splits-m129", 129, 512, 32, 0, True, (1, 1, 5, 2, 256)),
    ("k33-kt2-n512-m257-lda2n-unaligned", 257, 512, 33, 1024, False, (2, 2, 5, 2, 256)),
    ("k64-n896-three-splits-m1000", 1000, 896, 64, 0, True, (2, 8, 4, 3, 320)),
    ("k128-kt4-n896-m31-unaligned", 31, 896, 128, 0, False, (4, 1, 1, 3, 320)),
    ("k64-m1-n128", 1, 128, 64, 0, True, (2, 1, 1, 1, 128)),
]
# A of 256 MiB: the instantiations that stream A past the caches (id, m, n, k, bf16-stored A, plan)
X6_STREAMED = [("f32-32768x2048-k40", 32768, 2048, 40, False, (2, 4, 128, 256)), ("bf16-65536x2048-k40", 65536, 2048, 40, True, (2, 2, 128, 512))]


# ---------------------------------------------------------------------------------------------------------- float64 shape table
# The shapes of tests/test_gpu_exact_f64.py, each with the kernel variant it is there for, stated here and not asked of the library: tests/test_f64_plan.py
# asserts on the CPU, through dnmf_f64_plan, that every shape reaches its variant and that the table covers every instantiation the
# dispatch of csrc/dnmf_f64.hip can launch and both sides of its host branches; the GPU test asserts it again before it launches.
# Pitches beyond the 2 GiB descriptor window (buf_ok false: the `rt >>= 1` fallbacks and the refusals) need operands of hundreds of GB
# and are not covered.
# f64_nt_kernel<RT, NT, VEC> (aht; gram_hht is the same entry point at m = k): (m, n, k, RT, NT, VEC, splits, V)
F64_AHT = (
    [(40, n, 9, 1, 1, n % 4 == 0, 1, 0) for n in (70, 100, 130)]                 # NT = 1 is a ring of three: 3, 4, 5 trips of 32 columns
    + [(40, n, k, 1, nt, n % 4 == 0, 1, 0) for k, nt in ((9, 1), (20, 2), (40, 4), (100, 8)) for n in (70, 72) if (k, n) != (9, 70)]
    + [(600, 70, 20, 1, 2, False, 1, 0)]                                          # ten workgroups, the last wave ragged
    + [(8200, n, k, 2, nt, n % 4 == 0, 1, 0) for k, nt in ((9, 1), (20, 2), (40, 4), (100, 8)) for n in (70, 72)]
    + [(16400, n, k, 4, nt, n % 4 == 0, 1, 0) for k, nt in ((9, 1), (20, 2), (40, 4)) for n in (70, 72)]      # 16400 % 64 = 16: a ragged last wave
    + [(600, 1100, 9, 1, 1, True, 2, 1), (600, 1100, 20, 1, 2, True, 2, 2), (600, 1100, 40, 1, 4, True, 2, 2),      # splits of 560 + 540 columns
       (600, 1100, 100, 1, 8, True, 2, 2), (700, 1502, 33, 1, 4, False, 2, 1)])
# f64_tn_kernel<NT, VEC> (wta; gram_wtw is the same entry point at n = k): (m, n, k, NT, CT, VEC, chunks, rows per chunk, V).
# m = 40: one chunk; 130: chunks of 48 rows (the two-set ring ends on a half step); 600: ten chunks of 64, the last of 24
F64_WTA = [(m, n, k, nt, ct, vec, ch, rpc, 2 - n % 2)
           for m, ch, rpc in ((40, 1, 48), (130, 3, 48), (600, 10, 64))
           for n, k, nt, ct, vec in ((72, 9, 1, 4, True), (70, 9, 1, 4, False), (71, 9, 1, 4, False), (72, 20, 2, 4, True), (72, 21, 2, 4, False),
                                     (72, 40, 4, 4, True), (71, 40, 4, 4, False), (70, 100, 8, 2, True), (71, 100, 8, 2, False))]
# f64_kl_uht_kernel<NT, RT, VEC, FULL>: (m, n, k, NT, RT, VEC, FULL, splits, V); n = 64 / 68 / 70: mask-free / vector / generic
F64_KL_UHT = (
    [(m, n, k, nt, rt, n % 4 == 0, n == 64, 1, 0)
     for m, rt, ks in ((40, 1, ((9, 1), (20, 2), (40, 4))), (32800, 2, ((9, 1), (30, 2), (64, 4))), (65500, 4, ((9, 1), (20, 2))))
     for k, nt in ks for n in (64, 68, 70)]
    + [(1000, 2048, k, nt, 1, True, True, 4, 2 - k % 2) for k, nt in ((9, 1), (20, 2), (40, 4))]             # four whole splits of 512
    + [(700, 1500, k, nt, 1, True, False, 2, 2 - k % 2) for k, nt in ((9, 1), (20, 2), (40, 4))]             # 768 + 732 columns
    + [(700, 1502, 9, 1, 1, False, False, 2, 1)])
# RT > 1 together with a column split, A of 0.27 and 0.5 GB built on the device: (m, n, k, NT, RT, splits, V)
F64_KL_UHT_BIG = [(32768, 1024, 9, 1, 2, 2, 1), (65536, 1024, 16, 1, 4, 2, 2)]
# f64_kl_wtu_kernel<NT, CT, VEC>: (m, n, k, NT, CT, VEC, chunks, V)
F64_KL_WTU = [(m, n, k, nt, ct, vec, ch, 2 - n % 2)
              for m, ch in ((40, 1), (130, 3), (600, 10))
              for n, k, nt, ct, vec in ((72, 12, 1, 4, True), (72, 9, 1, 4, False), (72, 20, 2, 4, True), (70, 20, 2, 4, False),
                                        (72, 40, 4, 2, True), (71, 40, 4, 2, False))]
# f64_nn_cols_kernel<KS, MODE, VEC>, both images: (m, n, k, KS, CT, VEC, chunks).  k > 64 is the image path of the KL products.
# 16400 x 132 has more than 2^21 elements: the grid-stride loops of the sums and of the element-wise kernel take more than one trip
F64_IMAGE = [(130, 72, 8, 4, 4, True, 3), (130, 70, 9, 4, 4, False, 3), (130, 72, 20, 8, 4, True, 3), (130, 70, 21, 8, 4, False, 3),
             (130, 72, 40, 16, 4, True, 3), (130, 71, 41, 16, 4, False, 3), (130, 72, 100, 32, 2, True, 3), (130, 71, 99, 32, 2, False, 3),
             (40, 72, 65, 32, 2, False, 1), (16400, 132, 20, 8, 4, True, 257)]
F64_IMAGE_K = [c for c in F64_IMAGE if c[2] > 64]
# f64_nn_rows_kernel<KS, NN_UPD_W> and f64_upd_h_kernel<KS>: (m, n, k, KS); k % 4 != 0, m and n ragged at 16
F64_MU = [(130, 70, 9, 4), (130, 70, 21, 8), (130, 70, 41, 16), (130, 70, 99, 32)]
# dnmf_f64_fit, itr = 1: (m, n, k, family).  The tiny kernel takes what fits 160 KiB - 64 bytes of LDS at k <= 16: 20 x 300 at k = 16 has
# m k, k n and n above 256 (every strided loop takes a second trip); 119 x 119 (88 x 89 with the quotient image of KL) is the largest such
# shape, one more row or column leaves it to the chain
F64_FIT_FRO = [(20, 300, 16, "fit_tiny"), (40, 300, 1, "fit_tiny"), (119, 119, 16, "fit_tiny"), (120, 119, 16, "fit_chain"), (130, 72, 20, "fit_chain")]
F64_FIT_KL = [(24, 260, 12, "fit_tiny"), (30, 280, 1, "fit_tiny"), (88, 89, 16, "fit_tiny"), (89, 89, 16, "fit_chain"), (130, 72, 20, "fit_chain")]
F64_FIT_STACK = (20, 300, 16)


def f64_pitch(cols, aligned):
    """the pitch of a `Poisoned` view of `cols` float64 columns"""
    return -(-cols // 4) * 4 + 4 if aligned else cols + 3


# ---------------------------------------------------------------------------------------------------------- the fp32 dense MU/Frobenius path
# The shapes of tests/test_gpu_exact_dense.py, each named after the kernel variant or loop-trip class it is there for, with the fields
# dnmf_dense_plan must report for it (tests/test_dense_plan.py asserts them, and that the table reaches every instantiation the
# selectors of csrc/dnmf.hip can return, without a GPU).  (id, op, m, n, k, aligned, bf16-stored A, plan fields).  `aligned`: the
# operands are `Poisoned` views with 16-byte aligned rows (bf16: quantum 8); otherwise an odd start and pitch.
def _nt(pf, kt, nk, mode=0, **kw):
    return dict(family="nt", fast=1, pf=pf, kt=kt, nk=nk, mode=mode, **kw)


P2_M = 128 * 257 + 4             # 257 interior row tiles and a ragged one: 258 workgroups, more than the 256 below which PF 13 is chosen
P3_M = 2 * 128 + 44              # two interior tiles and a ragged one
DENSE_NT = (
    # nt_mainloop_p2 (PF 10): nk = 1 (prologue clamps, tail only), 2 (one trip, no tail), 3 (trip + tail), 4 (even), 5 (odd), every KT
    [("p2-k%d-nk%d" % (k, nk), "aht", P2_M, 32 * nk, k, True, False, _nt(10, k // 32, nk, interior=257, eligible=257, grid_x=258))
     for k in (32, 64, 128) for nk in (1, 2, 3, 4, 5)]
    + [("p2-fused-k%d-nk%d" % (k, nk), "aht_update_w", P2_M, 32 * nk, k, True, False, _nt(10, k // 32, nk, 1, wfast=1, eligible=257))
       for k, nk in ((32, 3), (64, 4), (128, 5), (64, 1), (128, 2))]
    + [("p2-hblocks-k64-nk4", "aht_hblocks", P2_M, 128, 64, True, False, _nt(10, 2, 4, eligible=257))]
    # nt_mainloop_p3t (PF 13): nk = 1, 2 (the prologue's prefetches clamp to the last tile) and every residue nk mod 6 behind a whole trip
    + [("p3t-k%d-nk%d" % (k, nk), "aht", P3_M + 128 * (nk % 2), 32 * nk, k, True, False,
        _nt(13, k // 32, nk, interior=2 + nk % 2, eligible=2 + nk % 2)) for k in (32, 64, 128) for nk in (1, 2, 6, 7, 8, 9, 10, 11)]
    + [("p3t-fused-k%d-nk%d" % (k, nk), "aht_update_w", P3_M, 32 * nk, k, True, False, _nt(13, k // 32, nk, 1, wfast=1, eligible=2))
       for k, nk in ((32, 7), (64, 11), (128, 8))]
    + [("p3t-hblocks-k32-nk8", "aht_hblocks", P3_M, 256, 32, True, False, _nt(13, 1, 8, eligible=2))]
    # the descriptor loops' other side: W of the fused form off the vector path; an unaligned A (the generic loop, PF 1); k < KP keeps
    # the fast kernel off its interior loop
    + [("fused-w-unaligned-k32", "aht_update_w", P3_M, 96, 32, "W", False, _nt(13, 1, 3, 1, wfast=0, eligible=2)),
       ("fast-edge-k%KP-k40", "aht", P3_M, 96, 40, True, False, _nt(13, 2, 3, interior=0, eligible=0)),
       ("fast-edge-n%32-k64", "aht", P3_M, 100, 64, True, False, _nt(13, 2, 4, interior=0, eligible=0)),
       ("fast-edge-k%KP-fused-k100", "aht_update_w", P3_M, 96, 100, True, False, _nt(13, 4, 3, 1, wfast=1, interior=0, eligible=0))]
    # bf16-stored A (PF 5): 64-wide tiles, nk = 1, 2 and odd
    + [("bf16-k%d-nk%d" % (k, nk), "aht", P3_M, 64 * nk, k, True, True, _nt(5, k // 32, nk, interior=2, eligible=0))
       for k in (32, 64, 128) for nk in (1, 2, 3)]
    + [("bf16-fused-k%d-nk%d" % (k, nk), "aht_update_w", P3_M, 64 * nk, k, True, True, _nt(5, k // 32, nk, 1, wfast=1, interior=2))
       for k, nk in ((32, 2), (64, 3), (128, 1))]
    + [("bf16-edge-n%64-k32", "aht", P3_M, 96, 32, True, True, _nt(5, 1, 2, interior=0))]
    # the generic kernels (FAST = false): unaligned operands, every KT, both modes, both storage types of A
    + [("generic-%s-k%d%s" % (op, k, "-bf16" if b else ""), op, P3_M, 96, k, False, b,
        dict(family="nt", fast=0, pf=1, kt=kt, mode=int(op != "aht"), wfast=0, interior=0, eligible=0))
       for op in ("aht", "aht_update_w") for k, kt in ((20, 1), (64, 2), (128, 4)) for b in (False, True)]
    # the 16-wide kernel: its pair loop with and without the odd tile
    + [("nt16-k16-nk3", "aht", P3_M, 96, 16, True, False, dict(family="nt16", nk=3)),
       ("nt16-fused-k9-nk2", "aht_update_w", P3_M, 64, 9, True, False, dict(family="nt16", nk=2, mode=1)),
       ("nt16-bf16-k8-nk1", "aht", P3_M, 64, 8, True, True, dict(family="nt16", nk=1)),
       ("nt16-bf16-fused-k12-nk2", "aht_update_w", P3_M, 128, 12, True, True, dict(family="nt16", nk=2, mode=1)),
       ("nt16-not-taken-n%32-k16", "aht", P3_M, 100, 16, True, False, _nt(13, 1, 4, interior=0))]
)
# H H^T: the store_all form (PF 1) in column splits; single-stage and two-stage reductions of the split tiles, ragged last split
DENSE_HHT = [
    ("hht-k64-1-split", "gram_hht", 0, 100, 64, True, False, dict(family="nt", pf=1, fast=1, count=1, reduce="single")),
    ("hht-k32-ragged-split", "gram_hht", 0, 300, 32, True, False, dict(family="nt", pf=1, fast=1, count=3, nk=4, aux=2, reduce="single")),
    ("hht-k128-unaligned", "gram_hht", 0, 301, 128, False, False, dict(family="nt", pf=1, fast=0, count=3, reduce="single")),
    ("hht-k64-34-splits", "gram_hht", 0, 66 * 128 + 36, 64, True, False,
     dict(family="nt", pf=1, fast=1, count=34, per=256, reduce="single")),
    ("hht-k20-two-stage-ragged-slice", "gram_hht", 0, 65 * 256 + 4, 20, True, False, dict(family="nt", pf=1, count=66, reduce="two_stage", slices=3)),
    ("hht-k128-two-stage", "gram_hht", 0, 64 * 256 + 32, 128, True, False, dict(family="nt", pf=1, count=65, reduce="two_stage", slices=3)),
]


def _tn(kt, nt, b0, bl, fast=1, **kw):
    return dict(family="tn", kt=kt, nt=nt, fast=fast, b0_full=b0[0], b0_tail=b0[1], bl_full=bl[0], bl_tail=bl[1], **kw)


# tn_kernel's row-batch pipeline (two batches of 8 rows per trip): the last chunk with 0, 1, an odd and an even number of full batches and
# tails of 1..7 rows; n and k short of the column tile (clamped lanes); the reductions
DENSE_TN = (
    [("tn-k%d-b%d-t%d" % (k, b, t), "wta", 8 * b + t, n, k, True, False, _tn(kt, nt, (b, t), (b, t), count=1, reduce="single"))
     for k, kt, nt, n, b, t in ((32, 1, 4, 128, 0, 5), (30, 1, 4, 100, 1, 1), (64, 2, 4, 132, 3, 2), (62, 2, 4, 128, 4, 3), (128, 4, 2, 68, 5, 4),
                                (100, 4, 2, 64, 6, 5), (32, 1, 4, 260, 7, 6), (64, 2, 4, 128, 8, 7), (128, 4, 2, 64, 2, 0))]
    + [("tn-k32-2-chunks-ragged", "wta", 300, 132, 32, True, False, _tn(1, 4, (20, 0), (17, 4), count=2, reduce="single")),
       ("tn-k64-gram-first", "wta_gram", 300, 128, 64, True, False, _tn(2, 4, (20, 0), (17, 4), count=2)),
       ("tn-k32-bf16", "wta", 301, 128, 32, True, True, _tn(1, 4, (20, 0), (17, 5), count=2, ntemp=1)),
       ("tn-k64-bf16", "wta_gram", 301, 128, 64, True, True, _tn(2, 4, (20, 0), (17, 5), count=2, ntemp=1)),
       ("tn-k128-bf16", "wta", 301, 136, 128, True, True, _tn(4, 2, (20, 0), (17, 5), count=2, ntemp=1))]
    + [("tn-generic-k%d%s" % (k, "-bf16" if b else ""), "wta", 301, 130, k, False, b, _tn(kt, nt, (0, 160), (0, 141), fast=0, count=2, ntemp=0))
       for k, kt, nt in ((32, 1, 4), (64, 2, 4), (128, 4, 2)) for b in (False, True)]
    + [
       ("tn-k33-odd-rank-at-kt2", "wta", 300, 128, 33, True, False, dict(family="tn", kt=2, fast=0)),
       ("tn-k32-wide-reduce", "wta", 300, 4096, 32, True, False, dict(family="tn", kt=1, count=2, reduce="wide")),
       ("tn-k32-two-stage-ragged-slice", "wta", 78 * 256 + 40, 64, 32, True, False,
        dict(family="tn", kt=1, count=79, per=256, reduce="two_stage", slices=3, bl_full=5, bl_tail=0))]
    # the 16-wide kernel (batches of 16 rows), alone and with the riding Gram; the workspace too small for its slabs falls to tn_kernel
    + [("tn16-k16-b0-t12", "wta", 12, 64, 16, True, False, dict(family="tn16", v=4, b0_full=0, b0_tail=12, reduce="single")),
       ("tn16-k9-b1-t3", "wta", 19, 128, 9, True, False, dict(family="tn16", v=4, bl_full=1, bl_tail=3)),
       ("tn16-k16-bf16-b2-t1", "wta", 33, 128, 16, True, True, dict(family="tn16", v=8, bl_full=2, bl_tail=1)),
       ("tn16-k16-gram-ragged", "wta_gram", 300, 128, 16, True, False, dict(family="tn16_gram", count=2, b0_full=10, bl_full=8, bl_tail=12)),
       ("tn16-k5-bf16-gram", "wta_gram", 301, 256, 5, True, True, dict(family="tn16_gram", v=8, bl_full=8, bl_tail=13)),
       ("tn16-k16-two-stage-gram-first", "wta_gram", 65 * 256 + 16, 64, 16, True, False,
        dict(family="tn16", count=66, reduce="two_stage", slices=3, bl_full=1)),
       ("tn16-n%64-falls-to-tn", "wta", 300, 100, 16, True, False, dict(family="tn", kt=1))]
)
# W^T W: tn_kernel<KT, NT = KT (2 at KT = 4)> on 128-row chunks; the two-stage reduction at more than 64 chunks, ragged last slice
DENSE_WTW = [
    ("wtw-k32-b3-t1", "gram_wtw", 25, 0, 32, True, False, _tn(1, 1, (3, 1), (3, 1), count=1, reduce="single")),
    ("wtw-k64-b1-t7", "gram_wtw", 15, 0, 64, True, False, _tn(2, 2, (1, 7), (1, 7), count=1, reduce="single")),
    ("wtw-k64-ragged", "gram_wtw", 300, 0, 64, True, False, _tn(2, 2, (14, 0), (9, 4), count=3, per=112, reduce="single")),
    ("wtw-k100-clamped", "gram_wtw", 301, 0, 100, True, False, _tn(4, 2, (14, 0), (9, 5), count=3, reduce="single")),
    ("wtw-k64-generic", "gram_wtw", 301, 0, 64, False, False, _tn(2, 2, (0, 112), (0, 77), fast=0, count=3)),
    ("wtw-k32-generic", "gram_wtw", 301, 0, 32, False, False, _tn(1, 1, (0, 112), (0, 77), fast=0, count=3)),
    ("wtw-k128-generic", "gram_wtw", 301, 0, 128, False, False, _tn(4, 2, (0, 112), (0, 77), fast=0, count=3)),
    ("wtw-k64-two-stage-ragged-slice", "gram_wtw", 8336, 0, 64, True, False,
     _tn(2, 2, (16, 0), (2, 0), count=66, per=128, reduce="two_stage", slices=3)),
    ("wtw-k128-two-stage-tail", "gram_wtw", 8325, 0, 128, True, False, _tn(4, 2, (16, 0), (0, 5), count=66, reduce="two_stage", slices=3)),
]
# the W update.  update_w16_kernel: the grid-stride loop's second, ragged trip behind the 1024-workgroup cap of KT >= 2; update_w_seq_kernel:
# V = 4 only with EDGE (an aligned W with whole ranks and whole 32-row tiles goes to update_w16_kernel), V = 1 in both
DENSE_UPD_W = [
    ("w16-k32-one-tile-per-wave", "mu_update_w", 65536 + 16, 0, 32, True, False,
     dict(family="update_w16", kt=1, block=256, occ=8, grid_x=1025, aux=1)),
    ("w16-k64-second-trip", "mu_update_w", 65536 + 16, 0, 64, True, False,
     dict(family="update_w16", kt=2, block=256, occ=8, grid_x=1024, count=4097, aux=2)),
    ("w16-k128-second-trip", "mu_update_w", 131072 + 48, 0, 128, True, False,
     dict(family="update_w16", kt=4, block=512, occ=4, grid_x=1024, count=8195, aux=2)),
    ("w16-k64-short-grid", "mu_update_w", 48, 0, 64, True, False, dict(family="update_w16", kt=2, grid_x=1, count=3, aux=1)),
] + [("wseq-k%d-v%d-edge%d" % (k, v, e), "mu_update_w", m, 0, k, v == 4, False,
      dict(family="update_w_seq", kt=kt, v=v, edge=e, occ=4 if kt == 4 else 5))
     for k, kt, m, v, e in ((32, 1, 100, 4, 1), (20, 1, 96, 4, 1), (64, 2, 72, 4, 1), (128, 4, 40, 4, 1), (32, 1, 96, 1, 0), (31, 1, 96, 1, 1),
                            (64, 2, 64, 1, 0), (64, 2, 70, 1, 1), (128, 4, 32, 1, 0), (100, 4, 33, 1, 1))
] + [("wseq-k128-second-trip", "mu_update_w", 131072 + 40, 0, 128, True, False,
      dict(family="update_w_seq", kt=4, v=4, edge=1, grid_x=1024, aux=2))]
# the H update.  Two columns per lane from 1024 tiles of 64 columns on; its nontemporal form from 64 MiB on; one column per lane in both
# EDGE values; the second trip behind the 1024-workgroup cap of KT = 4
DENSE_UPD_H = [
    ("h2-k32-n65536", "mu_update_h", 0, 65536, 32, True, False, dict(family="update_h_seq", kt=1, nt=2, occ=3, edge=0, ntemp=0)),
    ("h2-k64-n65536", "mu_update_h", 0, 65536, 64, True, False, dict(family="update_h_seq", kt=2, nt=2, occ=3, edge=0, ntemp=0)),
    ("h2-k128-n65536", "mu_update_h", 0, 65536, 128, True, False, dict(family="update_h_seq", kt=4, nt=2, occ=2, edge=0, ntemp=0)),
    ("h2-nontemporal-k128-n131072", "mu_update_h", 0, 131072, 128, True, False, dict(family="update_h_seq", kt=4, nt=2, occ=2, ntemp=1)),
    ("h2-nontemporal-k64-n262144", "mu_update_h", 0, 262144, 64, True, False, dict(family="update_h_seq", kt=2, nt=2, occ=3, ntemp=1)),
    ("h2-nontemporal-k32-n524288", "mu_update_h", 0, 524288, 32, True, False, dict(family="update_h_seq", kt=1, nt=2, occ=3, ntemp=1)),
    ("h1-k32-odd-pitch-n65536", "mu_update_h", 0, 65536, 32, False, False, dict(family="update_h_seq", kt=1, nt=1, edge=0)),
    ("h1-k128-second-trip", "mu_update_h", 0, 131072 + 36, 128, True, False,
     dict(family="update_h_seq", kt=4, nt=1, edge=1, grid_x=1024, aux=2)),
] + [("h1-k%d-n%d-edge%d" % (k, n, e), "mu_update_h", 0, n, k, al, False, dict(family="update_h_seq", kt=kt, nt=1, occ=4, edge=e))
     for k, kt, n, al, e in ((32, 1, 96, True, 0), (20, 1, 96, True, 1), (64, 2, 64, False, 0), (64, 2, 70, True, 1), (128, 4, 32, True, 0),
                             (65, 4, 33, False, 1))]
# the element-wise passes: (id, pass, rows, cols, aligned, plan fields) -- the long-row and the patch form, vector and scalar; the
# streaming form (>= 256 MiB) once
DENSE_EW = [
    ("ew-long-vec", "clamp_min", 10, 2000, True, dict(family="ew", mode=1, v=4, ntemp=0, grid_x=1, grid_y=10)),
    ("ew-long-vec-2-blocks", "kl_update_h", 3, 4100, True, dict(family="ew", mode=1, v=4, grid_x=2, grid_y=3)),
    ("ew-long-scalar", "scale_rows_mul", 10, 1030, False, dict(family="ew", mode=1, v=1, grid_x=2, grid_y=10)),
    ("ew-patch-vec", "scale_cols_div", 1000, 40, True, dict(family="ew", mode=0, v=4, aux=4, grid_x=16)),
    ("ew-patch-scalar", "kl_update_w", 1000, 37, False, dict(family="ew", mode=0, v=1, aux=6, grid_x=63)),
    ("ew-patch-vec-x-unaligned", "scale_cols_div", 100, 40, "x", dict(family="ew", mode=0, v=1)),
    ("ew-long-stream", "clamp_min", 16384, 4096, True, dict(family="ew", mode=1, v=4, ntemp=1)),
    ("ew-patch-stream", "clamp_min", 1 << 20, 64, True, dict(family="ew", mode=0, v=4, ntemp=1)),
]
# the KL products at 16 < k (csrc/dnmf_kl.hip).  U H^T: the pipelined kernel on the whole 128-row tiles of every KT with kl_uht_kernel on the
# ragged last one (both write into one output), alone on whole tiles, through column splits and their reduction, on H as column blocks
# (65 blocks: a two-stage reduction), on padded images of a ragged rank; kl_uht_kernel alone below one tile and on unaligned operands.
# W^T U: every KT fast and generic, a ragged last chunk, more than 64 chunks
KL_M = 2 * 128 + 44
DENSE_KL = (
    [("klpipe-k%d-ragged-tile" % k, "kl_uht", KL_M, 96, k, True, False,
      dict(family="kl_uht_pipe", kt=k // 32, fast=1, mode=0, edge=1, grid_x=2, aux=1, count=1, nk=3, reduce="none")) for k in (32, 64, 128)]
    + [("klpipe-k%d-whole-tiles" % k, "kl_uht", 256, 64, k, True, False, dict(family="kl_uht_pipe", kt=k // 32, mode=0, edge=0, grid_x=2, aux=0))
       for k in (32, 64, 128)]
    + [("klpipe-k%d-padded-m%d" % (k, m), "kl_uht", m, 1024, k, True, False,
        dict(family="kl_uht_pipe", kt=kt, fast=1, mode=1, edge=int(m % 128 > 0), count=4, reduce="single"))
       for k, kt in ((20, 1), (40, 2), (100, 4)) for m in (256, KL_M)]
    + [("kluht-k%d-padded-unsplit" % k, "kl_uht", KL_M, 96, k, True, False, dict(family="kl_uht", kt=kt, fast=1, mode=1, grid_x=3))
       for k, kt in ((20, 1), (40, 2), (100, 4))]
    + [("kluht-k%d-below-one-tile" % k, "kl_uht", 100, 96, k, True, False, dict(family="kl_uht", kt=k // 32, fast=1, mode=0, grid_x=1))
       for k in (32, 64, 128)]
    + [
       ("klpipe-k64-4-splits", "kl_uht", KL_M, 1024, 64, True, False, dict(family="kl_uht_pipe", kt=2, edge=1, count=4, per=256, reduce="single")),
       ("klpipe-k32-factors-unaligned-padded", "kl_uht", KL_M, 96, 32, "W,H", False, dict(family="kl_uht_pipe", kt=1, fast=1, mode=1)),
       ("klpipe-hblocks-k32", "kl_uht_hblocks", KL_M, 128, 32, True, False, dict(family="kl_uht_pipe", kt=1, edge=1, count=4, per=32, reduce="single")),
       ("klpipe-hblocks-k64-two-stage", "kl_uht_hblocks", KL_M, 65 * 32, 64, True, False,
        dict(family="kl_uht_pipe", kt=2, count=65, per=32, reduce="two_stage", slices=3)),
       ("kluht-k64-n%32", "kl_uht", KL_M, 100, 64, True, False, dict(family="kl_uht", kt=2, fast=1, grid_x=3))]
    + [("kluht-k%d-generic" % k, "kl_uht", KL_M, 97, k, False, False, dict(family="kl_uht", kt=kt, fast=0, mode=0, grid_x=3))
       for k, kt in ((20, 1), (64, 2), (128, 4))]
    + [("klwtu-k%d-ragged-chunk" % k, "kl_wtu", KL_M, 132, k, True, False,
        dict(family="kl_wtu", kt=kt, nt=nt, fast=1, mode=0, count=2, per=160, b0_full=5, bl_full=4, bl_tail=12, reduce="single"))
       for k, kt, nt in ((32, 1, 4), (64, 2, 2), (128, 4, 2))]
    + [("klwtu-k%d-generic" % k, "kl_wtu", KL_M, 131, k, False, False, dict(family="kl_wtu", kt=kt, fast=0, mode=0, count=2))
       for k, kt in ((20, 1), (64, 2), (100, 4))]
    + [("klwtu-k%d-padded" % k, "kl_wtu", KL_M, 132, k, True, False, dict(family="kl_wtu", kt=kt, fast=1, mode=1))
       for k, kt in ((20, 1), (40, 2), (100, 4))]
    + [
       ("klwtu-k32-two-stage-ragged-slice", "kl_wtu", 65 * 256 + 40, 64, 32, True, False,
        dict(family="kl_wtu", kt=1, fast=1, count=66, per=256, reduce="two_stage", slices=3, bl_full=1, bl_tail=8)),
       ("klwtu-k32-wide-reduce", "kl_wtu", KL_M, 4096, 32, True, False, dict(family="kl_wtu", kt=1, fast=1, reduce="wide"))]
)
# the 16-wide KL kernels of k <= 16 (csrc/dnmf_kl16.hip).  kl_uht16_kernel: friendly factors (k = 16, aligned) and factors padded to 16, one
# split stored directly and several splits through slabs, whole and ragged row tiles, an odd and an even number of k-tiles, H as column
# blocks (65 of them: a two-stage reduction); kl_wtu16_kernel: chunks of 16-row blocks taken two per trip (an even and an odd count, a
# ragged tail), more than 64 chunks, the wide reduction; and the shapes that keep the 32-wide kernels at k <= 16
def _k16(fam, mode, **kw):
    return dict(family=fam, kt=1, fast=1, mode=mode, **kw)


DENSE_KL16 = [
    ("kl16uht-k16-direct", "kl_uht", KL_M, 96, 16, True, False, _k16("kl16_uht", 0, edge=1, count=1, nk=3, grid_x=3, aux=44, reduce="none")),
    ("kl16uht-k16-direct-whole-tiles", "kl_uht", 256, 64, 16, True, False, _k16("kl16_uht", 0, edge=1, nk=2, grid_x=2, aux=0)),
    ("kl16uht-k16-4-splits", "kl_uht", KL_M, 1024, 16, True, False, _k16("kl16_uht", 0, edge=0, count=4, per=256, nk=8, reduce="single")),
    ("kl16uht-k16-out-unaligned", "kl_uht", KL_M, 96, 16, "UHT", False, _k16("kl16_uht", 0, edge=0, count=1, reduce="single")),
    ("kl16uht-k9-padded", "kl_uht", KL_M, 96, 9, True, False, _k16("kl16_uht", 1, edge=0, count=1, nk=3, reduce="single")),
    ("kl16uht-k1-padded-4-splits", "kl_uht", KL_M, 1024, 1, True, False, _k16("kl16_uht", 1, edge=0, count=4, reduce="single")),
    ("kl16uht-k16-factors-unaligned-padded", "kl_uht", KL_M, 32, 16, "W,H", False, _k16("kl16_uht", 1, edge=1, nk=1)),
    ("kl16uht-hblocks-k16", "kl_uht_hblocks", KL_M, 128, 16, True, False, _k16("kl16_uht", 0, edge=0, count=4, per=32, nk=1, reduce="single")),
    ("kl16uht-hblocks-k16-two-stage", "kl_uht_hblocks", KL_M, 65 * 32, 16, True, False,
     _k16("kl16_uht", 0, count=65, per=32, reduce="two_stage", slices=3)),
    ("kl16uht-not-taken-n%32", "kl_uht", KL_M, 100, 16, True, False, dict(family="kl_uht", kt=1, fast=1, mode=1)),
    ("kl16uht-not-taken-a-unaligned-k9", "kl_uht", KL_M, 97, 9, False, False, dict(family="kl_uht", kt=1, fast=0, mode=0)),
    ("kl16wtu-k16-odd-blocks-tail", "kl_wtu", 316, 128, 16, True, False,
     _k16("kl16_wtu", 0, count=5, per=64, b0_full=4, bl_full=3, bl_tail=12, reduce="single")),
    ("kl16wtu-k16-whole-chunks", "kl_wtu", 256, 64, 16, True, False, _k16("kl16_wtu", 0, count=4, per=64, bl_full=4, bl_tail=0)),
    ("kl16wtu-k9-padded", "kl_wtu", KL_M, 128, 9, True, False, _k16("kl16_wtu", 1, count=5, bl_full=2, bl_tail=12)),
    ("kl16wtu-k16-two-stage-ragged-slice", "kl_wtu", 65 * 64 + 20, 64, 16, True, False,
     _k16("kl16_wtu", 0, count=66, per=64, reduce="two_stage", slices=3, bl_full=1, bl_tail=4)),
    ("kl16wtu-k5-wide-reduce", "kl_wtu", KL_M, 4096, 5, True, False, _k16("kl16_wtu", 1, reduce="wide")),
    ("kl16wtu-not-taken-n%64", "kl_wtu", KL_M, 96, 16, True, False, dict(family="kl_wtu", kt=1, fast=1, mode=1)),
]
# the residual, the per-column error and the squared norm: resid_lds_kernel for every KT and both storage types at m = 4096 plus a ragged
# remainder (and on padded images of a ragged rank), resid_kernel below that size and on unaligned operands; colerr_kernel for every KT,
# FAST and storage type and with several row blocks per wave; sqnorm_kernel in both forms with a second grid-stride trip
RL_M = 4096 + 36
DENSE_RESID = (
    [("residlds-k%d%s" % (k, "-bf16" if b else ""), "resid_sqnorm", RL_M, 128, k, True, b, dict(family="resid_lds", kt=k // 32, fast=1, mode=0))
     for k in (32, 64, 128) for b in (False, True)]
    + [("residlds-k%d-padded%s" % (k, "-bf16" if b else ""), "resid_sqnorm", RL_M, 136, k, True, b, dict(family="resid_lds", kt=kt, fast=1, mode=1))
       for k, kt in ((20, 1), (40, 2), (100, 4)) for b in (False, True)]
    + [
       ("resid-k32-n-below-128", "resid_sqnorm", RL_M, 124, 32, True, False, dict(family="resid", kt=1, fast=1)),
       ("resid-k64-m-below-4096", "resid_sqnorm", 4095, 128, 64, True, True, dict(family="resid", kt=2, fast=1))]
    + [("resid-k%d-generic%s" % (k, "-bf16" if b else ""), "resid_sqnorm", KL_M, 130, k, False, b, dict(family="resid", kt=kt, fast=0, mode=0))
       for k, kt in ((20, 1), (64, 2), (128, 4)) for b in (False, True)]
    + [("resid-k%d-fast%s" % (k, "-bf16" if b else ""), "resid_sqnorm", KL_M, 132, k, True, b, dict(family="resid", kt=k // 32, fast=1, mode=0))
       for k in (32, 64, 128) for b in (False, True)]
    + [("colerr-k%d-%s%s" % (k, "fast" if al else "generic", "-bf16" if b else ""), "column_err", KL_M, 132 if al else 130, k, al, b,
        dict(family="colerr", kt=kt, fast=int(al), per=32)) for k, kt in ((32, 1), (64, 2), (128, 4)) for al in (True, False) for b in (False, True)]
    + [("colerr-k32-2-row-blocks-per-wave", "column_err", 8192 + 40, 4096, 32, True, False, dict(family="colerr", kt=1, fast=1, per=64, count=129))]
    + [("sqnorm-fast-2-trips", "sqnorm", 600, 4000, 1, True, False, dict(family="sqnorm", fast=1, grid_x=2048, aux=2)),
       ("sqnorm-fast-bf16", "sqnorm", 300, 136, 1, True, True, dict(family="sqnorm", fast=1, aux=1)),
       ("sqnorm-generic-2-trips", "sqnorm", 600, 1001, 1, False, False, dict(family="sqnorm", fast=0, grid_x=2048, aux=2)),
       ("sqnorm-generic-bf16", "sqnorm", 300, 130, 1, False, True, dict(family="sqnorm", fast=0))]
)
DENSE_REACH = DENSE_NT + DENSE_HHT + DENSE_TN + DENSE_WTW + DENSE_UPD_W + DENSE_UPD_H + DENSE_KL + DENSE_KL16 + DENSE_RESID
# What the table leaves out: only branches whose condition needs an operand above 1 GiB -- the 2 GiB descriptor-window fallbacks -- each
# with the test that keeps it, and what the selectors cannot return at all.  (The streaming element-wise forms, 256 MiB each, are run for
# one pass, clamp_min, in both the long-row and the patch form: the template's OP does not enter the choice.)
DENSE_EXEMPT = {
    "nt: interior, not eligible (a tile beyond the 2 GiB window of the PF 10 / 13 loops)": "test_gpu_kernels::test_a_beyond_2_and_4_gib, test_column_slice_leaves_the_window",
    "tn: a chunk beyond the 2 GiB window (the pointer form of the pipeline)": "test_gpu_kernels::test_a_beyond_2_and_4_gib",
    "kl_uht: a tile beyond the 2 GiB windows keeps kl_uht_kernel; kl_wtu: the chunk cap of plan_kl_wtu": "test_gpu_kernels::test_a_beyond_2_and_4_gib",
    "update_w16: a 16-row tile beyond the 2 GiB window -- not reachable: mu_update_w refuses pitches from 2^23 on": "tests/test_dense_plan.py::test_unreachable",
    "update_w_seq<KT, 4, OCC, false>: needs the window test above to fail -- not reachable": "tests/test_dense_plan.py::test_unreachable",
}


# (row chunks or column splits, rows or columns per chunk) of the cases whose CPU proofs walk the partition -- tests/test_exact_cpu.py stays
# free of the library; tests/test_dense_plan.py holds these to dnmf_dense_plan
DENSE_CHUNKS = {
    "hht-k64-1-split": (1, 128),
    "hht-k32-ragged-split": (3, 128),
    "hht-k128-unaligned": (3, 128),
    "hht-k64-34-splits": (34, 256),
    "hht-k20-two-stage-ragged-slice": (66, 256),
    "hht-k128-two-stage": (65, 256),
    "tn-k32-b0-t5": (1, 16),
    "tn-k30-b1-t1": (1, 16),
    "tn-k64-b3-t2": (1, 32),
    "tn-k62-b4-t3": (1, 48),
    "tn-k128-b5-t4": (1, 48),
    "tn-k100-b6-t5": (1, 64),
    "tn-k32-b7-t6": (1, 64),
    "tn-k64-b8-t7": (1, 80),
    "tn-k128-b2-t0": (1, 16),
    "tn-k32-2-chunks-ragged": (2, 160),
    "tn-k64-gram-first": (2, 160),
    "tn-k32-bf16": (2, 160),
    "tn-k64-bf16": (2, 160),
    "tn-k128-bf16": (2, 160),
    "tn-generic-k32": (2, 160),
    "tn-generic-k32-bf16": (2, 160),
    "tn-generic-k64": (2, 160),
    "tn-generic-k64-bf16": (2, 160),
    "tn-generic-k128": (2, 160),
    "tn-generic-k128-bf16": (2, 160),
    "tn-k33-odd-rank-at-kt2": (2, 160),
    "tn-k32-wide-reduce": (2, 160),
    "tn-k32-two-stage-ragged-slice": (79, 256),
    "tn16-k16-b0-t12": (1, 16),
    "tn16-k9-b1-t3": (1, 32),
    "tn16-k16-bf16-b2-t1": (1, 48),
    "tn16-k16-gram-ragged": (2, 160),
    "tn16-k5-bf16-gram": (2, 160),
    "tn16-k16-two-stage-gram-first": (66, 256),
    "tn16-n%64-falls-to-tn": (2, 160),
    "wtw-k32-b3-t1": (1, 32),
    "wtw-k64-b1-t7": (1, 16),
    "wtw-k64-ragged": (3, 112),
    "wtw-k100-clamped": (3, 112),
    "wtw-k64-generic": (3, 112),
    "wtw-k32-generic": (3, 112),
    "wtw-k128-generic": (3, 112),
    "wtw-k64-two-stage-ragged-slice": (66, 128),
    "wtw-k128-two-stage-tail": (66, 128),
    "klwtu-k32-ragged-chunk": (2, 160),
    "klwtu-k64-ragged-chunk": (2, 160),
    "klwtu-k128-ragged-chunk": (2, 160),
    "klwtu-k20-generic": (2, 160),
    "klwtu-k64-generic": (2, 160),
    "klwtu-k100-generic": (2, 160),
    "klwtu-k20-padded": (2, 160),
    "klwtu-k40-padded": (2, 160),
    "klwtu-k100-padded": (2, 160),
    "klwtu-k32-two-stage-ragged-slice": (66, 256),
    "klwtu-k32-wide-reduce": (2, 160),
    "kl16wtu-k16-odd-blocks-tail": (5, 64),
    "kl16wtu-k16-whole-chunks": (4, 64),
    "kl16wtu-k9-padded": (5, 64),
    "kl16wtu-k16-two-stage-ragged-slice": (66, 64),
    "kl16wtu-k5-wide-reduce": (5, 64),
    "kl16wtu-not-taken-n%64": (2, 160),
}


def dense_pitch(cols, aligned, bf16=False):
    """the pitch and the start (in elements) of a `Poisoned` view as tests/test_gpu_exact_dense.py makes them"""
    if not aligned:
        return cols + 3, 3
    q = 8 if bf16 else 4
    return -(-cols // q) * q + q, 8


DENSE_OPERANDS = {"aht": ("A", "H"), "aht_hblocks": ("A", "Hs"), "aht_update_w": ("A", "H", "W"), "wta": ("A", "W", "AtW"),
                  "wta_gram": ("A", "W", "AtW"), "gram_hht": ("H",), "gram_wtw": ("W",), "mu_update_w": ("W", "AH"), "mu_update_h": ("H", "AtW"),
                  "kl_uht": ("A", "W", "H", "UHT"), "kl_uht_hblocks": ("A", "W", "Hs", "UHT"), "kl_wtu": ("A", "W", "H", "WTU"),
                  "resid_sqnorm": ("A", "W", "H"), "column_err": ("A", "W", "H"), "sqnorm": ("A",)}
DENSE_HBLK = 32                                                    # the block width of the aht_hblocks cases


def dense_is_aligned(aligned, name):
    """`aligned` of a case: True, False, or the names of the operands that are not (comma separated)"""
    return aligned is True or (isinstance(aligned, str) and name not in aligned.split(","))


def dense_plan_args(op, m, n, k, aligned, bf16, quantum8=True):
    """the pitches and the addresses modulo 16 dnmf_dense_plan takes for a case, in the order of its operands (include/dnmf.h);
    quantum8=False: bf16 views as tests/test_gpu_exact.py makes them (pitches in steps of 4 elements)"""
    cols = {"A": n, "H": n, "W": k, "AtW": n, "AH": k, "UHT": k, "WTU": n}
    ld, off = [], []
    for name in DENSE_OPERANDS[op]:
        if name == "Hs":
            ld.append(DENSE_HBLK); off.append(0)
            continue
        b = bool(bf16) and name == "A"
        pitch, lead = dense_pitch(cols[name], dense_is_aligned(aligned, name), b and quantum8)
        ld.append(pitch); off.append(lead * (2 if b else 4) % 16)
    return ld, off


# ---------------------------------------------------------------------------------------------------------- ranks 128 < k <= 256
# The shapes of tests/test_gpu_exact_wide.py, in the layout of DENSE_REACH: (id, op, m, n, k, aligned, bf16-stored A, plan fields).  A wide
# rank is served by composition (csrc/dnmf_wide.hip): two panel calls of the tuned kernels, the second at r = k - 128 on sub-views, four
# block calls for a Gram, and the plain kernels wide_nn_rows_kernel / wide_upd_h_kernel.  The plan fields of a case:
#   panel     (family, kt, fast) of the LAST tuned call the entry point issues (`wide_panel_plans`): the second panel, block (1, 1) of a Gram
#   gram10    the family of block (1, 0) of W^T W, r x 128: the 16-wide kernel when W's rows are 16-byte aligned and r <= 16
#   grid_x, grid_y, aux   the launch of the plain kernel as dnmf_dense_plan reports it at the wide rank (aux: 16-column tiles of a full
#             column range; mu_update_h: 16-row tiles of k)
# tests/test_dense_plan.py asserts every entry and what the union covers without a GPU; tests/test_exact_cpu.py proves the operands.
_N16, _T16 = ("nt16", 1, 1), ("tn16", 1, 1)
# (class, m, n, k, aligned, second panel of the NT form, of the TN form, block (1, 1) of W^T W, family of block (1, 0) of W^T W)
WIDE_PANEL_CLASSES = [
    # r <= 16 on the 16-wide kernels: 16-byte aligned rows, n a multiple of 64
    ("r4-16wide", 300, 256, 132, True, _N16, _T16, ("tn", 1, 1), "tn16"),
    ("r16-16wide", 300, 256, 144, True, _N16, _T16, ("tn", 1, 1), "tn16"),
    # r <= 16 where they do not apply: 32-wide at KT = 1 -- an unaligned view, n % 32 != 0, k % 4 = 2 and 3
    ("r4-unaligned", 300, 256, 132, False, ("nt", 1, 0), ("tn", 1, 0), ("tn", 1, 0), "tn"),
    ("r16-n%32", 261, 332, 144, True, ("nt", 1, 1), ("tn", 1, 1), ("tn", 1, 1), "tn16"),
    ("r2-k%4=2", 261, 331, 130, True, ("nt", 1, 0), ("tn", 1, 0), ("tn", 1, 0), "tn16"),
    ("r3-k%4=3-unaligned", 261, 331, 131, False, ("nt", 1, 0), ("tn", 1, 0), ("tn", 1, 0), "tn"),
    # the two sides of the KT boundaries
    ("r17", 300, 256, 145, True, ("nt", 1, 1), ("tn", 1, 1), ("tn", 1, 0), "tn"),
    ("r32-unaligned", 261, 331, 160, False, ("nt", 1, 0), ("tn", 1, 0), ("tn", 1, 0), "tn"),
    ("r33", 300, 256, 161, True, ("nt", 2, 1), ("tn", 2, 0), ("tn", 2, 0), "tn"),
    ("r33-unaligned", 261, 331, 161, False, ("nt", 2, 0), ("tn", 2, 0), ("tn", 2, 0), "tn"),
    ("r64", 300, 256, 192, True, ("nt", 2, 1), ("tn", 2, 1), ("tn", 2, 1), "tn"),
    ("r65-unaligned", 261, 331, 193, False, ("nt", 4, 0), ("tn", 4, 0), ("tn", 4, 0), "tn"),
    ("r127", 300, 256, 255, True, ("nt", 4, 1), ("tn", 4, 0), ("tn", 4, 0), "tn"),
    ("r128", 300, 256, 256, True, ("nt", 4, 1), ("tn", 4, 1), ("tn", 4, 1), "tn"),
]
WIDE_BF16_CLASSES = ("r4-16wide", "r16-16wide", "r33", "r65-unaligned", "r127")      # bf16-stored A for the products: the same kernels
# the quotient image U of the KL products is 16-byte aligned whatever the caller's views are: W^T U of an unaligned case with whole
# 64-column blocks stays on the 16-wide kernel
WIDE_KLWTU_PANEL = {"r4-unaligned": _T16}


def _wpanel(p, **kw):
    return dict(panel=dict(family=p[0], kt=p[1], fast=p[2]), **kw)


def _wide_panel_cases():
    out = []
    for name, m, n, k, al, ntp, tnp, w11, w10 in WIDE_PANEL_CLASSES:
        gy, gx = -(-n // 64), -(-(-(-m // 16)) // 4)                # (these shapes: ranges of the minimum 64 columns, 4 tiles)
        out += [("aht-" + name, "aht", m, n, k, al, False, _wpanel(ntp)),
                ("wta-" + name, "wta", m, n, k, al, False, _wpanel(tnp)),
                ("wtagram-" + name, "wta_gram", m, n, k, al, False, _wpanel(tnp, gram10=w10)),
                ("hht-" + name, "gram_hht", 0, n, k, al, False, _wpanel(ntp)),
                ("wtw-" + name, "gram_wtw", m, 0, k, al, False, _wpanel(w11, gram10=w10)),
                ("kluht-" + name, "kl_uht", m, n, k, al, False, _wpanel(ntp, grid_x=gx, grid_y=gy, aux=4)),
                ("klwtu-" + name, "kl_wtu", m, n, k, al, False, _wpanel(WIDE_KLWTU_PANEL.get(name, tnp), grid_x=gx, grid_y=gy, aux=4))]
        if name in WIDE_BF16_CLASSES:
            out += [("aht-%s-bf16" % name, "aht", m, n, k, al, True, _wpanel(ntp)),
                    ("wta-%s-bf16" % name, "wta", m, n, k, al, True, _wpanel(tnp)),
                    ("wtagram-%s-bf16" % name, "wta_gram", m, n, k, al, True, _wpanel(tnp, gram10=w10))]
    return out


# The plain kernels.  wide_nn_rows_kernel<W_QUOT | W_SQSUM | W_COLERR> (through kl_uht / kl_wtu, resid_sqnorm, column_err): a wave per
# 16-row strip, grid_y column ranges of 16 aux columns.  BIG: 513 strips, ranges of 5 tiles, 13 of them, the last of 40 columns with a
# ragged last tile.  TALL: more than 8192 strips, where the launcher asks for ONE range whatever n is -- 5 tiles, the last ragged -- and
# the last of 2049 workgroups has one live wave (W alone is 64.5 MiB there: no m above 131072 keeps a wide W below 64 MiB).
WIDE_BIG, WIDE_TALL = (8200, 1000), (131088, 70)
WIDE_PLAIN = (
    [("%s-5-tile-ranges-ragged" % s, op, WIDE_BIG[0], WIDE_BIG[1], 130, al, False, dict(grid_x=129, grid_y=13, aux=5))
     for s, op, al in (("kluht", "kl_uht", True), ("klwtu-unaligned", "kl_wtu", False), ("resid", "resid_sqnorm", True),
                       ("colerr-unaligned", "column_err", False))]
    + [("%s-one-range-of-5-tiles" % s, op, WIDE_TALL[0], WIDE_TALL[1], 130, True, False, dict(grid_x=2049, grid_y=1, aux=5))
       for s, op in (("kluht", "kl_uht"), ("resid", "resid_sqnorm"), ("colerr", "column_err"))]
    # n < 16 and n = 1 (one ragged tile); m % 16 != 0; 17 strips: the last workgroup has one live wave; ranges of 4 tiles with a ragged last
    # range at k % 4 = 3 and at k = 256
    + [("%s-n9-k131" % s, op, 300, 9, 131, al, False, dict(grid_x=5, grid_y=1, aux=4))
       for s, op, al in (("kluht", "kl_uht", False), ("klwtu", "kl_wtu", True), ("resid", "resid_sqnorm", False), ("colerr", "column_err", True))]
    + [("%s-n1-k130" % s, op, 261, 1, 130, al, False, dict(grid_x=5, grid_y=1, aux=4))
       for s, op, al in (("kluht", "kl_uht", True), ("klwtu", "kl_wtu", False), ("resid", "resid_sqnorm", True), ("colerr", "column_err", False))]
    + [("%s-6-ranges-k%d%s" % (s, k, "" if al else "-unaligned"), op, 261, 331, k, al, False, dict(grid_x=5, grid_y=6, aux=4))
       for s, op in (("resid", "resid_sqnorm"), ("colerr", "column_err")) for k, al in ((131, False), (256, True))]
    # wide_nn_rows_kernel<W_UPD_W>: one range over the k columns of W -- k % 16 != 0 (a ragged last tile; k % 4 = 2, 3: the lane mask),
    # k = 255 and k = 256
    + [("updw-k%d%s" % (k, "" if al else "-unaligned"), "mu_update_w", m, 0, k, al, False, dict(grid_x=5, grid_y=1, aux=-(-k // 16)))
       for m, k, al in ((261, 130, True), (300, 131, False), (261, 255, False), (300, 256, True))]
    # wide_upd_h_kernel: a wave per 16 columns, a loop over the 16-row tiles of k -- a ragged last row tile, a ragged last column tile, a
    # partly filled last workgroup (21 tiles: 6 workgroups, the last with one wave), n = 1 and n = 9, whole tiles throughout at k = 256
    + [("updh-k%d-n%d%s" % (k, n, "" if al else "-unaligned"), "mu_update_h", 0, n, k, al, False,
        dict(grid_x=-(-(-(-n // 16)) // 4), grid_y=1, aux=-(-k // 16)))
       for n, k, al in ((331, 131, True), (1, 130, False), (9, 255, True), (331, 193, False), (256, 256, True))]
)
WIDE_REACH = _wide_panel_cases() + list(WIDE_PLAIN)
WIDE_ROWS_OPS = ("kl_uht", "kl_wtu", "resid_sqnorm", "column_err")      # the ops that launch wide_nn_rows_kernel over the columns of A
# whole fits on fixed points (tests/test_gpu_exact_wide.py): `fro_fixed`, `kl_fixed`, `kl_moved` at one shape (m, n not divisible by 3)
WIDE_FIT_SHAPE = (260, 334)
WIDE_FIT_KS = (130, 161, 255)
WIDE_FIT_STEPS = (1, 11, 12)                                        # the clamp step is i % 10 == 0: steps 0 and 10


def wide_panel_plans(op, m, n, k, ld, off, bf16=False, ws_bytes=None):
    """The tuned-kernel calls an entry point issues at a wide rank (128 < k <= 256; csrc/dnmf.hip: aht_impl, wta_impl, wide_gram;
    csrc/dnmf_kl.hip: wide_kl_product), as dnmf_dense_plan answers each one at the call's own rank, pitches and addresses modulo 16.
    ld / off: the pitches (elements) and addresses modulo 16 (bytes) of the op's operands in the order of include/dnmf.h; ws_bytes: the
    caller's workspace (None: dnmf_ws_bytes).  Returns (the wide plan, the calls' plans in the order they are issued): the products
    issue two -- rows of H, columns of W --, the Grams four blocks (p, q) = (0, 0), (0, 1), (1, 0), (1, 1), wta_gram the four of W^T W and
    then its two panels; the KL products run theirs on the quotient image U (pitch n rounded up to 4, in the workspace)."""
    from pydnmfk_amd import _lib as L
    m, n = max(m, 1), max(n, 1)
    if ws_bytes is None:
        ws_bytes = L.lib.dnmf_ws_bytes(m, n, k)
    wide = L.dense_plan(op, m, n, k, ld, off, bf16a=bf16, ws_bytes=ws_bytes)
    assert wide["family"] == "wide", (op, k, wide)
    per = wide["per"]
    ks = (per, k - per)
    assert 0 < ks[1] <= per and wide["count"] == (4 if op.startswith("gram") else 2)
    adv = lambda o, elems: (o + 4 * elems) % 16                      # a float32 operand advanced by `elems` elements

    def gram_wtw(ldw, offw):                                         # W_p^T W_q = "W^T A" with A = W_q, into the 256-pitch Gram buffer
        return [L.dense_plan("wta", m, ks[q], ks[p], [ldw, ldw, 256], [adv(offw, q * per), adv(offw, p * per), 0], ws_bytes=ws_bytes)
                for p in (0, 1) for q in (0, 1)]
    if op == "aht":
        plans = [L.dense_plan("aht", m, n, ks[j], ld[:2], [off[0], adv(off[1], j * per * ld[1])], bf16a=bf16) for j in (0, 1)]
    elif op in ("wta", "wta_gram"):
        plans = gram_wtw(ld[1], off[1]) if op == "wta_gram" else []
        plans += [L.dense_plan("wta", m, n, ks[j], ld[:3], [off[0], adv(off[1], j * per), adv(off[2], j * per * ld[2])], bf16a=bf16,
                               ws_bytes=ws_bytes) for j in (0, 1)]
    elif op == "gram_hht":                                           # H_p H_q^T = "A H^T" with A = H_p
        plans = [L.dense_plan("aht", ks[p], n, ks[q], [ld[0], ld[0]], [adv(off[0], p * per * ld[0]), adv(off[0], q * per * ld[0])])
                 for p in (0, 1) for q in (0, 1)]
    elif op == "gram_wtw":
        plans = gram_wtw(ld[0], off[0])
    elif op in ("kl_uht", "kl_wtu"):
        ldu = -(-n // 4) * 4
        ub = -(-m * ldu * 4 // 256) * 256
        assert ws_bytes >= ub
        inner = (ws_bytes - ub) // 256 * 256                         # what is left in front of U for the panel calls
        if op == "kl_uht":
            plans = [L.dense_plan("aht", m, n, ks[j], [ldu, ld[2]], [0, adv(off[2], j * per * ld[2])]) for j in (0, 1)]
        else:
            plans = [L.dense_plan("wta", m, n, ks[j], [ldu, ld[1], ld[3]], [0, adv(off[1], j * per), adv(off[3], j * per * ld[3])],
                                  ws_bytes=inner) for j in (0, 1)]
    else:
        raise ValueError("%s issues no panel calls" % op)
    assert all(p["family"] not in ("none", "wide") for p in plans), (op, m, n, k, plans)
    return wide, plans


def wide_case_plans(case, ws_bytes=None, ld=None, off=None):
    """(the wide plan, the tuned calls' plans) of a WIDE_REACH case -- at the pitches and addresses `dense_plan_args` derives for it, or
    at those of the views a test is about to pass (ld, off)"""
    from pydnmfk_amd import _lib as L
    cid, op, m, n, k, aligned, bf16, _ = case
    if ld is None:
        ld, off = dense_plan_args(op, m, n, k, aligned, bf16)
    if op in ("mu_update_w", "mu_update_h", "resid_sqnorm", "column_err"):            # the plain kernel alone
        return L.dense_plan(op, max(m, 1), max(n, 1), k, ld, off, bf16a=bf16, ws_bytes=ws_bytes), []
    return wide_panel_plans(op, m, n, k, ld, off, bf16, ws_bytes)


def wide_assert_plans(case, wide, plans):
    """a WIDE_REACH case reports the fields it is listed with"""
    cid, op, want = case[0], case[1], case[-1]
    assert wide["family"] == "wide" and wide["count"] == (4 if op.startswith("gram") else 2) and wide["per"] == 128, (cid, wide)
    if "panel" in want:
        assert {f: plans[-1][f] for f in ("family", "kt", "fast")} == want["panel"], (cid, plans[-1])
    if "gram10" in want:                                            # (the Gram's blocks come first: (0, 0), (0, 1), (1, 0), (1, 1))
        assert plans[2]["family"] == want["gram10"], (cid, plans[2])
    got = {f: wide[f] for f in ("grid_x", "grid_y", "aux") if f in want}
    assert got == {f: want[f] for f in got}, (cid, wide)
    assert wide["block"] == (256 if got else 0), (cid, wide)


def dense_nt_operands(m, n, k, seed=0):
    """A in 0..7, H and W in 1..3 (some zero rows of W, zero columns of H), G = H H^T: the operands of `products` without its H-phase
    denominators (W^T W) H, which outgrow 2^22 at the tall shapes of the descriptor loops.  A H^T is an integer below 2^24 and W G is 0
    or an integer in [2, 2^22) that absorbs eps.  Every 32-column tile of every 128-row block of A has a nonzero product with H."""
    rs = np.random.RandomState(seed + 1009 * m + 17 * n + k)
    A = rs.randint(0, 8, size=(m, n)).astype(np.float32)
    A[rs.rand(m, n) < 0.2] = 0
    H = rs.randint(1, 4, size=(k, n)).astype(np.float32)
    W = rs.randint(1, 4, size=(m, k)).astype(np.float32)
    W[rs.rand(m) < 0.05] = 0
    if n > 8:
        H[:, rs.rand(n) < 0.05] = 0
    A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
    G = H64 @ H64.T
    _bound(A64 @ H64.T, 1.0, np.float32, "A H^T")
    _bound(G, 1.0, np.float32, "H H^T")
    d = W64 @ G
    _bound(d, 0.25, np.float32, "W HH^T")
    assert np.all((d == 0) | (d >= 2))
    return A, W, H, G


def dense_tn_operands(m, n, k, seed=0):
    """A in 0..7 and W in 1..3 with some zero rows: W^T A and W^T W are integers below 2^24 in any order"""
    rs = np.random.RandomState(seed + 1013 * m + 19 * n + k)
    A = rs.randint(0, 8, size=(m, max(n, 1))).astype(np.float32)
    A[rs.rand(m, max(n, 1)) < 0.2] = 0
    W = rs.randint(1, 4, size=(m, k)).astype(np.float32)
    if m > 16:
        W[rs.rand(m) < 0.05] = 0
    _bound(W.astype(np.float64).T @ A.astype(np.float64), 1.0, np.float32, "W^T A")
    _bound(W.astype(np.float64).T @ W.astype(np.float64), 1.0, np.float32, "W^T W")
    return A, W


def dense_resid_operands(m, n, k, seed=0, whole=True, sum_dtype=np.float32):
    """W and H in {0, 1}, A = W H + R with R in 0..2: W H <= k <= 128 and A <= 130 are integers (exact in bfloat16 too), every residual
    square is at most 4 and every fp32 partial sum of squares -- of a row chunk, a column, the whole block -- stays an integer below
    2^24.  Every 32-row block of every 128-column block holds a nonzero residual.  Returns A, W, H and R (float64).
    sum_dtype: the type the kernel under test sums the squares in -- float64 for the plain kernels of csrc/dnmf_wide.hip, which square
    float32 differences (integers up to 258: exact) in float64 and add them there, so their sums stay exact up to 2^53."""
    rs = np.random.RandomState(seed + 1019 * m + 23 * n + k)
    W = (rs.rand(m, k) < 0.5).astype(np.float32)
    H = (rs.rand(k, n) < 0.5).astype(np.float32)
    R = rs.randint(0, 3, size=(m, n)).astype(np.float64)
    A = W.astype(np.float64) @ H.astype(np.float64) + R
    _bound((A ** 2).sum(0), 1.0, sum_dtype, "column sums of A^2")
    if whole:                                                       # (the per-column error sums columns only)
        _bound((R ** 2).sum(), 1.0, sum_dtype, "the residual sum")
    assert A.max() <= 256
    return A.astype(np.float32), W, H, R


def dense_update_operands(rows, k, seed=0):
    """X (rows x k) in 1..3 with some zero rows, S in 0..63, G symmetric in 2..3: the denominators X G are 0 (a zero row: the element
    stays 0) or integers in [2, 2^22) that absorb eps, the numerators are exact; transposed for the H update.  S differs from X G somewhere
    in every 16 rows, so an update that skips a tile leaves a wrong value there."""
    rs = np.random.RandomState(seed + 7 * rows + k)
    X = rs.randint(1, 4, size=(rows, k)).astype(np.float32)
    X[rs.rand(rows) < 0.05] = 0
    S = rs.randint(0, 64, size=(rows, k)).astype(np.float32)
    G = rs.randint(2, 4, size=(k, k))
    G = np.maximum(G, G.T).astype(np.float64)
    d = X.astype(np.float64) @ G
    _bound(d, 0.25, np.float32, "X G")
    assert np.all((d == 0) | (d >= 2))
    return X, S, G


# ---------------------------------------------------------------------------------------------------------- per-element comparison
def assert_ulp(got, q, c, what="", tile=(16, 32), q_hi=None):
    """|got - q| <= c * spacing(q in got's type) per element, q the float64 reference; q == 0 must be exactly 0 and c == 0 means
    bit-equal.  q_hi: the reference is only known to lie between q and q_hi (an order-dependent input such as a sum that may or may
    not absorb eps terms); got must be within c ulps of that interval.  On failure: the first bad (row, col), both bit patterns, the
    tile it falls in and whether that is an edge tile."""
    got = np.asarray(got)
    q = np.asarray(q, dtype=np.float64)
    assert got.shape == q.shape, "%s: shape %s, expected %s" % (what, got.shape, q.shape)
    ft = got.dtype.type
    g64 = got.astype(np.float64)
    lo, hi = (q, q) if q_hi is None else (np.minimum(q, q_hi), np.maximum(q, q_hi))
    if c == 0:
        bad = ~((g64 >= lo) & (g64 <= hi))
    else:
        tol = c * np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(ft)).astype(np.float64)
        bad = ~((g64 >= lo - tol) & (g64 <= hi + tol)) | ((lo == 0) & (hi == 0) & (g64 != 0))
    if not bad.any():
        return
    idx = tuple(int(i) for i in np.argwhere(bad)[0])
    it = {np.float32: np.uint32, np.float64: np.uint64}[ft]
    exp = ft(q[idx])
    where = ""
    if got.ndim == 2:
        r, col = idx
        tr, tc = r // tile[0], col // tile[1]
        last_r, last_c = (got.shape[0] - 1) // tile[0], (got.shape[1] - 1) // tile[1]
        where = " in tile (%d, %d) of (%d, %d)%s%s" % (tr, tc, last_r + 1, last_c + 1, " [last row tile]" if tr == last_r else "",
                                                      " [last column tile]" if tc == last_c else "")
    raise AssertionError("%s: %d of %d elements off by more than %g ulp; first at %s%s: got %r (0x%x), expected %r (0x%x), float64 %r"
                         % (what, int(bad.sum()), bad.size, c, idx, where, got[idx].item(), got[idx].view(it).item(),
                            exp.item(), np.array(exp).view(it).item(), q[idx]))


# ---------------------------------------------------------------------------------------------------------- poisoned views
SENTINEL = -12345.6875


class Poisoned:
    """A rows x cols view -- or a stack [B][rows][cols] of them, problem b at b rows ld -- inside a buffer: `lead` elements before it,
    pitch ld >= cols, `guard` elements after it; everything outside the view holds `fill` (NaN for operands, SENTINEL for outputs).
    aligned: lead and ld multiples of 4 (the vector paths; `quantum` elements instead of 4: 8 puts the members of a bf16 stack 16 bytes
    apart whatever the row count); otherwise an odd start and pitch (the generic paths).  packed: ld = cols (a contiguous view, for the
    entry points that require one).  ld: that pitch instead."""

    def __init__(self, torch, x, dtype=None, fill=float("nan"), aligned=True, guard=67, device="cuda", packed=False, quantum=4, ld=None):
        x = np.asarray(x)
        x3 = x if x.ndim == 3 else x[None]
        B, rows, cols = x3.shape
        self.torch = torch
        self.dtype = dtype or {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[x.dtype]
        self.lead = 8 if aligned else 3
        self.ld = cols if packed else (-(-cols // quantum) * quantum + quantum) if aligned else cols + 3
        if ld is not None:                                          # a pitch of the caller's (a column slice of a wider matrix)
            assert ld >= cols
            self.ld = ld
        self.rows, self.cols, self.fill = rows, cols, fill
        bs = rows * self.ld
        self.buf = torch.full((self.lead + B * bs + guard,), fill, dtype=self.dtype, device=device)
        v3 = self.buf.as_strided((B, rows, cols), (bs, self.ld, 1), self.lead)
        v3.copy_(torch.from_numpy(np.ascontiguousarray(x3)).to(self.dtype))
        self.view = v3 if x.ndim == 3 else v3[0]
        self.mask = np.zeros(self.buf.numel(), dtype=bool)
        self.mask[(self.lead + np.arange(B)[:, None, None] * bs + np.arange(rows)[None, :, None] * self.ld
                   + np.arange(cols)[None, None, :]).ravel()] = True

    @classmethod
    def out(cls, torch, rows, cols, dtype, aligned=True):
        npd = {torch.float32: np.float32, torch.float64: np.float64}[dtype]
        return cls(torch, np.full((rows, cols), SENTINEL, dtype=npd), dtype, fill=SENTINEL, aligned=aligned)

    def check(self, what="", allow_nan=False):
        """nothing outside the view changed; no NaN inside it (unless the case expects some: allow_nan).  Returns the view as numpy."""
        b = self.buf.float().cpu().numpy() if self.dtype == self.torch.bfloat16 else self.buf.cpu().numpy()
        out = b[~self.mask]
        ok = np.isnan(out) if np.isnan(self.fill) else out == np.asarray(self.fill, dtype=b.dtype)
        if not ok.all():
            i = int(np.flatnonzero(~self.mask)[np.argmin(ok)])
            raise AssertionError("%s: element %d of the buffer outside the view (view starts at %d, pitch %d) was written: %r"
                                 % (what, i, self.lead, self.ld, b[i]))
        v = self.view.cpu().numpy() if self.dtype != self.torch.bfloat16 else self.view.float().cpu().numpy()
        assert allow_nan or not np.isnan(v).any(), "%s: NaN inside the view at %s" % (what, tuple(np.argwhere(np.isnan(v))[0]))
        return v
