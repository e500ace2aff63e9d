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
    below 2^22, so eps is absorbed in every order (an integer below 2^22 is an even number of its own ulps)."""
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
        _bound(d, 0.25, np.float32, what)           # below 2^22
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
    _bound(cnt.T @ cnt, 0.25, np.float32, "H-phase denominators")                 # below 2^22 units of 2^(2a - t_g) >= 2
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
    entry points that require one)."""

    def __init__(self, torch, x, dtype=None, fill=float("nan"), aligned=True, guard=67, device="cuda", packed=False, quantum=4):
        x = np.asarray(x)
        x3 = x if x.ndim == 3 else x[None]
        B, rows, cols = x3.shape
        self.torch = torch
        self.dtype = dtype or {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[x.dtype]
        self.lead = 8 if aligned else 3
        self.ld = cols if packed else (-(-cols // quantum) * quantum + quantum) if aligned else cols + 3
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

    def check(self, what=""):
        """nothing outside the view changed; no NaN inside it.  Returns the view as numpy."""
        b = self.buf.float().cpu().numpy() if self.dtype == self.torch.bfloat16 else self.buf.cpu().numpy()
        out = b[~self.mask]
        ok = np.isnan(out) if np.isnan(self.fill) else out == np.asarray(self.fill, dtype=b.dtype)
        if not ok.all():
            i = int(np.flatnonzero(~self.mask)[np.argmin(ok)])
            raise AssertionError("%s: element %d of the buffer outside the view (view starts at %d, pitch %d) was written: %r"
                                 % (what, i, self.lead, self.ld, b[i]))
        v = self.view.cpu().numpy() if self.dtype != self.torch.bfloat16 else self.view.float().cpu().numpy()
        assert not np.isnan(v).any(), "%s: NaN inside the view at %s" % (what, tuple(np.argwhere(np.isnan(v))[0]))
        return v
