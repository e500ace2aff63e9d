"""Operands for the two scalar divergence reductions, tile_sum_kernel (csrc/dnmf_sums.h) behind dnmf_is_divergence and dnmf_beta_divergence, which share
slot_sum_kernel (TEST INFRASTRUCTURE, lives under tests/ only).

Both give a wave one 32 x 128 tile of the block (tile gw = row block * ncolblk + column block, its sum in slot gw of the workspace); a
lane adds the terms of 16 rows by 4 contiguous columns in fp32; everything after that is float64.  Nothing here encodes which rows a
lane holds: the unit is the CELL, a 32-row block by an aligned group of 4 columns, which bounds what one fp32 partial can see.

Factors: tests/_is.py::exact_factors -- every S = W H is a power of two in [2, 32] whose float32 image absorbs eps.  A is S with a
PLANTING:
    zero/own   every entry 0 or S.  At beta = 1 a zero gives the term s' = S and an own value a / s' = 1, log 1 = 0, term 0: the divergence
               is the sum of S over the zeros, an integer, and EVERY position is seen -- one that is missed, counted twice, read from
               padding or paired with another position's s' changes it (the last one to a non-integer).
    cells      A = S but at most one position per cell where A = 2 S.  The planted term is S (2 L - 1) at beta = 1 and 1 - L at beta = 0
               (L = logf(2)), every other term 0: each fp32 partial is 0 or ONE term and the float64 sums are exact in any order.
    single     A = S but A[0, 0] = 2 S[0, 0]: measures the one term on the machine.
    by value   a cells planting among the positions where S is one given value, in launches of at most MAX_PLANTED positions: all planted
               terms of a launch are equal, so each is at least 1 / MAX_PLANTED of their sum (the general form, by differences).
`emulate` states the reductions' arithmetic in numpy (fp32 over a cell, float64 from there on, the slots in several orders) for
tests/test_divergence_cases_cpu.py, which shows that the answers are exact in every order and that one faulty position breaks them.
"""
import numpy as np

from tests import _beta as B
from tests import _is as I

EPS = I.EPS
BOUND = 1e-5                                    # the project's bound (tests/test_gpu_beta.py)
HUGE = 3.0e38                                   # finite poison: read as data it would swamp any sum
SEEDS = (0, 1, 2, 3)
GEN_BETAS = (-2.0, -1.0, 0.5, 1.5, 2.0, 3.0, 4.0)
NEAR_BETAS = tuple(b0 + s * 2.0 ** -e for b0 in (1.0, 0.0) for e in (4, 7, 10) for s in (1, -1))
NEAR_SHAPE_K = (130, 97, 32)
MAX_PLANTED = 500                               # half of 1 / (100 * BOUND): every planted term of a launch is 200 * BOUND of their sum or more
LAYOUTS = ((True, float("nan")), (True, HUGE), (False, float("nan")), (False, HUGE))       # (aligned, poison)
BIG_LAYOUTS = (LAYOUTS[0], LAYOUTS[2])


def _cdiv(a, b):
    return -(-a // b)


def _case(shape, tiles, last_rows, last_cols, ks=I.EXACT_KS, layouts=LAYOUTS):
    """fast: the FAST kernels on aligned views at k % 4 == 0 (n a multiple of four).  last_rows, last_cols: of the last tile"""
    return {"shape": shape, "ks": ks, "tiles": tiles, "last_rows": last_rows, "last_cols": last_cols, "layouts": layouts,
            "fast": shape[1] % 4 == 0}


CASES = (
    _case((33, 131), 4, 1, 3),                                          # ncolblk = 2, both edges ragged, never FAST
    _case((36, 132), 4, 4, 4),                                          # the same through the vector loads
    _case((70, 300), 9, 6, 44),                                         # gw % 3, gw / 3, a last workgroup with one live wave
    _case((130, 97), 5, 2, 97), _case((257, 70), 9, 1, 70), _case((132, 96), 5, 4, 96),       # I.EXACT_SHAPES: one column block
    _case((8200, 9), 257, 8, 9, ks=(3, 128), layouts=BIG_LAYOUTS),      # slot 256 alone in the sum's second trip
    _case((5, 32900), 258, 5, 4, ks=(128, 3), layouts=BIG_LAYOUTS),     # 258 column blocks; FAST at k = 128, generic at k = 3
    _case((2130, 500), 268, 18, 116, ks=(32, 64), layouts=BIG_LAYOUTS),  # both indices move
)
assert tuple(c["shape"] for c in CASES[3:6]) == I.EXACT_SHAPES


def case_id(case):
    return "%dx%d" % case["shape"]


def geometry(m, n):
    """what the kernels derive from the shape: row blocks, column blocks, tiles, rows and columns of the last tile, 4-column groups"""
    nrb, ncb = _cdiv(m, 32), _cdiv(n, 128)
    return {"nrowblk": nrb, "ncolblk": ncb, "tiles": nrb * ncb, "last_rows": m - 32 * (nrb - 1), "last_cols": n - 128 * (ncb - 1),
            "ncolgrp": _cdiv(n, 4)}


def slot_of(r, c, n):
    return (r // 32) * _cdiv(n, 128) + c // 128


def required_slots(tiles):
    """the first slot, the ends of the sum kernel's first trip, the start of its second, the last slot -- where they exist"""
    return sorted({s for s in (0, 255, 256, tiles - 1) if s < tiles})


def corners(m, n):
    return ((0, 0), (0, n - 1), (m - 1, 0), (m - 1, n - 1))


# ---- factors
_FACTORS = {}


def factors(m, n, k):
    """(W, H float32, S float64), built once per process and shared: no test writes to them"""
    if (m, n, k) not in _FACTORS:
        W, H, S = I.exact_factors(np.random.RandomState(17 * m + 5 * n + 3 * k + 2), m, n, k)
        assert set(np.unique(S)) <= {2.0, 4.0, 8.0, 16.0, 32.0}
        _FACTORS[(m, n, k)] = (W.astype(np.float32), H.astype(np.float32), S)
    return _FACTORS[(m, n, k)]


def _f32(A):
    A32 = A.astype(np.float32)
    assert np.array_equal(A32.astype(np.float64), A)
    return A32


# ---- plantings
def zero_own(S, seed):
    """(A, zero, expected): each entry independently 0 or S; seed None: A = 0 everywhere.  expected = the sum of S over the zeros"""
    m, n = S.shape
    zero = np.ones((m, n), dtype=bool) if seed is None else np.random.RandomState(1000 * seed + 7 * m + 3 * n + 3).rand(m, n) < 0.5
    return _f32(np.where(zero, 0.0, S)), zero, float(S[zero].sum())


def cells(S, seed, allowed=None, p=0.5):
    """a boolean m x n planting with at most one position per cell: first the four corners (in an order that turns with the seed --
    where two of them share a cell, m <= 32 or n <= 4, the later one gives way, and the seeds together plant all four), then with
    probability p one random position of every other cell, then one in every tile that is still empty.  allowed: only there"""
    m, n = S.shape
    g = geometry(m, n)
    nrb, ncg, ncb = g["nrowblk"], g["ncolgrp"], g["ncolblk"]
    rs = np.random.RandomState(1000 * seed + 7 * m + 3 * n + 1)
    allowed = np.ones((m, n), dtype=bool) if allowed is None else allowed
    plant = np.zeros((m, n), dtype=bool)
    taken = np.zeros((nrb, ncg), dtype=bool)

    def put(r, c):
        if allowed[r, c] and not taken[r // 32, c // 4]:
            plant[r, c] = taken[r // 32, c // 4] = True

    cs = corners(m, n)
    for i in range(4):
        put(*cs[(i + seed) % 4])
    rows_in = np.minimum(32, m - 32 * np.arange(nrb))[:, None]
    cols_in = np.minimum(4, n - 4 * np.arange(ncg))[None, :]
    rr = 32 * np.arange(nrb)[:, None] + (rs.rand(nrb, ncg) * rows_in).astype(np.int64)
    cc = 4 * np.arange(ncg)[None, :] + (rs.rand(nrb, ncg) * cols_in).astype(np.int64)
    pick = (rs.rand(nrb, ncg) < p) & ~taken & allowed[rr, cc]
    plant[rr[pick], cc[pick]] = True
    taken |= pick
    for rb in range(nrb):
        for cb in range(ncb):
            tile = (slice(32 * rb, min(32 * rb + 32, m)), slice(128 * cb, min(128 * cb + 128, n)))
            if plant[tile].any():
                continue
            free = np.argwhere(allowed[tile] & ~np.repeat(taken[rb, 32 * cb: 32 * cb + 32], 4)[None, : tile[1].stop - tile[1].start])
            if len(free):
                r, c = free[rs.randint(len(free))]
                put(32 * rb + int(r), 128 * cb + int(c))
    assert cell_counts(plant).max() <= 1
    return plant


def cell_counts(plant):
    """planted positions per cell, [nrowblk][ncolgrp]"""
    m, n = plant.shape
    return np.pad(plant, ((0, (-m) % 32), (0, (-n) % 4))).reshape(_cdiv(m, 32), 32, _cdiv(n, 4), 4).sum(axis=(1, 3))


def planted(S, plant):
    """A = 2 S at the planted positions, S elsewhere"""
    return _f32(np.where(plant, 2.0 * S, S))


def single(S):
    plant = np.zeros(S.shape, dtype=bool)
    plant[0, 0] = True
    return plant


def by_value(S, seed):
    """[(value, planting)]: for every value of S a cells planting among its positions, split into launches of at most MAX_PLANTED"""
    out = []
    for v in np.unique(S):
        pos = np.argwhere(cells(S, seed, allowed=(S == v)))
        for i in range(0, len(pos), MAX_PLANTED):
            plant = np.zeros(S.shape, dtype=bool)
            plant[tuple(pos[i: i + MAX_PLANTED].T)] = True
            out.append((float(v), plant))
    return out


def planted_sum(S, plant, beta):
    """R: the float64 sum of the planted positions' terms d_beta(2 s | s + eps) (the statement of tests/_beta.py), and the smallest of them"""
    t = sum(B.terms_of(2.0 * S[plant], S[plant] + EPS, beta))
    return float(t.sum()), float(t.min())


# ---- the reductions' arithmetic in numpy
LN2 = np.float32(np.log(2.0))
T2, U1 = 1.0 - np.log(2.0), 2.0 * np.log(2.0) - 1.0              # the planted terms (beta = 0; beta = 1 per unit of S) in float64


def logf2_candidates(ulps=8):
    """every float32 within `ulps` ulp of ln 2: what logf(2) may return"""
    out = [LN2]
    lo = hi = LN2
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(1))
        out += [lo, hi]
    return sorted(out)


def _logf(q, L):
    """float32 log with logf(1) = 0 and logf(2) = L (q > 0)"""
    with np.errstate(divide="ignore"):
        lg = np.log(q.astype(np.float64)).astype(np.float32)
    return np.where(q == 2, np.float32(L), np.where(q == 1, np.float32(0), lg))


def terms(form, A, Sp, L, fma=False):
    """the float32 term of every position as the kernels compute it ('kl': a > 0 ? a logf(a / s') - a + s' : s', with the multiply-add
    contracted or not; 'is': q = a * (1 / s'), (q - 1) - logf(q)), A and Sp float32, logf(2) = L"""
    A, Sp = A.astype(np.float32), Sp.astype(np.float32)
    one = np.float32(1)
    if form == "is":
        q = A * (one / Sp)
        return (q - one) - _logf(q, L)
    assert form == "kl"
    pos = A > 0
    lg = _logf(np.where(pos, A, one) / Sp, L)
    if fma:
        t = (A.astype(np.float64) * lg.astype(np.float64) - A.astype(np.float64)).astype(np.float32)         # exact, then one rounding
    else:
        t = A * lg - A
    return np.where(pos, t + Sp, Sp)


def with_fault(form, A, S, L, fault, fma=False):
    """the terms with ONE faulty position (kind, r, c): 'drop' (not added), 'double' (added twice), 'shift' (paired with the model value
    of the position to its right, or to its left in the last column), 'shift_row' (of the row below, or above in the last row)"""
    kind, r, c = fault
    Sp = S.astype(np.float32).copy()
    m, n = S.shape
    if kind == "shift":
        Sp[r, c] = S[r, c + 1 if c + 1 < n else c - 1]
    elif kind == "shift_row":
        Sp[r, c] = S[r + 1 if r + 1 < m else r - 1, c]
    T = terms(form, A, Sp, L, fma)
    if kind == "drop":
        T[r, c] = 0
    elif kind == "double":
        T[r, c] = T[r, c] + T[r, c]
    return T


def emulate(T, seed=0):
    """{order: total} of the float32 terms T: a fp32 partial per cell (its 128 positions added forwards, backwards or in a random
    order; padding adds nothing), a tile's 32 cell partials and then the slots in float64 -- the slots forwards, backwards, in a random
    order, and as slot_sum_kernel does (thread t adds the slots t, t + 256, ..., then a tree over the 256 sums)"""
    m, n = T.shape
    g = geometry(m, n)
    nrb, ncb = g["nrowblk"], g["ncolblk"]
    Tp = np.pad(T.astype(np.float32), ((0, 32 * nrb - m), (0, 128 * ncb - n)))
    cell = Tp.reshape(nrb, 32, ncb, 32, 4).transpose(0, 2, 3, 1, 4).reshape(nrb * ncb, 32, 128)             # [slot][cell][position]
    rs = np.random.RandomState(seed + m + n)
    out = {}
    for name, order in (("forwards", np.arange(128)), ("backwards", np.arange(128)[::-1]), ("random", rs.permutation(128))):
        part = np.zeros(cell.shape[:2], dtype=np.float32)
        for i in order:
            part = part + cell[:, :, i]
        assert part.dtype == np.float32
        slots = np.cumsum(part.astype(np.float64), axis=1)[:, -1]
        nslots = len(slots)
        out[name, "forwards"] = float(np.cumsum(slots)[-1])
        out[name, "backwards"] = float(np.cumsum(slots[::-1])[-1])
        out[name, "random"] = float(np.cumsum(slots[rs.permutation(nslots)])[-1])
        sh = np.zeros(256)
        for i in range(0, nslots, 256):                                    # the trips of the sum kernel's loop
            trip = slots[i: i + 256]
            sh[: len(trip)] += trip
        w = 128
        while w >= 1:
            sh[:w] += sh[w: 2 * w]
            w //= 2
        out[name, "kernel"] = float(sh[0])
    return out
