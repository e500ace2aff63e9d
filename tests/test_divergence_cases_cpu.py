"""The operands of tests/test_gpu_divergence_exact.py, checked without a GPU: the construction of every case and planting, and a numpy
statement of the reductions' arithmetic (tests/_div.py::emulate: fp32 over a cell, float64 from there on, the slots in four orders)
with every float32 within 8 ulp of ln 2 as logf(2) -- the answers of the KL and Itakura-Saito forms are exact in every order, and one
dropped, doubled or shifted position breaks them, so the GPU test cannot pass on operands that could not see the fault."""
import numpy as np
import pytest

from tests import _div as D
from tests import _is as I

CANDIDATES = D.logf2_candidates()


def _same(outs, want, what):
    for order, got in outs.items():
        assert got == want, "%s, order %s: got %r, exact %r" % (what, order, got, want)


# ---- the planted terms themselves
def test_the_planted_terms_are_exact_for_every_logf_of_two():
    """17 candidates for logf(2).  beta = 1: the planted term a L - a + s' at a = 2 S, s' = S is exactly S (2 L - 1) in float32 with the
    multiply-add contracted or not, and 2 L - 1 has at most 22 significant bits and is within 2^-20 (+ the rounding of ln 2 itself) of 2 ln 2 - 1.
    beta = 0: the term is 1 - L exactly, within 2^-21 (likewise) of 1 - ln 2.  An own value gives exactly 0 and a zero (beta = 1) exactly S"""
    assert len(CANDIDATES) == 17 and len(set(float(x) for x in CANDIDATES)) == 17 and D.LN2 in CANDIDATES
    S = np.array([2.0, 4.0, 8.0, 16.0, 32.0])
    for L in CANDIDATES:
        u = 2.0 * float(L) - 1.0
        # (the candidates are counted from float32(ln 2), itself up to half an ulp, 2^-25, from ln 2)
        assert abs(u - D.U1) <= 2.0 ** -20 + 2.0 ** -24 and abs((1.0 - float(L)) - D.T2) <= 2.0 ** -21 + 2.0 ** -25
        assert u * 2.0 ** 23 == round(u * 2.0 ** 23) and u < 0.5                                   # a multiple of 2^-23 below 2^-1
        for fma in (False, True):
            t = D.terms("kl", 2.0 * S, S, L, fma)
            assert t.dtype == np.float32 and np.array_equal(t.astype(np.float64), S * u), (L, fma)
            assert np.array_equal(D.terms("kl", S, S, L, fma), np.zeros(5, dtype=np.float32))
            assert np.array_equal(D.terms("kl", 0.0 * S, S, L, fma).astype(np.float64), S)
        t = D.terms("is", 2.0 * S, S, L)
        assert np.array_equal(t.astype(np.float64), np.full(5, 1.0 - float(L))) and np.float32(1.0 - float(L)) == 1.0 - float(L)
        assert np.array_equal(D.terms("is", S, S, L), np.zeros(5, dtype=np.float32))


# ---- the construction
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_the_construction_of_every_case(case):
    """the geometry the table states; S a power of two in [2, 32] that absorbs eps; every cells planting has at most one position per
    cell, one in every tile (so in slots 0, 255, 256 and the last), the corners and the last in-block position of the last tile; the
    seeds together hit both row halves of the cells; the zero/own plantings hold about half zeros"""
    m, n = case["shape"]
    g = D.geometry(m, n)
    assert (g["tiles"], g["last_rows"], g["last_cols"]) == (case["tiles"], case["last_rows"], case["last_cols"])
    assert g["tiles"] == -(-m // 32) * -(-n // 128) and len(case["ks"]) >= 2 and len(D.SEEDS) >= 4
    for k in case["ks"]:
        W, H, S = D.factors(m, n, k)
        assert W.dtype == np.float32 and H.dtype == np.float32 and np.array_equal(W.astype(np.float64) @ H.astype(np.float64), S)
        assert S.min() >= 2 and S.max() <= 32 and np.array_equal(np.log2(S), np.round(np.log2(S))) and len(np.unique(S)) >= 3
        assert np.array_equal(S.astype(np.float32) + np.float32(D.EPS), S.astype(np.float32))
        assert ((W > 0).sum(1) == 1).all() and W.max() <= 4 and H.min() >= 2 and H.max() <= 8
        seen_corners, halves = set(), set()
        for seed in D.SEEDS:
            plant = D.cells(S, seed)
            assert D.cell_counts(plant).max() == 1
            r, c = np.nonzero(plant)
            slots = set(D.slot_of(r, c, n).tolist())
            assert slots == set(range(g["tiles"])) and set(D.required_slots(g["tiles"])) <= slots
            here = {rc for rc in D.corners(m, n) if plant[rc]}
            assert len(here) == 4 or m <= 32 or n <= 4, (seed, here)
            assert plant[D.corners(m, n)[seed % 4]]
            seen_corners |= here
            halves |= set(((r % 32) // 16).tolist())
            A = D.planted(S, plant)
            assert np.array_equal(A[plant], 2 * S[plant]) and np.array_equal(A[~plant], S[~plant])
            _, zero, want = D.zero_own(S, seed)
            assert 0.4 < zero.mean() < 0.6 and want == int(want) and want == S[zero].sum()
        assert seen_corners == set(D.corners(m, n)) and plant[m - 1, n - 1] | (m <= 32) | (n <= 4)
        assert halves == ({0, 1} if m > 16 else {0}), halves
        A, zero, want = D.zero_own(S, None)
        assert not A.any() and zero.all() and want == S.sum()
        assert D.single(S).sum() == 1 and D.single(S)[0, 0]
    assert D.required_slots(4) == [0, 3] and D.required_slots(257) == [0, 255, 256] and D.required_slots(268) == [0, 255, 256, 267]


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_the_by_value_plantings_meet_the_share_condition(case):
    """one by-value planting per value of S present (split at MAX_PLANTED positions): positions of that value only, at most one per
    cell, and for every beta of the general form every planted term is at least 100 * BOUND of their sum R > 0"""
    m, n = case["shape"]
    for k in case["ks"]:
        S = D.factors(m, n, k)[2]
        for seed in D.SEEDS:
            launches = D.by_value(S, seed)
            assert {v for v, _ in launches} == set(np.unique(S).tolist())
            for v, plant in launches:
                assert 1 <= plant.sum() <= D.MAX_PLANTED and (S[plant] == v).all() and D.cell_counts(plant).max() == 1
                for beta in D.GEN_BETAS:
                    R, smallest = D.planted_sum(S, plant, beta)
                    assert R > 0 and smallest >= 100 * D.BOUND * R, (k, seed, v, beta, R, smallest)
            whole = np.zeros((m, n), dtype=bool)
            for v in np.unique(S):
                mine = np.zeros((m, n), dtype=bool)
                for v2, plant in launches:
                    if v2 == v:
                        assert not (mine & plant).any()
                        mine |= plant
                tiles_with_v = {D.slot_of(r, c, n) for r, c in np.argwhere(S == v)}
                assert {D.slot_of(r, c, n) for r, c in np.argwhere(mine)} == tiles_with_v                # every tile that holds the value
                whole |= mine
            assert all(whole[rc] for rc in D.corners(m, n)[seed % 4: seed % 4 + 1])                      # this seed's first corner


# ---- the arithmetic: exact in every order
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_every_position_at_once_is_exact_in_every_order(case):
    """beta = 1 on the zero/own plantings (every seed, and A = 0 everywhere): the sum of S over the zeros, an integer, in all twelve
    orders, with the multiply-add contracted or not (no term meets logf(2), so one candidate serves)"""
    m, n = case["shape"]
    for k in case["ks"]:
        S = D.factors(m, n, k)[2]
        for seed in D.SEEDS + (None,):
            A, _, want = D.zero_own(S, seed)
            for fma in (False, True):
                _same(D.emulate(D.terms("kl", A, S, D.LN2, fma)), want, "kl zero/own %dx%d k=%d seed %s" % (m, n, k, seed))


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_the_cells_plantings_are_exact_in_every_order(case):
    """every candidate for logf(2): with u1 = D(single) / S[0, 0] the KL form gives (sum of S over the planted positions) * u1 and with
    t2 = D(single) the Itakura-Saito form gives count * t2, bit for bit in all twelve orders"""
    m, n = case["shape"]
    k = case["ks"][-1]
    S = D.factors(m, n, k)[2]
    A1 = D.planted(S, D.single(S))
    plants = [D.cells(S, seed) for seed in D.SEEDS]
    for L in CANDIDATES:
        one = D.emulate(D.terms("kl", A1, S, L))
        u1 = one["forwards", "kernel"] / S[0, 0]
        _same(one, S[0, 0] * u1, "kl single")
        assert u1 == 2.0 * float(L) - 1.0
        one = D.emulate(D.terms("is", A1, S, L))
        t2 = one["forwards", "kernel"]
        _same(one, t2, "is single")
        assert t2 == 1.0 - float(L)
        for seed, plant in zip(D.SEEDS, plants if L in (CANDIDATES[0], D.LN2, CANDIDATES[-1]) else plants[:1]):
            A = D.planted(S, plant)
            for fma in (False, True):
                _same(D.emulate(D.terms("kl", A, S, L, fma)), float(S[plant].sum()) * u1, "kl cells %dx%d seed %d L %r" % (m, n, seed, L))
            _same(D.emulate(D.terms("is", A, S, L)), int(plant.sum()) * t2, "is cells %dx%d seed %d L %r" % (m, n, seed, L))


# ---- one faulty position breaks them
def _fault_positions(S, plant):
    """the corners, a planted and an unplanted position inside, and a position in the last slot"""
    m, n = S.shape
    pos = list(D.corners(m, n))
    inner = np.argwhere(plant)
    pos.append(tuple(int(x) for x in inner[len(inner) // 2]))
    pos.append(tuple(int(x) for x in np.argwhere(~plant)[(~plant).sum() // 2]))
    return sorted(set(pos))


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_one_faulty_position_breaks_the_answers(case):
    """A = 0 everywhere at beta = 1 sees EVERY position dropped or doubled (its term is S >= 2).  A position paired with a neighbour's
    model value is seen by the zero/own and by the cells plantings wherever the two model values differ -- that is the case at more
    than half of all positions, and in every tile, along the rows; the columns within a row block differ likewise unless k is so small
    that neighbouring rows share their factor row.  A dropped or doubled PLANTED position breaks the cells answers of both forms.  A
    shifted own value at beta = 1 leaves a sum that is not an integer"""
    m, n = case["shape"]
    k = case["ks"][-1]
    S = D.factors(m, n, k)[2]
    differs = np.empty((m, n), dtype=bool)
    differs[:, :-1] = S[:, 1:] != S[:, :-1]
    differs[:, -1] = differs[:, -2]                                                  # (the last column looks to its left)
    assert differs.mean() > 0.5
    assert {D.slot_of(r, c, n) for r, c in np.argwhere(differs)} == set(range(case["tiles"]))
    A0, _, want0 = D.zero_own(S, None)
    Az, zero, wantz = D.zero_own(S, 1)
    plant = D.cells(S, 1)
    Ac = D.planted(S, plant)
    L = D.LN2
    u1, t2 = 2.0 * float(L) - 1.0, 1.0 - float(L)
    want_kl, want_is = float(S[plant].sum()) * u1, int(plant.sum()) * t2
    for r, c in _fault_positions(S, plant):
        for kind in ("drop", "double"):
            assert all(got != want0 for got in D.emulate(D.with_fault("kl", A0, S, L, (kind, r, c))).values()), (kind, r, c)
            if plant[r, c]:
                assert all(got != want_kl for got in D.emulate(D.with_fault("kl", Ac, S, L, (kind, r, c))).values()), (kind, r, c)
                assert all(got != want_is for got in D.emulate(D.with_fault("is", Ac, S, L, (kind, r, c))).values()), (kind, r, c)
        for kind in ("shift", "shift_row"):
            other = S[r, c + 1 if c + 1 < n else c - 1] if kind == "shift" else S[r + 1 if r + 1 < m else r - 1, c]
            if other == S[r, c]:
                continue
            for form, A, want in (("kl", A0, want0), ("kl", Az, wantz), ("kl", Ac, want_kl), ("is", Ac, want_is)):
                outs = D.emulate(D.with_fault(form, A, S, L, (kind, r, c)))
                assert all(got != want for got in outs.values()), (kind, form, r, c)
            if not zero[r, c]:
                got = D.emulate(D.with_fault("kl", Az, S, L, (kind, r, c)))["forwards", "kernel"]
                assert got != round(got), (kind, r, c, got)
    # a shift is seen somewhere among the corners
    assert any(differs[rc] for rc in D.corners(m, n)) or m * n < 8


def test_the_near_singular_betas():
    assert len(D.NEAR_BETAS) == 12 and all(np.float32(b) == b and -2 <= b <= 4 and b not in (0.0, 1.0) for b in D.NEAR_BETAS)
    assert sorted(abs(b - round(b)) for b in D.NEAR_BETAS) == sorted([2.0 ** -4, 2.0 ** -7, 2.0 ** -10] * 4)
    assert D.NEAR_SHAPE_K[:2] in I.EXACT_SHAPES
