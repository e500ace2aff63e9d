"""The two scalar divergence reductions on the GPU -- tile_sum_kernel<KT, FAST, BetaDivTerm<FORM, 1>>
(csrc/dnmf_sums.h) behind both entry points, ended by slot_sum_kernel -- through HIP_OPS.is_divergence and HIP_OPS.beta_divergence on planted exact
operands (tests/_div.py; tests/test_divergence_cases_cpu.py shows that the answers are exact in every order and that one faulty
position breaks them), tile by tile:

  1. beta = 1, zero/own plantings: the divergence IS the sum of S over the zeros, an integer -- every position at once;
  2. beta = 1, cells plantings: (sum of S over the planted positions) * u1, u1 = D(single) / S[0, 0] a float32 within 2^-20 of 2 ln 2 - 1;
  3. beta = 0 in both kernels, cells plantings: count * t2, t2 = D(single) a float32 within 2^-21 of 1 - ln 2, the kernels bit-equal;
  4. the general form at beta in {-2, -1, 0.5, 1.5, 2, 3, 4}, by differences of two launches against float64 within 1e-5;
  5. beta within 2^-4, 2^-7, 2^-10 of the singular points 0 and 1 on random data, within 1e-5 of the magnitudes of the terms.

Shapes (tests/_div.py::CASES): two column blocks with both edges ragged, generic and through the vector loads; a 3 x 3 grid of tiles
whose last workgroup has one live wave; the shapes of the pair tests; 257, 258 and 268 tiles (the sum kernel's second trip: one slot,
a row of column blocks, both indices).  Every case on views in NaN and in finite-huge poison, aligned and at an odd base and pitch
(the cases beyond 256 tiles: aligned and odd in NaN poison); operands and poison unchanged; two calls bit-identical.

Measured (one MI355X): this file prints every figure before it asserts."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _beta as B  # noqa: E402
from tests import _div as D  # noqa: E402
from tests import _exact as E  # noqa: E402

EPS = D.EPS
BOUND = D.BOUND


def _ops():
    from pydnmfk_amd.engine import HIP_OPS
    return HIP_OPS


def _tag(case, k, aligned, fill):
    return "%dx%d k=%d %s %s" % (case["shape"] + (k, "aligned" if aligned else "odd", "nan" if np.isnan(fill) else "huge"))


def _put(x, aligned, fill):
    p = E.Poisoned(torch, x, aligned=aligned, fill=fill)
    if not aligned:
        assert p.view.data_ptr() % 16 and p.ld == p.cols + 3
    return p


def _unchanged(p, x, what):
    """nothing outside the view was written (NaN or finite-huge poison) and the view holds what was put there"""
    assert np.array_equal(p.check(what), x), what


def _factors_on(case, k, aligned, fill):
    """(W, H, S, poisoned W, poisoned H) of a case whose geometry is the one its table entry states; FAST (asserted at every launch's
    views, _put_a): the vector kernels exactly when bases, pitches, n and k are multiples of four elements"""
    m, n = case["shape"]
    g = D.geometry(m, n)
    assert (g["tiles"], g["last_rows"], g["last_cols"]) == (case["tiles"], case["last_rows"], case["last_cols"])
    W, H, S = D.factors(m, n, k)
    Wp, Hp = _put(W, aligned, fill), _put(H, aligned, fill)
    return W, H, S, Wp, Hp


def _put_a(case, k, A, Wp, Hp, aligned, fill):
    """A on its view, and the FAST assertion on the three views of the launch"""
    Ap = _put(A, aligned, fill)
    fast = all(p.view.data_ptr() % 16 == 0 and p.ld % 4 == 0 for p in (Ap, Wp, Hp)) and Ap.cols % 4 == 0 and k % 4 == 0
    assert fast == (aligned and case["fast"] and k % 4 == 0), _tag(case, k, aligned, fill)
    return Ap


def _twice(call, what):
    """the value of two bit-identical calls"""
    d1, d2 = call().cpu().numpy(), call().cpu().numpy()
    assert d1.dtype == np.float64 and d1.shape == (1,) and np.array_equal(d1.view(np.int64), d2.view(np.int64)), (what, d1, d2)
    return float(d1[0])


def _beta_div(Ap, Wp, Hp, beta, what):
    return _twice(lambda: _ops().beta_divergence(Ap.view, Wp.view, Hp.view, EPS, beta), what)


def _is_div(Ap, Wp, Hp, what):
    return _twice(lambda: _ops().is_divergence(Ap.view, Wp.view, Hp.view, EPS), what)


def _is_float32(x):
    return float(np.float64(np.float32(x))) == x


# ---- 1. beta = 1: every position at once
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_kl_form_counts_every_position_exactly_once(case):
    """A is 0 or S at every position (four seeds, and 0 everywhere): beta_divergence(., 1.0) equals the sum of S over the zeros -- a zero
    gives the term s' = S, an own value a / s' = 1, logf 1 = 0 and the term 0, each fp32 partial is a sum of at most 64 integers <= 32.
    A position missed, counted twice, read from the poison or paired with another position's s' gives another number"""
    for k in case["ks"]:
        for aligned, fill in case["layouts"]:
            W, H, S, Wp, Hp = _factors_on(case, k, aligned, fill)
            for seed in D.SEEDS + (None,):
                A, zero, want = D.zero_own(S, seed)
                Ap = _put_a(case, k, A, Wp, Hp, aligned, fill)
                tag = "%s seed %s" % (_tag(case, k, aligned, fill), seed)
                got = _beta_div(Ap, Wp, Hp, 1.0, tag)
                assert got == want, "%s: got %r, the sum of S over the %d zeros is %r (difference %r)" % (tag, got, zero.sum(), want, got - want)
                _unchanged(Ap, A, tag + " A")
            _unchanged(Wp, W, "W")
            _unchanged(Hp, H, "H")


# ---- 2. beta = 1: the logarithm branch
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_kl_form_logarithm_branch_on_the_cells_plantings(case):
    """A = S but A = 2 S at one position per cell at most: u1 = D(single) / S[0, 0] is a float32 within 2^-20 of 2 ln 2 - 1 (eight ulp of
    logf, doubled), and D equals (the sum of S over the planted positions) * u1 bit for bit, for four seeds"""
    for k in case["ks"]:
        for aligned, fill in case["layouts"]:
            W, H, S, Wp, Hp = _factors_on(case, k, aligned, fill)
            tag = _tag(case, k, aligned, fill)
            A1 = D.planted(S, D.single(S))
            u1 = _beta_div(_put_a(case, k, A1, Wp, Hp, aligned, fill), Wp, Hp, 1.0, tag) / S[0, 0]
            print("%s: u1 = %r, %.3g from 2 ln 2 - 1" % (tag, u1, u1 - D.U1))
            assert _is_float32(u1) and abs(u1 - D.U1) <= 2.0 ** -20, (tag, u1)
            for seed in D.SEEDS:
                plant = D.cells(S, seed)
                A = D.planted(S, plant)
                Ap = _put_a(case, k, A, Wp, Hp, aligned, fill)
                got, want = _beta_div(Ap, Wp, Hp, 1.0, tag), float(S[plant].sum()) * u1
                assert got == want, "%s seed %d: got %r, %r * u1 is %r (difference %r)" % (tag, seed, got, S[plant].sum(), want, got - want)
                _unchanged(Ap, A, tag + " A")
            _unchanged(Wp, W, "W")
            _unchanged(Hp, H, "H")


# ---- 3. beta = 0 in both kernels
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_is_form_counts_the_planted_positions_in_both_kernels(case):
    """the same plantings: with t2 = D(single), a float32 within 2^-21 of 1 - ln 2, is_divergence and beta_divergence(., 0.0) both
    give count * t2 bit for bit, and each other's bits"""
    for k in case["ks"]:
        for aligned, fill in case["layouts"]:
            W, H, S, Wp, Hp = _factors_on(case, k, aligned, fill)
            tag = _tag(case, k, aligned, fill)
            A1p = _put_a(case, k, D.planted(S, D.single(S)), Wp, Hp, aligned, fill)
            t2 = _is_div(A1p, Wp, Hp, tag)
            print("%s: t2 = %r, %.3g from 1 - ln 2" % (tag, t2, t2 - D.T2))
            assert _is_float32(t2) and abs(t2 - D.T2) <= 2.0 ** -21, (tag, t2)
            assert _beta_div(A1p, Wp, Hp, 0.0, tag) == t2, tag
            for seed in D.SEEDS:
                plant = D.cells(S, seed)
                A = D.planted(S, plant)
                Ap = _put_a(case, k, A, Wp, Hp, aligned, fill)
                want = int(plant.sum()) * t2
                for which, got in (("is_divergence", _is_div(Ap, Wp, Hp, tag)), ("beta_divergence(0)", _beta_div(Ap, Wp, Hp, 0.0, tag))):
                    assert got == want, "%s seed %d %s: got %r, %d * t2 is %r (difference %r)" % (tag, seed, which, got, plant.sum(), want, got - want)
                _unchanged(Ap, A, tag + " A")
            _unchanged(Wp, W, "W")
            _unchanged(Hp, H, "H")


# ---- 4. the general form, by differences
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_general_form_by_differences(case):
    """beta in {-2, -1, 0.5, 1.5, 2, 3, 4}: D0 from A = S, D1 from a by-value planting (all planted terms of a launch equal, at most
    MAX_PLANTED of them, so each is at least 100 * BOUND of their float64 sum R -- asserted in tests/test_divergence_cases_cpu.py; the
    own-value terms of the float64 statement are below 1e-13 of R) and |(D1 - D0) - R| <= BOUND * R: the lanes without a planted
    position give identical partials in both launches, a lane with one adds it with at most 64 fp32 roundings (3.8e-6), the term's own
    error is below 2e-6 (the model at the top of tests/test_gpu_beta.py).  The four seeds are shared out among the layouts.  Whether D0
    is exactly 0 at the integer betas is printed, not asserted (exp2f / log2f at powers of two are not documented)"""
    worst, zero_d0 = (0.0, ""), {}
    layouts = case["layouts"]
    for k in case["ks"]:
        for li, (aligned, fill) in enumerate(layouts):
            W, H, S, Wp, Hp = _factors_on(case, k, aligned, fill)
            tag = _tag(case, k, aligned, fill)
            A0 = D.planted(S, np.zeros(S.shape, dtype=bool))
            A0p = _put_a(case, k, A0, Wp, Hp, aligned, fill)
            D0 = {beta: _beta_div(A0p, Wp, Hp, beta, tag) for beta in D.GEN_BETAS}
            for beta in D.GEN_BETAS:
                if beta == int(beta):
                    zero_d0.setdefault(beta, []).append(D0[beta] == 0.0)
            _unchanged(A0p, A0, tag + " A0")
            for seed in D.SEEDS[li::len(layouts)]:
                for v, plant in D.by_value(S, seed):
                    A = D.planted(S, plant)
                    Ap = _put_a(case, k, A, Wp, Hp, aligned, fill)
                    for beta in D.GEN_BETAS:
                        R, smallest = D.planted_sum(S, plant, beta)
                        assert smallest >= 100 * BOUND * R > 0
                        D1 = _beta_div(Ap, Wp, Hp, beta, tag)
                        d = abs((D1 - D0[beta]) - R) / R
                        worst = max(worst, (d, "beta=%g S=%g %s seed %d (%d planted, D0 %.3g)" % (beta, v, tag, seed, plant.sum(), D0[beta])))
                        assert d <= BOUND, "%s beta=%g S=%g seed %d: D1 - D0 = %r, R = %r, off by %.3e of R" % (tag, beta, v, seed, D1 - D0[beta], R, d)
                    _unchanged(Ap, A, tag + " A")
            _unchanged(Wp, W, "W")
            _unchanged(Hp, H, "H")
    print("general form %dx%d: largest |(D1 - D0) - R| / R = %.2e at %s" % (case["shape"] + worst))
    print("general form %dx%d: D0 (A = S) exactly 0 at integer beta: %s"
          % (case["shape"] + ({b: "%d of %d launches" % (sum(z), len(z)) for b, z in sorted(zero_d0.items())},)))


# ---- 5. near the singular points
@pytest.mark.parametrize("beta", D.NEAR_BETAS, ids=lambda b: "beta=%r" % b)
def test_general_form_near_the_singular_points(beta):
    """the random problem of tests/test_gpu_beta.py at 130 x 97, k = 32 (A with exact zeros for beta > 0, positive for beta < 0), beta
    within 2^-4, 2^-7 and 2^-10 of 1 and of 0, where c = 1 / (beta (beta - 1)) grows to about 1024: within BOUND of the sum of the
    magnitudes of the terms, on the four layouts; the error relative to the divergence itself is printed"""
    from tests.test_gpu_beta import _random_problem, _with_zeros
    m, n, k = D.NEAR_SHAPE_K
    A0, W, H = _random_problem(m, n, k)
    A = _with_zeros(A0) if beta > 0 else A0
    assert beta > 0 or (A > 0).all()
    ref, scale = B.divergence(A, W, H, beta), B.divergence_scale(A, W, H, beta)
    worst = (0.0, 0.0)
    for aligned, fill in D.LAYOUTS:
        Ap, Wp, Hp = (_put(x, aligned, fill) for x in (A, W, H))
        got = _beta_div(Ap, Wp, Hp, beta, "beta=%r" % beta)
        worst = max(worst, (abs(got - ref) / scale, abs(got - ref) / abs(ref)))
        for p, x in ((Ap, A), (Wp, W), (Hp, H)):
            _unchanged(p, x, "beta=%r" % beta)
    print("beta=%-14r c=%9.2f D=%.9g: off by %.2e of the magnitudes of its terms, %.2e of itself" % (beta, 1.0 / (beta * (beta - 1.0)), ref, *worst))
    assert worst[0] <= BOUND, (beta, worst)
