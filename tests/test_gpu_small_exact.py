"""The small whole-fit kernels (csrc/dnmf_small.h) held to exact operands over MANY steps, at every instantiation the plans can choose
(tests/_exact.py: SMALL_REACH, asserted against dnmf_small_fit_plan without a GPU by tests/test_capi_small.py).

`kl_fixed`, `fro_fixed` and `kl_moved` are fixed points of the whole MU step in fp32, in any summation order (proved by
tests/test_exact_cpu.py): after 1, 2, 3 or 11 steps -- the caller's H at step 0, the published {value, step} granules from step 1 on, the
partial slabs summed behind a barrier whose counter keeps running, the clamp again at step 10 -- the un-normalised factors are the
input, bit for bit, so what the fit returns is normalize_features of the input:
  s = colsum(W), exact (integers below 2^22 times a power of two: s + eps rounds to s);
  W / s  within 1 ulp  (ONE IEEE division, scale_cols_div; test_gpu_exact.py holds that kernel to c = 1);
  H s    within 1 ulp  (ONE product, scale_rows_mul);
  both exact (0 ulp) where s is a power of two, which `kl_fixed` / `kl_moved` guarantee;
  sq[:, 1] = sum A^2 exactly; sq[:, 0] = 0 where s is a power of two, else at most ((k + 4) 2^-24)^2 sum A^2 (W / s and H s are each
  within 2^-24 of the quotient, relatively, the k products and their sum add (k + 2) 2^-24 at most: every residual is below
  (k + 4) 2^-24 of its entry of A).
A term dropped in one column tile of one slab at one step changes a power of two by a factor: thousands of ulps, not the 2e-4 of the
largest entry that the float64 comparisons of test_gpu_fit.py allow.  The launch counters (dnmf_small_fit_launches) show that the
persistent kernel ran, not the launch chain behind it; on a few shapes the launch chain (dnmf_set_persistent(0)) is held to the same
answer.  What a fixed point cannot see: a workgroup that reads an H one step stale (except step 1 of `kl_moved`) -- the float64
comparisons over 12-31 steps stay the guard for that.  HALS (no exact fixed point: square roots, column norms): plan, counter, batched
equal to single bit for bit, and the float64 checker at the tolerance of test_gpu_fit.py."""
import ctypes
import functools

import numpy as np
import pytest

from tests import _exact as ex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
FAMILY_COUNTER = {"kl": 0, "fro": 1, "fro_bf16": 1, "kl_wfixed": None, "hals": 3, "hals_bf16": 3}     # (kl_wfixed: 2 on route 2, 0 on route 1)
GEN = {"kl": ex.kl_fixed, "fro": ex.fro_fixed, "fro_bf16": ex.fro_fixed, "kl_wfixed": ex.kl_moved}
MU = [e for e in ex.SMALL_REACH if e[0] in ("kl", "fro", "fro_bf16")]
WFIXED = [e for e in ex.SMALL_REACH if e[0] == "kl_wfixed"]
HALS = [e for e in ex.SMALL_REACH if e[0].startswith("hals")]
CHAIN = [e for e in ex.SMALL_REACH if e[1:3] in ((130, 37), (530, 21)) and not e[0].startswith("hals")]     # one shape per family and KP: k = 5 and k = 17


def _id(e):
    return "%s-%dx%d-k%d" % e[:4]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pydnmfk_amd import engine
    from pydnmfk_amd._lib import lib
    return engine, lib


def _launches(lib):
    out = (ctypes.c_ulonglong * 4)()
    assert lib.dnmf_small_fit_launches(out) == 0
    return list(out)


def _plan(lib, family, m, n, k):
    out = (ctypes.c_int * 8)()
    assert lib.dnmf_small_fit_plan(*ex.SMALL_FAMILIES[family], m, n, k, out) == 0, lib.dnmf_last_error()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _problem(family, m, n, k, seed):
    return GEN[family](m, n, k, seed=seed)


def _stacks(probs, B, adt):
    """A, W, H of B problems as [B][rows][cols] stacks (one problem: matrices) in NaN-poisoned buffers, members 16 bytes apart"""
    q = 8 if adt == torch.bfloat16 else 4
    P = [ex.Poisoned(torch, np.stack([p[i] for p in probs]) if B > 1 else probs[0][i], dtype=adt if i == 0 else None, quantum=q if i == 0 else 4)
         for i in range(3)]
    return P, tuple(x.view for x in P)


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _expected_launches(plan, B, split=False):
    """launches of one fit call: the W-fixed kernel needs no residency (one launch); a barrier or HALS kernel runs as one launch when
    the B x P workgroups of the batch fit the device at one workgroup per CU (resident_launch, csrc/dnmf_fit.hip) -- asserted, so a
    smaller device says so here instead of failing a count.  split: a batch that cannot be resident at once -- a CU holds at most 32
    waves, four 8-wave workgroups, whatever occupancy the compiler reaches -- so at least 2 launches (asserted too: a larger device says so)"""
    if split:
        assert plan[0] != 2 and plan[2] == 8 and B * plan[4] > 4 * _cus(), \
            "%d problems x %d workgroups fit the %d CUs of this device at four 8-wave workgroups each: the batch may be one launch" % (B, plan[4], _cus())
        return 2
    if plan[0] != 2:
        assert B * plan[4] <= _cus(), "%d problems x %d workgroups exceed the %d CUs of this device: the batch takes several launches" % (B, plan[4], _cus())
    return 1


def _counter(family, plan):
    return FAMILY_COUNTER[family] if family != "kl_wfixed" else (2 if plan[0] == 2 else 0)


def _run_fixed(env, family, m, n, k, plan, itr, B, persistent=True, split=False):
    """one fit of B fixed-point problems (different seeds); every check of the module docstring.  split: the batch takes several
    launches (_expected_launches gives their least number, not their number)"""
    engine, lib = env
    ops = engine.HIP_OPS
    what = "%s %dx%d k=%d itr=%d batch=%d%s" % (family, m, n, k, itr, B, "" if persistent else " (launch chain)")
    probs = [_problem(family, m, n, k, b) for b in range(B)]
    (Ap, Wp, Hp), args = _stacks(probs, B, torch.bfloat16 if family == "fro_bf16" else torch.float32)
    before = _launches(lib)
    sq = ops.fit("mu", "kl" if family.startswith("kl") else "fro", *args, EPS, family != "kl_wfixed", itr)
    after = _launches(lib)
    ops.hals_check()
    want = list(before)
    if persistent:
        want[_counter(family, plan)] += _expected_launches(plan, B, split)
    if split:
        c = _counter(family, plan)
        print("%s: %d launches" % (what, after[c] - before[c]))
        want[c] = max(want[c], after[c])
    assert after == want, "%s: launches %s -> %s, expected %s {kl, fro, W-fixed, hals} (%d CUs)" % (what, before, after, want, _cus())
    Ap.check(what + " A")
    w3, h3 = Wp.check(what + " W"), Hp.check(what + " H")
    if B == 1:
        w3, h3 = w3[None], h3[None]
    sq = sq.cpu().numpy()
    for b, (A, W, H) in enumerate(probs):
        A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
        if family == "kl_wfixed":
            H64 = 2 * H64                                                    # step 0 doubles H, every later step keeps it
        s = W64.sum(0)
        pow2 = bool(np.all(np.frexp(s)[0] == 0.5))
        assert pow2 or family.startswith("fro")
        c = 0 if pow2 else 1
        ex.assert_ulp(w3[b], W64 / s[None, :], c, "%s [%d] W = W / colsum(W)" % (what, b))
        ex.assert_ulp(h3[b], H64 * s[:, None], c, "%s [%d] H = H colsum(W)" % (what, b))
        sa = float((A64 ** 2).sum())
        assert sq[b, 1] == sa, "%s [%d]: sum A^2 is %r, expected %r" % (what, b, sq[b, 1], sa)
        lim = 0.0 if pow2 else ((k + 4) * 2.0 ** -24) ** 2 * sa
        assert 0.0 <= sq[b, 0] <= lim, "%s [%d]: sum (A - W H)^2 is %r, at most %r expected" % (what, b, sq[b, 0], lim)


@pytest.mark.parametrize("B", [1, 3], ids=["single", "batch3"])
@pytest.mark.parametrize("itr", [1, 2, 3, 11])
@pytest.mark.parametrize("entry", MU, ids=_id)
def test_mu_fixed_points(env, entry, itr, B):
    """every MU/KL and MU/FRO instantiation (fp32 and bf16-stored A) returns a fixed point of the step after 1, 2, 3 and 11 steps"""
    family, m, n, k, plan = entry
    assert _plan(env[1], family, m, n, k) == plan
    _run_fixed(env, family, m, n, k, plan, itr, B)


@pytest.mark.parametrize("B", [1, 3], ids=["single", "batch3"])
@pytest.mark.parametrize("itr", [1, 2, 11])
@pytest.mark.parametrize("entry", WFIXED, ids=_id)
def test_kl_w_fixed_moves_once(env, entry, itr, B):
    """MU/KL with W fixed on `kl_moved` (A = 2 W H): H doubles at step 0 and stays -- on the W-fixed kernel and on the barrier kernel
    with w_update = 0, where step 1 is the first to read the granules instead of the caller's H"""
    family, m, n, k, plan = entry
    assert _plan(env[1], family, m, n, k) == plan
    _run_fixed(env, family, m, n, k, plan, itr, B)


@pytest.mark.parametrize("entry", CHAIN, ids=_id)
def test_launch_chain_agrees_on_the_fixed_points(env, entry):
    """the same operands through the per-step kernels (dnmf_set_persistent(0)): mu_quot, the fused KL step and the IEEE divisions are
    exact there too, so the two routes are held to ONE answer -- and no persistent kernel is counted"""
    family, m, n, k, plan = entry
    was = env[1].dnmf_set_persistent(0)
    try:
        for itr in (1, 3, 11):
            _run_fixed(env, family, m, n, k, plan, itr, 3, persistent=False)
    finally:
        env[1].dnmf_set_persistent(was)


@pytest.mark.parametrize("entry", HALS, ids=_id)
def test_hals_reach(env, entry):
    """every HALS geometry, A streamed as fp32, resident as bf16, streamed as bf16: the plan, the counter, finite factors, a batch of 3
    equal to single fits bit for bit, and the checker's loop in float64 at the tolerance of tests/test_gpu_fit.py (1e-3 of the largest entry)"""
    from tests.test_gpu_fit import _checker_fit_f64, _close
    engine, lib = env
    ops = engine.HIP_OPS
    family, m, n, k, plan = entry
    assert _plan(lib, family, m, n, k) == plan
    itr, B = 11, 3
    adt = torch.bfloat16 if family == "hals_bf16" else torch.float32
    # the random data of tests/test_gpu_fit.py (zero columns at odd seeds) wherever the float64 loop is well-conditioned, rank-k data at the
    # four shapes where it is not (tests/_exact.py: hals_problem; both statements proved by tests/test_exact_cpu.py)
    probs = [ex.hals_problem(m, n, k, seed) for seed in ex.HALS_SEEDS]
    before = _launches(lib)
    (Ap, Wp, Hp), args = _stacks(probs, B, adt)
    ops.fit("hals", "fro", *args, EPS, True, itr)
    ops.hals_check()
    singles = []
    for b in range(B):
        P1, a1 = _stacks(probs[b:b + 1], 1, adt)
        ops.fit("hals", "fro", *a1, EPS, True, itr)
        ops.hals_check()
        singles.append(P1)
    want = list(before)
    want[3] += (1 + B) * _expected_launches(plan, B)
    assert _launches(lib) == want, "launches %s -> %s, expected %s" % (before, _launches(lib), want)
    Ap.check("A")
    w3, h3 = Wp.check("W"), Hp.check("H")
    assert np.isfinite(w3).all() and np.isfinite(h3).all()
    for b in range(B):
        w1, h1 = singles[b][1].check("single W"), singles[b][2].check("single H")
        assert np.array_equal(w3[b].view(np.uint32), w1.view(np.uint32)) and np.array_equal(h3[b].view(np.uint32), h1.view(np.uint32)), \
            "problem %d of the batch differs from its single fit" % b
        A, W, H = (torch.from_numpy(x).cuda() for x in probs[b])
        Wr, Hr = _checker_fit_f64(A.to(adt), W, H, itr, True, "fro", "hals")
        for X, Y, name in ((w3[b], Wr, "W"), (h3[b], Hr, "H")):
            X = torch.from_numpy(X).cuda()
            print("%s %dx%d k=%d [%d] %s: max |x - f64| = %.3e of max %.3e" % (family, m, n, k, b, name, float((X.double() - Y).abs().max()), float(Y.abs().max())))
            assert _close(X, Y, 1e-3), (b, name, float((X.double() - Y).abs().max()), float(Y.abs().max()))
    assert not np.array_equal(w3[0], w3[1])


@pytest.mark.parametrize("family", ["kl", "hals"])
def test_batch_split_over_several_launches(env, family):
    """a batch that resident_launch cannot keep resident at once runs as several launches, the later ones with z0 > 0: 17 problems of
    8191 x 20, k = 3 (P = 64 workgroups of 8 waves each; 11 MB of data).  MU/KL: every problem is held to its fixed point; HALS: every
    problem of the batch equals its single fit bit for bit.  The family's counter grows by at least 2, no other counter moves."""
    engine, lib = env
    ops = engine.HIP_OPS
    m, n, k, B = 8191, 20, 3, 17
    plan, = [e[4] for e in ex.SMALL_REACH if e[:4] == (family, m, n, k)]
    assert plan[2] == 8 and plan[4] == 64 and _plan(lib, family, m, n, k) == plan
    assert B * 64 > 4 * _cus(), "17 problems x 64 workgroups fit the %d CUs of this device at four 8-wave workgroups each: no split to test" % _cus()
    if family == "kl":
        for itr in (1, 3):
            _run_fixed(env, family, m, n, k, plan, itr, B, split=True)
        return
    itr = 3
    probs = [ex.hals_problem(m, n, k, seed) for seed in range(10, 10 + B)]
    before = _launches(lib)
    (Ap, Wp, Hp), args = _stacks(probs, B, torch.float32)
    ops.fit("hals", "fro", *args, EPS, True, itr)
    ops.hals_check()
    after = _launches(lib)
    print("hals %dx%d k=%d itr=%d batch=%d: %d launches" % (m, n, k, itr, B, after[3] - before[3]))
    assert after[3] - before[3] >= _expected_launches(plan, B, split=True) and after[:3] == before[:3], "launches %s -> %s" % (before, after)
    Ap.check("A")
    w3, h3 = Wp.check("W"), Hp.check("H")
    assert np.isfinite(w3).all() and np.isfinite(h3).all()
    for b in range(B):
        P1, a1 = _stacks(probs[b:b + 1], 1, torch.float32)
        ops.fit("hals", "fro", *a1, EPS, True, itr)
        ops.hals_check()
        w1, h1 = P1[1].check("single W"), P1[2].check("single H")
        assert np.array_equal(w3[b].view(np.uint32), w1.view(np.uint32)) and np.array_equal(h3[b].view(np.uint32), h1.view(np.uint32)), \
            "problem %d of the batch differs from its single fit" % b
    assert _launches(lib)[3] == after[3] + B
    assert not np.array_equal(w3[0], w3[16])
