"""Per-entry weights on the MI355X (csrc/dnmf_weighted.h): 0/1 weights against the unweighted entry points bit for bit, `a` unread under a
zero weight, exact operands, general weights against float64 (tests/_weighted.py), PyNMF with params.weights."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _exact as E  # noqa: E402
from tests import _is as I  # noqa: E402
from tests import _weighted as Wt  # noqa: E402
from tests._golden import rel_fro  # noqa: E402

EPS = I.EPS
BOUND = 1e-5                       # pairs and updates of every pair rule (tests/test_gpu_beta.py); the multiply by v adds one rounding
FIT_BOUND, ERR_BOUND = 1e-4, 1e-5  # a fit against float64: the factors, the error (the existing bounds)
# (shape, k, what dnmf_weighted_plan must say it reaches, twice at least): a second column split (generic, and FAST with tiles to refill
# under the quarter MFMAs), a short last chunk of row blocks (k = 32: the two-group H walk over more than one block), the ending's second trip
LOOP_CASES = (((70, 2085), 64, "nsplit"), ((68, 2084), 64, "nsplit"), ((2130, 70), 64, "nchunks"), ((2130, 70), 32, "nchunks"),
              ((16400, 41), 128, "w_reduce_trips"))
CASES = [(s, k, None) for s in I.EXACT_SHAPES for k in I.EXACT_KS] + list(LOOP_CASES)
LAYOUTS = ("contiguous", "odd views")
ONES_NORMS = (("is", 0.0), ("beta", 0.5), ("beta", 3.0))
_ID = lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v)      # noqa: E731


def _ops():
    from pydnmfk_amd.engine import HIP_OPS
    return HIP_OPS


def _problem(m, n, k):
    """A, V, W, H: the random problem of tests/test_gpu_beta.py with weights in [0.25, 4), a quarter of them zero"""
    from tests.test_gpu_beta import _random_problem
    A, W, H = _random_problem(m, n, k)
    return A, Wt.weights((m, n), m + n + k, 0.25), W, H


def _both_sides(call, arrays, k, layout, allow_nan=()):
    """call(side, *views, num, den) for both sides on `layout` inside NaN poison -> [num_w, den_w, num_h, den_h]; the poison is intact"""
    kw = {"packed": True} if layout == "contiguous" else {"aligned": False}
    ps = [E.Poisoned(torch, x, **kw) for x in arrays]
    m, n = arrays[0].shape
    out = []
    for side, (r, c) in (("w", (m, k)), ("h", (k, n))):
        num, den = (E.Poisoned.out(torch, r, c, torch.float32, aligned=layout != "odd views") for _ in range(2))
        call(side, *(p.view for p in ps), num.view, den.view)
        out += [num.check(side + " num"), den.check(side + " den")]
    for i, (p, x) in enumerate(zip(ps, arrays)):
        assert np.array_equal(p.check("operand %d" % i, allow_nan=i in allow_nan), x, equal_nan=True)
    return out


def _weighted_pairs(A, V, W, H, norm, beta, layout):
    return _both_sides(lambda side, a, v, w, h, num, den: _ops().weighted_pair_into(side, a, v, w, h, EPS, norm, beta, num, den),
                       (A, V, W, H), W.shape[1], layout, allow_nan=(0,))


def _updates(fn_w, fn_h, arrays, W, H):
    """(new W, new H with the clamp) from the same W, H, on contiguous device copies"""
    t = [torch.from_numpy(x).cuda() for x in arrays]
    W1, H1 = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
    fn_w(*t, W1, torch.from_numpy(H).cuda())
    fn_h(*t, torch.from_numpy(W).cuda(), H1)
    return W1, H1


# ---- 1. 0/1 weights are the masked path; all-ones weights the unweighted Itakura-Saito / beta path
def _twin(norm, beta):
    """the unweighted entry points of the norm on (a, w, h): pair_into, update_w, update_h (clamped), fit"""
    from pydnmfk_amd.engine import HIP_MASKED_OPS as M
    from pydnmfk_amd.masked import MaskedDenseBlock as Blk
    mode = (beta,) if norm == "beta" else ()
    if norm in ("fro", "kl"):
        return (lambda s, a, w, h, nu, de: M.masked_pair_into(s, Blk(a), w, h, EPS, norm, nu, de), lambda a, w, h: M.masked_update_w(Blk(a), w, h, EPS, norm),
                lambda a, w, h: M.masked_update_h(Blk(a), w, h, EPS, norm, clamp=True), lambda a, w, h, itr: M.fit("mu", norm, Blk(a), w, h, EPS, True, itr))
    f = lambda name: getattr(_ops(), norm + "_" + name)      # noqa: E731
    return (lambda s, a, w, h, nu, de: f("pair_into")(s, a, w, h, EPS, *mode, nu, de), lambda a, w, h: f("update_w")(a, w, h, EPS, *mode),
            lambda a, w, h: f("update_h")(a, w, h, EPS, *mode, clamp=True), lambda a, w, h, itr: f("fit")(a, w, h, EPS, *mode, True, itr))


def _twin_data(norm, A, V):
    """(data, weights): NaN at the zeros of 0/1 weights for the masked twins (fro, kl), all-ones weights for is / beta"""
    V01 = (V > 0).astype(np.float32)
    return (np.where(V01 > 0, A, np.float32(np.nan)), V01) if norm in ("fro", "kl") else (A, np.ones_like(A))


@pytest.mark.parametrize("shape,k,reach", CASES, ids=_ID)
def test_zero_one_weights_are_the_unweighted_kernels_bit_for_bit(shape, k, reach):
    from pydnmfk_amd._lib import lib
    ops, (m, n) = _ops(), shape
    A, V, W, H = _problem(m, n, k)
    for code in range(4 if reach else 0):
        out = (ctypes.c_long * 8)()
        assert lib.dnmf_weighted_plan(m, n, k, code, out) == 0
        p = I.plan_reach(m, n, k, out)
        assert p[reach] >= 2 and (reach != "nchunks" or 1 <= p["last_chunk_blks"] < p["rowblks_per_chunk"]), (code, p)
    for norm, beta in (("fro", 0.0), ("kl", 0.0)) + ONES_NORMS:
        pair, upd_w, upd_h, _ = _twin(norm, beta)
        D, Vt = _twin_data(norm, A, V)
        for layout in LAYOUTS:
            got = _weighted_pairs(D, Vt, W, H, norm, beta, layout)
            for g, r, what in zip(got, _both_sides(pair, (D, W, H), k, layout, allow_nan=(0,)), ("num_w", "den_w", "num_h", "den_h")):
                assert np.array_equal(g, r), (norm, beta, layout, what)
        got = _updates(lambda a, v, w, h: ops.weighted_update_w(a, v, w, h, EPS, norm, beta),
                       lambda a, v, w, h: ops.weighted_update_h(a, v, w, h, EPS, norm, beta, clamp=True), (D, Vt), W, H)
        ref = _updates(upd_w, upd_h, (D,), W, H)                                    # the fused endings
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (norm, beta)


@pytest.mark.parametrize("itr", [1, 11])
def test_the_whole_fit_with_zero_one_weights_is_the_unweighted_whole_fit(itr):
    A, V, W, H = _problem(130, 97, 32)
    for norm, beta in (("fro", 0.0), ("kl", 0.0)) + ONES_NORMS:
        a, v, w, h, a2, w2, h2 = (torch.from_numpy(x).cuda() for x in _twin_data(norm, A, V) + (W, H, _twin_data(norm, A, V)[0], W, H))
        _ops().weighted_fit(a, v, w, h, EPS, norm, beta, True, itr)
        _twin(norm, beta)[3](a2, w2, h2, itr)
        assert torch.equal(w, w2) and torch.equal(h, h2), (norm, beta, itr)


# ---- 2. `a` is not read where v = 0
@pytest.mark.parametrize("norm,beta", (("fro", 0.0), ("kl", 0.0), ("is", 0.0), ("beta", 0.5)), ids=lambda v: str(v))
def test_data_under_a_zero_weight_are_not_read(norm, beta):
    A, V, W, H = _problem(130, 97, 32)
    ref = _weighted_pairs(np.where(V > 0, A, np.float32(1.0)), V, W, H, norm, beta, "odd views")
    for planted in (np.nan, np.inf, 0.0, -1.0):
        got = _weighted_pairs(np.where(V > 0, A, np.float32(planted)), V, W, H, norm, beta, "odd views")
        for g, r in zip(got, ref):
            assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), (norm, planted)


# ---- 3. exact operands: every S a power of two, weights powers of two in [2^-3, 2^3] with 25 % zeros
@pytest.mark.parametrize("shape,k", [(s, k) for s in I.EXACT_SHAPES for k in I.EXACT_KS], ids=_ID)
def test_exact_operands_with_power_of_two_weights(shape, k):
    A, W, H, _ = I.exact_problem(shape[0], shape[1], k)
    V = Wt.weights(shape, shape[0] + k, 0.25, pow2=True)
    for norm, beta in (("fro", 0.0), ("beta", 2.0)):
        ref = Wt.pair(A, V, W, H, "w", norm, beta, eps=0.0) + Wt.pair(A, V, W, H, "h", norm, beta, eps=0.0)     # (eps is absorbed by every S)
        for layout in LAYOUTS:
            got = _weighted_pairs(A, V, W, H, norm, beta, layout)
            for g, r, what in zip(got, ref, ("num_w", "den_w", "num_h", "den_h")):
                assert np.array_equal(g.astype(np.float64), r), (norm, layout, what, int((g != r).sum()))


# ---- 4. general weights against float64
@pytest.mark.parametrize("shape,k", [c[:2] for c in CASES], ids=_ID)
def test_general_weights_against_float64(shape, k):
    ops = _ops()
    A, V, W, H = _problem(shape[0], shape[1], k)
    An = np.where(V > 0, A, np.float32(np.nan))
    t = [torch.from_numpy(x).cuda() for x in (An, V)]
    worst = {}
    for norm, beta in (("fro", 0.0), ("kl", 0.0), ("is", 0.0), ("beta", -2.0), ("beta", 0.5), ("beta", 1.5), ("beta", 4.0)):
        ref = Wt.pair(A, V, W, H, "w", norm, beta) + Wt.pair(A, V, W, H, "h", norm, beta)
        for layout in LAYOUTS:
            got = _weighted_pairs(An, V, W, H, norm, beta, layout)
            worst["pair"] = max(worst.get("pair", 0.0), max(rel_fro(g, r) for g, r in zip(got, ref)))
        W1, H1 = _updates(lambda a, v, w, h: ops.weighted_update_w(a, v, w, h, EPS, norm, beta),
                          lambda a, v, w, h: ops.weighted_update_h(a, v, w, h, EPS, norm, beta, clamp=True), (An, V), W, H)
        worst["update"] = max(worst.get("update", 0.0), rel_fro(W1.cpu().numpy(), Wt.rule(W, ref[0], ref[1], norm, beta)),
                              rel_fro(H1.cpu().numpy(), Wt.rule(H, ref[2], ref[3], norm, beta, clamp=True)))
        w, h = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
        terms = Wt.terms(A, V, W, H, norm, beta)
        div = float(ops.weighted_divergence(*t, w, h, EPS, norm, beta).cpu())
        assert div == float(ops.weighted_divergence(*t, w, h, EPS, norm, beta).cpu())                       # stored, fixed order
        worst["divergence"] = max(worst.get("divergence", 0.0), abs(div - sum(x.sum() for x in terms)) / sum(np.abs(x).sum() for x in terms))
    sq, (r0, r1) = ops.weighted_resid_sqnorm(*t, w, h).cpu().numpy(), Wt.resid(A, V, W, H)
    S = W.astype(np.float64) @ H.astype(np.float64)
    scale = float(np.sum(V * (A.astype(np.float64) ** 2 + 2 * A * S + S ** 2)))
    worst["resid"] = max(abs(sq[0] - r0) / scale, abs(sq[1] - r1) / r1)
    print("weighted %dx%d k=%d maxima against float64:" % (shape + (k,)), {k_: "%.2e" % v for k_, v in sorted(worst.items())})
    assert max(worst.values()) <= BOUND, worst


# ---- 5. PyNMF with params.weights
def _pynmf(A, V, W0, H0, k, itr, norm, beta, **kw):
    from pydnmfk_amd.pyDNMF import PyNMF
    d = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in (A, W0, H0)]
    return PyNMF(d[0], factors=d[1:], params=Wt.args(k, itr, norm, beta, weights=V.astype(np.float32), **kw))


def test_the_step_loop_is_the_one_call_fit_bit_for_bit():
    A, V, W0, H0, k = Wt.problem(300, 200, 4, seed=3)
    one, loop = _pynmf(A, V, W0, H0, k, 30, "beta", 0.5), _pynmf(A, V, W0, H0, k, 30, "beta", 0.5, fit_loop="python")
    assert one._whole_fit_ok(one._ops()) and not loop._whole_fit_ok(loop._ops())
    (W1, H1, e1), (W2, H2, e2) = one.fit(), loop.fit()
    assert torch.equal(W1, W2) and torch.equal(H1, H2) and e1 == e2 and one.weighted_divergence() == loop.weighted_divergence()


@pytest.mark.parametrize("norm,beta", Wt.NORMS, ids=lambda v: str(v))
def test_a_fit_against_float64(norm, beta):
    A, V, W0, H0, k = Wt.problem(200, 136, 5, seed=2)
    A32, W32, H32 = (x.astype(np.float32).astype(np.float64) for x in (A, W0, H0))
    nmf = _pynmf(A, V, W0, H0, k, 30, norm, beta)
    W, H, err = nmf.fit()
    Wr, Hr, err_r = Wt.fit(A32, V, W32, H32, norm, beta, 30)
    d = (rel_fro(W.cpu().numpy(), Wr), rel_fro(H.cpu().numpy(), Hr), abs(err - err_r) / err_r)
    print("weighted fit %s beta=%g against float64: dW=%.2e dH=%.2e derr=%.2e" % ((norm, beta) + d))
    assert d[0] <= FIT_BOUND and d[1] <= FIT_BOUND and d[2] <= ERR_BOUND, d


@pytest.mark.parametrize("grid", [(2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_grids_against_the_float64_statement(grid):
    """both ranks on the one GPU; the replicated factor is bit-identical across the ranks (run_grid asserts it)"""
    for key, d in Wt.run_grid(grid, use_hip=True, timeout=300).items():
        print("weighted gpu grid %dx%d" % grid, "%s beta=%g" % key, "dW=%.2e dH=%.2e derr=%.2e dobj=%.2e" % d)
        assert d[0] <= FIT_BOUND and d[1] <= FIT_BOUND and d[2] <= ERR_BOUND, (grid, key, d)


def test_main_norm_is_with_weights_end_to_end(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    A, V, W0, H0, k = Wt.problem(200, 136, 5, seed=2)
    np.save(tmp_path / "spectra.npy", A.astype(np.float32))
    np.save(tmp_path / "sigma.npy", V.astype(np.float32))
    cmd = [sys.executable, os.path.join(root, "main.py"), "--process=pyDNMF", "--p_r=1", "--p_c=1", "--fpath=%s/" % tmp_path, "--fname=spectra",
           "--ftype=npy", "--weights=sigma", "--k=5", "--itr=30", "--norm=is", "--method=mu", "--results_path=%s/res/" % tmp_path]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    err = float(out.stdout.strip().split("relative error =")[-1])
    W, H = np.load(tmp_path / "res" / "W_factors" / "W_0.npy"), np.load(tmp_path / "res" / "H_factors" / "H_0.npy")
    assert W.shape == (200, 5) and H.shape == (5, 136) and np.isfinite(W).all() and np.isfinite(H).all()
    r = Wt.resid(A, V, W, H)
    assert abs(np.sqrt(r[0] / r[1]) - err) < 1e-4
