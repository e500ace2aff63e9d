"""The beta-divergence (`params.norm = 'beta'`) on the GPU (csrc/dnmf_beta.h through engine.HipOps): pairs, updates and the divergence
against the float64 statement of tests/_beta.py on contiguous tensors and on views of NaN-poisoned buffers, for beta over the whole
accepted range; exact operands element by element at beta = 2 at every loop of the launch geometry; the whole fit against the Python
step loop, bit for bit; a fit and the divergence along it against float64; beta = 0 and beta = 1 against what exists; 1D grids with the
ranks stacked on the one GPU; main.py.

Measured maxima (one MI355X; also in DESIGN.md section 7): see the table there -- this file prints every figure before it asserts."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _beta as B  # noqa: E402
from tests import _exact as E  # noqa: E402
from tests import _is as I  # noqa: E402
from tests._golden import rel_fro  # noqa: E402

EPS = B.EPS
# The project's bound for the pairs and updates of every pair rule: 1e-5 in relative Frobenius norm.  Error model of the element-wise
# step p = exp2(e * log2 s): the relative error of p is about ln 2 times the absolute error of e * log2 s.  With correctly rounded
# float32 log2 / exp2 and S in [0.05, 200] that is at most 1.3e-6 (measured on the CPU in float32 for beta = -1, 0.5, 1.5, 3, 4; largest
# at beta = -1); the one-instruction v_log_f32 / v_exp_f32 of the kernel are 1 ulp each, which adds (1 + |e|) ulp(log2 s) to the
# argument: a few 1e-7 more per element, before the averaging of the second products.
BOUND = 1e-5
# a fit against float64 (the bounds of the Itakura-Saito and masked fits): the factors to 1e-4, the error to 1e-5
FIT_BOUND, ERR_BOUND = 1e-4, 1e-5
BETAS = B.GPU_BETAS


def _ops():
    from pydnmfk_amd.engine import HIP_OPS
    return HIP_OPS


def _rel(got, ref):
    return float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))


_PROBLEMS = {}


def _random_problem(m, n, k):
    """A in [0.05, 1.05), factors in [0.01, 1.01) (H three times that at k >= 64): S = W H runs from about 0.01 at k = 3 to about 100 at
    k = 128.  Built once per shape and shared: no test writes to it"""
    if (m, n, k) not in _PROBLEMS:
        rs = np.random.RandomState(11 * m + 3 * n + k)
        _PROBLEMS[(m, n, k)] = ((rs.rand(m, n) + 0.05).astype(np.float32), (rs.rand(m, k) + 0.01).astype(np.float32),
                                (rs.rand(k, n) * (3.0 if k >= 64 else 1.0) + 0.01).astype(np.float32))
    return _PROBLEMS[(m, n, k)]


def _with_zeros(A):
    """a copy with every 29th entry an exact zero: legal data for beta > 0"""
    A = A.copy()
    A.reshape(-1)[::29] = 0.0
    return A


def _expected(A, W, H, beta):
    """float64: both pairs, both updated factors (each from the SAME W, H), the divergence and the sum of the magnitudes of its terms"""
    (nw, dw), (nh, dh) = B.pair(A, W, H, "w", beta), B.pair(A, W, H, "h", beta)
    return {"pairs": (nw, dw, nh, dh), "W": B.rule(W, nw, dw, beta), "H": B.rule(H, nh, dh, beta),
            "div": B.divergence(A, W, H, beta), "scale": B.divergence_scale(A, W, H, beta)}


# ---- 1. pairs, updates and divergence against float64
@pytest.mark.parametrize("shape", I.EXACT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_beta_kernels_against_float64(shape):
    """random A, W, H at k = 3, 32, 64, 128 and beta in {-2, -1, 0.5, 1, 1.5, 2, 3, 4} (A with exact zeros for beta > 0): on contiguous
    tensors, on 16-byte aligned padded views and on views with an odd start and pitch, all inside NaN-poisoned buffers -- the poison
    survives, every output is finite, pairs and updates are within BOUND of float64 in relative Frobenius norm, and the divergence
    within BOUND of the sum of the magnitudes of its terms (what its per-term error scales with; the error relative to the divergence
    itself is printed, without a threshold)"""
    ops = _ops()
    m, n = shape
    worst = {}
    for k in I.EXACT_KS:
        A0, W, H = _random_problem(m, n, k)
        for beta in BETAS:
            A = _with_zeros(A0) if beta > 0 else A0
            exp = _expected(A, W, H, beta)
            for layout in ("contiguous", "aligned views", "odd views"):
                kw = {"packed": True} if layout == "contiguous" else {"aligned": layout == "aligned views"}
                Ap, Wp, Hp = (E.Poisoned(torch, x, **kw) for x in (A, W, H))
                assert Ap.view.is_contiguous() == (layout == "contiguous")
                outs = [E.Poisoned.out(torch, r, c, torch.float32, aligned=layout != "odd views") for r, c in ((m, k), (m, k), (k, n), (k, n))]
                ops.beta_pair_into("w", Ap.view, Wp.view, Hp.view, EPS, beta, outs[0].view, outs[1].view)
                ops.beta_pair_into("h", Ap.view, Wp.view, Hp.view, EPS, beta, outs[2].view, outs[3].view)
                got = [o.check("%s k=%d beta=%g %s" % (layout, k, beta, what)) for o, what in zip(outs, ("num_w", "den_w", "num_h", "den_h"))]
                d = [_rel(g, r) for g, r in zip(got, exp["pairs"])]
                div = float(ops.beta_divergence(Ap.view, Wp.view, Hp.view, EPS, beta).cpu())
                dd, dd_rel = abs(div - exp["div"]) / exp["scale"], abs(div - exp["div"]) / exp["div"]
                assert float(ops.beta_divergence(Ap.view, Wp.view, Hp.view, EPS, beta).cpu()) == div             # stored, fixed order
                # the fused endings and the stand-alone rule, each from the same W, H
                W1, H1, H2, W3, H3 = (E.Poisoned(torch, x, **kw) for x in (W, H, H, W, H))
                ops.beta_update_w(Ap.view, W1.view, Hp.view, EPS, beta)
                ops.beta_update_h(Ap.view, Wp.view, H1.view, EPS, beta)
                ops.beta_update_h(Ap.view, Wp.view, H2.view, EPS, beta, clamp=True)
                ops.beta_ratio_update(W3.view, outs[0].view, outs[1].view, EPS, beta)
                ops.beta_ratio_update(H3.view, outs[2].view, outs[3].view, EPS, beta, clamp=True)
                du = [_rel(W1.check("W1"), exp["W"]), _rel(H1.check("H1"), exp["H"]), _rel(H2.check("H2"), np.maximum(exp["H"], EPS)),
                      _rel(W3.check("W3"), exp["W"]), _rel(H3.check("H3"), np.maximum(exp["H"], EPS))]
                assert np.array_equal(W1.check(), W3.check()) and np.array_equal(H2.check(), H3.check())       # one function, one result
                for p_, what in ((Ap, "A"), (Wp, "W"), (Hp, "H")):                                             # operands: not written
                    assert np.array_equal(p_.check(what), {"A": A, "W": W, "H": H}[what])
                print("beta=%4g %dx%d k=%3d %-14s W: num %.2e den %.2e | H: num %.2e den %.2e | updates %.2e | divergence %.2e of its "
                      "terms, %.2e of itself" % (beta, m, n, k, layout, *d, max(du), dd, dd_rel))
                for key, val in (("pair", max(d)), ("update", max(du)), ("divergence / terms", dd), ("divergence / itself", dd_rel)):
                    worst[key] = max(worst.get(key, (0.0, 0.0)), (val, beta))
                assert max(d) <= BOUND and max(du) <= BOUND and dd <= BOUND, (shape, k, beta, layout, d, du, dd)
    print("beta %dx%d maxima (value, at beta):" % shape, {k_: "%.2e at %g" % v for k_, v in sorted(worst.items())})


def test_a_quotient_of_zero_gives_zero():
    """the rule on a stored pair whose numerator holds zeros (and a zero over a zero denominator): 0^gamma is 0 for every gamma, the
    clamp lifts it to eps, nothing is NaN"""
    ops = _ops()
    num = torch.tensor([[0.0, 2.0, 0.0], [3.0, 0.0, 1.0]], device="cuda")
    den = torch.tensor([[1.0, 4.0, 0.0], [6.0, 2.0, 1.0]], device="cuda")
    for beta in BETAS:
        X = torch.full((2, 3), 5.0, device="cuda")
        ops.beta_ratio_update(X, num, den, EPS, beta)
        ref = B.rule(np.full((2, 3), 5.0), num.cpu().numpy(), den.cpu().numpy(), beta)
        got = X.cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got == 0, num.cpu().numpy() == 0) and _rel(got, ref) <= BOUND, (beta, got)
        ops.beta_ratio_update(X, num, den, EPS, beta, clamp=True)
        assert float(X.min()) == np.float32(EPS)


# ---- 2. exact operands at beta = 2, element by element
def _exact_pairs(A, W, H, k, beta, aligned=True):
    ops = _ops()
    m, n = A.shape
    Ap, Wp, Hp = (E.Poisoned(torch, x, aligned=aligned) for x in (A, W, H))
    out = []
    for side, (r, c) in (("w", (m, k)), ("h", (k, n))):
        num, den = E.Poisoned.out(torch, r, c, torch.float32, aligned=aligned), E.Poisoned.out(torch, r, c, torch.float32, aligned=aligned)
        ops.beta_pair_into(side, Ap.view, Wp.view, Hp.view, EPS, beta, num.view, den.view)
        out += [num.check("beta %s num k=%d" % (side, k)), den.check("beta %s den k=%d" % (side, k))]     # (nothing outside the outputs)
    for p_ in (Ap, Wp, Hp):
        assert np.isnan(p_.buf.cpu().numpy()[~p_.mask]).all()
    fast = all(p_.view.data_ptr() % 16 == 0 and p_.ld % 4 == 0 for p_ in (Ap, Wp, Hp)) and n % 4 == 0 and k % 4 == 0
    return out, fast


def _differences(shape, k, beta, aligned=True):
    """(where the pairs differ from the exact answers: one line per output, FAST, the pairs) -- and two calls are bit-identical"""
    m, n = shape
    A, W, H, ref = B.exact_problem(m, n, k, beta)
    got, fast = _exact_pairs(A, W, H, k, beta, aligned)
    bad = []
    for g, r, what in zip(got, ref["w"] + ref["h"], ("num_w", "den_w", "num_h", "den_h")):
        diff = np.argwhere(g.astype(np.float64) != r)
        if len(diff):
            i = tuple(int(x) for x in diff[0])
            bad.append("beta=%g exact %dx%d k=%d %s: %d of %d elements differ; first at %s: got %r, exact %r"
                       % (beta, m, n, k, what, len(diff), g.size, i, g[i].item(), r[i].item()))
    again, _ = _exact_pairs(A, W, H, k, beta, aligned)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (shape, k, beta, "second call differs")
    return bad, fast, got


@pytest.mark.parametrize("shape", I.EXACT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_beta_two_exact_operands(shape):
    """tests/_beta.py::exact at beta = 2 (every S a power of two >= 2 that absorbs eps, A in 1..7; e = 0, so p = exp2(0) = 1, u_n = a and
    u_d = s): num and den of both sides equal the float64 answers element by element, on padded views in poisoned buffers; (132, 96)
    takes the 16-byte vector kernels at k % 4 == 0, and (130, 97) once more on views with an odd start and pitch"""
    for k in I.EXACT_KS:
        bad, fast, _ = _differences(shape, k, 2.0)
        assert not bad, bad
        assert fast == (shape[1] % 4 == 0 and k % 4 == 0)
    if shape == (130, 97):
        for k in I.EXACT_KS:
            bad, fast, _ = _differences(shape, k, 2.0, aligned=False)
            assert not bad and not fast, bad


@pytest.mark.parametrize("case", I.EXACT_LOOP_CASES, ids=lambda c: "%dx%d" % c["shape"])
def test_beta_two_exact_operands_in_the_loops(case):
    """the same at the smallest shapes whose launch plan (dnmf_beta_plan, asserted here and in tests/test_capi_beta.py) gives a
    workgroup of the W side three tiles with a ragged last one, a wave of the H side two row blocks and the last chunk one, and the
    ending a second grid-stride trip -- generic and 16-byte vector kernels; each pair twice, bit-identical"""
    import ctypes
    from pydnmfk_amd._lib import lib
    m, n = case["shape"]
    for k in case["ks"]:
        out = (ctypes.c_long * 8)()
        assert lib.dnmf_beta_plan(m, n, k, out) == 0
        p = I.plan_reach(m, n, k, out)
        for what, want in case["reach"].items():
            assert p[what] == want, (case["shape"], k, what, p[what], want)
        bad, fast, _ = _differences(case["shape"], k, 2.0)
        assert not bad, bad
        assert fast == (case["fast"] and k % 4 == 0), (case["shape"], k)


@pytest.mark.parametrize("beta", [1.0, 3.0], ids=lambda b: "beta=%g" % b)
def test_integer_beta_on_power_of_two_operands_is_recorded(beta):
    """integer beta != 2 with every S a power of two: P = S^(beta - 2) is a power of two and the answers are exact in float32 IF v_log_f32
    and v_exp_f32 are exact at powers of two and at small integers, which is not documented.  Recorded (printed), not asserted; the
    pairs stay within BOUND of the exact answers"""
    for shape in I.EXACT_SHAPES:
        for k in I.EXACT_KS:
            bad, _, got = _differences(shape, k, beta)
            print("beta=%g %dx%d k=%d on power-of-two S: %s" % (beta, shape[0], shape[1], k, "exact, element by element" if not bad else "; ".join(bad)))
            ref = B.exact_problem(shape[0], shape[1], k, beta)[3]
            assert max(_rel(g, r) for g, r in zip(got, ref["w"] + ref["h"])) <= BOUND


# ---- 3. fits on one rank
def _fit_problem():
    A, W0, H0, k = I.problem(200, 136, 5, seed=9)
    return A.astype(np.float32), W0.astype(np.float32), H0.astype(np.float32), k


def _pynmf(A, W0, H0, k, itr, beta, **kw):
    from pydnmfk_amd.pyDNMF import PyNMF
    return PyNMF(torch.from_numpy(A).cuda(), factors=[torch.from_numpy(W0).cuda(), torch.from_numpy(H0).cuda()],
                 params=B.one_rank_args(k, itr, beta, **kw))


def _whole_fit_problem(m, n, k):
    rs = np.random.RandomState(m + n + k)
    A = ((rs.rand(m, k) + 0.1) @ (rs.rand(k, n) + 0.1) * rs.gamma(4.0, 0.25, size=(m, n)) / k).astype(np.float32)
    return np.maximum(A, 1e-3), (rs.rand(m, k) + 0.05).astype(np.float32), (rs.rand(k, n) + 0.05).astype(np.float32)


@pytest.mark.parametrize("wu", [True, False], ids=["W_update", "W_fixed"])
@pytest.mark.parametrize("beta", [0.5, 3.0], ids=lambda b: "beta=%g" % b)
@pytest.mark.parametrize("shape_k", [(300, 200, 4), (130, 97, 32)], ids=lambda s: "%dx%d-k%d" % s)
def test_whole_fit_equals_the_python_step_loop_bit_for_bit(shape_k, beta, wu):
    """dnmf_beta_mu_fit through PyNMF against params.fit_loop = 'python' (the same launches, sequenced from Python): torch.equal on W
    and H after 1, 11 and 30 steps (one, two and three clamps); a second whole fit is bit-identical"""
    m, n, k = shape_k
    A, W0, H0 = _whole_fit_problem(m, n, k)
    for itr in (1, 11, 30):
        whole = _pynmf(A, W0, H0, k, itr, beta, W_update=wu)
        assert whole._whole_fit_ok(whole._ops()) and whole._ops().name == "hip" and whole.norm == "beta"
        loop = _pynmf(A, W0, H0, k, itr, beta, W_update=wu, fit_loop="python")
        assert not loop._whole_fit_ok(loop._ops())
        (W1, H1, e1), (W2, H2, e2), (W3, H3, e3) = whole.fit(), loop.fit(), _pynmf(A, W0, H0, k, itr, beta, W_update=wu).fit()
        assert torch.equal(W1, W2) and torch.equal(H1, H2) and torch.equal(W1, W3) and torch.equal(H1, H3), (shape_k, beta, wu, itr)
        assert torch.isfinite(W1).all() and torch.isfinite(H1).all() and abs(e1 - e2) <= 1e-12 and abs(e1 - e3) <= 1e-12
        assert not torch.equal(H1, torch.from_numpy(H0).cuda())
    if not wu:
        ops = _ops()
        Wn = torch.from_numpy(W0).cuda()
        s = ops.colsum(Wn, ops.zeros((k,), Wn))
        ops.scale_cols_div(Wn, s, EPS)
        assert torch.equal(W1, Wn)                                                  # the whole fit: W0 normalised, nothing else


@pytest.mark.parametrize("beta", [0.5, 1.5, 3.0], ids=lambda b: "beta=%g" % b)
def test_thirty_step_fit_against_float64(beta):
    """200 x 136, k = 5, gamma noise, 30 steps: factors within 1e-4 and the error within 1e-5 of the float64 statement (the bounds of the
    Itakura-Saito and masked fits); the divergence of the fitted factors within 1e-5 of the magnitudes of its terms"""
    A, W0, H0, k = _fit_problem()
    nmf = _pynmf(A, W0, H0, k, 30, beta)
    W, H, err = nmf.fit()
    Wr, Hr, err_r = B.fit(A, W0, H0, beta, 30)
    dw, dh, de = rel_fro(W.cpu().numpy(), Wr), rel_fro(H.cpu().numpy(), Hr), abs(err - err_r) / err_r
    div, div_r, scale = nmf.beta_divergence(), B.divergence(A, Wr, Hr, beta), B.divergence_scale(A, Wr, Hr, beta)
    print("beta=%g fit 200x136 k=5, 30 steps against float64: dW=%.2e dH=%.2e derr=%.2e ddiv=%.2e of its terms, %.2e of itself (err %.6g, D %.6g)"
          % (beta, dw, dh, de, abs(div - div_r) / scale, abs(div - div_r) / div_r, err_r, div_r))
    assert dw <= FIT_BOUND and dh <= FIT_BOUND and de <= ERR_BOUND and abs(div - div_r) <= BOUND * scale


@pytest.mark.parametrize("beta", [0.5, 3.0], ids=lambda b: "beta=%g" % b)
def test_the_divergence_never_rises_along_the_python_loop(beta):
    """beta_divergence() after each of 30 steps of the Python loop: consecutive values, compared in float64, never rise by more than
    1e-6 of their own value.  The check binds only while the float64 statement's own per-step decrease exceeds that slack: its smallest
    decrease on THIS problem is computed and printed, and must exceed the slack at all 30 steps"""
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    A, W0, H0, k = _fit_problem()
    slack = 1e-6
    W, H = W0.astype(np.float64), H0.astype(np.float64)
    ref = [B.divergence(A, W, H, beta)]
    for i in range(30):
        W, H = B.step(A, W, H, beta, EPS, True, clamp=(i % 10 == 0))
        ref.append(B.divergence(A, W, H, beta))
    drop = -np.diff(ref) / np.array(ref[:-1])
    print("beta=%g divergence (float64): %.6g -> %.6g, smallest relative decrease per step %.3e" % (beta, ref[0], ref[-1], drop.min()))
    assert drop.min() > slack, drop
    nmf = _pynmf(A, W0, H0, k, 30, beta, fit_loop="python")
    d = [nmf.beta_divergence()]
    for i in range(30):
        nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update(clamp=(i % 10 == 0))
        d.append(nmf.beta_divergence())
        assert d[-1] <= d[-2] * (1.0 + slack), (i, d[-2], d[-1])
        assert abs(d[-1] - ref[i + 1]) <= 1e-4 * ref[i + 1], (i, d[-1], ref[i + 1])
    print("beta=%g divergence (gpu):     %.6g -> %.6g, largest relative change per step %.3e" % (beta, d[0], d[-1], (np.diff(d) / np.array(d[:-1])).max()))


# ---- 4. against what exists
def test_beta_zero_through_pynmf_is_the_itakura_saito_fit():
    A, W0, H0, k = _fit_problem()
    got = _pynmf(A, W0, H0, k, 23, 0.0)
    assert got.norm == "is" and got._whole_fit_ok(got._ops())
    from pydnmfk_amd.pyDNMF import PyNMF
    ref = PyNMF(torch.from_numpy(A).cuda(), factors=[torch.from_numpy(W0).cuda(), torch.from_numpy(H0).cuda()], params=I.one_rank_args(k, 23))
    (W1, H1, e1), (W2, H2, e2) = got.fit(), ref.fit()
    assert torch.equal(W1, W2) and torch.equal(H1, H2) and e1 == e2 and got.is_divergence() == ref.is_divergence()


def test_beta_one_divergence_is_the_kl_objective():
    """beta_divergence() at beta = 1 against a float64 KL objective sum a log(a / s') - a + s' of the same factors (zeros in A give s'),
    within BOUND of the magnitudes of its terms; the C entry point at beta = 0 against the float64 Itakura-Saito objective likewise"""
    A, W0, H0, k = _fit_problem()
    A = _with_zeros(A)
    nmf = _pynmf(A, W0, H0, k, 12, 1.0)
    nmf.fit()
    W, H = nmf.W_i.cpu().numpy().astype(np.float64), nmf.H_j.cpu().numpy().astype(np.float64)
    S = W @ H + EPS
    A64 = A.astype(np.float64)
    pos = A64 > 0
    kl = float(np.sum(np.where(pos, A64 * np.log(np.where(pos, A64, 1.0) / S), 0.0) - A64 + S))
    scale = float(np.sum(np.abs(np.where(pos, A64 * np.log(np.where(pos, A64, 1.0) / S), 0.0)) + A64 + S))
    got = nmf.beta_divergence()
    print("beta=1 divergence %.9g against the float64 KL objective %.9g: %.2e of its terms, %.2e of itself" % (got, kl, abs(got - kl) / scale, abs(got - kl) / kl))
    assert abs(got - kl) <= BOUND * scale
    A, W0, H0, k = _fit_problem()
    d0 = float(_ops().beta_divergence(torch.from_numpy(A).cuda(), torch.from_numpy(W0).cuda(), torch.from_numpy(H0).cuda(), EPS, 0.0).cpu())
    assert abs(d0 - I.divergence(A, W0, H0)) <= BOUND * B.divergence_scale(A, W0, H0, 0.0)


def test_beta_out_of_range_is_refused_before_any_launch():
    from pydnmfk_amd._lib import DnmfError
    A, W0, H0, k = _fit_problem()
    t = [torch.from_numpy(x).cuda() for x in (A, W0, H0)]
    for beta in (-2.5, 4.5, float("nan")):
        with pytest.raises(ValueError, match="-2 <= beta <= 4"):
            _ops().beta_update_w(*t, EPS, beta)
    assert torch.equal(t[1], torch.from_numpy(W0).cuda())
    assert issubclass(DnmfError, RuntimeError)


# ---- 5. 1D grids, two processes on the one GPU
GRID_BETAS = (0.5, 1.5, 3.0)


@pytest.mark.parametrize("grid", [(2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_grids_against_the_float64_statement(grid):
    """50 x 39, k = 3, 20 steps, beta in {0.5, 1.5, 3} (every branch of gamma), W_update on and off, the ranks stacked on the one GPU:
    factors, error and divergence within the fit bounds of the whole-matrix float64 statement; replicated factors bit-identical across
    the ranks (run_grid asserts it)"""
    got = B.run_grid(grid, GRID_BETAS, use_hip=True, timeout=300)
    for (beta, wu), (Wr, Hr, err_r, div_r, scale) in B.reference_fits(GRID_BETAS, dtype=np.float32).items():
        W, H, err, div = got[(beta, wu)]
        dw, dh, de, dd = rel_fro(W, Wr), rel_fro(H, Hr), abs(err - err_r) / err_r, abs(div - div_r) / scale
        print("beta=%g gpu grid %dx%d W_update=%s against float64: dW=%.2e dH=%.2e derr=%.2e ddiv=%.2e of its terms"
              % ((beta,) + grid + (wu, dw, dh, de, dd)))
        assert W.dtype == np.float32 and dw <= FIT_BOUND and dh <= FIT_BOUND and de <= ERR_BOUND and dd <= BOUND, (grid, beta, wu, dw, dh, de, dd)


# ---- 6. main.py --norm beta --beta 0.5
def test_main_norm_beta_end_to_end(tmp_path):
    """main.py --norm beta --beta 0.5 on one rank, in a fresh child process: reads a .npy, fits on the GPU (init rand), writes the factor
    layout; the printed Frobenius relative error is that of the written factors, which are finite and positive"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    A = _fit_problem()[0]
    np.save(tmp_path / "spectra.npy", A)
    cmd = [sys.executable, os.path.join(root, "main.py"), "--process=pyDNMF", "--p_r=1", "--p_c=1", "--fpath=%s/" % tmp_path,
           "--fname=spectra", "--ftype=npy", "--k=5", "--itr=30", "--norm=beta", "--beta=0.5", "--method=mu", "--results_path=%s/res/" % tmp_path]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    err = float(out.stdout.strip().split("relative error =")[-1])
    W = np.load(tmp_path / "res" / "W_factors" / "W_0.npy")
    H = np.load(tmp_path / "res" / "H_factors" / "H_0.npy")
    assert W.shape == (200, 5) and H.shape == (5, 136) and W.dtype == np.float32
    assert np.isfinite(W).all() and np.isfinite(H).all() and (W > 0).all() and (H > 0).all()
    assert abs(np.linalg.norm(A - W @ H) / np.linalg.norm(A) - err) < 1e-4
    rs = np.random.RandomState(0)
    assert B.divergence(A, W, H, 0.5) < B.divergence(A, rs.rand(200, 5) + 0.05, rs.rand(5, 136) + 0.05, 0.5)      # better than a random start
