"""The Itakura-Saito objective (`params.norm = 'is'`) on the GPU (csrc/dnmf_is.h through engine.HipOps): pairs, updates and the
divergence against the float64 statement of tests/_is.py on contiguous tensors and on views of NaN-poisoned buffers; exact operands
element by element at every loop of the launch geometry; the whole fit against the Python step loop, bit for bit; a fit and the
divergence along it against float64; 1D grids with the ranks stacked on the one GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _exact as E  # noqa: E402
from tests import _is as I  # noqa: E402
from tests._golden import rel_fro  # noqa: E402

EPS = I.EPS
# The project's bound for the structurally identical KL pair (tests/test_gpu_masked_dense.py): 1e-5 in relative Frobenius norm.  Per
# element the IS step is one v_rcp_f32 (1 ulp) and two multiplies (half an ulp each) next to the fp32 MFMA sums: a few 2^-24 ~ 6e-8
# per term, summed over non-negative terms -- more than a decade below.
BOUND = 1e-5
# a fit against float64 (the bounds of the masked fits, tests/test_gpu_masked_dense.py): the factors to 1e-4, the error to 1e-5
FIT_BOUND, ERR_BOUND = 1e-4, 1e-5


def _ops():
    from pydnmfk_amd.engine import HIP_OPS
    return HIP_OPS


def _rel(got, ref):
    return float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))


def _random_problem(m, n, k):
    rs = np.random.RandomState(11 * m + 3 * n + k)
    return ((rs.rand(m, n) + 0.05).astype(np.float32), (rs.rand(m, k) + 0.01).astype(np.float32), (rs.rand(k, n) + 0.01).astype(np.float32))


def _expected(A, W, H):
    """float64: both pairs, both updated factors (each from the SAME W, H), the clamped H, the divergence"""
    (nw, dw), (nh, dh) = I.pair(A, W, H, "w"), I.pair(A, W, H, "h")
    W1 = W.astype(np.float64) * np.sqrt(nw / (dw + EPS))
    H1 = H.astype(np.float64) * np.sqrt(nh / (dh + EPS))
    return {"pairs": (nw, dw, nh, dh), "W": W1, "H": H1, "div": I.divergence(A, W, H)}


# ---- 1. pairs, updates and divergence against float64
@pytest.mark.parametrize("shape", I.EXACT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_is_kernels_against_float64(shape):
    """random positive A, W, H at k = 3, 32, 64, 128: on contiguous tensors, on 16-byte aligned padded views and on views with an odd
    start and pitch, all inside NaN-poisoned buffers -- the poison survives, every output is finite and within BOUND of float64"""
    ops = _ops()
    m, n = shape
    worst = {}
    for k in I.EXACT_KS:
        A, W, H = _random_problem(m, n, k)
        exp = _expected(A, W, H)
        for layout in ("contiguous", "aligned views", "odd views"):
            kw = {"packed": True} if layout == "contiguous" else {"aligned": layout == "aligned views"}
            Ap, Wp, Hp = (E.Poisoned(torch, x, **kw) for x in (A, W, H))
            assert Ap.view.is_contiguous() == (layout == "contiguous")
            outs = [E.Poisoned.out(torch, r, c, torch.float32, aligned=layout != "odd views") for r, c in ((m, k), (m, k), (k, n), (k, n))]
            ops.is_pair_into("w", Ap.view, Wp.view, Hp.view, EPS, outs[0].view, outs[1].view)
            ops.is_pair_into("h", Ap.view, Wp.view, Hp.view, EPS, outs[2].view, outs[3].view)
            got = [o.check("%s k=%d %s" % (layout, k, what)) for o, what in zip(outs, ("num_w", "den_w", "num_h", "den_h"))]
            d = [_rel(g, r) for g, r in zip(got, exp["pairs"])]
            div = float(ops.is_divergence(Ap.view, Wp.view, Hp.view, EPS).cpu())
            dd = abs(div - exp["div"]) / exp["div"]
            assert float(ops.is_divergence(Ap.view, Wp.view, Hp.view, EPS).cpu()) == div                 # stored, fixed order
            # the fused endings and the stand-alone rule, each from the same W, H
            W1, H1, H2, W3, H3 = (E.Poisoned(torch, x, **kw) for x in (W, H, H, W, H))
            ops.is_update_w(Ap.view, W1.view, Hp.view, EPS)
            ops.is_update_h(Ap.view, Wp.view, H1.view, EPS)
            ops.is_update_h(Ap.view, Wp.view, H2.view, EPS, clamp=True)
            ops.is_ratio_update(W3.view, outs[0].view, outs[1].view, EPS)
            ops.is_ratio_update(H3.view, outs[2].view, outs[3].view, EPS, clamp=True)
            du = [_rel(W1.check("W1"), exp["W"]), _rel(H1.check("H1"), exp["H"]), _rel(H2.check("H2"), np.maximum(exp["H"], EPS)),
                  _rel(W3.check("W3"), exp["W"]), _rel(H3.check("H3"), np.maximum(exp["H"], EPS))]
            assert np.array_equal(W1.check(), W3.check()) and np.array_equal(H2.check(), H3.check())       # one expression, one result
            for p_, what in ((Ap, "A"), (Wp, "W"), (Hp, "H")):                                             # operands: not written
                assert np.array_equal(p_.check(what), {"A": A, "W": W, "H": H}[what])
            print("is %dx%d k=%3d %-14s W: num %.2e den %.2e | H: num %.2e den %.2e | updates %.2e | divergence %.2e"
                  % (m, n, k, layout, *d, max(du), dd))
            worst["pair"] = max(worst.get("pair", 0.0), *d)
            worst["update"] = max(worst.get("update", 0.0), *du)
            worst["divergence"] = max(worst.get("divergence", 0.0), dd)
            assert max(d) <= BOUND and max(du) <= BOUND and dd <= BOUND, (shape, k, layout, d, du, dd)
    print("is %dx%d maxima:" % shape, {k_: "%.2e" % v for k_, v in sorted(worst.items())})


# ---- 2. exact operands, element by element
def _exact_pairs(A, W, H, k, aligned=True):
    ops = _ops()
    m, n = A.shape
    Ap, Wp, Hp = (E.Poisoned(torch, x, aligned=aligned) for x in (A, W, H))
    out = []
    for side, (r, c) in (("w", (m, k)), ("h", (k, n))):
        num, den = E.Poisoned.out(torch, r, c, torch.float32, aligned=aligned), E.Poisoned.out(torch, r, c, torch.float32, aligned=aligned)
        ops.is_pair_into(side, Ap.view, Wp.view, Hp.view, EPS, num.view, den.view)
        out += [num.check("is %s num k=%d" % (side, k)), den.check("is %s den k=%d" % (side, k))]
    for p_ in (Ap, Wp, Hp):
        assert np.isnan(p_.buf.cpu().numpy()[~p_.mask]).all()
    fast = all(p_.view.data_ptr() % 16 == 0 and p_.ld % 4 == 0 for p_ in (Ap, Wp, Hp)) and n % 4 == 0 and k % 4 == 0
    return out, fast


def _assert_exact(shape, k, aligned=True):
    m, n = shape
    A, W, H, ref = I.exact_problem(m, n, k)
    got, fast = _exact_pairs(A, W, H, k, aligned)
    want = ref["w"] + ref["h"]
    for g, r, what in zip(got, want, ("num_w", "den_w", "num_h", "den_h")):
        if not np.array_equal(g.astype(np.float64), r):
            bad = np.argwhere(g.astype(np.float64) != r)
            i = tuple(int(x) for x in bad[0])
            raise AssertionError("is exact %dx%d k=%d %s: %d of %d elements differ; first at %s: got %r, exact %r"
                                 % (m, n, k, what, len(bad), g.size, i, g[i].item(), r[i].item()))
    again, _ = _exact_pairs(A, W, H, k, aligned)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (shape, k, "second call differs")
    return fast


@pytest.mark.parametrize("shape", I.EXACT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_is_exact_operands(shape):
    """tests/_is.py::exact (every S a power of two >= 2, A in 1..7; tests/test_is_cpu.py proves every sum exact in any order): num and
    den of both sides equal the float64 answers element by element, on padded views in poisoned buffers; (132, 96) takes the 16-byte
    vector kernels at k % 4 == 0, and (130, 97) once more on views with an odd start and pitch"""
    for k in I.EXACT_KS:
        fast = _assert_exact(shape, k)
        assert fast == (shape[1] % 4 == 0 and k % 4 == 0)
    if shape == (130, 97):
        for k in I.EXACT_KS:
            assert not _assert_exact(shape, k, aligned=False)


@pytest.mark.parametrize("case", I.EXACT_LOOP_CASES, ids=lambda c: "%dx%d" % c["shape"])
def test_is_exact_operands_in_the_loops(case):
    """the same at the smallest shapes whose launch plan (dnmf_is_plan, asserted in tests/test_capi_is.py) gives a workgroup of the W
    side three tiles with a ragged last one, a wave of the H side two row blocks and the last chunk one, and the ending a second
    grid-stride trip -- generic and 16-byte vector kernels; each pair twice, bit-identical"""
    for k in case["ks"]:
        fast = _assert_exact(case["shape"], k)
        assert fast == (case["fast"] and k % 4 == 0), (case["shape"], k)


# ---- 3. fits on one rank
def _fit_problem():
    A, W0, H0, k = I.problem(200, 136, 5, seed=9)
    return A.astype(np.float32), W0.astype(np.float32), H0.astype(np.float32), k


def _pynmf(A, W0, H0, k, itr, **kw):
    from pydnmfk_amd.pyDNMF import PyNMF
    return PyNMF(torch.from_numpy(A).cuda(), factors=[torch.from_numpy(W0).cuda(), torch.from_numpy(H0).cuda()],
                 params=I.one_rank_args(k, itr, **kw))


@pytest.mark.parametrize("wu", [True, False], ids=["W_update", "W_fixed"])
def test_whole_fit_equals_the_python_step_loop_bit_for_bit(wu):
    """dnmf_is_mu_fit through PyNMF against params.fit_loop = 'python' (the same launches, sequenced from Python): torch.equal on W and
    H over 23 steps (three clamps); a second whole fit is bit-identical; W_update=False leaves W's bits alone until the normalisation"""
    A, W0, H0, k = _fit_problem()
    whole = _pynmf(A, W0, H0, k, 23, W_update=wu)
    assert whole._whole_fit_ok(whole._ops()) and whole._ops().name == "hip"
    loop = _pynmf(A, W0, H0, k, 23, W_update=wu, fit_loop="python")
    assert not loop._whole_fit_ok(loop._ops())
    (W1, H1, e1), (W2, H2, e2), (W3, H3, e3) = whole.fit(), loop.fit(), _pynmf(A, W0, H0, k, 23, W_update=wu).fit()
    assert torch.equal(W1, W2) and torch.equal(H1, H2) and torch.equal(W1, W3) and torch.equal(H1, H3)
    assert torch.isfinite(W1).all() and torch.isfinite(H1).all() and abs(e1 - e2) <= 1e-12 and abs(e1 - e3) <= 1e-12
    if not wu:
        from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
        ops = _ops()
        step = _pynmf(A, W0, H0, k, 11, W_update=False)
        for i in range(11):                                                         # (the steps 0 and 10 clamp: W0 > eps stays as it is)
            nmf_algorithms_1D(step.A_ij, step.W_i, step.H_j, params=step.params, ops=ops).update(clamp=(i % 10 == 0))
        assert torch.equal(step.W_i, torch.from_numpy(W0).cuda()) and not torch.equal(step.H_j, torch.from_numpy(H0).cuda())
        Wn = torch.from_numpy(W0).cuda()
        s = ops.colsum(Wn, ops.zeros((k,), Wn))
        ops.scale_cols_div(Wn, s, EPS)
        assert torch.equal(W1, Wn)                                                  # the whole fit: W0 normalised, nothing else


def test_thirty_step_fit_against_float64():
    """200 x 136, k = 5, gamma noise, 30 steps: factors within 1e-4 and the error within 1e-5 of the float64 statement (the bounds of the
    masked fits); the divergence of the fitted factors within 1e-5"""
    A, W0, H0, k = _fit_problem()
    nmf = _pynmf(A, W0, H0, k, 30)
    W, H, err = nmf.fit()
    Wr, Hr, err_r = I.fit(A, W0, H0, 30)
    dw, dh, de = rel_fro(W.cpu().numpy(), Wr), rel_fro(H.cpu().numpy(), Hr), abs(err - err_r) / err_r
    div, div_r = nmf.is_divergence(), I.divergence(A, Wr, Hr)
    print("is fit 200x136 k=5, 30 steps against float64: dW=%.2e dH=%.2e derr=%.2e ddiv=%.2e (err %.6g, D %.6g)"
          % (dw, dh, de, abs(div - div_r) / div_r, err_r, div_r))
    assert dw <= FIT_BOUND and dh <= FIT_BOUND and de <= ERR_BOUND and abs(div - div_r) <= BOUND * div_r


def test_the_divergence_never_rises_along_the_python_loop():
    """is_divergence() after each of 30 steps of the Python loop: consecutive values, compared in float64, never rise by more than
    1e-6 of their own value (fp32 rounding of the sum: 64 fp32 terms per lane, float64 from there).  The check binds only while the
    float64 statement's own per-step decrease exceeds that slack: asserted for those steps, which must be all 30 on this problem"""
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    A, W0, H0, k = _fit_problem()
    slack = 1e-6
    W, H = W0.astype(np.float64), H0.astype(np.float64)
    ref = [I.divergence(A, W, H)]
    for i in range(30):
        W, H = I.step(A, W, H, EPS, True, clamp=(i % 10 == 0))
        ref.append(I.divergence(A, W, H))
    drop = -np.diff(ref) / np.array(ref[:-1])
    steps = int(np.argmax(drop <= slack)) if (drop <= slack).any() else 30
    print("is divergence (float64): %.6g -> %.6g, smallest relative decrease per step %.3e; binding steps: %d" % (ref[0], ref[-1], drop.min(), steps))
    assert steps == 30, drop
    nmf = _pynmf(A, W0, H0, k, 30, fit_loop="python")
    d = [nmf.is_divergence()]
    for i in range(steps):
        nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update(clamp=(i % 10 == 0))
        d.append(nmf.is_divergence())
        assert d[-1] <= d[-2] * (1.0 + slack), (i, d[-2], d[-1])
        assert abs(d[-1] - ref[i + 1]) <= 1e-4 * ref[i + 1], (i, d[-1], ref[i + 1])
    print("is divergence (gpu):     %.6g -> %.6g, largest relative change per step %.3e" % (d[0], d[-1], (np.diff(d) / np.array(d[:-1])).max()))


# ---- 4. 1D grids, two processes on the one GPU
@pytest.mark.parametrize("grid", [(2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_grids_against_the_float64_statement(grid):
    """50 x 39, k = 3, 20 steps, W_update on and off, the ranks stacked on the one GPU: factors, error and divergence within the fit
    bounds of the whole-matrix float64 statement; replicated factors bit-identical across the ranks (run_grid asserts it)"""
    got = I.run_grid(grid, use_hip=True, timeout=300)
    for wu, (Wr, Hr, err_r, div_r) in I.reference_fits(dtype=np.float32).items():
        W, H, err, div = got[wu]
        dw, dh, de, dd = rel_fro(W, Wr), rel_fro(H, Hr), abs(err - err_r) / err_r, abs(div - div_r) / div_r
        print("is gpu grid %dx%d W_update=%s against float64: dW=%.2e dH=%.2e derr=%.2e ddiv=%.2e" % (grid + (wu, dw, dh, de, dd)))
        assert W.dtype == np.float32 and dw <= FIT_BOUND and dh <= FIT_BOUND and de <= ERR_BOUND and dd <= BOUND, (grid, wu, dw, dh, de, dd)


# ---- 5. main.py --norm is
def test_main_norm_is_end_to_end(tmp_path):
    """main.py --norm is on one rank: reads a .npy, fits on the GPU (init rand), writes the factor layout; the printed Frobenius
    relative error is that of the written factors, which are finite and positive"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    A = _fit_problem()[0]
    np.save(tmp_path / "spectra.npy", A)
    cmd = [sys.executable, os.path.join(root, "main.py"), "--process=pyDNMF", "--p_r=1", "--p_c=1", "--fpath=%s/" % tmp_path,
           "--fname=spectra", "--ftype=npy", "--k=5", "--itr=30", "--norm=is", "--method=mu", "--results_path=%s/res/" % tmp_path]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    err = float(out.stdout.strip().split("relative error =")[-1])
    W = np.load(tmp_path / "res" / "W_factors" / "W_0.npy")
    H = np.load(tmp_path / "res" / "H_factors" / "H_0.npy")
    assert W.shape == (200, 5) and H.shape == (5, 136) and W.dtype == np.float32
    assert np.isfinite(W).all() and np.isfinite(H).all() and (W > 0).all() and (H > 0).all()
    assert abs(np.linalg.norm(A - W @ H) / np.linalg.norm(A) - err) < 1e-4
    rs = np.random.RandomState(0)
    assert I.divergence(A, W, H) < I.divergence(A, rs.rand(200, 5) + 0.05, rs.rand(5, 136) + 0.05)      # better than a random start
