"""The HALS sweeps (csrc/dnmf_hals.h, csrc/dnmf_wide.hip, the float64 ones of csrc/dnmf_f64.hip) against the exact answer of ONE sweep from
a chosen state, element by element: `hals_w_problem` / `hals_h_problem` (tests/_exact.py, proved in every summation order by
tests/test_exact_cpu.py) build the operands backwards from the answer, so every element of the new factor and every column's sum of
squares is known exactly -- one wrong row (the ragged last one, the row a dead lane borrows), one wrong element of a 16-byte row store,
one missed piece of the lagging triangular update or one dropped workgroup slot of a column norm fails here, where a Frobenius norm
over the factor cannot see it.  Operands are views in NaN-poisoned buffers, as in tests/test_gpu_exact.py.

Bounds per element: W_new, H_new                                        exact (c = 0), with eps = 2^-3 and with eps = 2^-23
                    ss2, eps = 2^-3                                     exact
                    ss2, eps = 2^-23                                    4^p within ss2_tol = n_c (2^-46 + (2 p + 5) spacing(4^p) / 2), n_c the
                                                                        clamped rows (`hals_w_problem`); (float)sqrt(ss2) = 2^p throughout
One whole step (`hals_step_problem`): the W phase is exact, so the W a fit of ONE step returns is max(W_new, eps) / (colsum + eps) within
1 ulp (exact numerator and denominator, one IEEE division) and the W of a step without normalisation is W_new bit for bit; the H phase
of a step cannot be made exact (see `hals_step_problem`): it is held to the derived forward bound H_err of that generator.
float64 W sweep with eps = 2^-23: the derived relative bound W_rel per column (`hals_w_problem`).
Every W case asserts the plan (dnmf_hals_sweep_plan) before it runs: the route, the transform variant and the sweep's row access are the
ones the case is named after; the shape table is HALS_W_CASES."""
import functools

import numpy as np
import pytest

from tests import _exact as ex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPSS = [pytest.param(ex.HALS_EPS_A, id="eps2^-3"), pytest.param(ex.HALS_EPS_B, id="eps2^-23")]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pydnmfk_amd import engine
    from pydnmfk_amd._lib import lib
    return engine, lib


@functools.lru_cache(maxsize=4)
def _w_problem(m, k, eps, dtype=np.float32):
    return ex.hals_w_problem(m, k, eps, dtype=dtype)


def _P(x, aligned=True, dtype=None):
    return ex.Poisoned(torch, x, dtype=dtype, aligned=aligned)


def _gram(engine, G, dtype=torch.float32):
    """G zero-padded to KP x KP, as new_gram hands it to the kernels"""
    k = G.shape[0]
    out = engine.new_gram(k, torch.device("cuda")).to(dtype)
    out[:k, :k] = torch.from_numpy(np.ascontiguousarray(G)).cuda().to(dtype)
    return out


def _bits(x):
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _check_w(w, ss2, P, what):
    if P["W_rel"].any():                                        # float64 with eps = 2^-23: the derived relative bound per column
        bad = np.abs(w - P["W_new"]) > P["W_rel"][None, :] * P["W_new"]
        assert not bad.any(), "%s: W%s = %r, expected %r within %g of it" % (what, tuple(np.argwhere(bad)[0]), w[tuple(np.argwhere(bad)[0])],
                                                                            P["W_new"][tuple(np.argwhere(bad)[0])], P["W_rel"][np.argwhere(bad)[0][1]])
    else:
        ex.assert_ulp(w, P["W_new"], 0, what + ": W", tile=(ex.HALS_ROWS, 4))
    bad = np.abs(ss2 - P["ss2"]) > P["ss2_tol"]
    assert not bad.any(), "%s: ss2[%d] = %r, expected %r within %g" % (what, np.argmax(bad), ss2[np.argmax(bad)], P["ss2"][np.argmax(bad)],
                                                                     P["ss2_tol"][np.argmax(bad)])


def _run_w(env, m, k, aligned, eps, plan, ops=None, dtype=np.float32):
    """one W problem through the persistent entry point, the column entry point and explicit column calls, twice each"""
    engine, lib = env
    f32 = dtype == np.float32
    ops = ops or engine.HIP_OPS
    tdt = torch.float32 if f32 else torch.float64
    P = _w_problem(m, k, eps, dtype)
    G = _gram(engine, P["G"], tdt)
    AHv = _P(P["AH"].astype(dtype), aligned)
    for route in ("sweep", "columns", "explicit"):
        first = None
        for rep in range(2):
            Wv = _P(P["W_old"].astype(dtype), aligned)
            what = "%d x %d, %s, call %d" % (m, k, route, rep)
            if route == "sweep":
                if f32:
                    got = ops.hals_sweep_plan(Wv.view, AHv.view)
                    assert got[:5] == plan, "%s: plan %s, expected %s (cap %d)" % (what, got[:5], plan, got[5])
                    assert got[0] == 0 or got[2] <= got[5]
                ss2 = ops.hals_update_w(Wv.view, AHv.view, G, eps)
                ops.hals_check()
                ss2 = ss2.cpu().numpy()
            elif route == "columns":
                ss2 = ops.hals_update_w_columns(Wv.view, AHv.view, G, eps).cpu().numpy()
            else:
                s = ops.hals_ss2(k, Wv.view)
                for kk in range(k):
                    ops.hals_w_col(Wv.view, AHv.view, G, kk, s, eps)
                ops.hals_w_scale(Wv.view, k - 1, s)
                ss2 = s.cpu().numpy()
            w = Wv.check(what)
            AHv.check(what + ": AH")
            _check_w(w, ss2, P, what)
            if rep == 0:
                first = (w.copy(), ss2.copy())
            else:
                assert np.array_equal(_bits(w), _bits(first[0])) and np.array_equal(_bits(ss2), _bits(first[1])), what + ": a second call differs"
    assert np.array_equal(G.cpu().numpy()[:k, :k], P["G"].astype(dtype)), "G was written"


# ------------------------------------------------------------------------------------------------------------- W sweep
@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("case", ex.HALS_W_CASES, ids=[c[0] for c in ex.HALS_W_CASES])
def test_w_sweep(env, case, eps):
    """every route of the W sweep at every shape of the table: bit-equal factors, exact column norms, the asserted plan"""
    _, m, k, aligned, plan = case
    _run_w(env, m, k, aligned, eps, plan)


@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("over", [0, 1], ids=["cap", "cap+1"])
def test_w_sweep_at_full_residency(env, over, eps):
    """as many workgroups as the device holds resident (the plan's `cap`), the last with one live row: the persistent sweep; one more:
    column launches -- and the same bits"""
    engine, _ = env
    k = ex.HALS_POLL_K
    probe = torch.zeros(8, k + 1, device="cuda")[:, :k]
    cap = engine.HIP_OPS.hals_sweep_plan(probe, probe)[5]
    assert cap in ex.HALS_CAPS, "resident workgroups of the KP = 32 sweep: %d -- add it to HALS_CAPS so that tests/test_exact_cpu.py proves its shapes" % cap
    nwg = cap + over
    m = ex._slots(nwg)
    plan = (1, 32, nwg, 2, 0) if not over else (0, 32, min(-(-m // 256), 2048), -1, 0)
    _run_w(env, m, k, True, eps, plan)


@pytest.mark.parametrize("m,k", ex.HALS_W_F64)
def test_w_sweep_f64(env, m, k):
    """the float64 column kernels on the same operands, eps = 2^-3: bit for bit"""
    engine, _ = env
    for aligned in (True, False):
        _run_w(env, m, k, aligned, ex.HALS_EPS_A, None, ops=engine.HIP_OPS_F64, dtype=np.float64)


@pytest.mark.parametrize("m,k", ex.HALS_W_F64_B)
def test_w_sweep_f64_library_eps(env, m, k):
    """float64 with eps = 2^-23: the clamped terms are not absorbed, the column norms are no powers of two and every later column sees
    a W off in the last bits -- held to the derived relative bound per column (`hals_w_problem`: W_rel, 1e-12 at k = 7, 5.5e-9 at
    k = 33; at 513 x 128 the bound reaches the clamp decisions and nothing can be asserted)"""
    engine, _ = env
    for aligned in (True, False):
        _run_w(env, m, k, aligned, ex.HALS_EPS_B, None, ops=engine.HIP_OPS_F64, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------- H sweep
def _run_h(env, k, n, eps, ops, dtype):
    engine, _ = env
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    H0, AtW, G2, Hn = ex.hals_h_problem(k, n, eps)
    G = _gram(engine, G2, tdt)
    for aligned in (True, False):
        Hv, Av = _P(H0.astype(dtype), aligned), _P(AtW.astype(dtype), aligned)
        ops.hals_update_h(Hv.view, Av.view, G, eps)
        what = "H sweep %d x %d%s" % (k, n, "" if aligned else ", odd start and pitch")
        ex.assert_ulp(Hv.check(what), Hn, 0, what, tile=(1, 64))
        Av.check(what + ": AtW")


@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("k,n", ex.HALS_H_CASES)
def test_h_sweep(env, k, n, eps):
    """hals_h_kernel<32> / <64>, hals_h_kernel_lds and the wide kernel: every element of the new H, bit for bit"""
    _run_h(env, k, n, eps, env[0].HIP_OPS, np.float32)


@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("k,n", ex.HALS_H_F64)
def test_h_sweep_f64(env, k, n, eps):
    _run_h(env, k, n, eps, env[0].HIP_OPS_F64, np.float64)


# ------------------------------------------------------------------------------------------------------------- the W phase of one whole step
STEP_SMALL = [e for e in ex.SMALL_REACH if e[0] == "hals" or (e[0] == "hals_bf16" and e[1:4] not in ex.HALS_STEP_BF16_LEFT)]


@pytest.mark.parametrize("B", [1, 3], ids=["single", "batch3"])
@pytest.mark.parametrize("entry", STEP_SMALL, ids=lambda e: "%s-%dx%d-k%d" % e[:4])
def test_whole_step_w_phase_small_fit(env, entry, B):
    """fit(itr = 1) on the small whole-fit HALS kernel (csrc/dnmf_small.h), every float-A and bf16-A geometry of the reach table, single and as a
    batch of 3: the plan, the launch counter, and the returned W = max(W_new, eps) / (colsum + eps) within 1 ulp at every element"""
    from tests.test_gpu_small_exact import _expected_launches, _launches, _plan, _stacks
    engine, lib = env
    ops = engine.HIP_OPS
    family, m, n, k, plan = entry
    assert _plan(lib, family, m, n, k) == plan
    eps = ex.HALS_EPS_A
    bf16 = family == "hals_bf16"
    probs = [ex.hals_step_problem(m, n, k, seed=b, bf16=bf16) for b in range(B)]
    before = _launches(lib)
    (Ap, Wp, Hp), args = _stacks([(P["A"], P["W_old"], P["H_old"]) for P in probs], B, torch.bfloat16 if bf16 else torch.float32)
    ops.fit("hals", "fro", *args, eps, True, 1)
    ops.hals_check()
    want = list(before)
    want[3] += _expected_launches(plan, B)
    assert _launches(lib) == want, "launches %s -> %s, expected %s" % (before, _launches(lib), want)
    Ap.check("A")
    w3, h3 = Wp.check("W"), Hp.check("H")
    if B == 1:
        w3, h3 = w3[None], h3[None]
    assert np.isfinite(h3).all() and (h3 > 0).all()
    f32 = np.float32
    for b, P in enumerate(probs):
        Wc = np.maximum(P["W_new"], eps)                       # the clamp after step 0 (pyDNMF.py:170-172)
        s = Wc.sum(0)
        assert np.array_equal((s + eps).astype(np.float32).astype(np.float64), s + eps)
        ex.assert_ulp(w3[b], Wc / (s + eps)[None, :], 1, "%d x %d k = %d [%d]: W = max(W_new, eps) / (colsum + eps)" % (m, n, k, b), tile=(16, 16))
        # H s: the derived bound of the H sweep (H_err) times s, and the rounding of the one product
        want = P["H_new"] * s[:, None]
        lim = (P["H_err"] * s[:, None]) * (1 + 2.0 ** -20) + np.spacing(np.abs(want).astype(f32)).astype(np.float64)
        bad = np.abs(h3[b] - want) > lim
        print("%d x %d k = %d [%d]: max |H s - f64| / bound = %.3g" % (m, n, k, b, np.max(np.abs(h3[b] - want) / lim)))
        assert not bad.any(), "%d x %d k = %d [%d]: H s at %s is %r, expected %r within %g" % (
            m, n, k, b, tuple(np.argwhere(bad)[0]), h3[b][tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])], lim[tuple(np.argwhere(bad)[0])])


@pytest.mark.parametrize("m,n,k", ex.HALS_STEP_BIG)
def test_whole_step_w_phase_big_path(env, m, n, k):
    """one step of the one-rank 1D route (A H^T, H H^T, then dnmf_hals_sweep_w; no normalisation): W_new bit for bit"""
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.utils import parse
    P = ex.hals_step_problem(m, n, k)
    comms = MPI_comm(None, 1, 1)
    p = parse()
    p.comm1, p.comm, p.p_r, p.p_c, p.k, p.m, p.n = comms.comm, comms, 1, 1, k, m, n
    p.row_comm, p.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    p.norm, p.method, p.W_update, p.eps = "fro", "hals", True, ex.HALS_EPS_A
    Av, Wv, Hv = (ex.Poisoned(torch, P[x], packed=True) for x in ("A", "W_old", "H_old"))
    nmf_algorithms_1D(Av.view, Wv.view, Hv.view, params=p).update()
    env[0].HIP_OPS.hals_check()
    Av.check("A")
    ex.assert_ulp(Wv.check("W"), P["W_new"], 0, "%d x %d k = %d: W after one step" % (m, n, k), tile=(ex.HALS_ROWS, 4))
    h = Hv.check("H")
    assert np.isfinite(h).all() and (h >= ex.HALS_EPS_A).all()
    bad = np.abs(h - P["H_new"]) > P["H_err"]                       # the derived bound of the H sweep (loose from k of about 16 on)
    print("%d x %d k = %d: max |H - f64| / bound = %.3g" % (m, n, k, np.max(np.abs(h - P["H_new"]) / P["H_err"])))
    assert not bad.any(), "H at %s is %r, expected %r within %g" % (tuple(np.argwhere(bad)[0]), h[tuple(np.argwhere(bad)[0])],
                                                                   P["H_new"][tuple(np.argwhere(bad)[0])], P["H_err"][tuple(np.argwhere(bad)[0])])
