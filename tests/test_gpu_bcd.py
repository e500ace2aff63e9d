"""method='bcd' on the MI355X: the BCD entry points (csrc/dnmf_bcd.hip) against float64 restatements, the reference's outputs
(tests/golden/bcd_*.npz) through the whole-fit call and the Python choreography (bit-identical to each other), the stacked-rank
grids, the reference's own acceptance test, determinism, fit_batch / PyNMFk, and the combinations that are refused."""
import numpy as np
import pytest

from tests import _exact as ex
from tests._bcd import ACC, LH, LH_OLD, LW, LW_OLD, OBJ_OLD, T_OLD, WH, WW, XN, bcd_case_names, check_tolerances, load_bcd, run_bcd
from tests._golden import rel_fro

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KS = [1, 2, 17, 32, 33, 64, 100, 128, 256]
SLOTS = dict(ACC=ACC, LH=LH, LH_OLD=LH_OLD, LW=LW, LW_OLD=LW_OLD, OBJ_OLD=OBJ_OLD, T_OLD=T_OLD, WH=WH, WW=WW, XN=XN)


def _ops():
    from pydnmfk_amd.engine import HIP_OPS
    return HIP_OPS


def _gram(k, rs, sym=True):
    from pydnmfk_amd.engine import new_gram
    G = new_gram(k, "cuda")
    g = rs.rand(k, k).astype(np.float32)
    if sym:
        g = (g + g.T).astype(np.float32)
    G[:k, :k] = torch.from_numpy(g).cuda()
    return G, g.astype(np.float64)


def _state(**slots):
    st = torch.zeros(16, dtype=torch.float64)
    for key, v in slots.items():
        st[SLOTS[key]] = v
    return st.cuda()


# ------------------------------------------------------------------------------------------------ (a) the entry points
@pytest.mark.parametrize("k", KS)
def test_bcd_update_w_and_scale(k):
    rs = np.random.RandomState(k)
    m = 131
    ops = _ops()
    Wm = ex.Poisoned(torch, rs.rand(m, k).astype(np.float32), aligned=(k % 2 == 0))
    AH = ex.Poisoned(torch, (rs.rand(m, k) * k).astype(np.float32), aligned=(k % 2 == 1))
    G, g = _gram(k, rs)
    L = float(np.float32(np.linalg.norm(g)))
    st = _state(LW=L)
    W = ex.Poisoned.out(torch, m, k, torch.float32, aligned=(k % 3 == 0))
    s = torch.full((k + 5,), 7.0, dtype=torch.float32, device="cuda")
    ops.bcd_update_w(Wm.view, AH.view, G, st, W.view, s[:k])
    w = W.check("bcd_update_w")
    wm, ah = Wm.view.cpu().double().numpy(), AH.view.cpu().double().numpy()
    ref = np.maximum(0, wm - (wm @ g - ah) / L)
    scale = np.abs(wm).max() + np.abs(wm @ g - ah).max() / L
    assert np.abs(w - ref).max() <= 3e-6 * scale
    assert np.abs(s[:k].cpu().numpy() - w.astype(np.float64).sum(0)).max() <= 1e-5 * np.abs(w).sum(0).max()
    assert (s[k:].cpu().numpy() == 7.0).all()
    before = W.view.cpu().numpy().copy()
    ops.bcd_scale_cols(W.view, s[:k])
    np.testing.assert_array_equal(W.check("bcd_scale_cols"), before / s[:k].cpu().numpy()[None, :])


@pytest.mark.parametrize("k", KS)
def test_bcd_update_h(k):
    rs = np.random.RandomState(100 + k)
    n = 203
    ops = _ops()
    Hm = ex.Poisoned(torch, rs.rand(k, n).astype(np.float32), aligned=(k % 2 == 1))
    AtW = ex.Poisoned(torch, (rs.rand(k, n) * k).astype(np.float32), aligned=(k % 2 == 0))
    G, g = _gram(k, rs, sym=False)            # read as stored: G Hm, no symmetry assumed
    L = float(np.float32(np.linalg.norm(g)))
    st = _state(LH=L)
    H = ex.Poisoned.out(torch, k, n, torch.float32, aligned=(k % 3 == 1))
    ops.bcd_update_h(Hm.view, AtW.view, G, st, H.view)
    h = H.check("bcd_update_h")
    hm, a = Hm.view.cpu().double().numpy(), AtW.view.cpu().double().numpy()
    ref = np.maximum(0, hm - (g @ hm - a) / L)
    scale = np.abs(hm).max() + np.abs(g @ hm - a).max() / L
    assert np.abs(h - ref).max() <= 3e-6 * scale


@pytest.mark.parametrize("k", [1, 33, 256])
def test_bcd_state_init_factor_and_lipschitz(k):
    rs = np.random.RandomState(k)
    ops = _ops()
    sq = torch.tensor([12.5, 3.0, 7.0], dtype=torch.float64, device="cuda")
    st = torch.full((16,), -1.0, dtype=torch.float64, device="cuda")
    ops.bcd_state_init(st, sq)
    s = st.cpu().numpy()
    assert (s[XN], s[1], s[2], s[OBJ_OLD], s[T_OLD], s[LW], s[LH], s[ACC]) == (12.5, 3.0, 7.0, 6.25, 1.0, 1.0, 1.0, 0.0)
    X0 = ex.Poisoned(torch, rs.rand(57, k).astype(np.float32), aligned=False)
    Xo, Xm = ex.Poisoned.out(torch, 57, k, torch.float32), ex.Poisoned.out(torch, 57, k, torch.float32, aligned=False)
    ops.bcd_init_factor(X0.view, Xo.view, Xm.view, st, 0)
    want = X0.view.cpu().numpy() / np.float32(np.sqrt(3.0)) * np.float32(np.sqrt(np.sqrt(12.5)))
    np.testing.assert_array_equal(Xo.check("X_old"), want)
    np.testing.assert_array_equal(Xm.check("X_m"), want)
    G, g = _gram(k, rs)
    ops.bcd_lipschitz(G, k, st, 0)
    ops.bcd_lipschitz(G, k, st, 0)
    ops.bcd_lipschitz(G, k, st, 1)
    s = st.cpu().numpy()
    nrm = np.linalg.norm(g)
    assert s[LW] == s[LW_OLD] == s[LH] and s[LH_OLD] == 1.0
    assert abs(s[LW] - nrm) <= 1e-7 * nrm and s[LW] == float(np.float32(s[LW]))


def test_bcd_decide_both_branches():
    ops = _ops()
    st = _state(OBJ_OLD=10.0, T_OLD=1.0, LW=4.0, LW_OLD=1.0, LH=2.0, LH_OLD=8.0)
    ops.bcd_decide(st, torch.tensor([30.0], dtype=torch.float64, device="cuda"))       # obj 15 >= 10: restart
    s = st.cpu().numpy()
    assert s[ACC] == 0 and s[OBJ_OLD] == 10.0 and s[T_OLD] == 1.0
    ops.bcd_decide(st, torch.tensor([20.0], dtype=torch.float64, device="cuda"))       # obj 10 >= 10 (a tie): restart
    assert st.cpu().numpy()[ACC] == 0
    ops.bcd_decide(st, torch.tensor([4.0], dtype=torch.float64, device="cuda"))        # obj 2 < 10: accept
    s = st.cpu().numpy()
    t = (1 + np.sqrt(5.0)) / 2
    assert s[ACC] == 1 and s[OBJ_OLD] == 2.0 and s[T_OLD] == t and s[WW] == 0.0 and s[WH] == 0.0      # w = (t_old - 1) / t = 0
    ops.bcd_decide(st, torch.tensor([2.0], dtype=torch.float64, device="cuda"))
    s = st.cpu().numpy()
    t2 = (1 + np.sqrt(1 + 4 * t * t)) / 2
    w = (t - 1) / t2
    assert s[ACC] == 1 and s[T_OLD] == t2
    assert s[WW] == min(w, 0.5) and s[WH] == min(w, 2.0)


@pytest.mark.parametrize("accept", [True, False])
@pytest.mark.parametrize("k", [2, 33, 256])
def test_bcd_extrapolate(accept, k):
    rs = np.random.RandomState(k + accept)
    ops = _ops()
    m, n = 45, 38

    def P(r, c, al=True):
        return ex.Poisoned(torch, rs.rand(r, c).astype(np.float32), aligned=al)
    bufs = dict(W=P(m, k), Wo=P(m, k, False), Wm=P(m, k), H=P(k, n, False), Ho=P(k, n), Hm=P(k, n, False), AH=P(m, k), AHk=P(m, k, False))
    G, _ = _gram(k, rs)
    Gk, _ = _gram(k, rs)
    before = {nm: t.view.cpu().numpy().copy() for nm, t in bufs.items()}
    g0, gk0 = G.cpu().numpy().copy(), Gk.cpu().numpy().copy()
    st = _state(ACC=1.0 if accept else 0.0, WW=0.375, WH=0.6)
    b = {nm: t.view for nm, t in bufs.items()}
    ops.bcd_extrapolate(b["W"], b["Wo"], b["Wm"], b["H"], b["Ho"], b["Hm"], b["AH"], b["AHk"], G, Gk, st)
    got = {nm: t.check(nm) for nm, t in bufs.items()}
    np.testing.assert_array_equal(got["W"], before["W"])
    np.testing.assert_array_equal(got["H"], before["H"])
    if accept:
        for x, o, p, w in (("W", "Wo", "Wm", 0.375), ("H", "Ho", "Hm", 0.6)):
            np.testing.assert_array_equal(got[p], before[x] + np.float32(w) * (before[x] - before[o]))
            np.testing.assert_array_equal(got[o], before[x])
        np.testing.assert_array_equal(got["AHk"], before["AH"])
        np.testing.assert_array_equal(got["AH"], before["AH"])
        np.testing.assert_array_equal(Gk.cpu().numpy(), g0)
    else:
        np.testing.assert_array_equal(got["Wm"], before["Wo"])
        np.testing.assert_array_equal(got["Hm"], before["Ho"])
        np.testing.assert_array_equal(got["AH"], before["AHk"])
        np.testing.assert_array_equal(G.cpu().numpy(), gk0)


# ------------------------------------------------------------------------------------------------ (b) the 1 x 1 fixtures
def _args(k, itr, **kw):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.utils import parse
    comms = MPI_comm(None, 1, 1)
    args = parse()
    args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, 1, 1, k
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    args.itr, args.init, args.verbose, args.prune = itr, "rand", False, False
    args.norm, args.method, args.W_update = "fro", "bcd", True
    for key, v in kw.items():
        setattr(args, key, v)
    return args


@pytest.mark.parametrize("name", bcd_case_names((1, 1)))
def test_bcd_fixture_whole_fit_equals_python_loop(name):
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    meta, A, W0, H0, z = load_bcd(name)
    k = meta["k"]
    for N in meta["steps"]:
        nmf = PyNMF(A, factors=[W0, H0], params=_args(k, N))
        W, H = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params).update()
        dw, dh = rel_fro(W.cpu().numpy(), z["r0_step%d_W" % N]), rel_fro(H.cpu().numpy(), z["r0_step%d_H" % N])
        assert dw <= 1e-5 * N and dh <= 1e-5 * N, (name, N, dw, dh)
    for N in meta["itrs"]:
        fits = [PyNMF(A, factors=[W0, H0], params=_args(k, N, **kw)).fit() for kw in ({}, {"fit_loop": "python"})]
        (W1, H1, e1), (W2, H2, e2) = fits
        np.testing.assert_array_equal(W1, W2)
        np.testing.assert_array_equal(H1, H2)
        assert e1 == e2
        assert W1.dtype == z["r0_fit%d_W" % N].dtype
        dw, dh, de = rel_fro(W1, z["r0_fit%d_W" % N]), rel_fro(H1, z["r0_fit%d_H" % N]), abs(e1 - float(z["r0_fit%d_err" % N]))
        assert dw <= 1e-4 and dh <= 1e-4 and de <= 1e-5, (name, N, dw, dh, de)


def test_bcd_whole_fit_is_one_library_call(monkeypatch):
    """A single-rank fit goes through HipOps.fit once (dnmf_bcd_fro_fit) and never through the step primitives."""
    from pydnmfk_amd import engine
    from pydnmfk_amd.pyDNMF import PyNMF
    meta, A, W0, H0, _ = load_bcd("t24x12_1x1")
    calls = []
    real_fit = engine.HipOps.fit

    def fit(self, *a, **kw):
        calls.append(a[0])
        return real_fit(self, *a, **kw)
    monkeypatch.setattr(engine.HipOps, "fit", fit)
    monkeypatch.setattr(engine.HipOps, "bcd_update_w", lambda *a, **kw: pytest.fail("step primitive called"))
    PyNMF(A, factors=[W0, H0], params=_args(meta["k"], 20)).fit()
    assert calls == ["bcd"]


# ------------------------------------------------------------------------------------------------ (c) stacked ranks
@pytest.mark.parametrize("name", [nm for nm in bcd_case_names() if not nm.endswith("_1x1")])
def test_bcd_fixture_on_stacked_ranks(name):
    check_tolerances(name, run_bcd(name, use_hip=True))


# ------------------------------------------------------------------------------------------------ (d) the reference's acceptance
@pytest.mark.parametrize("grid", [(1, 1), (1, 2), (2, 1)])
def test_bcd_reference_acceptance(grid):
    """the reference's tests/test_dist_nmf_1d.py:39-47 loops over ['mu', 'bcd', 'hals'] and asserts rel_err < 1e-3"""
    from tests._bcd import run_acceptance
    errs = run_acceptance(grid, 2000)
    assert all(e < 1e-3 for e in errs), errs


# ------------------------------------------------------------------------------------------------ (e) determinism, (f) batch / NMFk
def test_bcd_fits_are_bit_identical():
    from pydnmfk_amd.pyDNMF import PyNMF
    meta, A, W0, H0, _ = load_bcd("swim_1x1")
    a = PyNMF(A, factors=[W0, H0], params=_args(meta["k"], 50)).fit()
    b = PyNMF(A, factors=[W0, H0], params=_args(meta["k"], 50)).fit()
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2]


def test_bcd_fit_batch_equals_single_fits():
    from pydnmfk_amd.pyDNMF import PyNMF
    meta, A, _, _, _ = load_bcd("swim_1x1")
    rs = np.random.RandomState(5)
    inits = [(rs.rand(A.shape[0], 4), rs.rand(4, A.shape[1])) for _ in range(3)]
    batch = PyNMF.fit_batch([PyNMF(A, factors=list(f), params=_args(4, 30)) for f in inits])
    single = [PyNMF(A, factors=list(f), params=_args(4, 30)).fit() for f in inits]
    for (W1, H1, e1), (W2, H2, e2) in zip(batch, single):
        np.testing.assert_array_equal(W1, W2)
        np.testing.assert_array_equal(H1, H2)
        assert e1 == e2


def test_bcd_nmfk_sweep(tmp_path):
    from pydnmfk_amd.pyDNMFk import PyNMFk
    meta, A, _, _, _ = load_bcd("t24x12_1x1")
    args = _args(2, 200)
    args.fpath, args.fname, args.ftype = str(tmp_path) + "/", "t24", "npy"
    args.start_k, args.end_k, args.step_k, args.sill_thr, args.perturbations = 1, 3, 1, 0.6, 3
    args.checkpoint, args.results_path = False, str(tmp_path) + "/results/"
    k_opt = PyNMFk(A, factors=None, params=args).fit()
    assert 1 <= k_opt <= 3


# ------------------------------------------------------------------------------------------------ (g) refused combinations
@pytest.mark.parametrize("combo", ["float64", "bfloat16", "bf16x6"])
def test_bcd_refused_combinations(combo):
    from pydnmfk_amd.pyDNMF import PyNMF
    meta, A, W0, H0, _ = load_bcd("t24x12_1x1")
    kw = {"precision": "bfloat16"} if combo == "bfloat16" else ({"gemm": "bf16x6"} if combo == "bf16x6" else {})
    data = A.astype(np.float64) if combo == "float64" else A
    with pytest.raises(NotImplementedError, match="bcd"):
        PyNMF(data, factors=[W0, H0], params=_args(meta["k"], 5, **kw)).fit()
