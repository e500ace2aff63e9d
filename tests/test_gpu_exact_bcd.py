"""The BCD kernels (csrc/dnmf_bcd.h) element by element, at the sizes their loops are built for.

The projected-gradient step runs on `bcd_pg_problem` operands (tests/_exact.py, proved in every summation order by
tests/test_exact_cpu.py): with L = 2^6 every element of the result is the float64 answer and the column sums are float32(exact sum);
with L = float32(||G||_F) the product is still exact and the quotient, the subtraction and the clamp are one IEEE operation each, so
the result equals the numpy float32 expression bit for bit (the column sums keep the 1e-5 relative bound of tests/test_gpu_bcd.py
there: their order is the kernel's).  The Gram buffers carry NaN in their padding -- rows >= k and the columns up to KP -- and the
state block NaN in every slot a kernel has no business reading.  The element-wise kernels run past one trip of their grid-stride
loops (more than 8192 x 256 elements) and the column sums past 256 workgroup partials, against the numpy float32 expressions of the
small tests.  Operands are views in NaN-poisoned buffers, outputs views in sentinel-filled ones (tests/test_gpu_exact.py).

Whole fits at tall and wide-rank shapes are held to the numpy checker (tests/_bcd.BcdOracleOps) run on the CPU, after asserting from
the checker's own decisions that none is a near tie: see test_whole_fit_against_the_checker."""
import numpy as np
import pytest

from tests import _exact as ex
from tests._bcd import ACC, LH, LH_OLD, LW, LW_OLD, OBJ, OBJ_OLD, SH, SW, WH, WW, XN, BcdOracleOps, check_tolerances
from tests._golden import rel_fro

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = np.float32
EW_TRIP = 8192 * 256                                              # elements of one trip of an element-wise kernel (ew_grid, csrc/dnmf_bcd.hip)


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pydnmfk_amd import engine
    return engine, engine.HIP_OPS


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want, dtype=F32)
    assert got.dtype == F32 and got.shape == want.shape, what
    bad = _bits(got) != _bits(want)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ in bits; first at %s: got %r (0x%08x), expected %r (0x%08x)"
                             % (what, int(bad.sum()), bad.size, i, got[i].item(), _bits(got)[i], want[i].item(), _bits(want)[i]))


def _nan_gram(engine, g):
    """g in the k x k corner of the KP x KP buffer, NaN everywhere else"""
    k = g.shape[0]
    n = engine.kp(k)
    G = torch.full((n, n), NAN, dtype=torch.float32, device="cuda")
    G[:k, :k] = torch.from_numpy(np.ascontiguousarray(g, dtype=F32)).cuda()
    return G


def _gram_intact(G, g, what):
    k = g.shape[0]
    b = G.cpu().numpy()
    assert np.array_equal(b[:k, :k], g) and np.isnan(b[k:]).all() and np.isnan(b[:k, k:]).all(), what + ": the Gram buffer was written"


def _state(**slots):
    """NaN in every slot but the named ones"""
    st = torch.full((16,), NAN, dtype=torch.float64)
    for key, v in slots.items():
        st[{"LW": LW, "LH": LH, "LW_OLD": LW_OLD, "LH_OLD": LH_OLD, "ACC": ACC, "WW": WW, "WH": WH, "XN": XN, "SW": SW, "SH": SH}[key]] = v
    return st.cuda()


def _run_pg(env, P, side, aligned, what, nan_ok=False):
    """one step on the problem P; returns the output, s (W side) and checks that no operand, padding or guard element changed"""
    engine, ops = env
    k = P["G"].shape[0]
    Xv = ex.Poisoned(torch, P["Xm"], aligned=aligned[0])
    Pv = ex.Poisoned(torch, P["P"], aligned=aligned[1])
    Ov = ex.Poisoned.out(torch, P["Xm"].shape[0], P["Xm"].shape[1], torch.float32, aligned=aligned[2])
    G = _nan_gram(engine, P["G"])
    s = None
    if side == "w":
        st = _state(LW=P["L"])
        s = torch.full((k + 5,), 7.0, dtype=torch.float32, device="cuda")
        ops.bcd_update_w(Xv.view, Pv.view, G, st, Ov.view, s[:k])
        s = s.cpu().numpy()
        assert (s[k:] == 7.0).all(), what + ": s was written past k"
        s = s[:k]
    else:
        st = _state(LH=P["L"])
        ops.bcd_update_h(Xv.view, Pv.view, G, st, Ov.view)
    out = Ov.check(what, allow_nan=nan_ok)
    assert np.array_equal(_bits(Xv.check(what + ": Xm", allow_nan=nan_ok)), _bits(P["Xm"])), what + ": Xm was written"
    assert np.array_equal(Pv.check(what + ": P"), P["P"]), what + ": P was written"
    _gram_intact(G, P["G"], what)
    return out, s


def _check_pg(env, R, k, side, L, aligned, seed=0):
    P = ex.bcd_pg_problem(R, k, seed=seed, L=L, side=side)
    what = "%s side, %d x %d, L = %r, aligned %s" % (side, R, k, P["L"], aligned)
    out, s = _run_pg(env, P, side, aligned, what)
    ex.assert_ulp(out, P["expected"], 0, what, tile=(64, 16) if side == "w" else (16, 64))
    _same_bits(out, P["expected"], what)
    if side == "w":
        if P["pow2"]:
            _same_bits(s, P["s"], what + ": column sums")
        else:
            exact = out.astype(np.float64).sum(0)
            assert np.abs(s - exact).max() <= 1e-5 * np.abs(out).sum(0).max(), what + ": column sums"
    return P


# ------------------------------------------------------------------------------------------------ the projected-gradient step
@pytest.mark.parametrize("side", ["w", "h"])
@pytest.mark.parametrize("k", ex.BCD_PG_K)
def test_pg_step(env, k, side):
    """bcd_pg_kernel<false> / <true> at every rank that sits on a 16-column wave group, the 32-wide LDS slab, a 4-wave blockIdx.y
    group or a KP, with 1, 63, 64, 65 and 131 rows: L = 2^6 -- the float64 answer; L = ||G||_F -- the numpy float32 expression"""
    for R in ex.BCD_PG_R:
        for n, L in enumerate((ex.BCD_L, None)):
            v = R + k + n
            P = _check_pg(env, R, k, side, L, (v % 2 == 0, v % 3 == 0, v % 2 == 1), seed=k)
            if R * k >= 100:
                sh = P["shares"]
                assert sh["clamped"] >= 0.1 and sh["zero"] >= 0.1 and sh["positive"] >= 0.3, sh


@pytest.mark.parametrize("L", [ex.BCD_L, None], ids=["L2^6", "Lnorm"])
@pytest.mark.parametrize("m,k", ex.BCD_COLSUM)
def test_column_sums_beyond_256_partials(env, m, k, L):
    """bcd_colsum_kernel takes a second (19137 rows: 300 partials, the last workgroup one row) and a third trip (40001: 626)"""
    assert -(-m // 64) > 256
    if (m, k) == (19137, 17):
        assert -(-m // 64) == 300 and m % 64 == 1
    _check_pg(env, m, k, "w", L, (True, False, m % 2 == 0), seed=1)


@pytest.mark.parametrize("side,R,k", [("w", 131, 17), ("w", 65, 1), ("h", 131, 17), ("h", 203, 33)])
def test_pg_step_keeps_a_nan(env, side, R, k):
    """"a NaN stays NaN": one NaN in Xm makes exactly its row (H side: its column) of the result NaN -- NaN * 0 included -- and every
    column sum; every other element is the exact answer"""
    for L in (ex.BCD_L, None):
        P = ex.bcd_pg_problem(R, k, seed=3, L=L, side=side)
        i, c = R - 61, k // 2
        P["Xm"][(i, c) if side == "w" else (c, i)] = NAN
        what = "%s side, %d x %d, NaN at element (%d, %d), L = %r" % (side, R, k, i, c, P["L"])
        out, s = _run_pg(env, P, side, (True, False, True), what, nan_ok=True)
        out, want = (out, P["expected"]) if side == "w" else (out.T, P["expected"].T)
        assert np.isnan(out[i]).all(), what + ": the NaN was dropped"
        rest = np.arange(R) != i
        _same_bits(out[rest], want[rest], what + ": the other rows")
        if side == "w":
            assert np.isnan(s).all(), what + ": a column sum lost the NaN"


def test_zero_column_sum_scales_to_nan_and_inf(env):
    """"a zero column sum gives inf / NaN, as in the reference": a column of W clamped to 0 throughout has s = 0 and becomes 0 / 0;
    then bcd_scale_cols alone against numpy's float32 x / 0 and x / tiny (a subnormal and a small normal sum)"""
    _, ops = env
    R, k, c0 = 131, 17, 5
    P = ex.bcd_pg_problem(R, k, seed=4, side="w")
    S = P["Xm"].astype(np.float64) @ P["G"].astype(np.float64)
    P["P"][:, c0] = (S[:, c0] - ex.BCD_L * (P["Xm"][:, c0] + 1)).astype(F32)
    P["expected"][:, c0] = 0.0
    Xv, Pv = ex.Poisoned(torch, P["Xm"]), ex.Poisoned(torch, P["P"], aligned=False)
    Wv = ex.Poisoned.out(torch, R, k, torch.float32, aligned=False)
    s = torch.full((k,), 7.0, dtype=torch.float32, device="cuda")
    ops.bcd_update_w(Xv.view, Pv.view, _nan_gram(env[0], P["G"]), _state(LW=P["L"]), Wv.view, s)
    w = Wv.check("update_w")
    _same_bits(w, P["expected"], "update_w with a dead column")
    sn = s.cpu().numpy()
    _same_bits(sn, P["expected"].sum(0).astype(F32), "column sums")
    assert sn[c0] == 0.0 and (np.delete(sn, c0) > 0).all()
    ops.bcd_scale_cols(Wv.view, s)
    with np.errstate(all="ignore"):
        want = w / sn[None, :]
    got = Wv.check("scale_cols", allow_nan=True)
    assert np.isnan(want[:, c0]).all() and np.array_equal(np.isnan(got), np.isnan(want)), "0 / 0 is not NaN where numpy's is"
    _same_bits(got[~np.isnan(want)], want[~np.isnan(want)], "scale_cols beside the dead column")
    # x / 0, 0 / 0 and x / tiny
    rs = np.random.RandomState(8)
    x = (rs.rand(70, 6) + 0.25).astype(F32)
    x[::3, 1] = 0.0
    x[:, 2] = 0.0
    sv = np.array([0.0, 0.0, 0.0, 2.0 ** -130, 2.0 ** -120, 3.0], dtype=F32)
    assert sv[3] > 0 and sv[3] < np.finfo(F32).tiny
    Xs = ex.Poisoned(torch, x, aligned=False)
    ops.bcd_scale_cols(Xs.view, torch.from_numpy(sv).cuda())
    got = Xs.check("scale_cols", allow_nan=True)
    with np.errstate(all="ignore"):
        want = x / sv[None, :]
    assert np.isinf(want[:, 0]).all() and np.isnan(want[:, 2]).all() and np.isinf(want[:, 3]).all() and np.isfinite(want[:, 4]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), "NaN / inf not where numpy has them"
    _same_bits(got[~np.isnan(want)], want[~np.isnan(want)], "scale_cols by 0 and by tiny sums")


# ------------------------------------------------------------------------------------------------ the Lipschitz bound
@pytest.mark.parametrize("k", [1, 15, 16, 17, 33, 256])
def test_lipschitz_stops_at_k(env, k):
    """L = float32(sqrt(sum G[:k, :k]^2)) on an integer Gram (the sum of squares is exact) with NaN padding; L_old moved; nothing else"""
    engine, ops = env
    rs = np.random.RandomState(40 + k)
    for which, slot in ((0, LW), (1, LH)):
        g = rs.randint(0, 6, size=(k, k)).astype(F32)
        g[0, 0] = max(g[0, 0], 1)
        G = _nan_gram(engine, g)
        before = np.arange(16, dtype=np.float64) + 100.25
        st = torch.from_numpy(before.copy()).cuda()
        ops.bcd_lipschitz(G, k, st, which)
        got = st.cpu().numpy()
        ssq = int((g.astype(np.int64) ** 2).sum())
        want = before.copy()
        want[slot + 1], want[slot] = before[slot], float(F32(np.sqrt(float(ssq))))
        assert got[slot] == want[slot], "k = %d: L = %r, expected %r (sum of squares %d)" % (k, got[slot], want[slot], ssq)
        assert np.array_equal(got, want), "k = %d: the state block" % k
        _gram_intact(G, g, "lipschitz")


# ------------------------------------------------------------------------------------------------ grid-stride loops, second trip
BIG_MK = [(8200, 256), (699051, 3)]


@pytest.mark.parametrize("m,k", BIG_MK)
def test_scale_cols_second_trip(env, m, k):
    _, ops = env
    assert m * k > EW_TRIP
    rs = np.random.RandomState(m + k)
    w = rs.rand(m, k).astype(F32)
    s = (rs.rand(k) + 0.5).astype(F32)
    for aligned in (True, False):
        Wv = ex.Poisoned(torch, w, aligned=aligned)
        ops.bcd_scale_cols(Wv.view, torch.from_numpy(s).cuda())
        _same_bits(Wv.check("scale_cols"), w / s[None, :], "scale_cols %d x %d%s" % (m, k, "" if aligned else ", odd start and pitch"))


@pytest.mark.parametrize("pair", ["pow2", "generic"])
@pytest.mark.parametrize("rows,cols,which", [(8200, 256, 0), (699051, 3, 0), (256, 8200, 1), (3, 699051, 1)])
def test_init_factor_second_trip(env, rows, cols, which, pair):
    """X_old = X_m = X0 / a * b in float32, a = float32(sqrt(sum X0^2)), b = float32(sqrt(sqrt(sum A^2))) read from the state block:
    powers of two (sum X0^2 = 4^3, sum A^2 = 16^5) and a generic pair"""
    _, ops = env
    assert rows * cols > EW_TRIP
    sx, xn = (4.0 ** 3, 16.0 ** 5) if pair == "pow2" else (3.0, 12.5)
    rs = np.random.RandomState(rows + cols)
    x0 = rs.rand(rows, cols).astype(F32)
    st = _state(XN=xn, **{"SW" if which == 0 else "SH": sx})
    X0 = ex.Poisoned(torch, x0, aligned=(which == 0))
    Xo = ex.Poisoned.out(torch, rows, cols, torch.float32, aligned=(which == 1))
    Xm = ex.Poisoned.out(torch, rows, cols, torch.float32, aligned=(pair == "pow2"))
    ops.bcd_init_factor(X0.view, Xo.view, Xm.view, st, which)
    a, b = F32(np.sqrt(sx)), F32(np.sqrt(np.sqrt(xn)))
    if pair == "pow2":
        assert (a, b) == (8.0, 32.0)
    want = x0 / a * b
    assert want.dtype == F32
    _same_bits(Xo.check("X_old"), want, "X_old")
    _same_bits(Xm.check("X_m"), want, "X_m")
    assert np.array_equal(X0.check("X0"), x0)


@pytest.mark.parametrize("accept", [True, False], ids=["accept", "restart"])
@pytest.mark.parametrize("m,n,k", [(8200, 5, 256), (699051, 7, 3), (5, 8200, 256), (7, 699051, 3)])
def test_extrapolate_second_trip(env, m, n, k, accept):
    """bcd_extrapolate_kernel past one trip, the m x k jobs the larger ones and the k x n job the larger one, in both branches:
    p = x + w (x - o) uncontracted and o = x, or p = o and the kept products back"""
    engine, ops = env
    assert max(m * k, k * n) > EW_TRIP
    rs = np.random.RandomState(m + n + k + accept)

    def P(r, c, al):
        return ex.Poisoned(torch, rs.rand(r, c).astype(F32), aligned=al)
    bufs = dict(W=P(m, k, True), Wo=P(m, k, False), Wm=P(m, k, True), H=P(k, n, False), Ho=P(k, n, True), Hm=P(k, n, False), AH=P(m, k, False),
                AHk=P(m, k, True))
    kp = engine.kp(k)
    G, Gk = (torch.from_numpy(rs.rand(kp, kp).astype(F32)).cuda() for _ in range(2))
    before = {nm: t.view.cpu().numpy().copy() for nm, t in bufs.items()}
    g0, gk0 = G.cpu().numpy().copy(), Gk.cpu().numpy().copy()
    st = _state(ACC=1.0 if accept else 0.0, WW=0.375 + 2.0 ** -20, WH=0.6)
    b = {nm: t.view for nm, t in bufs.items()}
    ops.bcd_extrapolate(b["W"], b["Wo"], b["Wm"], b["H"], b["Ho"], b["Hm"], b["AH"], b["AHk"], G, Gk, st)
    got = {nm: t.check(nm) for nm, t in bufs.items()}
    _same_bits(got["W"], before["W"], "W")
    _same_bits(got["H"], before["H"], "H")
    if accept:
        for x, o, p, w in (("W", "Wo", "Wm", 0.375 + 2.0 ** -20), ("H", "Ho", "Hm", 0.6)):
            _same_bits(got[p], before[x] + F32(w) * (before[x] - before[o]), p)
            _same_bits(got[o], before[x], o)
        _same_bits(got["AHk"], before["AH"], "AH kept")
        _same_bits(got["AH"], before["AH"], "AH")
        assert np.array_equal(Gk.cpu().numpy(), g0) and np.array_equal(G.cpu().numpy(), g0)
    else:
        _same_bits(got["Wm"], before["Wo"], "Wm")
        _same_bits(got["Hm"], before["Ho"], "Hm")
        _same_bits(got["Wo"], before["Wo"], "W_old")
        _same_bits(got["Ho"], before["Ho"], "H_old")
        _same_bits(got["AH"], before["AHk"], "AH")
        _same_bits(got["AHk"], before["AHk"], "AH kept")
        assert np.array_equal(G.cpu().numpy(), gk0) and np.array_equal(Gk.cpu().numpy(), gk0)


# ------------------------------------------------------------------------------------------------ whole fits against the checker
class _Recorder(BcdOracleOps):
    """the checker, keeping every decision's (obj_old before it, obj, accepted)"""

    def __init__(self):
        self.decisions = []

    def bcd_decide(self, st, sq):
        old = float(st.numpy()[OBJ_OLD])
        super().bcd_decide(st, sq)
        self.decisions.append((old, float(st.numpy()[OBJ]), bool(st.numpy()[ACC])))


FITS = [(40001, 67, 4, 3, (35793, 35091, 35066)), (19137, 80, 17, 3, (22377, 22172, 22162)), (8200, 300, 256, 2, (32786, 32596)),
        (2049, 515, 200, 3, (14937, 14861, 14851))]


@pytest.mark.parametrize("m,n,k,itr,objs", FITS, ids=["%dx%d-k%d" % f[:3] for f in FITS])
def test_whole_fit_against_the_checker(env, m, n, k, itr, objs):
    """dnmf_bcd_fro_fit at tall m, m k > 2^21 and the wide ranks -- shapes at which a fit was only ever compared with itself -- equals
    the Python choreography bit for bit, and both meet the numpy checker run on the CPU at the project's fit tolerances (rel-Frobenius
    <= 1e-4 on W and H, |d err| <= 1e-5).  Precondition, asserted from the checker's decisions: every iteration accepts and lowers the
    objective by at least 1e-4 relative -- ten times the 1e-5 the residual sums are held to -- so no decision is a near tie.
    The checker's objectives per iteration are the `objs` of FITS.
    Measured on an MI355X against the checker (rel-Fro W, rel-Fro H, |d err|):
        40001 x 67 k = 4, 3 iterations    1.41e-06  1.41e-06  2.32e-07
        19137 x 80 k = 17, 3 iterations   1.61e-06  1.60e-06  1.18e-07
        8200 x 300 k = 256, 2 iterations  1.37e-06  1.22e-06  2.07e-07
        2049 x 515 k = 200, 3 iterations  8.89e-07  7.53e-07  7.33e-08
    and between the library fit and the Python choreography: W and H bit-equal, the error equal or one ulp of the double apart."""
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests.test_gpu_bcd import _args
    rs = np.random.RandomState(m + n + k)
    A = (rs.rand(m, 5) @ rs.rand(5, n) + 0.01 * rs.rand(m, n)).astype(F32)
    W0, H0 = rs.rand(m, k).astype(F32), rs.rand(k, n).astype(F32)
    rec = _Recorder()
    Wc, Hc, ec = PyNMF(A, factors=[W0, H0], params=_args(k, itr), ops=rec).fit()
    assert len(rec.decisions) == itr
    for it, (old, obj, acc) in enumerate(rec.decisions):
        assert acc and (old - obj) >= 1e-4 * old, "iteration %d of the checker: %r -> %r, accepted %r" % (it, old, obj, acc)
        assert abs(obj - objs[it]) <= 1e-3 * objs[it], "iteration %d: the checker's objective %r, expected about %d" % (it, obj, objs[it])
    (W1, H1, e1), (W2, H2, e2) = [PyNMF(A, factors=[W0, H0], params=_args(k, itr, **kw)).fit() for kw in ({}, {"fit_loop": "python"})]
    _same_bits(W1, W2, "W: library fit against the Python choreography")
    _same_bits(H1, H2, "H: library fit against the Python choreography")
    # (the two squared norms behind the error are fp64 atomic sums over the workgroups, whose order is free: 1e-12 relative, as
    # tests/test_gpu_bcd_batch.py and tests/test_gpu_fit.py hold them; measured here: equal or one ulp of the double apart)
    assert abs(e1 - e2) <= 1e-12 * max(1.0, abs(e2)), (e1, e2)
    assert W1.dtype == Wc.dtype and np.isfinite(W1).all() and np.isfinite(H1).all()
    dw, dh, de = rel_fro(W1, Wc), rel_fro(H1, Hc), abs(e1 - ec)
    print("bcd fit %d x %d k = %d, %d iterations: rel-Fro W %.3g, H %.3g, |d err| %.3g" % (m, n, k, itr, dw, dh, de))
    check_tolerances("%dx%d k%d" % (m, n, k), {0: {"fit%d" % itr: (dw, dh, de)}})
