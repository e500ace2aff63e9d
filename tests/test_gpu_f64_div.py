"""norm='is' and norm='beta' on float64 data (csrc/dnmf_f64_div.h; needs a GPU): the pairs, the rules and the divergence against a long-double
statement, exact operands on one and on several column splits / row chunks, fits through PyNMF on one rank and on the 1D grids, refusals."""
import traceback

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _beta as B  # noqa: E402
from tests import _exact as E  # noqa: E402
from tests import _is as I  # noqa: E402
from tests.test_f64_div_cpu import EPS64, LD, statement  # noqa: E402

BOUND = 1.9e-14                      # the family's fp32 bound for these operations (1e-5) scaled by eps64 / eps32
MODES = ("is", -2.0, -1.0, 0.3, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0)      # 0.3 takes the general power
SEEN = {}


def _ops():
    from pydnmfk_amd import engine
    return engine.HIP_OPS_F64


def _rel(got, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.linalg.norm((np.asarray(got, dtype=LD) - ref).ravel()) / np.linalg.norm(ref.ravel()))


def _call(mode, name, *a):
    """ops.<norm>_<name>(*a) with "eps" in `a` standing for eps, and under norm='beta' for eps, beta"""
    fn = getattr(_ops(), ("is_" if mode == "is" else "beta_") + name)
    i = [isinstance(x, str) and x == "eps" for x in a].index(True)
    return fn(*a[:i], EPS64, *(() if mode == "is" else (mode,)), *a[i + 1:])


# ---- 1. against the long-double statement
@pytest.mark.parametrize("mode", MODES, ids=str)
@pytest.mark.parametrize("k", (3, 16, 33, 64))
@pytest.mark.parametrize("shape", I.EXACT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_pairs_updates_divergence_against_long_double(shape, k, mode):
    """every pair half, both updated factors and the divergence within 1.9e-14 of the long-double statement, on contiguous tensors and
    on odd-start, odd-pitch views inside NaN-poisoned buffers; the fused update equals the rule on the stored pair bit for bit.
    Measured maxima (MI355X): see DESIGN.md section 7."""
    m, n = shape
    A, W, H, _ = B.problem(m, n, k, seed=7, zeros=0.3 if mode != "is" and mode > 0 else 0.0)
    ref = statement(A, W, H, None if mode == "is" else mode)
    worst = {}
    for packed in (True, False):
        P = lambda x: E.Poisoned(torch, x, aligned=packed, packed=packed)      # noqa: E731
        Av, Wv, Hv = P(A), P(W), P(H)
        for side, X, Xv in (("w", W, Wv), ("h", H, Hv)):
            num, den = (E.Poisoned.out(torch, *X.shape, torch.float64, aligned=packed) for _ in range(2))
            _call(mode, "pair_into", side, Av.view, Wv.view, Hv.view, "eps", num.view, den.view)
            gn, gd = num.check(side + " num"), den.check(side + " den")
            worst[side + " num"], worst[side + " den"] = _rel(gn, ref[side][0]), _rel(gd, ref[side][1])
            by_rule = P(X)
            _call(mode, "ratio_update", by_rule.view, num.view, den.view, "eps")
            fused = [P(W), P(H)]
            _call(mode, "update_" + side, Av.view, *(f.view for f in fused), "eps")
            got = fused[side == "h"].check("update_" + side)
            assert np.array_equal(got, by_rule.check("ratio_update")), (side, packed)
            assert np.array_equal(fused[side == "w"].check("the other factor"), H if side == "w" else W)
            worst["update_" + side] = _rel(got, ref["upd_" + side])
        d1 = float(_call(mode, "divergence", Av.view, Wv.view, Hv.view, "eps").cpu())
        d2 = float(_call(mode, "divergence", Av.view, Wv.view, Hv.view, "eps").cpu())
        assert d1 == d2
        worst["divergence"] = abs(float(LD(d1) - ref["div"])) / float(ref["div_scale"])
        for v, x in ((Av, A), (Wv, W), (Hv, H)):
            assert np.array_equal(v.check("operand"), x)
        print("f64 %s %dx%d k=%d packed=%s: %s" % (mode, m, n, k, packed, " ".join("%s=%.2e" % kv for kv in sorted(worst.items()))))
        for what, err in worst.items():
            SEEN[what] = max(SEEN.get(what, 0.0), err)
            assert err <= BOUND, (what, err, packed)
    print("f64 div maxima so far:", " ".join("%s=%.2e" % kv for kv in sorted(SEEN.items())))


# ---- 2. exact operands: one column split / row chunk (48 x 80) and several of each (130 x 1100: two splits, three chunks)
@pytest.mark.parametrize("beta", (0.0, 2.0))
@pytest.mark.parametrize("k", (16, 64))
@pytest.mark.parametrize("shape", ((48, 80), (130, 1100)), ids=lambda s: "%dx%d" % s)
def test_exact_operands(shape, k, beta):
    """W holds one power of two per row, H powers of two, A small integers: S is a power of two >= 2 that absorbs eps, so R and A R R
    (beta = 0) and P = 1 (beta = 2) make every sum exact in any order -- num and den of both sides equal the answers element by element"""
    m, n = shape
    A, W, H, ref = I.exact_problem(m, n, k) if beta == 0.0 else B.exact_problem(m, n, k, 2)
    A, W, H = (x.astype(np.float64) for x in (A, W, H))
    assert np.array_equal(W @ H + EPS64, W @ H)
    for packed in (True, False):
        Av, Wv, Hv = (E.Poisoned(torch, x, aligned=packed, packed=packed) for x in (A, W, H))
        for side, X in (("w", W), ("h", H)):
            num, den = (E.Poisoned.out(torch, *X.shape, torch.float64, aligned=packed) for _ in range(2))
            _ops().beta_pair_into(side, Av.view, Wv.view, Hv.view, EPS64, beta, num.view, den.view)
            for what, got, want in (("num", num, ref[side][0]), ("den", den, ref[side][1])):
                g = got.check(what)
                assert np.array_equal(g, want), (side, what, packed, int((g != want).sum()))
        if beta == 0.0:                                             # norm='is' is the same pair
            num, den = (E.Poisoned.out(torch, m, k, torch.float64, aligned=packed) for _ in range(2))
            _ops().is_pair_into("w", Av.view, Wv.view, Hv.view, EPS64, num.view, den.view)
            assert np.array_equal(num.check("num"), ref["w"][0]) and np.array_equal(den.check("den"), ref["w"][1])


# ---- 3. fits through the public interface: 200 x 136, k = 5, 30 steps
FIT = (200, 136, 5, 30)
FIT_MODES = (("is", None), ("beta", 0.5))


def _fit_args(comms, grid, norm, beta, itr):
    m, n, k, _ = FIT
    return I.args_for(comms, grid[0], grid[1], k, itr, norm=norm) if norm == "is" else B.args_for(comms, grid[0], grid[1], k, itr, beta)


def _fit_rank(rank, world, port, grid, q):
    """this rank's slice of the float64 problem: per norm the 30-step fit and its divergence; on one rank the fits of 1, 2, ..., 30 steps
    from the same factors (the same steps: the clamps fall on the same i), whose divergences are the objective along the fit"""
    try:
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        I._setup_rank(rank, world, port, True)
        m, n, k, itr = FIT
        A, W0, H0, _ = I.problem(m, n, k)
        comms = MPI_comm(None, grid[0], grid[1])
        sl, (w0, w1), (h0, h1) = I._slices(rank, grid, A.shape)
        out = {}
        for norm, beta in FIT_MODES:
            divs = []
            for steps in ((itr,) if world > 1 else range(1, itr + 1)):
                nmf = PyNMF(A[sl], factors=[W0[w0:w1], H0[:, h0:h1]], params=_fit_args(comms, grid, norm, beta, steps))
                assert nmf._ops().name == "hip-f64"
                W, H, err = nmf.fit()
                divs.append(nmf.is_divergence() if norm == "is" else nmf.beta_divergence())
            out[norm] = ((w0, w1), (h0, h1), np.asarray(W), np.asarray(H), float(err), divs)
        q.put((rank, out, None))
        I._teardown_rank(world)
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("grid", ((1, 1), (2, 1), (1, 2)), ids=lambda g: "%dx%d" % g)
def test_fit_through_pynmf(grid):
    """W, H and the error within 1e-10 of the float64 statement (tests/_is.py, tests/_beta.py with eps = EPS64), float64 factors back,
    and on one rank the divergence never rises along the 30 steps by more than 1e-12 of its value"""
    m, n, k, itr = FIT
    A, W0, H0, _ = I.problem(m, n, k)
    res = I.spawn(_fit_rank, grid, (), 300)
    for norm, beta in FIT_MODES:
        Wr, Hr, err_r = I.fit(A, W0, H0, itr, EPS64) if norm == "is" else B.fit(A, W0, H0, beta, itr, EPS64)
        W, H = np.full((m, k), np.nan), np.full((k, n), np.nan)
        for rank, out in res:
            (w0, w1), (h0, h1), Wp, Hp, err, divs = out[norm]
            assert Wp.dtype == np.float64 and Hp.dtype == np.float64
            W[w0:w1], H[:, h0:h1] = Wp, Hp
            assert abs(err - err_r) <= 1e-10, (norm, rank, err, err_r)
            d = np.asarray(divs)
            assert np.all(np.diff(d) <= 1e-12 * np.abs(d[:-1])), (norm, d)
            want = I.divergence(A, Wr, Hr, EPS64) if norm == "is" else B.divergence(A, Wr, Hr, beta, EPS64)
            assert abs(d[-1] - want) <= 1e-10 * abs(want), (norm, d[-1], want)
        print("f64 fit %s %dx%d: rel dW=%.2e dH=%.2e" % (norm, grid[0], grid[1], _rel(W, Wr), _rel(H, Hr)))
        assert _rel(W, Wr) <= 1e-10 and _rel(H, Hr) <= 1e-10, (norm, grid)


# ---- 4. what stays refused
def test_refusals():
    from pydnmfk_amd.pyDNMF import PyNMF
    from pydnmfk_amd.pyDNMFk import PyNMFk
    A = np.ones((4, 200))
    for norm, kw in (("is", {}), ("beta", {"beta": 0.5})):
        with pytest.raises(NotImplementedError, match="norm='%s'.*k = 65.*1 <= k <= 64" % norm):
            PyNMF(A, params=I.one_rank_args(65, 3, norm=norm, **kw))
    with pytest.raises(NotImplementedError, match="PyNMFk with norm='is' is not provided by operator set 'hip-f64'"):
        PyNMFk(A, params=I.one_rank_args(3, 3))
