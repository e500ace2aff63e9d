"""norm='huber' on the GPU (csrc/dnmf_huber.h) against the float64 statement of tests/_huber.py; the bounds of tests/test_gpu_beta.py"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from pydnmfk_amd.engine import HIP_OPS as OPS  # noqa: E402
from tests import _exact as E  # noqa: E402
from tests import _huber as Hb  # noqa: E402
from tests import _is as I  # noqa: E402
from tests._golden import rel_fro  # noqa: E402

EPS, INF, BOUND, FIT_BOUND, ERR_BOUND = Hb.EPS, float("inf"), 1e-5, 1e-4, 1e-5


def _pynmf(A, W0, H0, itr, **kw):
    from pydnmfk_amd.pyDNMF import PyNMF
    return PyNMF(torch.from_numpy(A).cuda(), factors=[torch.from_numpy(W0).cuda(), torch.from_numpy(H0).cuda()],
                 params=I.one_rank_args(W0.shape[1], itr, **kw))


@pytest.mark.parametrize("shape", I.EXACT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_pairs_updates_and_loss_against_float64(shape):
    """A = W H with noise of +-10 % and, at 10 % of the entries, spikes of 5 to 10 times its mean; delta = 7 % of that mean, inside the noise:
    both branches occur, many residuals lie near delta.  Aligned (vector kernels where n, k allow) and odd views in NaN-poisoned buffers"""
    ops, (m, n) = OPS, shape
    for k in I.EXACT_KS:
        rs = np.random.RandomState(m + k)
        W, H = (rs.rand(m, k) + 0.01).astype(np.float32), (rs.rand(k, n) + 0.01).astype(np.float32)
        S = W.astype(np.float64) @ H
        A = np.where(rs.rand(m, n) < 0.1, S.mean() * 5 * (1 + rs.rand(m, n)), S * (1 + 0.2 * (rs.rand(m, n) - 0.5))).astype(np.float32)
        delta = 0.07 * float(S.mean())
        (nw, dw), (nh, dh), (want, scale, share) = Hb.pair(A, W, H, "w", delta), Hb.pair(A, W, H, "h", delta), Hb.loss(A, W, H, delta)
        assert 0.05 <= share <= 0.5, (shape, k, share)
        ref = (nw, dw, nh, dh, W * nw / (dw + EPS), H * nh / (dh + EPS), np.maximum(H * nh / (dh + EPS), EPS))
        for aligned in (True, False):
            Ap, Wp, Hp, W1, H1, H2 = (E.Poisoned(torch, x, aligned=aligned) for x in (A, W, H, W, H, H))
            outs = [E.Poisoned(torch, np.zeros(s, dtype=np.float32), aligned=aligned) for s in ((m, k), (m, k), (k, n), (k, n))]
            for side, i in (("w", 0), ("h", 2)):
                ops.huber_pair_into(side, Ap.view, Wp.view, Hp.view, EPS, delta, outs[i].view, outs[i + 1].view)
            ops.huber_update_w(Ap.view, W1.view, Hp.view, EPS, delta), ops.huber_update_h(Ap.view, Wp.view, H1.view, EPS, delta)
            ops.huber_update_h(Ap.view, Wp.view, H2.view, EPS, delta, clamp=True)
            got = float(ops.huber_loss(Ap.view, Wp.view, Hp.view, EPS, delta).cpu())
            d = [rel_fro(p.check("k=%d output %d" % (k, i)), r) for i, (p, r) in enumerate(zip(outs + [W1, H1, H2], ref))]
            assert all(np.array_equal(p.check(), x) for p, x in ((Ap, A), (Wp, W), (Hp, H)))       # (nothing outside the views, operands unwritten)
            print("huber %dx%d k=%d aligned=%d share %.2f: pairs %.2e updates %.2e loss %.2e" % (m, n, k, aligned, share, max(d[:4]), max(d[4:]), abs(got - want) / scale))
            assert max(d) <= BOUND and abs(got - want) <= BOUND * scale, (shape, k, aligned, d, got, want)


@pytest.mark.parametrize("shape_k", [(300, 200, 4), (130, 97, 32), (257, 70, 100)], ids=lambda s: "%dx%d-k%d" % s)
def test_delta_inf_is_the_beta_two_rule_bit_for_bit(shape_k):
    """p = 1 exactly at every element and the plans are PAIR_BETA's, so the MFMA chains are: updates and a 10-step fit are torch.equal"""
    ops, (m, n, k) = OPS, shape_k
    A, _, W0, H0 = Hb.spiked(m, n, k, seed=k)
    At, Wh, Hh, Wb, Hb2 = (torch.from_numpy(x).cuda() for x in (A, W0, H0, W0, H0))
    ops.huber_update_w(At, Wh, Hh, EPS, INF), ops.beta_update_w(At, Wb, Hb2, EPS, 2.0)
    ops.huber_update_h(At, Wh, Hh, EPS, INF, clamp=True), ops.beta_update_h(At, Wb, Hb2, EPS, 2.0, clamp=True)
    assert torch.equal(Wh, Wb) and torch.equal(Hh, Hb2) and not torch.equal(Wh, torch.from_numpy(W0).cuda())
    hub, beta = _pynmf(A, W0, H0, 10, norm="huber", delta=INF), _pynmf(A, W0, H0, 10, norm="beta", beta=2.0)
    (W1, H1, e1), (W2, H2, e2) = hub.fit(), beta.fit()
    assert hub._whole_fit_ok(hub._ops()) and hub.norm == "huber" and torch.equal(W1, W2) and torch.equal(H1, H2) and e1 == e2


@pytest.mark.parametrize("wu", [True, False], ids=["W_update", "W_fixed"])
@pytest.mark.parametrize("shape_k", [(300, 200, 4), (130, 97, 32)], ids=lambda s: "%dx%d-k%d" % s)
def test_whole_fit_equals_the_python_step_loop_bit_for_bit(shape_k, wu):
    A, _, W0, H0 = Hb.spiked(*shape_k, seed=shape_k[0], share=0.05, height=20.0, noise=0.2)
    for itr in (1, 11, 30):                                                               # (one, two and three clamps)
        whole, loop = (_pynmf(A, W0, H0, itr, norm="huber", delta=0.5, W_update=wu, **kw) for kw in ({}, {"fit_loop": "python"}))
        assert whole._whole_fit_ok(whole._ops()) and not loop._whole_fit_ok(loop._ops())
        (W1, H1, e1), (W2, H2, e2) = whole.fit(), loop.fit()
        assert torch.equal(W1, W2) and torch.equal(H1, H2) and abs(e1 - e2) <= 1e-12 and torch.isfinite(H1).all(), (shape_k, wu, itr)


def test_thirty_step_fit_against_float64_and_the_loss_never_rises():
    """200 x 136, k = 5, 5 % spikes, 30 steps against float64; along the Python step loop huber_loss() never rises by more than 1e-6 of its
    own value (the slack of the beta test of that name), while the float64 statement's own smallest decrease per step exceeds that slack"""
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    A, _, W0, H0 = Hb.spiked(200, 136, 5, seed=9, share=0.05, height=20.0, noise=0.2)
    delta, slack, nmf = 0.5, 1e-6, _pynmf(A, W0, H0, 30, norm="huber", delta=0.5)
    (W, H, err), (Wr, Hr, err_r) = nmf.fit(), Hb.fit(A, W0, H0, delta, 30)
    dw, dh, de, (want, scale, _) = rel_fro(W.cpu().numpy(), Wr), rel_fro(H.cpu().numpy(), Hr), abs(err - err_r) / err_r, Hb.loss(A, Wr, Hr, delta)
    print("huber fit 200x136 k=5: dW=%.2e dH=%.2e derr=%.2e dloss=%.2e of its terms" % (dw, dh, de, abs(nmf.huber_loss() - want) / scale))
    assert dw <= FIT_BOUND and dh <= FIT_BOUND and de <= ERR_BOUND and abs(nmf.huber_loss() - want) <= BOUND * scale
    W, H, ref = W0.astype(np.float64), H0.astype(np.float64), [Hb.loss(A, W0, H0, delta)[0]]
    loop = _pynmf(A, W0, H0, 30, norm="huber", delta=delta, fit_loop="python")
    d = [loop.huber_loss()]
    for i in range(30):
        W, H = Hb.step(A, W, H, delta, EPS, True, clamp=(i % 10 == 0))
        ref.append(Hb.loss(A, W, H, delta)[0])
        nmf_algorithms_1D(loop.A_ij, loop.W_i, loop.H_j, params=loop.params, ops=loop._ops()).update(clamp=(i % 10 == 0))
        d.append(loop.huber_loss())
        assert d[-1] <= d[-2] * (1.0 + slack) and abs(d[-1] - ref[-1]) <= 1e-4 * ref[-1], (i, d[-2], d[-1], ref[-1])
    assert (-np.diff(ref) / np.array(ref[:-1])).min() > slack, ref                       # (measured: 1.0e-4)


@pytest.mark.parametrize("grid", [(2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_grids_against_the_float64_statement(grid):
    """50 x 39, k = 3, 20 steps, W_update on and off, the ranks stacked on the one GPU: the pair through allreduce, then the ratio"""
    res = I.spawn(Hb.grid_rank, grid, (), 300)
    A, _, W0, H0 = Hb.spiked(**Hb.GRID["problem"])
    for wu in (True, False):
        Wr, Hr, err_r = Hb.fit(A, W0, H0, Hb.GRID["delta"], Hb.GRID["itr"], W_update=wu)
        want, scale, _ = Hb.loss(A, Wr, Hr, Hb.GRID["delta"])
        for rank, out in res:
            rows, cols, W, H, err, got = out[wu]
            d = (rel_fro(W, Wr[rows]), rel_fro(H, Hr[:, cols]), abs(float(err) - err_r) / err_r, abs(got - want) / scale)
            assert d[0] <= FIT_BOUND and d[1] <= FIT_BOUND and d[2] <= ERR_BOUND and d[3] <= BOUND, (grid, rank, wu, d)


def test_the_clean_entries_are_fitted_better_than_under_fro():
    """planted rank 3, 120 x 90, 2 % of the entries replaced by spikes of 50 to 100 times the mean; 60 steps from equal starts.  The float64
    statement's error on the unspiked entries: 0.079 under delta = 1 against 2.60 under delta = inf, a factor of 33: the order is asserted"""
    A, clean, W0, H0 = Hb.spiked(120, 90, 3, seed=1)
    err = {}
    for norm, kw in (("huber", {"delta": 1.0}), ("fro", {})):
        W, H, _ = _pynmf(A, W0, H0, 60, norm=norm, **kw).fit()
        R = A.astype(np.float64) - W.cpu().numpy().astype(np.float64) @ H.cpu().numpy()
        err[norm] = float(np.linalg.norm(R[clean]) / np.linalg.norm(A[clean]))
    print("relative error on the unspiked entries: huber %.4f, fro %.4f" % (err["huber"], err["fro"]))
    assert err["huber"] < err["fro"]
