"""`params.fit_loop = 'slab'` on the GPU (csrc/dnmf_slab.h): Itakura-Saito / beta-divergence / weighted fits, every step two launches for the
whole batch, against the float64 statements of tests/_is.py, tests/_beta.py and tests/_weighted.py; a batch against its members fitted
alone, bit for bit, on contiguous stacks and on views of NaN-filled buffers; shared weights; the refusal; an NMFk sweep."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _beta as B  # noqa: E402
from tests import _is as I  # noqa: E402
from tests import _is_nmfk as K  # noqa: E402
from tests import _weighted as Wt  # noqa: E402
from tests._golden import rel_fro  # noqa: E402
from tests.test_gpu_is import ERR_BOUND, FIT_BOUND  # noqa: E402  (the project's bounds for a pair-rule fit against float64)
from tests.test_slab_plan import GPU_SHAPES  # noqa: E402

ITR = 23                                    # the clamps of the steps 0, 10 and 20 are crossed
SHAPES = tuple(GPU_SHAPES)
RULES = (("is", None), ("beta", -0.75), ("beta", 1.5), ("beta", 3.0))     # sqrt; gamma = 1 / (2 - beta), 1 and 1 / (beta - 1)
_ID = lambda v: "%dx%dk%d" % v if isinstance(v, tuple) and len(v) == 3 else str(v)      # noqa: E731


def _problem(m, n, k, seed=5):
    A, W0, H0, _ = I.problem(m, n, k, seed)
    return A.astype(np.float32), W0.astype(np.float32), H0.astype(np.float32)


def _pynmf(A, W0, H0, norm, beta, V=None, **kw):
    from pydnmfk_amd.pyDNMF import PyNMF
    k = W0.shape[1]
    if V is not None:
        args = Wt.args(k, ITR, norm, beta, weights=V, **kw)
    else:
        args = I.one_rank_args(k, ITR, norm=norm, **kw) if beta is None else B.one_rank_args(k, ITR, beta, **kw)
    return PyNMF(torch.from_numpy(A).cuda(), factors=[torch.from_numpy(W0).cuda(), torch.from_numpy(H0).cuda()], params=args)


def _check(nmf, ref, what):
    assert nmf._slab and not nmf._resident and nmf.kind.batchable and nmf._whole_fit_ok(nmf._ops())
    W, H, err = nmf.fit()
    Wr, Hr, err_r = ref
    dw, dh, de = rel_fro(W.cpu().numpy(), Wr), rel_fro(H.cpu().numpy(), Hr), abs(err - err_r) / err_r
    print("slab %s against float64: dW=%.2e dH=%.2e derr=%.2e (err %.6g)" % (what, dw, dh, de, err_r))
    assert torch.isfinite(W).all() and torch.isfinite(H).all()
    assert dw <= FIT_BOUND and dh <= FIT_BOUND and de <= ERR_BOUND, (dw, dh, de)


@pytest.mark.parametrize("shape, wu", [(s, True) for s in SHAPES] + [(SHAPES[0], False), (SHAPES[-1], False)], ids=_ID)
@pytest.mark.parametrize("norm, beta", RULES, ids=_ID)
def test_slab_fit_against_float64(norm, beta, shape, wu):
    """23 steps from the same float32 factors: W and H within FIT_BOUND and the error within ERR_BOUND of the float64 fit"""
    A, W0, H0 = _problem(*shape)
    ref = I.fit(A, W0, H0, ITR, W_update=wu) if beta is None else B.fit(A, W0, H0, beta, ITR, W_update=wu)
    _check(_pynmf(A, W0, H0, norm, beta, W_update=wu, fit_loop="slab"), ref, "%s %s %s W_update=%s" % (norm, beta, shape, wu))


def _weighted_problem(m, n, k, seed=5, V=None):
    """Wt.problem (30 % zero weights) as float32, NaN and -7 planted under the zeros of V"""
    A, V0, W0, H0, _ = Wt.problem(m, n, k, seed)
    V = (V0 if V is None else V).astype(np.float32)
    A = np.where(V > 0, I.problem(m, n, k, seed)[0], np.resize(np.float32([np.nan, -7.0]), (m, n))).astype(np.float32)
    return A, V, W0.astype(np.float32), H0.astype(np.float32)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=_ID)
@pytest.mark.parametrize("norm, beta", Wt.NORMS, ids=_ID)
def test_weighted_slab_fit_against_float64(norm, beta, shape):
    """fro / kl / is / beta under weights with 30 % zeros over NaN and -7: factors and weighted error against the float64 fit"""
    A, V, W0, H0 = _weighted_problem(*shape)
    ref = Wt.fit(*(x.astype(np.float64) for x in (A, V, W0, H0)), norm, beta, ITR)
    _check(_pynmf(A, W0, H0, norm, beta, V=V, fit_loop="slab"), ref, "weighted %s %s %s" % (norm, beta, shape))


def _views(mats):
    """rows 1.., columns 3.. of [3][rows + 3][cols + 5] buffers of NaN: odd pitches and member distances, nothing aligned"""
    out = []
    for stack in mats:
        buf = torch.full((3, stack[0].shape[0] + 3, stack[0].shape[1] + 5), float("nan"), device="cuda")
        view = buf[:, 1:1 + stack[0].shape[0], 3:3 + stack[0].shape[1]]
        for b in range(3):
            view[b].copy_(torch.from_numpy(stack[b]))
        out.append((buf, view))
    return out


@pytest.mark.parametrize("norm, beta, weighted", [("is", None, False), ("beta", 1.5, False), ("kl", 0.0, True)], ids=_ID)
def test_batch_equals_single_fits_bit_for_bit(norm, beta, weighted):
    """three different 130 x 290 problems at k = 16: PyNMF.fit_batch (contiguous stacks) and ops.slab_fit on views inside NaN-filled buffers
    both give the bits of each problem fitted alone; the NaNs outside the views survive and A is unwritten.  Under weights: ONE weights
    matrix shared by the batch (stride 0) and a stacked copy of it give the same bits too"""
    from pydnmfk_amd.pyDNMF import PyNMF
    m, n, k = SHAPES[1]
    V = _weighted_problem(m, n, k)[1] if weighted else None
    probs = [(_weighted_problem(m, n, k, seed, V=V) if weighted else _problem(m, n, k, seed)) for seed in (5, 6, 7)]
    Vd = torch.from_numpy(V).cuda() if weighted else None
    make = lambda: [_pynmf(p[0], p[-2], p[-1], norm, beta, V=Vd, fit_loop="slab") for p in probs]      # noqa: E731
    single, fits = [f.fit() for f in make()], make()
    batch = PyNMF.fit_batch(fits)
    assert fits[0]._stack is fits[2]._stack                                     # (they did run together)
    for (W1, H1, e1), (W2, H2, e2) in zip(single, batch):
        assert torch.equal(W1, W2) and torch.equal(H1, H2) and e1 == e2
    assert not torch.equal(single[0][0], single[1][0])
    (Ab, Av), (Wb, Wv), (Hb, Hv) = bufs = _views([[p[0] for p in probs], [p[-2] for p in probs], [p[-1] for p in probs]])
    ops = fits[0]._ops()
    runs = [(Wv, Hv, Vd)]
    if weighted:                                                                # the stacked copy of the shared weights, in a view as well
        Vb, Vv = _views([[V] * 3])[0]
        bufs.append((Vb, Vv))
        runs.append((Wv.clone(), Hv.clone(), Vv))
    for Wx, Hx, Vx in runs[::-1]:
        sq = ops.slab_fit(norm, beta or 0.0, Av, Wx, Hx, I.EPS, True, ITR, V=Vx).cpu()
        for b, (W1, H1, e1) in enumerate(single):
            assert torch.equal(Wx[b], W1) and torch.equal(Hx[b], H1)
            assert float(np.sqrt(float(sq[b, 0]))) / float(np.sqrt(float(sq[b, 1]))) == e1
    for b in range(3):                                                          # A is never written (NaN under the zero weights included)
        assert torch.equal(Av[b].cpu().view(torch.int32), torch.from_numpy(probs[b][0]).view(torch.int32))
    for buf, view in bufs:
        assert int(torch.isnan(buf).sum()) == buf.numel() - view.numel() + int(torch.isnan(view).sum())     # nothing outside the blocks was written


def test_k_beyond_the_limit_is_refused_and_the_default_untouched():
    A, W0, H0 = _problem(70, 66, 65)
    with pytest.raises(NotImplementedError, match="1 <= k <= 64"):
        _pynmf(A, W0, H0, "is", None, fit_loop="slab")
    nmf = _pynmf(A, W0, H0, "is", None)
    assert not nmf._slab and not nmf.kind.batchable
    W, H, err = nmf.fit()
    assert torch.isfinite(W).all() and torch.isfinite(H).all() and 0.0 < err < 1.0


def test_planted_sweep_estimates_three_in_batched_launches(tmp_path):
    """tests/_is_nmfk.py::scaled_problem(1), k = 1..5, 6 perturbations, 300 iterations: the six fits of a rank run as one call and the
    sweep estimates 3, as the default sweep does; both wall times are printed (no threshold)"""
    from pydnmfk_amd.pyDNMFk import PyNMFk
    A = K.scaled_problem(1)
    walls = {}
    for loop in ("slab", None):
        args = K.sweep_args(tmp_path / ("is-%s" % loop), **({"fit_loop": loop} if loop else {}))
        nmfk = PyNMFk(A, params=args)
        assert nmfk._batch_size() == (args.perturbations if loop else 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nopt = nmfk.fit()
        torch.cuda.synchronize()
        walls[loop] = time.perf_counter() - t0
        assert nopt == 3, (loop, K.min_silhouettes(nmfk))
    print("is sweep (120 x 90, k = 1..5, 6 perturbations, 300 iterations): %.2f s fit_loop='slab', %.2f s default" % (walls["slab"], walls[None]))
