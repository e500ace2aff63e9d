"""`params.fit_loop = 'resident'` together with `params.weights` on the GPU (pair_resident_weighted_kernel, csrc/dnmf_resident.h): the whole
weighted fit of a small problem in one workgroup against the float64 statement of tests/_weighted.py; unit weights against the
unweighted resident kernel and junk under zero weights, bit for bit; a batch against its members fitted alone; the refusal; a sweep.

Measured on one MI355X over the 40 cases of the first test: dW <= 1.8e-06 (fro, 33x290 k=16), dH <= 3.6e-06 (kl, 290x33 k=17, W fixed),
derr <= 5.5e-08 (fro, 290x33 k=17)."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _is as I  # noqa: E402
from tests import _masked_nmfk as N  # noqa: E402
from tests import _weighted as Wt  # noqa: E402
from tests._golden import rel_fro  # noqa: E402
from tests.test_gpu_weighted import ERR_BOUND, FIT_BOUND  # noqa: E402  (a weighted fit against float64)
from tests.test_resident_plan import GPU_SHAPES  # noqa: E402

ITR = 23                                    # the clamps of the steps 0, 10 and 20 are crossed
JUNK = np.array([np.nan, -7.0, np.inf, 0.0], dtype=np.float32)
_ID = lambda v: "%dx%dk%d" % v if isinstance(v, tuple) and len(v) == 3 else str(v)      # noqa: E731


def _problem(m, n, k, seed=5, junk=JUNK, V=None):
    """Wt.problem (30 % zero weights) as float32, `junk` written under the zeros of V (its own weights, or the ones handed over)"""
    A, V0, W0, H0, _ = Wt.problem(m, n, k, seed)
    V = (V0 if V is None else V).astype(np.float32)
    A = np.where(V > 0, I.problem(m, n, k, seed)[0], np.resize(junk, (m, n))).astype(np.float32)
    return A, V, W0.astype(np.float32), H0.astype(np.float32)


def _pynmf(A, V, W0, H0, norm, beta, **kw):
    from pydnmfk_amd.pyDNMF import PyNMF
    d = [torch.from_numpy(x).cuda() for x in (A, W0, H0)]
    if V is not None:
        kw["weights"] = V
    return PyNMF(d[0], factors=d[1:], params=Wt.args(W0.shape[1], ITR, norm, beta, **kw))


@pytest.mark.parametrize("wu", [True, False], ids=["W_update", "W_fixed"])
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=_ID)
@pytest.mark.parametrize("norm, beta", Wt.NORMS, ids=_ID)
def test_weighted_resident_fit_against_float64(norm, beta, shape, wu):
    """23 steps, NaN / -7 / inf / 0 under the zero weights: W, H and the weighted error against the float64 fit of the same operands"""
    A, V, W0, H0 = _problem(*shape)
    nmf = _pynmf(A, V, W0, H0, norm, beta, W_update=wu, fit_loop="resident")
    assert nmf._resident and nmf.kind.batchable and nmf._whole_fit_ok(nmf._ops())
    W, H, err = nmf.fit()
    Wr, Hr, err_r = Wt.fit(*(x.astype(np.float64) for x in (A, V, W0, H0)), norm, beta, ITR, W_update=wu)
    dw, dh, de = rel_fro(W.cpu().numpy(), Wr), rel_fro(H.cpu().numpy(), Hr), abs(err - err_r) / err_r
    print("weighted resident %s beta=%g %dx%d k=%d %s against float64: dW=%.2e dH=%.2e derr=%.2e"
          % ((norm, beta) + shape + ("W_update" if wu else "W_fixed", dw, dh, de)))
    assert torch.isfinite(W).all() and torch.isfinite(H).all()
    assert dw <= FIT_BOUND and dh <= FIT_BOUND and de <= ERR_BOUND, (dw, dh, de)


@pytest.mark.parametrize("shape", [GPU_SHAPES[0], GPU_SHAPES[2], GPU_SHAPES[3]], ids=_ID)
@pytest.mark.parametrize("norm, beta", [("is", 0.0), ("beta", 1.5)], ids=_ID)
def test_unit_weights_are_the_unweighted_resident_kernel_bit_for_bit(norm, beta, shape):
    A, _, W0, H0 = _problem(*shape, V=np.ones(shape[:2]))
    (W1, H1, e1), (W2, H2, e2) = (_pynmf(A, V, W0, H0, norm, beta, fit_loop="resident").fit() for V in (np.ones_like(A), None))
    assert torch.equal(W1, W2) and torch.equal(H1, H2) and e1 == e2


@pytest.mark.parametrize("norm, beta", [("fro", 0.0), ("kl", 0.0), ("is", 0.0), ("beta", 0.5)], ids=_ID)
def test_data_under_a_zero_weight_are_not_read(norm, beta):
    fits = [_pynmf(*_problem(50, 39, 3, junk=junk), norm, beta, fit_loop="resident").fit() for junk in (JUNK, np.float32([1.0, np.inf, np.nan]))]
    (W1, H1, e1), (W2, H2, e2) = fits
    assert torch.equal(W1, W2) and torch.equal(H1, H2) and e1 == e2 and torch.isfinite(W1).all() and np.isfinite(e1)


@pytest.mark.parametrize("norm, beta", [("kl", 0.0), ("beta", 0.5)], ids=_ID)
def test_batch_equals_single_fits_bit_for_bit(norm, beta):
    """three 50 x 39 problems at k = 3 (-7 under the zero weights): PyNMF.fit_batch with ONE weights tensor (handed over once, stride 0)
    and with three, and ops.resident_fit on odd-pitched views inside NaN-filled buffers, give the bits of each problem fitted alone"""
    from pydnmfk_amd.pyDNMF import PyNMF
    m, n, k = 50, 39, 3
    shared = torch.from_numpy(_problem(m, n, k)[1]).cuda()
    for V in (shared, None):
        probs = [_problem(m, n, k, seed, junk=np.float32([-7.0]), V=None if V is None else V.cpu().numpy()) for seed in (5, 6, 7)]
        make = lambda: [_pynmf(A, Vb if V is None else V, W0, H0, norm, beta, fit_loop="resident") for A, Vb, W0, H0 in probs]   # noqa: E731
        single, fits = [f.fit() for f in make()], make()
        assert all(f.kind.batchable for f in fits)
        assert (len({f.V_ij.data_ptr() for f in fits}) == 1) == (V is not None)          # one storage: the stride-0 case
        batch = PyNMF.fit_batch(fits)
        assert fits[0]._stack is fits[2]._stack                                          # (they did run together)
        for (W1, H1, e1), (W2, H2, e2) in zip(single, batch):
            assert torch.equal(W1, W2) and torch.equal(H1, H2) and e1 == e2
        assert not torch.equal(single[0][0], single[1][0])
    # views (the three different weights): rows 1.., columns 3.. of [3][rows + 3][cols + 5] buffers of NaN
    bufs = {}
    for name, idx, (rows, cols) in (("A", 0, (m, n)), ("V", 1, (m, n)), ("W", 2, (m, k)), ("H", 3, (k, n))):
        buf = torch.full((3, rows + 3, cols + 5), float("nan"), device="cuda")
        view = buf[:, 1:1 + rows, 3:3 + cols]
        for b in range(3):
            view[b].copy_(torch.from_numpy(probs[b][idx]))
        bufs[name] = (buf, view)
    sq = fits[0]._ops().resident_fit(norm, beta, bufs["A"][1], bufs["W"][1], bufs["H"][1], I.EPS, True, ITR, V=bufs["V"][1]).cpu()
    for b, (W1, H1, e1) in enumerate(single):
        assert torch.equal(bufs["W"][1][b], W1) and torch.equal(bufs["H"][1][b], H1)
        assert float(np.sqrt(float(sq[b, 0]))) / float(np.sqrt(float(sq[b, 1]))) == e1
        assert all(torch.equal(bufs[x][1][b].cpu(), torch.from_numpy(probs[b][i])) for i, x in enumerate("AV"))   # never written
    for name, (buf, view) in bufs.items():
        assert int(torch.isnan(buf).sum()) == buf.numel() - view.numel(), name           # nothing outside the blocks was written


def test_k_beyond_the_limit_is_refused_and_the_default_untouched():
    A, V, W0, H0 = _problem(64, 64, 33)
    with pytest.raises(NotImplementedError, match="1 <= k <= 32"):
        _pynmf(A, V, W0, H0, "kl", 0.0, fit_loop="resident")
    nmf = _pynmf(A, V, W0, H0, "kl", 0.0)
    assert not nmf._resident and not nmf.kind.batchable
    W, H, err = nmf.fit()
    assert torch.isfinite(W).all() and torch.isfinite(H).all() and 0.0 < err < 1.0


def test_planted_sweep_under_01_weights_runs_in_batched_launches(tmp_path):
    """missing_problem() as 0/1 weights over junk, k = 1..5, 6 perturbations, 300 iterations: the six fits of a rank run as one launch
    and the sweep estimates what the default sweep does, 3; both wall times are printed (no threshold)"""
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests.test_gpu_sparse_nmfk import missing_problem
    A, mask = missing_problem()
    data = torch.from_numpy(np.where(mask, A, np.resize(JUNK, A.shape)).astype(np.float32)).cuda()
    walls, nopt = {}, {}
    for loop in ("resident", None):
        args = N.missing_args(tmp_path / str(loop), None)
        vars(args).update(weights=mask.astype(np.float32), **({"fit_loop": loop} if loop else {}))
        nmfk = PyNMFk(data, params=args)
        assert nmfk._batch_size() == (args.perturbations if loop else 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nopt[loop] = nmfk.fit()
        torch.cuda.synchronize()
        walls[loop] = time.perf_counter() - t0
        print("0/1-weights sweep (%s): estimate %d, minimum silhouettes %s" % (loop or "default", nopt[loop], N.min_silhouettes(nmfk)))
    print("0/1-weights sweep (120 x 90, k = 1..5, 6 perturbations, 300 iterations): %.2f s fit_loop='resident', %.2f s default"
          % (walls["resident"], walls[None]))
    assert nopt["resident"] == nopt[None] == 3, nopt
