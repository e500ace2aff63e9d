"""Batched method='bcd' fits (dnmf_bcd_fro_fit with batch > 1; csrc/dnmf_bcd.h with blockIdx.z = problem): every check compares ONE
batched call with the fits of the same problems one after another on the same GPU.  The contract is the project's contract for
batches (csrc/dnmf_common.h "batched launches"): problem z runs the instructions of a single fit on its own operands, so the factors
are BIT-identical (torch.equal / assert_array_equal); the two squared norms come from fp64 atomic sums whose order is free, so the
error is held to 1e-12 relative, as tests/test_gpu_fit.py does for MU and HALS.  What needs no GPU: tests/test_bcd_batch_cpu.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ACC = 9           # slot of the accept / restart decision in the state block (csrc/dnmf_bcd.h BcdSlot)

# m, n, k, itr: the ranks cross the dispatch boundaries the fit touches (one 16-column wave group / several, the 16-, 32-, 64-, 128-wide
# tuned products, the wide ranks), m and n are ragged against the 64-row workgroups and the 4-float vectors, the tall cases give the
# split reductions and the column-sum partials of the W step hundreds of blocks; itr with the final clamp ((itr - 1) % 10 == 0) and without
CASES = [
    (131, 203, 1, 11),
    (131, 203, 17, 7),
    (131, 203, 33, 11),
    (1024, 256, 4, 21),
    (1024, 256, 16, 12),
    (1024, 256, 32, 11),
    (2049, 515, 64, 11),
    (2049, 515, 128, 5),
    (2049, 515, 200, 4),
    (131, 203, 200, 11),
    (40001, 67, 4, 11),
    (40960, 132, 17, 6),
]


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


def _problem(m, n, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.rand(m, n, device="cuda", generator=g) + 0.01
    if seed % 2:
        A[:, ::7] = 0.0
    return A, torch.rand(m, k, device="cuda", generator=g), torch.rand(k, n, device="cuda", generator=g)


def _same(batched, single):
    for b, ((W1, H1, e1), (W2, H2, e2)) in enumerate(zip(batched, single)):
        assert torch.equal(W1, W2) and torch.equal(H1, H2), (b, float((W1 - W2).abs().max()), float((H1 - H2).abs().max()))
        assert abs(e1 - e2) <= 1e-12 * max(1.0, abs(e2)) and np.isfinite(e1), (b, e1, e2)


@pytest.mark.parametrize("m,n,k,itr", CASES)
def test_batched_bcd_fit_is_bit_identical_to_single_fits(m, n, k, itr):
    from pydnmfk_amd.pyDNMF import PyNMF
    B = 5
    probs = [_problem(m, n, k, 10 + b) for b in range(B)]
    single = [PyNMF(A, factors=[W0, H0], params=_args(k, itr)).fit() for A, W0, H0 in probs]
    fits = [PyNMF(A, factors=[W0, H0], params=_args(k, itr)) for A, W0, H0 in probs]
    batched = PyNMF.fit_batch(fits)
    assert getattr(fits[0], "_stack", None) is not None and fits[0]._stack.shape[0] == B          # it ran as ONE batch
    _same(batched, single)
    assert not torch.equal(batched[0][0], batched[1][0])           # (a batch that mapped every z to problem 0 would pass for b = 0 only)
    assert all(bool(torch.isfinite(W).all()) and bool(torch.isfinite(H).all()) for W, H, _ in batched)


def test_batched_bcd_fit_is_one_library_call(monkeypatch):
    from pydnmfk_amd import engine
    from pydnmfk_amd.pyDNMF import PyNMF
    calls = []
    real_fit = engine.HipOps.fit

    def fit(self, *a, **kw):
        calls.append((a[0], a[1], tuple(a[2].shape)))
        return real_fit(self, *a, **kw)
    monkeypatch.setattr(engine.HipOps, "fit", fit)
    monkeypatch.setattr(engine.HipOps, "bcd_update_w", lambda *a, **kw: pytest.fail("step primitive called"))
    probs = [_problem(96, 64, 3, 20 + b) for b in range(3)]
    PyNMF.fit_batch([PyNMF(A, factors=[W0, H0], params=_args(3, 12)) for A, W0, H0 in probs])
    assert calls == [("bcd", "fro", (3, 96, 64))]
    calls.clear()
    mixed = probs[:2] + [_problem(96, 60, 3, 29)]
    PyNMF.fit_batch([PyNMF(A, factors=[W0, H0], params=_args(3, 12)) for A, W0, H0 in mixed])
    assert [c[2] for c in calls] == [(96, 64), (96, 64), (96, 60)]                               # none batched


# ------------------------------------------------------------------------------------------------ divergent decisions
T = 80
SEEDS = (0, 2, 3)


def _lowrank():
    rs = np.random.RandomState(99)
    A = (rs.rand(96, 3) @ rs.rand(3, 64)).astype(np.float32)
    inits = []
    for seed in SEEDS:
        r = np.random.RandomState(seed)
        inits.append((r.rand(96, 3).astype(np.float32), r.rand(3, 64).astype(np.float32)))
    return A, inits


def _history(A, W0, H0):
    """ACC after iteration N for N = 1 .. T, read from the Python choreography on the GPU (bit-identical to the whole fit,
    tests/test_gpu_bcd.py::test_bcd_fixture_whole_fit_equals_python_loop): one update() with params.itr = N per point"""
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    h = []
    for N in range(1, T + 1):
        nmf = PyNMF(A, factors=[W0, H0], params=_args(3, N, fit_loop="python"))
        alg = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops())
        alg.update()
        h.append(int(alg._bcd_st.cpu().numpy()[ACC] != 0))
    return h


def test_batched_bcd_problems_decide_independently():
    """Three problems of ONE batch whose accept / restart histories differ: in some iteration one problem restarts while another
    accepts.  Each problem's state block sits in its own workspace slice and the host sequence does not depend on a decision, so the
    batched fits must still equal the single fits bit for bit.

    Problem: the exact rank-3 matrix A = (rs.rand(96, 3) @ rs.rand(3, 64)).float32 with rs = RandomState(99), k = 3, initial factors
    RandomState(seed).rand(96, 3), .rand(3, 64) for seed in (0, 2, 3), T = 80 iterations.  Restart iterations (1-based):
      numpy checker (tests/_bcd.BcdOracleOps):  seed 0: [47, 59]   seed 2: [45, 68, 75]   seed 3: [37]
      MI355X (this test's _history):            seed 0: [47, 59]   seed 2: [45, 68, 75]   seed 3: [37]
    The precondition is ASSERTED, not assumed: the histories must differ, both outcomes must occur in one iteration, and the first
    restart of seed 3 must lie at least 5 iterations from those of seeds 0 and 2 (8 and 10 in the checker; float32 products on the GPU
    may move a restart by an iteration, a near tie could not be told from luck)."""
    from pydnmfk_amd.pyDNMF import PyNMF
    A, inits = _lowrank()
    hist = [_history(A, W0, H0) for W0, H0 in inits]
    restarts = [[N + 1 for N, acc in enumerate(h) if not acc] for h in hist]
    print("restart iterations per seed %s: %s" % (SEEDS, restarts))
    assert all(r for r in restarts), restarts                                                  # every problem restarts within T
    split = [N + 1 for N in range(T) if len({h[N] for h in hist}) == 2]
    assert split, restarts                                                                     # one restarts while another accepts
    first = [r[0] for r in restarts]
    assert min(abs(first[2] - first[0]), abs(first[2] - first[1])) >= 5, first
    dev = torch.device("cuda")
    Ad = torch.from_numpy(A).to(dev)
    mk = lambda: [PyNMF(Ad, factors=[torch.from_numpy(W0).to(dev), torch.from_numpy(H0).to(dev)], params=_args(3, T)) for W0, H0 in inits]  # noqa: E731
    single = [f.fit() for f in mk()]
    fits = mk()
    batched = PyNMF.fit_batch(fits)
    assert fits[0]._stack.shape[0] == len(SEEDS)
    _same(batched, single)
    # ... and at an iteration count that ends inside the divergent stretch (the last decision differs between the problems)
    N = split[0]
    single = [PyNMF(Ad, factors=[torch.from_numpy(W0).to(dev), torch.from_numpy(H0).to(dev)], params=_args(3, N)).fit() for W0, H0 in inits]
    batched = PyNMF.fit_batch([PyNMF(Ad, factors=[torch.from_numpy(W0).to(dev), torch.from_numpy(H0).to(dev)], params=_args(3, N))
                               for W0, H0 in inits])
    _same(batched, single)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_batched_bcd_c_api_argument_errors():
    """batch = 2 is accepted; strides that do not span a problem / are not 16-byte multiples, overlapping operands -> -1, a workspace
    one byte short -> -2 (the checks of dnmf_mu_fro_fit, tests/test_gpu_fit.py::test_fit_c_api_argument_errors)"""
    from pydnmfk_amd._lib import lib
    m, n, k, B = 256, 128, 8, 2
    A = torch.rand(B, m, n, device="cuda")
    W = torch.rand(B, m, k, device="cuda")
    H = torch.rand(B, k, n, device="cuda")
    sq = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
    nb = lib.dnmf_bcd_ws_bytes_fit(m, n, k, B)
    assert nb == 2 * lib.dnmf_bcd_ws_bytes(m, n, k) > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(a_stride=m * n, w_stride=m * k, h_stride=k * n, wsb=nb, Wp=None):
        return lib.dnmf_bcd_fro_fit(A.data_ptr(), m, n, n, (Wp if Wp is not None else W).data_ptr(), k, H.data_ptr(), n, k, 1.2e-7, 1, 3,
                                    B, a_stride, w_stride, h_stride, sq.data_ptr(), ws.data_ptr(), wsb, st)
    assert call() == 0, lib.dnmf_last_error()
    assert call(a_stride=m * n - 4) == -1            # does not span a problem
    assert call(w_stride=m * k + 1) == -1            # not a multiple of 16 bytes
    assert call(wsb=nb - 1) == -2
    assert call(Wp=A) == -1                          # W inside A: operands overlap
    assert b"overlap" in lib.dnmf_last_error()
    # every refusal left the thread's batch state clean: a single fit and a batched fit still go through
    assert lib.dnmf_bcd_fro_fit(A.data_ptr(), m, n, n, W.data_ptr(), k, H.data_ptr(), n, k, 1.2e-7, 1, 3, 1, 0, 0, 0, sq.data_ptr(),
                                ws.data_ptr(), nb, st) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sq).all()) and bool((sq[:, 1] > 0).all())


@pytest.mark.parametrize("aligned", [True, False])
def test_batched_bcd_on_padded_views(aligned):
    """A, W, H as stacks of views with leading dimensions larger than their widths, the padding poisoned with NaN: nothing outside
    the views is touched, the factors are finite and bit-identical to single fits on views of the same pitch and alignment and
    (aligned = True: 16-byte aligned starts, pitches multiples of 4 floats, the alignment class of a contiguous matrix of these
    widths) to the fits of contiguous copies.  aligned = False: odd starts and pitches, the generic paths of every product; the
    sizes are chosen so that the distance between two problems is still a multiple of 16 bytes."""
    from pydnmfk_amd.engine import HIP_OPS
    from tests._exact import Poisoned
    B, m, n, k, itr, eps = 3, 132, 76, 8, 11, 1.1920929e-07
    rs = np.random.RandomState(4)
    A = (rs.rand(B, m, n) + 0.01).astype(np.float32)
    W0, H0 = rs.rand(B, m, k).astype(np.float32), rs.rand(B, k, n).astype(np.float32)
    pa, pw, ph = (Poisoned(torch, x, aligned=aligned) for x in (A, W0, H0))
    assert all(p.view.stride(0) % 4 == 0 and p.ld > p.cols for p in (pa, pw, ph))
    sq = HIP_OPS.fit("bcd", "fro", pa.view, pw.view, ph.view, eps, True, itr)
    torch.cuda.synchronize()
    pa.check("A")
    Wb, Hb = pw.check("W"), ph.check("H")
    np.testing.assert_array_equal(pa.view.cpu().numpy(), A)
    assert np.isfinite(Wb).all() and np.isfinite(Hb).all()
    assert not np.array_equal(Wb[0], Wb[1])
    for b in range(B):
        qa, qw, qh = (Poisoned(torch, x[b], aligned=aligned) for x in (A, W0, H0))
        sq1 = HIP_OPS.fit("bcd", "fro", qa.view, qw.view, qh.view, eps, True, itr)
        np.testing.assert_array_equal(Wb[b], qw.check("W single"))
        np.testing.assert_array_equal(Hb[b], qh.check("H single"))
        np.testing.assert_allclose(sq[b].cpu().numpy(), sq1[0].cpu().numpy(), rtol=1e-12)
        if aligned:
            Ac, Wc, Hc = (torch.from_numpy(np.ascontiguousarray(x[b])).cuda() for x in (A, W0, H0))
            HIP_OPS.fit("bcd", "fro", Ac, Wc, Hc, eps, True, itr)
            np.testing.assert_array_equal(Wb[b], Wc.cpu().numpy())
            np.testing.assert_array_equal(Hb[b], Hc.cpu().numpy())


def test_batched_bcd_reruns_are_bit_identical():
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests._bcd import load_bcd
    meta, A, _, _, _ = load_bcd("swim_1x1")
    rs = np.random.RandomState(7)
    inits = [(rs.rand(A.shape[0], 4), rs.rand(4, A.shape[1])) for _ in range(4)]
    a = PyNMF.fit_batch([PyNMF(A, factors=list(f), params=_args(4, 50)) for f in inits])
    b = PyNMF.fit_batch([PyNMF(A, factors=list(f), params=_args(4, 50)) for f in inits])
    for (W1, H1, e1), (W2, H2, e2) in zip(a, b):
        np.testing.assert_array_equal(W1, W2)
        np.testing.assert_array_equal(H1, H2)
        assert abs(e1 - e2) <= 1e-12 * max(1.0, abs(e2))
    assert not np.array_equal(a[0][0], a[1][0])


# ------------------------------------------------------------------------------------------------ NMFk
def _nmfk(A, tmp, tag, batch):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from pydnmfk_amd.utils import parse
    comms = MPI_comm(None, 1, 1)
    args = parse()
    args.comm1, args.comm, args.p_r, args.p_c = comms.comm, comms, 1, 1
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    args.fpath, args.fname, args.ftype = str(tmp) + "/", "b", "npy"
    args.start_k, args.end_k, args.step_k, args.sill_thr, args.itr, args.init = 2, 5, 1, 0.8, 80, "rand"
    args.noise_var, args.verbose, args.norm, args.method, args.checkpoint = 0.03, False, "fro", "bcd", False
    args.prune, args.perturbations = True, 6
    args.results_path = str(tmp) + "/results_%s/" % tag
    args.nmfk_batch = batch
    nm = PyNMFk(A, factors=None, params=args)
    return nm, nm.fit()


@pytest.mark.parametrize("io", ["numpy", "torch"])
def test_bcd_nmfk_batched_equals_one_by_one(tmp_path, io, monkeypatch):
    """the pattern of tests/test_gpu_fit.py::test_nmfk_batched_equals_one_by_one with method='bcd'"""
    from pydnmfk_amd import engine
    rs = np.random.RandomState(5)
    A = (rs.rand(384, 3) @ rs.rand(3, 192) + 0.01 * rs.rand(384, 192)).astype(np.float32)
    A[5, :] = 0                                        # one all-zero row: prune=True drops it in every perturbation
    X = A if io == "numpy" else torch.from_numpy(A).cuda()
    depths = []
    real_fit = engine.HipOps.fit

    def fit(self, *a, **kw):
        if a[0] == "bcd" and a[2].dim() == 3:
            depths.append(a[2].shape[0])
        return real_fit(self, *a, **kw)
    monkeypatch.setattr(engine.HipOps, "fit", fit)
    a, nopt_a = _nmfk(X, tmp_path, "batched", True)
    assert depths == [6] * 4                                                        # k = 2 .. 5: one batch of all six perturbations each
    del depths[:]
    b, nopt_b = _nmfk(X, tmp_path, "single", False)
    assert depths == []
    c, nopt_c = _nmfk(X, tmp_path, "four", 4)          # 6 perturbations as a batch of 4 and a batch of 2
    assert depths == [4, 2] * 4
    assert a._batch_size() == 6 and b._batch_size() == 1 and c._batch_size() == 4
    assert nopt_a == nopt_b == nopt_c
    for k in a.stats:
        for key in ("recon_err", "avgErr", "clusterSilhouetteCoefficients", "avgSilhouetteCoefficients", "L_err", "L_errDist"):
            for other in (b, c):
                np.testing.assert_allclose(np.asarray(a.stats[k][key], dtype=np.float64), np.asarray(other.stats[k][key], dtype=np.float64),
                                           rtol=1e-12, atol=0, err_msg="%s k=%d" % (key, k))
