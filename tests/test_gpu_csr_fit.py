"""Whole sparse MU fits, one problem or a batch over a shared pattern (csrc/dnmf_csr_batch.h, dnmf_csr_mu_fit_batch) on the GPU: the bits of
the step loop problem by problem, a float64 reference, nothing written outside the blocks, and one NMFk sweep."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
ITR = 12                                  # clamps after the steps 0 and 10
M, N, NPROB = 70, 1100, 9                 # NPROB = the largest BT + 1


def _mask():
    """70 x 1100: row 0 and column 0 empty, row 1 with exactly 64 stored entries, row 2 with 65, row 3 full but for column 0 (1099 entries:
    more than CSR_SEG = 1024, a long row), 2 % elsewhere"""
    rs = np.random.RandomState(21)
    mask = rs.rand(M, N) < 0.02
    mask[0] = False
    mask[1] = False; mask[1, rs.choice(np.arange(1, N), 64, replace=False)] = True
    mask[2] = False; mask[2, rs.choice(np.arange(1, N), 65, replace=False)] = True
    mask[3] = True
    mask[:, 0] = False
    return mask


@pytest.fixture(scope="module")
def data():
    """per side ('A': the long row in the block's image, 'At': in the transpose's): the mask and NPROB value sets"""
    rs = np.random.RandomState(22)
    mask = _mask()
    assert mask[1].sum() == 64 and mask[2].sum() == 65 and mask[3].sum() == N - 1 > 1024 and not mask[0].any() and not mask[:, 0].any()
    vals = [np.where(mask, rs.rand(M, N) + 0.05, 0.0).astype(np.float32) for _ in range(NPROB)]
    return {"A": (mask, vals), "At": (mask.T.copy(), [v.T.copy() for v in vals])}


def _blocks(mask, vals, missing):
    from pydnmfk_amd.sparse import SparseBlock
    from tests._masked import observed
    base = SparseBlock.from_any(observed(vals[0], mask), torch.device("cuda", 0), keep_zeros=missing is not None, missing=missing)
    assert base.nnz == int(mask.sum())
    perm = base.transpose_perm()
    out = [base]
    for v in vals[1:]:
        val = torch.from_numpy(v[mask]).cuda()
        out.append(base.with_values(val, val[perm]))
    return out


def _params(k, norm, w_update, missing, loop=None):
    from tests.test_gpu_parity import _args
    args = _args(k, ITR, norm, w_update, "mu", False)
    if missing:
        args.missing = missing
    if loop:
        args.fit_loop = loop
    return args


def _factors(k, m, n):
    rs = np.random.RandomState(1000 + k)
    return [((rs.rand(m, k) + 0.01).astype(np.float32), (rs.rand(k, n) + 0.01).astype(np.float32)) for _ in range(NPROB)]


CASES = [(norm, missing, k, wu) for norm in ("fro", "kl") for missing in (None, "unstored") for k in (3, 17, 33) for wu in (True, False)]
CASES.append(("fro", None, 129, True))


@pytest.mark.parametrize("norm, missing, k, w_update", CASES)
def test_batched_fit_has_the_bits_of_the_step_loop(data, norm, missing, k, w_update):
    from pydnmfk_amd._lib import csr_fit_plan
    from pydnmfk_amd.engine import HIP_CSR_OPS
    from pydnmfk_amd.pyDNMF import PyNMF
    for side in ("A", "At"):
        mask, vals = data[side]
        m, n = mask.shape
        blocks = _blocks(mask, vals, missing)
        assert (blocks[0].n_long, blocks[0].t_n_long) == ((1, 0) if side == "A" else (0, 1))
        bt = csr_fit_plan(m, n, k, batch=2)["bt"]                  # (a single problem runs at BT = 1)
        f0 = _factors(k, m, n)
        nprob = bt + 1
        # a direct call on one block is taken (the parent refuses a SparseBlock here)
        Wd, Hd = torch.from_numpy(f0[0][0]).cuda(), torch.from_numpy(f0[0][1]).cuda()
        sq = HIP_CSR_OPS.fit("mu", norm, blocks[0], Wd, Hd, EPS, w_update, ITR)
        assert tuple(sq.shape) == (1, 2) and bool(torch.isfinite(sq).all())
        ref = [PyNMF(blocks[b], factors=list(f0[b]), params=_params(k, norm, w_update, missing, "python")).fit() for b in range(nprob)]
        for batch in sorted({1, bt - 1, bt, bt + 1}):
            args = _params(k, norm, w_update, missing)
            fits = [PyNMF(blocks[b], factors=list(f0[b]), params=args) for b in range(batch)]
            assert all(f._whole_fit_ok(f._ops()) and f.kind.batchable for f in fits)
            got = PyNMF.fit_batch(fits)
            for b in range(batch):
                assert torch.equal(got[b][0], ref[b][0]) and torch.equal(got[b][1], ref[b][1]), (side, batch, b)
                assert got[b][2] == ref[b][2], (side, batch, b, got[b][2], ref[b][2])
        assert torch.equal(Wd, ref[0][0]) and torch.equal(Hd, ref[0][1])


@pytest.mark.parametrize("norm", ["fro", "kl"])
@pytest.mark.parametrize("missing", [None, "unstored"])
def test_fit_against_float64(data, norm, missing):
    """After the 12 steps: bound max(tol, 2 d_ref) with d_ref the distance of the reference's float32 run from its float64 run and tol the
    fit tolerance of tests/test_gpu_parity.py::_tols (the bound of test_sparse_steps_along_a_float64_trajectory, for a fit of 12 steps)"""
    from oracle import nmf_oracle as orc
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests import _masked as mk
    from tests._golden import rel_fro
    from tests.test_gpu_parity import _tols
    mask, vals = data["A"]
    k, A = 17, vals[0]
    W0, H0 = _factors(k, M, N)[0]
    if missing:
        csr = mk.coo_of(mk.observed(A, mask))
        r64 = mk.fit(csr, A.shape, W0, H0, ITR, norm, EPS, True, np.float64)
        r32 = mk.fit(csr, A.shape, W0, H0, ITR, norm, EPS, True, np.float32)
    else:
        r64 = orc.fit_single(A.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64), ITR, norm=norm, method="mu", eps=EPS)
        r32 = orc.fit_single(A, W0.copy(), H0.copy(), ITR, norm=norm, method="mu", eps=EPS)
    blk = _blocks(mask, vals[:1], missing)[0]
    nmf = PyNMF(blk, factors=[W0, H0], params=_params(k, norm, True, missing))
    assert nmf._whole_fit_ok(nmf._ops())
    Wg, Hg, err = nmf.fit()
    tol = _tols({"method": "mu"})[1]
    for nm, g, a32, a64 in (("W", Wg.cpu().numpy(), r32[0], r64[0]), ("H", Hg.cpu().numpy(), r32[1], r64[1])):
        d_ref, d_gpu = rel_fro(a32, a64), rel_fro(g, a64)
        print("float64 %s/%s %s: d_ref=%.2e gpu=%.2e bound=%.2e" % (norm, missing, nm, d_ref, d_gpu, max(tol, 2 * d_ref)))
        assert d_gpu <= max(tol, 2 * d_ref), (norm, missing, nm, d_gpu, d_ref)
    assert abs(err - r64[2]) <= 1e-5 * max(1.0, abs(r64[2])), (err, r64[2])


@pytest.mark.parametrize("norm, missing", [("fro", None), ("kl", "unstored")])
def test_nothing_outside_the_blocks_is_written(data, norm, missing):
    from pydnmfk_amd.engine import HIP_CSR_OPS
    mask, vals = data["At"]
    m, n = mask.shape
    k, B = 17, 5
    blocks = _blocks(mask, vals[:B], missing)
    nnz, perm = blocks[0].nnz, blocks[0].transpose_perm()
    vs = nnz + 4 - nnz % 4 + 4                                     # rows of the value stacks: padded, a multiple of 16 bytes apart
    ldw, ldh, ws_, hs_ = k + 3, n + 5, m * (k + 3) + 4 - (m * (k + 3)) % 4 + 8, k * (n + 5) + 4 - (k * (n + 5)) % 4 + 8
    bufs = {nm: torch.full((B * st + 16,), float("nan"), device="cuda") for nm, st in (("val", vs), ("t_val", vs), ("W", ws_), ("H", hs_))}
    val, t_val = (bufs[nm][4:].as_strided((B, nnz), (vs, 1)) for nm in ("val", "t_val"))
    W, H = bufs["W"][4:].as_strided((B, m, k), (ws_, ldw, 1)), bufs["H"][4:].as_strided((B, k, n), (hs_, ldh, 1))
    f0 = _factors(k, m, n)
    for b in range(B):
        val[b].copy_(blocks[b].val); t_val[b].copy_(val[b][perm])
        W[b].copy_(torch.from_numpy(f0[b][0])); H[b].copy_(torch.from_numpy(f0[b][1]))
    held = [blocks[0].with_values(val[b], t_val[b]) for b in range(B)]
    assert all(h.val.data_ptr() == val[b].data_ptr() for b, h in enumerate(held))
    before = {nm: t.clone() for nm, t in (("val", val), ("t_val", t_val))}
    sq = HIP_CSR_OPS.fit("mu", norm, held, W, H, EPS, True, ITR)
    assert bool(torch.isfinite(sq).all()) and bool(torch.isfinite(W).all()) and bool(torch.isfinite(H).all())
    assert torch.equal(val, before["val"]) and torch.equal(t_val, before["t_val"])
    for nm, view in (("val", val), ("t_val", t_val), ("W", W), ("H", H)):
        keep = bufs[nm].clone()
        view.fill_(float("nan"))                                   # what is left once the blocks themselves are taken out
        assert bool(torch.isnan(bufs[nm]).all()), nm
        bufs[nm].copy_(keep)
    Wc, Hc = W.contiguous(), H.contiguous()                        # the same batch from packed stacks
    from pydnmfk_amd.engine import stack_alloc
    W2, H2 = stack_alloc(B, m, k, torch.float32, Wc.device), stack_alloc(B, k, n, torch.float32, Wc.device)
    for b in range(B):
        W2[b].copy_(torch.from_numpy(f0[b][0])); H2[b].copy_(torch.from_numpy(f0[b][1]))
    HIP_CSR_OPS.fit("mu", norm, blocks, W2, H2, EPS, True, ITR)
    assert torch.allclose(Wc, W2, rtol=1e-4, atol=1e-7) and torch.allclose(Hc, H2, rtol=1e-4, atol=1e-7)


def test_one_sweep_equals_the_step_loop_sweep(tmp_path):
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests.test_gpu_sparse_nmfk import _small_args, _sparse_counts
    A = _sparse_counts()
    stats, wall = {}, {}
    for loop in (None, "python"):
        args = _small_args(tmp_path / str(loop), rng="device")
        if loop:
            args.fit_loop = loop
        nmfk = PyNMFk(torch.from_numpy(A).cuda().to_sparse_csr(), params=args)
        assert nmfk._batch_size() == args.perturbations == 4
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nmfk.fit()
        wall[loop] = time.perf_counter() - t0
        stats[loop] = nmfk.stats
    print("sparse sweep wall time: batched whole fits %.3f s, step loop %.3f s" % (wall[None], wall["python"]))
    for k in (2, 3):
        for key in ("clusterSilhouetteCoefficients", "avgSilhouetteCoefficients", "L_err"):
            assert np.array_equal(np.asarray(stats[None][k][key]), np.asarray(stats["python"][k][key]), equal_nan=True), (k, key)
