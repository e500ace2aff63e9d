"""Sparse data whose unstored entries are missing (`params.missing = 'unstored'`) on the GPU (csrc/dnmf_csr.h, modes 3-5, through
engine.HipCsrOps): the masked passes against float64, their fused endings against their pair-writing endings, single steps along a
float64 trajectory, the reference's goldens on fully stored blocks, 1D grids, recovery of held-out entries, bit-reproducibility."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

from tests import _masked as M  # noqa: E402
from tests._golden import rel_fro  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = M.EPS
KS = (1, 3, 16, 17, 32, 64, 100, 128, 192, 256)


def _ops():
    from pydnmfk_amd.engine import HIP_CSR_OPS
    return HIP_CSR_OPS


def _block(S):
    from pydnmfk_amd.sparse import SparseBlock
    return SparseBlock.from_any(S, torch.device("cuda", 0), keep_zeros=True, missing="unstored")


def _args(k, itr, norm, W_update=True, missing="unstored"):
    from pydnmfk_amd.dist_comm import MPI_comm
    return M.args_for(MPI_comm(None, 1, 1), 1, 1, k, itr, norm, W_update, missing=missing)


# ---- check 1: the kernels against float64
def _observed_block(rs, m, n, density):
    """values in [0.05, 1.05) under a random mask of the given density, a few of the observed values set to zero"""
    A = (rs.rand(m, n) + 0.05).astype(np.float32)
    mask = np.ones((m, n), dtype=bool) if density >= 1.0 else rs.rand(m, n) < density
    r, c = np.nonzero(mask)
    if r.size:
        z = rs.choice(r.size, size=min(5, r.size), replace=False)
        A[r[z], c[z]] = 0.0
    return A, mask


def _pairs64(A, mask, W, H):
    """float64 numpy: {norm: (num_w, den_w, num_h, den_h)} and the masked residual (the shapes are small: dense algebra)"""
    A64, W64, H64, Mk = A.astype(np.float64), W.astype(np.float64), H.astype(np.float64), mask.astype(np.float64)
    D = W64 @ H64
    PA, PD = Mk * A64, Mk * D
    Q = Mk * A64 / (D + EPS)
    return ({"fro": (PA @ H64.T, PD @ H64.T, W64.T @ PA, W64.T @ PD), "kl": (Q @ H64.T, Mk @ H64.T, W64.T @ Q, W64.T @ Mk)},
            float(np.sum(Mk * (A64 - D) ** 2)))


def _rel(x, ref):
    nr = np.linalg.norm(ref)
    return float(np.linalg.norm(x.astype(np.float64) - ref) / nr) if nr > 0 else float(np.abs(x).max(initial=0.0))


def _ulp_apart(got, exp):
    return np.abs(got.astype(np.float64) - exp.astype(np.float64)) <= np.spacing(np.abs(exp)).astype(np.float64)


def _check_kernels(tag, A, mask, blk, W, H):
    ops = _ops()
    m, n = blk.shape
    k = W.shape[1]
    ref, ref_r = _pairs64(A, mask, W, H)
    Wd, Hd = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
    empty_rows, empty_cols = mask.sum(1) == 0, mask.sum(0) == 0
    for norm, bound in (("fro", 2e-6), ("kl", 1e-5)):
        bw, bh = torch.full((2 * m * k,), np.nan, device="cuda"), torch.full((2 * k * n,), np.nan, device="cuda")
        nw, dw = ops.masked_aht_pair(blk, Wd, Hd, EPS, norm, bw)
        nh, dh = ops.masked_wta_pair(blk, Wd, Hd, EPS, norm, bh)
        assert nw.data_ptr() == bw.data_ptr() and dw.data_ptr() == bw.data_ptr() + 4 * m * k          # ONE contiguous [num | den]
        got = [t.cpu().numpy() for t in (nw, dw, nh, dh)]
        d = [_rel(g, r) for g, r in zip(got, ref[norm])]
        print("masked %-26s %s k=%3d nnz=%7d  W: num %.2e den %.2e | H: num %.2e den %.2e" % (tag, norm, k, blk.nnz, *d))
        for g in got:
            assert np.isfinite(g).all(), (tag, norm)                  # every output element was written
        for g in got[:2]:
            assert not g[empty_rows].any(), (tag, norm)               # exact zeros, not small values
        for g in got[2:]:
            assert not g[:, empty_cols].any(), (tag, norm)
        assert max(d) <= bound, (tag, norm, k, d)
        # the fused endings: the factor the pass writes equals X * num / (den + eps) from the pair-writing ending's own output
        e = np.float32(EPS)
        W1, H1, H2 = Wd.clone(), Hd.clone(), Hd.clone()
        ops.masked_update_w(blk, W1, Hd, EPS, norm)
        ops.masked_update_h(blk, Wd, H1, EPS, norm)
        ops.masked_update_h(blk, Wd, H2, EPS, norm, clamp=True)
        expW, expH = W * (got[0] / (got[1] + e)), H * (got[2] / (got[3] + e))
        assert _ulp_apart(W1.cpu().numpy(), expW).all(), (tag, norm, k, "fused W")
        assert _ulp_apart(H1.cpu().numpy(), expH).all(), (tag, norm, k, "fused H")
        assert _ulp_apart(H2.cpu().numpy(), np.maximum(expH, e)).all(), (tag, norm, k, "fused H, clamped")
        # ... and so does the element-wise pass that follows an allreduce
        W3, H3 = Wd.clone(), Hd.clone()
        ops.ratio_update(W3, nw, dw, EPS)
        ops.ratio_update(H3, nh, dh, EPS, clamp=True)
        assert _ulp_apart(W3.cpu().numpy(), expW).all() and _ulp_apart(H3.cpu().numpy(), np.maximum(expH, e)).all(), (tag, norm, k, "ratio")
    r = float(ops.resid_sqnorm(blk, Wd, Hd).cpu())
    dr = abs(r - ref_r) / ref_r if ref_r > 0 else abs(r)
    print("masked %-26s resid k=%3d: %.2e" % (tag, k, dr))
    assert dr <= 1e-5, (tag, k, r, ref_r)


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (1000, 333)], ids=lambda s: "%dx%d" % s)
def test_masked_kernels_against_float64(shape):
    rs = np.random.RandomState(300 + shape[0])
    m, n = shape
    for density in (0.0, 0.001, 0.05, 1.0):
        A, mask = _observed_block(rs, m, n, density)
        blk = _block(M.observed(A, mask))
        assert blk.nnz == int(mask.sum()) and blk.missing == "unstored"
        for k in KS:
            W, H = (rs.rand(m, k) + 0.01).astype(np.float32), (rs.rand(k, n) + 0.01).astype(np.float32)
            _check_kernels("%dx%d d=%g" % (m, n, density), A, mask, blk, W, H)


def test_masked_kernels_long_rows_in_both_images():
    rs = np.random.RandomState(301)
    m, n = 1500, 2100
    A, mask = _observed_block(rs, m, n, 0.01)
    mask[7, :] = True
    mask[:, 11] = True
    mask[20, :] = False                                               # (an empty row next to the long ones; column 11 keeps its entry)
    mask[20, 11] = False
    blk = _block(M.observed(A, mask))
    assert blk.n_long >= 1 and blk.t_n_long >= 1 and blk.nseg >= 2 and blk.t_nseg >= 2
    for k in (3, 16, 64, 256):
        W, H = (rs.rand(m, k) + 0.01).astype(np.float32), (rs.rand(k, n) + 0.01).astype(np.float32)
        _check_kernels("1500x2100 long both", A, mask, blk, W, H)


# ---- check 2: single steps along a float64 trajectory
def _traj_problem():
    rs = np.random.RandomState(100)
    m, n, k = 1500, 1000, 32
    A = (rs.rand(m, n) + 0.05).astype(np.float32)
    mask = rs.rand(m, n) < 0.02
    W0, H0 = rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)
    return A, mask, W0, H0, k


@pytest.mark.parametrize("norm", ["fro", "kl"])
def test_masked_steps_along_a_float64_trajectory(norm):
    """From the helper's float64 states after t = 0, 5, 19 steps (cast to float32): ONE masked step on the GPU against the helper's
    float64 step; bound max(tol_step, 2 d_ref), d_ref = distance of the helper's float32 step from its float64 step."""
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests.test_gpu_parity import _tols
    A, mask, W0, H0, k = _traj_problem()
    tol_step = _tols({"method": "mu"})[0]
    S = M.observed(A, mask)
    csr = M.coo_of(S)
    for t in (0, 5, 19):
        Wt, Ht = M.iterate(csr, A.shape, W0.astype(np.float64), H0.astype(np.float64), t, norm)
        Wt, Ht = Wt.astype(np.float32), Ht.astype(np.float32)
        W64, H64, _ = M.fit(csr, A.shape, Wt, Ht, 1, norm, dtype=np.float64)
        W32, H32, _ = M.fit(csr, A.shape, Wt, Ht, 1, norm, dtype=np.float32)
        nmf = PyNMF(S, factors=[Wt, Ht], params=_args(k, 1, norm))
        assert nmf.A_ij.missing == "unstored" and nmf._ops().name == "hip-csr"
        Wg, Hg, _ = nmf.fit()
        for nm, g, r32, r64 in (("W", Wg, W32, W64), ("H", Hg, H32, H64)):
            d_ref, d_gpu = rel_fro(r32, r64), rel_fro(g, r64)
            print("masked trajectory %s t=%2d %s: d_ref=%.2e gpu=%.2e bound=%.2e" % (norm, t, nm, d_ref, d_gpu, max(tol_step, 2 * d_ref)))
            assert d_gpu <= max(tol_step, 2 * d_ref), (norm, t, nm, d_gpu, d_ref)


# ---- check 3: a fully stored block is the reference
@pytest.mark.parametrize("name", M.FULL_GOLDENS)
def test_fully_stored_block_meets_the_reference_golden_on_the_gpu(name):
    from tests._sparse import judge_with_run_case
    out = M.full_case(name, None)
    print("masked full %s (gpu):" % name, {k_: tuple("%.2e" % v for v in vals) for k_, vals in out.items()})
    judge_with_run_case(name, [(0, out, None)])


# ---- check 4: 1D grids, two processes on the one GPU
@pytest.fixture(scope="module")
def one_rank_gpu_fits():
    return M.run_grid((1, 1), use_hip=True)


@pytest.mark.parametrize("grid", [(2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_masked_grids_match_the_one_rank_gpu_fit(grid, one_rank_gpu_fits):
    got = M.run_grid(grid, use_hip=True, timeout=400)
    for combo, (Wr, Hr, err_r) in one_rank_gpu_fits.items():
        W, H, err = got[combo]
        dw, dh, de = rel_fro(W, Wr), rel_fro(H, Hr), abs(err - err_r) / err_r
        print("masked gpu grid %dx%d %s W_update=%s: dW=%.2e dH=%.2e derr=%.2e" % (grid + combo + (dw, dh, de)))
        assert dw <= 1e-5 and dh <= 1e-5 and de <= 1e-5, (grid, combo, dw, dh, de)


def test_one_rank_gpu_fit_matches_the_float64_fit(one_rank_gpu_fits):
    for combo, (Wr, Hr, err_r) in M.reference_fits().items():
        W, H, err = one_rank_gpu_fits[combo]
        dw, dh, de = rel_fro(W, Wr), rel_fro(H, Hr), abs(err - err_r) / err_r
        print("masked gpu 1x1 %s W_update=%s against float64: dW=%.2e dH=%.2e derr=%.2e" % (combo + (dw, dh, de)))
        assert dw <= 1e-4 and dh <= 1e-4 and de <= 1e-5, (combo, dw, dh, de)      # (the fit row of tests/_mp.py::run_case's table)


# ---- check 5: recovery of held-out entries
def test_recovery_of_held_out_entries():
    """planted rank 4, 300 x 200, 30 % observed, 200 MU/FRO iterations: the masked fit predicts the entries it never saw, the
    zero-filled fit of the same stored entries does not"""
    from pydnmfk_amd.pyDNMF import PyNMF
    rs = np.random.RandomState(4)
    m, n, k = 300, 200, 4
    A = (rs.rand(m, k) @ rs.rand(k, n)).astype(np.float32)
    mask = rs.rand(m, n) < 0.3
    W0, H0 = rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)
    S = M.observed(A, mask)
    held = ~mask

    def held_out(W, H):
        R = (A.astype(np.float64) - np.asarray(W, dtype=np.float64) @ np.asarray(H, dtype=np.float64))[held]
        return float(np.linalg.norm(R) / np.linalg.norm(A.astype(np.float64)[held]))

    Wr, Hr, _ = M.fit(M.coo_of(S), A.shape, W0, H0, 200, "fro")
    Wg, Hg, _ = PyNMF(S, factors=[W0, H0], params=_args(k, 200, "fro")).fit()
    Wz, Hz, _ = PyNMF(S, factors=[W0, H0], params=_args(k, 200, "fro", missing=None)).fit()
    e_ref, e_gpu, e_zero = held_out(Wr, Hr), held_out(Wg, Hg), held_out(Wz, Hz)
    print("recovery: held-out error float64 helper %.3e, gpu masked %.3e, gpu zero-filled %.3e" % (e_ref, e_gpu, e_zero))
    assert e_gpu <= 2 * e_ref and e_gpu <= 0.05
    assert e_zero >= 0.5


# ---- check 6: bit-reproducible
_REPRO = r"""
import sys
sys.path.insert(0, %r)
from tests.test_gpu_masked import _repro_digest
print("DIGEST", _repro_digest())
"""


def _repro_digest():
    import hashlib
    from pydnmfk_amd.pyDNMF import PyNMF
    A, mask, W0, H0, k = _traj_problem()
    S = M.observed(A, mask)
    h = hashlib.sha256()
    for norm, itr in (("fro", 20), ("kl", 12)):
        W, H, err = PyNMF(S, factors=[W0, H0], params=_args(k, itr, norm)).fit()
        h.update(W.tobytes()); h.update(H.tobytes()); h.update(np.float64(err).tobytes())
    return h.hexdigest()


def test_masked_bit_reproducible():
    """20 masked MU/FRO and 12 masked MU/KL iterations: twice in this process and once in a fresh child process, identical bit for bit"""
    a, b = _repro_digest(), _repro_digest()
    assert a == b
    res = subprocess.run([sys.executable, "-c", _REPRO % ROOT], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    child = [ln.split()[1] for ln in res.stdout.splitlines() if ln.startswith("DIGEST")]
    assert child == [a], (child, a)
