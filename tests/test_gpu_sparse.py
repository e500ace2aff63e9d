"""Sparse data blocks on the GPU (csrc/dnmf_csr.h through engine.HipCsrOps): the kernels against float64, the reference's goldens
with the block handed over as scipy.sparse.csr_matrix (one rank and 1D grids), single sparse steps along a float64 trajectory,
bit-reproducibility, and one block whose dense image would not fit.  Every test constructs PyNMF / the operator set from a sparse
object, which the dense-only code refuses."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

from tests._golden import load_case, rel_fro  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float32).eps)
KS = (1, 3, 4, 16, 17, 32, 64, 100, 128, 192, 256)


def _ops():
    from pydnmfk_amd.engine import HIP_CSR_OPS
    return HIP_CSR_OPS


def _block(x):
    from pydnmfk_amd.sparse import SparseBlock
    return SparseBlock.from_any(x, torch.device("cuda", 0))


def _random_block(rs, m, n, density):
    if density >= 1.0:
        A = (rs.rand(m, n) + 0.05).astype(np.float32)
    else:
        A = ((rs.rand(m, n) + 0.05) * (rs.rand(m, n) < density)).astype(np.float32)
    return A


def _skewed(rs, m, n):
    """empty rows, and one row and one column that together hold more than 30 % of all stored entries"""
    A = ((rs.rand(m, n) + 0.05) * (rs.rand(m, n) < 0.004)).astype(np.float32)
    A[:, 5] = rs.rand(m) + 0.05
    A[::7, :] = 0                                                # (row 3 is not one of them)
    A[3, :] = rs.rand(n) + 0.05
    heavy = int((A[3] != 0).sum() + (A[:, 5] != 0).sum() - 1)
    assert heavy >= 0.3 * int((A != 0).sum())
    return A.astype(np.float32)


def _products64(A, W, H):
    """float64 numpy evaluation of the five sparse operations from the same arrays (the shapes here are small: dense algebra)"""
    A64, W64, H64 = A.astype(np.float64), W.astype(np.float64), H.astype(np.float64)
    D = W64 @ H64
    Q = np.where(A64 != 0, A64 / (D + EPS), 0.0)
    return A64 @ H64.T, W64.T @ A64, Q @ H64.T, W64.T @ Q, float(np.sum((A64 - D) ** 2))


def _gpu_products(blk, W, H):
    ops = _ops()
    m, n = blk.shape
    k = W.shape[1]
    Wd, Hd = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
    aht, uht = torch.full((m, k), np.nan, device="cuda"), torch.full((m, k), np.nan, device="cuda")
    wta, wtu = torch.full((k, n), np.nan, device="cuda"), torch.full((k, n), np.nan, device="cuda")
    ops.aht(blk, Hd, aht)
    ops.wta(blk, Wd, wta)
    ops.kl_uht(blk, Wd, Hd, EPS, uht)
    ops.kl_wtu(blk, Wd, Hd, EPS, wtu)
    r = ops.resid_sqnorm(blk, Wd, Hd)
    return aht.cpu().numpy(), wta.cpu().numpy(), uht.cpu().numpy(), wtu.cpu().numpy(), float(r.cpu())


def _rel(x, ref):
    nr = np.linalg.norm(ref)
    return float(np.linalg.norm(x.astype(np.float64) - ref) / nr) if nr > 0 else float(np.abs(x).max(initial=0.0))


def _check_kernels(tag, A, blk, W, H):
    got = _gpu_products(blk, W, H)
    ref = _products64(A, W, H)
    d = [_rel(g, r) for g, r in zip(got[:4], ref[:4])]
    dr = abs(got[4] - ref[4]) / max(ref[4], 1e-300)
    print("kernels %-28s k=%3d nnz=%8d  aht %.2e wta %.2e | uht %.2e wtu %.2e | resid %.2e" % (tag, W.shape[1], blk.nnz, d[0], d[1], d[2], d[3], dr))
    for g in got[:4]:
        assert np.isfinite(g).all(), tag                    # every output element was written
    empty_rows, empty_cols = (A != 0).sum(1) == 0, (A != 0).sum(0) == 0
    for g in (got[0], got[2]):
        assert not g[empty_rows].any(), tag                 # exact zeros, not small values
    for g in (got[1], got[3]):
        assert not g[:, empty_cols].any(), tag
    assert d[0] <= 2e-6 and d[1] <= 2e-6, (tag, d)
    assert d[2] <= 1e-5 and d[3] <= 1e-5, (tag, d)
    assert dr <= 1e-5, (tag, got[4], ref[4])


def test_kernels_against_float64():
    rs = np.random.RandomState(100)
    shapes = ((1, 1), (7, 5), (1000, 333), (4097, 513))
    for (m, n) in shapes:
        for density in (0.0, 0.001, 0.05, 1.0):
            A = _random_block(rs, m, n, density)
            blk = _block(sp.csr_matrix(A))
            assert blk.nnz == int((A != 0).sum())
            for k in KS:
                W, H = (rs.rand(m, k) + 0.01).astype(np.float32), (rs.rand(k, n) + 0.01).astype(np.float32)
                _check_kernels("%dx%d d=%g" % (m, n, density), A, blk, W, H)
    for (m, n) in ((1000, 333), (4097, 513)):
        A = _skewed(rs, m, n)
        blk = _block(sp.csr_matrix(A))
        for k in KS:
            W, H = (rs.rand(m, k) + 0.01).astype(np.float32), (rs.rand(k, n) + 0.01).astype(np.float32)
            _check_kernels("%dx%d skewed" % (m, n), A, blk, W, H)
        assert blk.t_n_long >= 1 or m <= 1024                   # the heavy column is a long row of the transpose
    # the same skew the other way round: the BLOCK has rows of more than one segment (the row pass of aht / kl_uht leaves them to
    # the segment kernels, the residual adds their float64 partials), the transpose has none
    A = np.ascontiguousarray(_skewed(rs, 4097, 513).T)
    blk = _block(sp.csr_matrix(A))
    assert blk.n_long >= 1 and blk.nseg >= 2 * blk.n_long and blk.t_n_long == 0
    for k in KS:
        W, H = (rs.rand(513, k) + 0.01).astype(np.float32), (rs.rand(k, 4097) + 0.01).astype(np.float32)
        _check_kernels("513x4097 skewed rows", A, blk, W, H)
    # long rows in BOTH images
    A = (rs.rand(1500, 2100) + 0.05).astype(np.float32) * (rs.rand(1500, 2100) < 0.01)
    A[7, :] = rs.rand(2100) + 0.05
    A[:, 11] = rs.rand(1500) + 0.05
    A = A.astype(np.float32)
    blk = _block(sp.csr_matrix(A))
    assert blk.n_long >= 1 and blk.t_n_long >= 1
    for k in (3, 16, 64, 100, 256):
        W, H = (rs.rand(1500, k) + 0.01).astype(np.float32), (rs.rand(k, 2100) + 0.01).astype(np.float32)
        _check_kernels("1500x2100 long both", A, blk, W, H)


def test_residual_of_a_fully_stored_low_rank_block():
    """1000 x 333 from rank-k factors plus 1 % noise, evaluated AT those factors: the residual is ~1e-4 of ||A||^2, so the
    stored-entry sum and the Gram term cancel to four digits"""
    rs = np.random.RandomState(7)
    m, n = 1000, 333
    for k in KS:
        W, H = rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)
        P = W.astype(np.float64) @ H.astype(np.float64)
        A = np.abs(P * (1.0 + 0.01 * rs.randn(m, n))).astype(np.float32)
        A[A == 0] = 1e-3
        blk = _block(sp.csr_matrix(A))
        assert blk.nnz == m * n
        got = float(_ops().resid_sqnorm(blk, torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()).cpu())
        ref = float(np.sum((A.astype(np.float64) - P) ** 2))
        den = float(np.sum(A.astype(np.float64) ** 2))
        print("low-rank resid k=%3d: ||R||^2/||A||^2 = %.3e, rel diff %.2e" % (k, ref / den, abs(got - ref) / ref))
        assert abs(got - ref) <= 1e-5 * ref, (k, got, ref)


# ---- check 2: the reference's goldens on one rank, the block as scipy.sparse.csr_matrix
def _args(k, itr, norm, W_update=True, method="mu", prune=False):
    from tests.test_gpu_parity import _args as parity_args
    return parity_args(k, itr, norm, W_update, method, prune)


SINGLE = (["swim_1x1_fro_float32", "swim_1x1_kl_float32", "swim_1x1_hals_float32", "swim_1x1_fro_float32_noW", "swim_1x1_hals_float32_noW",
           "t24x12z_1x1_fro_float32_prune", "t24x12z_1x1_kl_float32_prune"] +
          ["%s_1x1_%s_float32" % (d, f) for d in ("lr136x100k32", "lr200x136k64", "lr150x140k128") for f in ("fro", "kl", "hals")])


@pytest.mark.parametrize("name", SINGLE)
def test_goldens_one_rank_sparse(name):
    """W, H, recon_err of every fit<N> and the bare step1 within tests/test_gpu_parity.py::_tols, applied as that file applies them"""
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests.test_gpu_parity import _tols
    meta, A, W0, H0, z = load_case(name)
    tol_step, tol_fit, tol_err = _tols(meta)
    S = sp.csr_matrix(A)
    for itr in meta["itrs"]:
        args = _args(meta["k"], itr, meta["norm"], meta["W_update"], meta.get("method", "mu"), meta.get("prune", False))
        nmf = PyNMF(S, factors=[W0, H0], params=args)
        assert nmf.A_ij.is_sparse_block and nmf._ops().name == "hip-csr"
        W, H, err = nmf.fit()
        assert isinstance(W, np.ndarray) and W.dtype == z["r0_fit%d_W" % itr].dtype and H.dtype == z["r0_fit%d_H" % itr].dtype
        ref = float(z["r0_fit%d_err" % itr])
        dw, dh = rel_fro(W, z["r0_fit%d_W" % itr]), rel_fro(H, z["r0_fit%d_H" % itr])
        print("golden %s fit%d: dW=%.2e dH=%.2e derr=%.2e (err %.6g)" % (name, itr, dw, dh, abs(err - ref), ref))
        assert dw <= tol_fit, itr
        assert dh <= (5e-4 if meta.get("method") == "hals" else tol_fit), itr
        assert abs(err - ref) <= tol_err * max(1.0, abs(ref)), itr
    if meta.get("prune"):
        return                                                   # pruned cases are pinned through fit(), as in the dense suite
    args = _args(meta["k"], 1, meta["norm"], meta["W_update"], meta.get("method", "mu"))
    args.m, args.n, args.eps = meta["m"], meta["n"], EPS
    W, H = torch.from_numpy(W0).cuda(), torch.from_numpy(H0).cuda()
    W1, H1 = nmf_algorithms_1D(_block(S), W, H, params=args).update()
    assert W1 is W and H1 is H
    dw, dh = rel_fro(W.cpu().numpy(), z["r0_step1_W"]), rel_fro(H.cpu().numpy(), z["r0_step1_H"])
    print("golden %s step1: dW=%.2e dH=%.2e" % (name, dw, dh))
    assert dw <= tol_step and dh <= tol_step


def test_bcd_on_a_sparse_block_matches_reference_golden():
    """method='bcd' reaches A through aht, wta_gram, resid_sqnorm and sqnorm only: pinned against the reference's BCD golden on swim"""
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests._bcd import _params, check_tolerances, load_bcd
    meta, A, W0, H0, z = load_bcd("swim_1x1")
    comms = MPI_comm(None, 1, 1)
    S = sp.csr_matrix(A)
    out = {}
    for N in meta["steps"]:
        nmf = PyNMF(S, factors=[W0, H0], params=_params(comms, meta, N, None))
        assert nmf._ops().name == "hip-csr"
        W1, H1 = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update()
        out["step%d" % N] = (rel_fro(W1.cpu().numpy(), z["r0_step%d_W" % N]), rel_fro(H1.cpu().numpy(), z["r0_step%d_H" % N]), 0.0)
    for N in meta["itrs"]:
        W, H, err = PyNMF(S, factors=[W0, H0], params=_params(comms, meta, N, None)).fit()
        out["fit%d" % N] = (rel_fro(W, z["r0_fit%d_W" % N]), rel_fro(H, z["r0_fit%d_H" % N]), abs(err - float(z["r0_fit%d_err" % N])))
    print("bcd swim_1x1 sparse:", {k_: tuple("%.2e" % v for v in vals) for k_, vals in out.items()})
    check_tolerances("swim_1x1", {0: out})


# ---- check 3: 1D grids, ranks as processes on the one GPU over gloo
GRID4 = ["swim_4x1_fro_float32", "swim_1x4_fro_float32"]
GRID2 = ["%s_%s_%s_float32" % (d, g, f) for d in ("lr200x136k64", "lr136x100k32") for g in ("2x1", "1x2") for f in ("kl", "hals")]


@pytest.mark.parametrize("names", [GRID4, GRID2], ids=["four_ranks", "two_ranks"])
def test_goldens_1d_grids_sparse(names):
    """each rank passes its sparse block; the cases of one world size share their rank processes (a GPU process takes seconds to
    start); every case is then judged by tests/_mp.py::run_case's own tolerance table"""
    from tests._sparse import judge_with_run_case, run_cases_sparse_shared
    res = run_cases_sparse_shared(names, use_hip=True, timeout=400)
    for nm in names:
        judge_with_run_case(nm, res[nm])


# ---- check 4: single sparse steps along a float64 trajectory
def _traj_problem():
    rs = np.random.RandomState(100)
    m, n, k = 1500, 1000, 32
    A = ((rs.rand(m, n) + 0.05) * (rs.rand(m, n) < 0.02)).astype(np.float32)
    W0, H0 = rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)
    return A, W0, H0, k


@pytest.mark.parametrize("norm,method", [("fro", "mu"), ("fro", "hals"), ("kl", "mu")])
def test_sparse_steps_along_a_float64_trajectory(norm, method):
    """From the float64 oracle's states after t = 0, 5, 19 steps (cast to float32): ONE step of the sparse GPU path against the
    oracle's float64 step; bound max(tol_step, 2 d_ref), d_ref = distance of the oracle's float32 step from its float64 step."""
    from oracle import nmf_oracle as orc
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests.test_gpu_parity import _tols
    A, W0, H0, k = _traj_problem()
    tol_step = _tols({"method": method})[0]
    S = sp.csr_matrix(A)
    A64 = A.astype(np.float64)
    for t in (0, 5, 19):
        if t == 0:
            Wt, Ht = W0, H0
        else:
            Wt, Ht, _ = orc.fit_single(A64, W0.astype(np.float64), H0.astype(np.float64), t, norm=norm, method=method, eps=EPS)
            Wt, Ht = Wt.astype(np.float32), Ht.astype(np.float32)
        W64, H64, _ = orc.fit_single(A64, Wt.astype(np.float64), Ht.astype(np.float64), 1, norm=norm, method=method, eps=EPS)
        W32, H32, _ = orc.fit_single(A, Wt.copy(), Ht.copy(), 1, norm=norm, method=method, eps=EPS)
        Wg, Hg, _ = PyNMF(S, factors=[Wt, Ht], params=_args(k, 1, norm, True, method)).fit()
        for nm, g, r32, r64 in (("W", Wg, W32, W64), ("H", Hg, H32, H64)):
            d_ref, d_gpu = rel_fro(r32, r64), rel_fro(g, r64)
            print("trajectory %s/%s t=%2d %s: d_ref=%.2e gpu=%.2e bound=%.2e" % (norm, method, t, nm, d_ref, d_gpu, max(tol_step, 2 * d_ref)))
            assert d_gpu <= max(tol_step, 2 * d_ref), (norm, method, t, nm, d_gpu, d_ref)


# ---- check 5: bit-reproducible
_REPRO = r"""
import sys, hashlib
sys.path.insert(0, %r)
import numpy as np, scipy.sparse as sp, torch
from tests.test_gpu_sparse import _repro_digest
print("DIGEST", _repro_digest())
"""


def _repro_digest():
    import hashlib
    from pydnmfk_amd.pyDNMF import PyNMF
    A, W0, H0, k = _traj_problem()
    S = sp.csr_matrix(A)
    h = hashlib.sha256()
    for norm, itr in (("fro", 20), ("kl", 12)):
        W, H, err = PyNMF(S, factors=[W0, H0], params=_args(k, itr, norm, True, "mu")).fit()
        h.update(W.tobytes()); h.update(H.tobytes()); h.update(np.float64(err).tobytes())
    rs = np.random.RandomState(5)
    B = _skewed(rs, 4097, 513)
    Wk, Hk = (rs.rand(4097, 17) + 0.01).astype(np.float32), (rs.rand(17, 513) + 0.01).astype(np.float32)
    got = _gpu_products(_block(sp.csr_matrix(B)), Wk, Hk)
    for g in (got[0], got[1], got[2]):
        h.update(g.tobytes())
    return h.hexdigest()


def test_bit_reproducible():
    """20 MU/FRO and 12 MU/KL iterations and three products on the skewed matrix: twice in this process and once in a fresh
    child process, identical bit for bit"""
    a, b = _repro_digest(), _repro_digest()
    assert a == b
    res = subprocess.run([sys.executable, "-c", _REPRO % ROOT], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    child = [ln.split()[1] for ln in res.stdout.splitlines() if ln.startswith("DIGEST")]
    assert child == [a], (child, a)


# ---- check 6: a block whose dense image could not sit in HBM next to its factors
def test_beyond_dense():
    """2^20 x 2^16 (a 256 GiB dense image) with 5e7 uniformly placed stored entries built on the GPU, k = 16, five MU/FRO steps"""
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.sparse import SparseBlock
    dev = torch.device("cuda", 0)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    m, n, k, nnz = 2 ** 20, 2 ** 16, 16, 50_000_000
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    rows = torch.randint(0, m, (nnz,), device=dev, generator=g, dtype=torch.int32)
    cols = torch.randint(0, n, (nnz,), device=dev, generator=g, dtype=torch.int32)
    vals = torch.rand(nnz, device=dev, generator=g) + 0.05
    blk = SparseBlock.from_coo(rows, cols, vals, (m, n))
    del rows, cols, vals
    assert blk.shape == (m, n) and 0.99 * nnz < blk.nnz <= nnz
    W = torch.rand(m, k, device=dev, generator=g)
    H = torch.rand(k, n, device=dev, generator=g)
    args = _args(k, 5, "fro", True, "mu")
    args.m, args.n, args.eps = m, n, EPS
    ops = _ops()
    sq = [float(ops.resid_sqnorm(blk, W, H).cpu())]
    for i in range(5):
        nmf_algorithms_1D(blk, W, H, params=args, ops=ops).update(clamp=(i % 10 == 0))
        sq.append(float(ops.resid_sqnorm(blk, W, H).cpu()))
    peak = torch.cuda.max_memory_allocated()
    print("beyond dense: nnz=%d, ||A - WH||^2 = %s, peak %.2f GB" % (blk.nnz, ["%.6e" % v for v in sq], peak / 1e9))
    assert peak < 8e9, peak
    assert all(b < a for a, b in zip(sq[:-1], sq[1:])), sq
    # the same formula in float64 torch from the CSR arrays and the float32 factors, in slices of the stored entries
    W64, HT64 = W.double(), H.double().t().contiguous()
    rowid = torch.repeat_interleave(torch.arange(m, device=dev, dtype=torch.int32), blk.nnz_per_row())
    tot = torch.zeros((), dtype=torch.float64, device=dev)
    step = 4_000_000
    for p0 in range(0, blk.nnz, step):
        r, c, a = rowid[p0:p0 + step].long(), blk.col[p0:p0 + step].long(), blk.val[p0:p0 + step].double()
        d = (W64[r] * HT64[c]).sum(1)
        tot += (a * (a - 2.0 * d)).sum()
    ref = float(tot + ((W64.t() @ W64) * (HT64.t() @ HT64)).sum())
    print("beyond dense: library %.9e, float64 torch %.9e, rel diff %.2e" % (sq[-1], ref, abs(sq[-1] - ref) / ref))
    assert abs(sq[-1] - ref) <= 1e-5 * ref
