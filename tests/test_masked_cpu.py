"""Sparse data whose unstored entries are missing (`params.missing = 'unstored'`), without a GPU: construction with stored zeros,
the reference's goldens on fully stored blocks (where the masked rules are the reference's rules), the choreography on one rank
and on gloo 1D grids against the float64 numpy statement of the rules (tests/_masked.py), pruning by observation, the refusals."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

from tests import _masked as M  # noqa: E402
from tests._golden import rel_fro  # noqa: E402


def _block(x, **kw):
    from pydnmfk_amd.sparse import SparseBlock
    return SparseBlock.from_any(x, "cpu", **kw)


def _same(a, b):
    for f in ("crow", "col", "val", "t_crow", "t_col", "t_val"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.shape == b.shape and a.nnz == b.nnz


def _args(k, itr, norm, **kw):
    from pydnmfk_amd.dist_comm import MPI_comm
    grid = kw.pop("grid", (1, 1))
    return M.args_for(MPI_comm(None, 1, 1), grid[0], grid[1], k, itr, norm, **kw)


# ---- 1. construction
def test_keep_zeros_keeps_explicit_zeros_and_entries_that_sum_to_zero():
    from pydnmfk_amd.sparse import SparseBlock
    rows = torch.tensor([2, 0, 2, 0, 1, 2, 1])
    cols = torch.tensor([3, 1, 3, 0, 2, 0, 2])
    vals = torch.tensor([1.0, 2.0, 0.5, 0.0, 4.0, 3.0, -4.0])          # (2,3) twice; (0,0) explicit zero; (1,2) sums to zero
    b = SparseBlock.from_coo(rows, cols, vals, (3, 4), keep_zeros=True, missing="unstored")
    assert b.missing == "unstored"
    assert b.crow.tolist() == [0, 2, 3, 5] and b.col.tolist() == [0, 1, 2, 0, 3] and b.val.tolist() == [0.0, 2.0, 0.0, 3.0, 1.5]
    assert b.t_crow.tolist() == [0, 2, 3, 4, 5] and b.t_col.tolist() == [0, 2, 0, 1, 2] and b.t_val.tolist() == [0.0, 3.0, 2.0, 0.0, 1.5]
    assert b.nnz_per_row().tolist() == [2, 1, 2] and b.nnz_per_col().tolist() == [2, 1, 1, 1]
    # the default is today's block: zeros dropped, unstored entries are zeros
    d = SparseBlock.from_coo(rows, cols, vals, (3, 4))
    assert d.missing is None and d.crow.tolist() == [0, 1, 1, 3] and d.col.tolist() == [1, 0, 3] and d.val.tolist() == [2.0, 3.0, 1.5]
    # raw arrays: unsorted CSR with a duplicate and a stored zero
    raw = SparseBlock(torch.tensor([0, 3, 4]), torch.tensor([2, 0, 2, 1]), torch.tensor([1.0, 5.0, 2.0, 0.0]), (2, 3), keep_zeros=True)
    assert raw.crow.tolist() == [0, 2, 3] and raw.col.tolist() == [0, 2, 1] and raw.val.tolist() == [5.0, 3.0, 0.0] and raw.missing is None
    # the meaning travels with the block
    assert b.to("cpu").missing == "unstored"
    keep_r, keep_c = torch.tensor([True, True, True]), torch.tensor([True, True, True, True])
    assert b.compact(keep_r, keep_c).missing == "unstored" and b.compact(keep_r, keep_c).val.tolist() == b.val.tolist()
    with pytest.raises(ValueError, match="missing"):
        SparseBlock.from_coo(rows, cols, vals, (3, 4), missing="nan")


def test_construction_with_stored_zeros_is_the_same_from_every_source():
    A, mask, _, _, _ = M.small_problem()
    S = M.observed(A, mask)
    assert S.nnz == int(mask.sum()) and int((S.data == 0).sum()) == 4
    ref = _block(S, keep_zeros=True, missing="unstored")
    assert ref.nnz == int(mask.sum()) and ref.missing == "unstored"
    rows, col, val = M.coo_of(S)
    assert np.array_equal(ref.col.numpy(), col) and np.array_equal(ref.val.numpy(), val)
    assert np.array_equal(ref.nnz_per_row().numpy(), mask.sum(1)) and np.array_equal(ref.nnz_per_col().numpy(), mask.sum(0))
    crow = torch.from_numpy(S.indptr.astype(np.int64))
    tcsr = torch.sparse_csr_tensor(crow, torch.from_numpy(S.indices.astype(np.int64)), torch.from_numpy(S.data), size=S.shape)
    tcoo = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, col])), torch.from_numpy(val), size=S.shape)
    for src in (S.tocsc(), S.tocoo(), tcsr, tcoo):
        _same(_block(src, keep_zeros=True, missing="unstored"), ref)
    from pydnmfk_amd.sparse import SparseBlock
    _same(SparseBlock(ref.crow, ref.col, ref.val, ref.shape, keep_zeros=True, missing="unstored"), ref)
    # without keep_zeros the block equals today's: the four stored zeros are dropped
    today = _block(S)
    assert today.missing is None and today.nnz == ref.nnz - 4
    _same(today, _block(sp.csr_matrix(np.where(mask, A, 0).astype(np.float32))))


def test_pynmf_builds_the_flagged_block_and_prunes_by_observation():
    from pydnmfk_amd.pyDNMF import PyNMF
    A, mask, W0, H0, k = M.small_problem()
    mask = mask.copy()
    mask[9, :] = False
    mask[9, 4] = True
    A = A.copy()
    A[9, 4] = 0.0                                                        # row 9: one observation, and it is a zero
    S = M.observed(A, mask)
    nmf = PyNMF(S, factors=[W0, H0], params=_args(k, 3, "fro", prune=True), ops=M.MaskedOracleOps())
    assert nmf.A_ij.missing == "unstored" and nmf.A_ij.nnz == int(mask.sum())
    assert nmf.A_ij.shape == (23, 11)                                    # row 5 and column 7 hold no observation; row 9 stays
    assert nmf._masks[0].tolist() == [r != 5 for r in range(24)] and nmf._masks[1].tolist() == [c != 7 for c in range(12)]
    W, H, err = nmf.fit()
    assert W.shape == (24, k) and H.shape == (k, 12) and not W[5].any() and not H[:, 7].any() and np.isfinite(err)
    # today's meaning drops the stored zeros, so row 9 goes too
    nmf = PyNMF(S, factors=[W0, H0], params=_args(k, 3, "fro", prune=True, missing=None), ops=M.MaskedOracleOps())
    assert nmf.A_ij.missing is None and nmf.A_ij.shape == (22, 11)


# ---- 2. a fully stored block is the reference
@pytest.mark.parametrize("name", M.FULL_GOLDENS)
def test_fully_stored_block_meets_the_reference_golden(name):
    """every position stored, zeros as explicit entries: the masked rules are the reference's up to summation order, so the golden
    holds at the case's row of tests/_mp.py::run_case's table"""
    from tests._sparse import judge_with_run_case
    out = M.full_case(name, M.MaskedOracleOps())
    print("masked full %s:" % name, {k_: tuple("%.2e" % v for v in vals) for k_, vals in out.items()})
    judge_with_run_case(name, [(0, out, None)])


# ---- 3. grids
@pytest.fixture(scope="module")
def reference_fits():
    return M.reference_fits()


@pytest.mark.parametrize("grid", [(1, 1), (2, 1), (1, 2), (3, 1)], ids=lambda g: "%dx%d" % g)
def test_grids_against_the_float64_fit(grid, reference_fits):
    """24 x 12, ~40 % stored, an empty row, an empty column, stored zeros: 20 iterations, fro and kl, W_update on and off; every
    assembled result within 1e-5 relative of the one-rank float64 numpy fit (float32 storage of a 20-iteration fit)"""
    got = M.run_grid(grid, use_hip=False)
    for combo, (Wr, Hr, err_r) in reference_fits.items():
        W, H, err = got[combo]
        dw, dh, de = rel_fro(W, Wr), rel_fro(H, Hr), abs(err - err_r) / err_r
        print("masked grid %dx%d %s W_update=%s: dW=%.2e dH=%.2e derr=%.2e (err %.6g)" % (grid + combo + (dw, dh, de, err_r)))
        assert dw <= 1e-5 and dh <= 1e-5 and de <= 1e-5, (grid, combo, dw, dh, de)


def test_the_masked_fit_differs_from_the_zero_filled_fit():
    """the same stored entries under the two meanings: the flagged fit follows the masked rules, the default fit the reference's"""
    from pydnmfk_amd.pyDNMF import PyNMF
    A, mask, W0, H0, k = M.small_problem()
    S = M.observed(A, mask)
    Wm, Hm, em = PyNMF(S, factors=[W0, H0], params=_args(k, 20, "fro"), ops=M.MaskedOracleOps()).fit()
    Wz, Hz, ez = PyNMF(S, factors=[W0, H0], params=_args(k, 20, "fro", missing=None), ops=M.MaskedOracleOps()).fit()
    assert rel_fro(Wm, Wz) > 1e-2 and em < ez


# ---- 4. refusals
def test_refusals_name_missing():
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    A, mask, W0, H0, k = M.small_problem()
    S = M.observed(A, mask)
    ops = M.MaskedOracleOps()
    with pytest.raises(NotImplementedError, match="missing.*dense"):
        PyNMF(np.where(mask, A, 0).astype(np.float32), params=_args(k, 3, "fro"), ops=ops)
    for method in ("hals", "bcd"):
        with pytest.raises(NotImplementedError, match="missing.*%s" % method):
            PyNMF(S, params=_args(k, 3, "fro", method=method), ops=ops)
    with pytest.raises(ValueError, match="missing"):
        PyNMF(S, params=_args(k, 3, "fro", missing="nan"), ops=ops)
    # a block the caller built must carry the meaning the fit asks for, either way round
    with pytest.raises(ValueError, match="missing"):
        PyNMF(_block(S), params=_args(k, 3, "fro"), ops=ops)
    with pytest.raises(ValueError, match="missing"):
        PyNMF(_block(S, keep_zeros=True, missing="unstored"), params=_args(k, 3, "fro", missing=None), ops=ops)
    blk = _block(S, keep_zeros=True, missing="unstored")
    assert PyNMF(blk, factors=[W0, H0], params=_args(k, 3, "fro"), ops=ops).A_ij is blk
    # the choreography dispatches on the block: HALS / BCD on a flagged block are refused there too, whatever params say
    for method in ("hals", "bcd"):
        a = _args(k, 3, "fro", method=method, missing=None)
        a.m, a.n, a.eps = 24, 12, M.EPS
        with pytest.raises(NotImplementedError, match="missing"):
            nmf_algorithms_1D(blk, torch.from_numpy(W0.copy()), torch.from_numpy(H0.copy()), params=a, ops=ops).update()
    # ... and an operator set without the masked operations is named, not tripped over
    from tests._sparse import SparseOracleOps
    a = _args(k, 3, "fro")
    a.m, a.n, a.eps = 24, 12, M.EPS
    with pytest.raises(NotImplementedError, match="missing"):
        nmf_algorithms_1D(blk, torch.from_numpy(W0.copy()), torch.from_numpy(H0.copy()), params=a, ops=SparseOracleOps()).update()
    # the existing sparse refusals hold under the flag: 2D grids, NMFk
    with pytest.raises(NotImplementedError, match="sparse data on a 2D grid"):
        PyNMF(S, params=_args(k, 3, "fro", grid=(2, 2)), ops=ops)
    from pydnmfk_amd.pyDNMFk import PyNMFk
    with pytest.raises(NotImplementedError, match="PyNMFk on sparse data"):
        PyNMFk(S, params=_args(k, 3, "fro"), ops=ops)
