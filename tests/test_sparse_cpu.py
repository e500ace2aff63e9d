"""Sparse data blocks without a GPU: construction of pydnmfk_amd.sparse.SparseBlock, pruning, the choreography on sparse blocks
(one rank and gloo 1D grids) against the reference's goldens with the checker back end tests/_sparse.py::SparseOracleOps, and
the refusals.  A sparse fit is the dense fit on the densified matrix up to summation order, so the goldens captured from the
reference on dense data are the expected outputs."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

from tests._golden import load_case, rel_fro  # noqa: E402
from tests._sparse import SparseOracleOps, run_case_sparse, to_sparse  # noqa: E402


def _block(x):
    from pydnmfk_amd.sparse import SparseBlock
    return SparseBlock.from_any(x, "cpu")


def _same(a, b):
    for f in ("crow", "col", "val", "t_crow", "t_col", "t_val"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.shape == b.shape and a.nnz == b.nnz


def _args(k, itr, norm, method="mu", W_update=True, prune=False, grid=(1, 1)):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.utils import parse
    comms = MPI_comm(None, 1, 1)
    args = parse()
    args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, grid[0], grid[1], k
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    args.itr, args.init, args.verbose, args.prune = itr, "rand", False, prune
    args.norm, args.method, args.W_update = norm, method, W_update
    return args


def test_construction_is_the_same_from_every_source():
    rs = np.random.RandomState(3)
    A = (rs.rand(37, 23) * (rs.rand(37, 23) < 0.2)).astype(np.float32)
    A[5, :] = 0
    A[:, 7] = 0
    ref = _block(sp.csr_matrix(A))
    assert ref.shape == (37, 23) and ref.dtype == torch.float32 and ref.is_sparse_block and ref.nnz == int((A != 0).sum())
    assert ref.crow.dtype == ref.col.dtype == ref.t_crow.dtype == ref.t_col.dtype == torch.int32 and ref.val.dtype == torch.float32
    assert np.array_equal(ref.to_dense().numpy(), A)
    for kind in ("scipy_csc", "scipy_coo", "torch_csr", "torch_coo"):
        _same(_block(to_sparse(A, kind)), ref)
    from pydnmfk_amd.sparse import SparseBlock
    _same(SparseBlock(ref.crow, ref.col, ref.val, ref.shape), ref)                  # raw arrays
    # the CSR images are what scipy builds: sorted columns, and the transpose is the CSC of the block
    c, t = sp.csr_matrix(A), sp.csr_matrix(A.T)
    c.sort_indices(); t.sort_indices()
    assert np.array_equal(ref.crow.numpy(), c.indptr) and np.array_equal(ref.col.numpy(), c.indices) and np.array_equal(ref.val.numpy(), c.data)
    assert np.array_equal(ref.t_crow.numpy(), t.indptr) and np.array_equal(ref.t_col.numpy(), t.indices) and np.array_equal(ref.t_val.numpy(), t.data)
    assert np.array_equal(ref.nnz_per_row().numpy(), (A != 0).sum(1)) and np.array_equal(ref.nnz_per_col().numpy(), (A != 0).sum(0))


def test_duplicates_summed_zeros_dropped_columns_sorted():
    from pydnmfk_amd.sparse import SparseBlock
    rows = torch.tensor([2, 0, 2, 0, 1, 2, 1])
    cols = torch.tensor([3, 1, 3, 0, 2, 0, 2])
    vals = torch.tensor([1.0, 2.0, 0.5, 0.0, 4.0, 3.0, -4.0])          # (2,3) twice; (0,0) explicit zero; (1,2) sums to zero
    b = SparseBlock.from_coo(rows, cols, vals, (3, 4))
    assert b.crow.tolist() == [0, 1, 1, 3] and b.col.tolist() == [1, 0, 3] and b.val.tolist() == [2.0, 3.0, 1.5]
    assert b.t_crow.tolist() == [0, 1, 2, 2, 3] and b.t_col.tolist() == [2, 0, 2] and b.t_val.tolist() == [3.0, 2.0, 1.5]
    # unsorted raw CSR with a duplicate and a stored zero is normalised
    raw = SparseBlock(torch.tensor([0, 3, 4]), torch.tensor([2, 0, 2, 1]), torch.tensor([1.0, 5.0, 2.0, 0.0]), (2, 3))
    assert raw.crow.tolist() == [0, 2, 2] and raw.col.tolist() == [0, 2] and raw.val.tolist() == [5.0, 3.0]
    empty = SparseBlock.from_coo(torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long), torch.zeros(0), (4, 5))
    assert empty.nnz == 0 and empty.crow.tolist() == [0] * 5 and empty.t_crow.tolist() == [0] * 6


def test_long_rows_are_listed_per_image():
    from pydnmfk_amd import sparse as S
    seg = S._seg()
    A = np.zeros((6, 3 * seg + 5), dtype=np.float32)
    A[1, :] = 1.0                                   # 3 * seg + 5 entries: four segments
    A[4, : seg + 1] = 2.0                           # two segments
    A[3, :seg] = 3.0                                # exactly seg entries: not long
    b = _block(sp.csr_matrix(A))
    assert b.long_rows.tolist() == [1, 4] and b.long_segptr.tolist() == [0, 4, 6] and (b.n_long, b.nseg) == (2, 6)
    assert (b.t_n_long, b.t_nseg) == (0, 0) and b.t_long_segptr.tolist() == [0]


def test_limits_raise_by_name():
    from pydnmfk_amd.sparse import SparseBlock, _check_dims
    with pytest.raises(ValueError, match="nnz < 2\\^31"):
        _check_dims(10, 10, 2 ** 31)
    with pytest.raises(ValueError, match="m, n < 2\\^31"):
        _check_dims(2 ** 31, 10, 5)
    with pytest.raises(ValueError, match="m, n < 2\\^31"):
        SparseBlock.from_coo(torch.tensor([0]), torch.tensor([0]), torch.tensor([1.0]), (3, 2 ** 31))
    with pytest.raises(ValueError, match="outside"):
        SparseBlock.from_coo(torch.tensor([3]), torch.tensor([0]), torch.tensor([1.0]), (3, 2))
    with pytest.raises(NotImplementedError, match="float64 sparse data"):
        _block(sp.csr_matrix(np.eye(3)))
    with pytest.raises(NotImplementedError, match="float64 sparse data"):
        _block(torch.eye(3, dtype=torch.float64).to_sparse_csr())


@pytest.mark.parametrize("name", ["t24x12z_1x1_fro_float32_prune", "t24x12z_1x1_kl_float32_prune"])
def test_prune_on_a_sparse_block(name):
    """same masks, same pruned shape and the same fit as the golden gives for the dense matrix; numpy float64 factors back"""
    from pydnmfk_amd.pyDNMF import PyNMF
    meta, A, W0, H0, z = load_case(name)
    for itr in meta["itrs"]:
        args = _args(meta["k"], itr, meta["norm"], meta.get("method", "mu"), meta["W_update"], prune=True)
        nmf = PyNMF(sp.csr_matrix(A), factors=[W0, H0], params=args, ops=SparseOracleOps())
        dense = PyNMF(A, factors=[W0, H0], params=_args(meta["k"], itr, meta["norm"], meta.get("method", "mu"), meta["W_update"], prune=True),
                      ops=SparseOracleOps())
        for a, b in zip(nmf._masks, dense._masks):
            assert torch.equal(a, b)
        assert nmf.A_ij.is_sparse_block and nmf.A_ij.shape == tuple(dense.A_ij.shape) and nmf.A_ij.shape != A.shape
        assert np.array_equal(nmf.A_ij.to_dense().numpy(), dense.A_ij.numpy())
        W, H, err = nmf.fit()
        assert isinstance(W, np.ndarray) and W.dtype == np.float64 and H.dtype == np.float64
        assert W.shape == z["r0_fit%d_W" % itr].shape and H.shape == z["r0_fit%d_H" % itr].shape
        dw, dh, de = rel_fro(W, z["r0_fit%d_W" % itr]), rel_fro(H, z["r0_fit%d_H" % itr]), abs(err - float(z["r0_fit%d_err" % itr]))
        print("prune %s fit%d: dW=%.2e dH=%.2e derr=%.2e" % (name, itr, dw, dh, de))
        assert dw <= 1e-4 and dh <= 1e-4 and de <= 1e-5


CASES = ["swim_1x1_fro_float32", "swim_1x1_kl_float32", "swim_1x1_hals_float32", "swim_1x1_fro_float32_noW", "swim_1x1_hals_float32_noW",
         "swim_4x1_fro_float32", "swim_4x1_hals_float32", "swim_1x4_fro_float32",
         "lr136x100k32_2x1_fro_float32", "lr136x100k32_2x1_kl_float32", "lr136x100k32_2x1_hals_float32",
         "lr136x100k32_1x2_fro_float32", "lr136x100k32_1x2_kl_float32", "lr136x100k32_1x2_hals_float32"]


@pytest.mark.parametrize("name", CASES)
def test_choreography_on_sparse_blocks_matches_reference_golden(name):
    """tests/_mp.py::run_case's own tolerance table; the one HALS regression case (W fixed, relative error ~73) takes the error
    bound of tests/test_gpu_parity.py::_tols, see tests/_sparse.py::regression_tols"""
    from tests._sparse import regression_tols
    run_case_sparse(name, use_hip=False, tols=regression_tols(name) if name == "swim_1x1_hals_float32_noW" else None)


def test_torch_sparse_input_gives_tensors_back():
    from pydnmfk_amd.pyDNMF import PyNMF
    meta, A, W0, H0, z = load_case("swim_1x1_fro_float32")
    itr = meta["itrs"][0]
    args = _args(meta["k"], itr, "fro", prune=False)
    W, H, err = PyNMF(torch.from_numpy(A).to_sparse_csr(), factors=[torch.from_numpy(W0), torch.from_numpy(H0)], params=args,
                      ops=SparseOracleOps()).fit()
    assert isinstance(W, torch.Tensor) and W.dtype == torch.float32
    assert rel_fro(W.numpy(), z["r0_fit%d_W" % itr]) <= 1e-4 and abs(err - float(z["r0_fit%d_err" % itr])) <= 1e-5


def test_refusals_name_sparse_data():
    from pydnmfk_amd.pyDNMF import PyNMF
    from pydnmfk_amd.pyDNMFk import PyNMFk
    A = sp.csr_matrix(np.abs(np.random.RandomState(0).rand(12, 8)).astype(np.float32))
    ops = SparseOracleOps()
    with pytest.raises(NotImplementedError, match="sparse data on a 2D grid"):
        PyNMF(A, params=_args(2, 3, "fro", grid=(2, 2)), ops=ops)
    a = _args(2, 3, "fro")
    a.init = "nnsvd"
    with pytest.raises(NotImplementedError, match="nnsvd.*sparse data"):
        PyNMF(A, params=a, ops=ops)
    with pytest.raises(NotImplementedError, match="PyNMFk on sparse data"):
        PyNMFk(A, params=_args(2, 3, "fro"), ops=ops)
    with pytest.raises(NotImplementedError, match="float64 sparse data"):
        PyNMF(A.astype(np.float64), params=_args(2, 3, "fro"), ops=ops)
    a = _args(2, 3, "fro")
    a.precision = "bfloat16"
    with pytest.raises(NotImplementedError, match="bfloat16.*sparse data"):
        PyNMF(A, params=a, ops=ops)
    a = _args(2, 3, "fro")
    a.gemm = "bf16x6"
    with pytest.raises(NotImplementedError, match="bf16x6.*sparse data"):
        PyNMF(A, params=a, ops=ops)
    # the 2D choreography itself refuses a sparse block too
    from pydnmfk_amd.dist_nmf import nmf_algorithms_2D
    from pydnmfk_amd.sparse import SparseBlock
    a = _args(2, 3, "fro", grid=(2, 2))
    a.m, a.n, a.eps = 12, 8, 1e-7
    with pytest.raises(NotImplementedError, match="sparse data on a 2D grid"):
        nmf_algorithms_2D(SparseBlock.from_any(A, "cpu"), torch.zeros(6, 2), torch.zeros(2, 4), params=a, ops=ops)
