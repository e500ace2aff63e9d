"""NMFk over sparse data on the CPU: the driver (pydnmfk_amd.pyDNMFk) with a sparse block where the dense `A_ij` stands, over the
checker back end of tests/_sparse_nmfk.py.  On a FULLY STORED matrix the sparse sweep is the dense sweep -- the same numpy stream
for the perturbations and the rand init, the same rules up to summation order -- so the reference's own statistics (nmfk_1x1.npz,
nmfk_2x1.npz) are held with the assertions of tests/test_nmfk_cpu.py, unchanged."""
import types

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")


def test_sparse_nmfk_matches_reference_statistics(tmp_path, golden_dir):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._sparse_nmfk import SparseNmfkOracleOps, full_scipy
    from tests.test_nmfk_cpu import _args, check_against_golden
    z = np.load(golden_dir + "/nmfk_1x1.npz")
    S = full_scipy(z["A"])                                   # precondition: every position of A is stored
    nmfk = PyNMFk(S, factors=None, params=_args(tmp_path, MPI_comm(None, 1, 1)), ops=SparseNmfkOracleOps())
    assert nmfk.A_ij.is_sparse_block and nmfk.A_ij.nnz == z["A"].size and nmfk._batch_size() == 1
    nopt = nmfk.fit()
    check_against_golden(nmfk, nopt, z)


def test_sparse_nmfk_two_ranks_match_reference_statistics(golden_dir):
    from tests._sparse_nmfk import run_nmfk_golden_sparse
    from tests.test_nmfk_cpu import check_nmfk_fixture
    check_nmfk_fixture(run_nmfk_golden_sparse("nmfk_2x1.npz", use_hip=False, timeout=600), np.load(golden_dir + "/nmfk_2x1.npz"), tight=True)


@pytest.mark.parametrize("chunk", [1, 5, 37])
def test_chunked_host_perturbation_is_the_reference_stream(chunk):
    """the uniforms are drawn over the dense shape in row chunks and kept at the stored positions: the values of the dense path
    there, and the generator in the dense path's state afterwards"""
    from pydnmfk_amd.pyDNMFk import host_uniform_values
    rs = np.random.RandomState(5)
    dense = np.where(rs.rand(37, 23) < 0.2, rs.rand(37, 23) + 0.5, 0.0).astype(np.float32)
    S = sp.csr_matrix(dense)
    assert 0.1 < S.nnz / dense.size < 0.3
    nv = 0.03
    np.random.seed(4000)
    M = 2 * nv * np.random.random_sample(dense.shape).astype(dense.dtype) + nv
    want = np.multiply(dense, M + 1)
    state = np.random.get_state()
    np.random.seed(4000)
    got = host_uniform_values(S.indptr, S.indices, S.data, S.shape, nv, chunk_rows=chunk)
    after = np.random.get_state()
    r, c = S.nonzero()
    assert got.dtype == np.float32 and np.array_equal(got, want[r, c])
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]


def test_sample_on_a_block_follows_the_reference_stream_and_keeps_the_pattern():
    """`sample` on a CPU block: the reference's values in both images, the index arrays shared with the source, not copied;
    poisson: integer counts on the source's pattern, a draw of 0 stays stored"""
    import torch
    from pydnmfk_amd.pyDNMFk import sample
    from pydnmfk_amd.sparse import SparseBlock
    rs = np.random.RandomState(6)
    dense = np.where(rs.rand(19, 11) < 0.3, rs.randint(1, 4, size=(19, 11)), 0).astype(np.float32)
    blk = SparseBlock.from_any(sp.csr_matrix(dense), torch.device("cpu"))
    per = sample(blk, 0.03, "uniform", seed=2000).fit()
    np.random.seed(2000)
    want = np.multiply(dense, 2 * 0.03 * np.random.random_sample(dense.shape).astype(np.float32) + 0.03 + 1)
    assert np.array_equal(per.to_dense().numpy(), want)
    assert np.array_equal(per.to_dense().numpy().T[np.nonzero(dense.T)], per.t_val.numpy())
    for name in ("crow", "col", "t_crow", "t_col", "long_rows", "long_segptr", "t_long_rows", "t_long_segptr"):
        assert getattr(per, name) is getattr(blk, name), name
    assert per.missing == blk.missing and per.val is not blk.val and getattr(per, "_sqnorm", None) is None
    poi = sample(blk, 0.03, "poisson", seed=1000).fit()
    g = torch.Generator()
    g.manual_seed(1000)
    assert torch.equal(poi.val, torch.poisson(blk.val, generator=g)) and poi.nnz == blk.nnz and poi.col is blk.col
    assert (poi.val == 0).any() and np.array_equal(poi.to_dense().numpy().T[np.nonzero(dense.T)], poi.t_val.numpy())


def test_operator_sets_without_the_two_operations_are_refused(tmp_path):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from tests._masked import MaskedOracleOps
    from tests._sparse import SparseOracleOps
    from tests._sparse_nmfk import SparseNmfkOracleOps
    from tests.test_nmfk_cpu import _args
    S = sp.csr_matrix(np.abs(np.random.RandomState(0).rand(12, 8)).astype(np.float32))
    comms = MPI_comm(None, 1, 1)
    for ops in (SparseOracleOps(), MaskedOracleOps()):
        with pytest.raises(NotImplementedError, match="^PyNMFk on sparse data is not provided by operator set '%s'" % ops.name):
            PyNMFk(S, params=_args(tmp_path, comms), ops=ops)
    nmfk = PyNMFk(S, params=_args(tmp_path, comms), ops=SparseNmfkOracleOps())
    assert nmfk.A_ij.is_sparse_block and nmfk.A_ij.missing is None
    a = _args(tmp_path, comms)
    a.missing = "unstored"
    assert PyNMFk(S, params=a, ops=SparseNmfkOracleOps()).A_ij.missing == "unstored"
    # what PyNMF refuses for sparse data is refused at construction, in PyNMF's words
    a = _args(tmp_path, comms)
    a.p_r = a.p_c = 2
    with pytest.raises(NotImplementedError, match="sparse data on a 2D grid"):
        PyNMFk(S, params=a, ops=SparseNmfkOracleOps())
    with pytest.raises(NotImplementedError, match="float64 sparse data"):
        PyNMFk(S.astype(np.float64), params=_args(tmp_path, comms), ops=SparseNmfkOracleOps())


def test_column_err_of_the_oracle_equals_the_dense_statement():
    """the helper the sweeps above rest on: per-column sums from the CSR arrays against the dense float64 statement, both meanings"""
    from tests._sparse_nmfk import column_err_sums64
    rs = np.random.RandomState(3)
    m, n, k = 14, 9, 3
    mask = rs.rand(m, n) < 0.5
    mask[:, 4] = False
    A = np.where(mask, rs.rand(m, n) + 0.1, 0.0)
    W, H = rs.rand(m, k), rs.rand(k, n)
    r, c = np.nonzero(mask)
    D = W @ H
    for masked, num, den in ((False, ((A - D) ** 2).sum(0), (A * A).sum(0)), (True, (mask * (A - D) ** 2).sum(0), (A * A).sum(0))):
        gn, gd = column_err_sums64(r, c, A[r, c], n, W, H, masked)
        assert np.allclose(gn, num, rtol=1e-12, atol=1e-13) and np.allclose(gd, den, rtol=1e-12) and gd[4] == 0


@pytest.mark.parametrize("grid", [(1, 1), (2, 1), (1, 2)])
def test_spnpz_reader_cuts_the_ranks_block(tmp_path, grid):
    from pydnmfk_amd.data_io import data_read
    from pydnmfk_amd.utils import determine_block_params, parse
    rs = np.random.RandomState(8)
    dense = np.where(rs.rand(13, 10) < 0.3, rs.rand(13, 10), 0.0).astype(np.float32)
    sp.save_npz(str(tmp_path / "mat.npz"), sp.coo_matrix(dense))
    for rank in range(grid[0] * grid[1]):
        args = parse()
        args.fpath, args.fname, args.ftype, args.p_r, args.p_c = str(tmp_path) + "/", "mat", "spnpz", grid[0], grid[1]
        args.comm1 = types.SimpleNamespace(rank=rank)
        blk = data_read(args).read()
        s, e = determine_block_params(rank, grid, dense.shape).determine_block_index_range_asymm()
        assert sp.issparse(blk) and blk.format == "csr" and blk.dtype == np.float32
        assert np.array_equal(blk.toarray(), dense[s[0]:e[0] + 1, s[1]:e[1] + 1])
    args.ftype = "nope"
    with pytest.raises(ValueError, match="spnpz"):
        data_read(args)
