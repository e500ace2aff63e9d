"""Dense data whose missing entries are NaN (`params.missing = 'nan'`), without a GPU: the refusals, the block and its oracle operator
set through PyNMF on one rank and on gloo 1D grids against the float64 numpy statement of the rules (tests/_masked.py), main.py's
flag, and the float64 proof that the exact operands of the GPU test stay integers below 2^24 under a mask."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

from tests import _masked as M  # noqa: E402
from tests import _masked_dense as D  # noqa: E402
from tests._golden import rel_fro  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(k, itr, norm, **kw):
    from pydnmfk_amd.dist_comm import MPI_comm
    grid = kw.pop("grid", (1, 1))
    return D.args_for(MPI_comm(None, 1, 1), grid[0], grid[1], k, itr, norm, **kw)


def _problem():
    A, mask, W0, H0, k = M.small_problem()
    return D.nan_marked(A, mask), mask, W0, H0, k


# ---- 1. the block, the refusals, what stays as it is
def test_pynmf_wraps_the_nan_marked_block():
    from pydnmfk_amd.dist_nmf import _is_masked, _is_sparse
    from pydnmfk_amd.masked import MaskedDenseBlock
    from pydnmfk_amd.pyDNMF import PyNMF
    An, mask, W0, H0, k = _problem()
    assert np.isnan(An).sum() == (~mask).sum() and int((An == 0).sum()) == 4          # the four observed zeros stay observations
    for data in (An, torch.from_numpy(An)):
        nmf = PyNMF(data, factors=[W0, H0], params=_args(k, 3, "fro"), ops=D.MaskedDenseOracleOps())
        blk = nmf.A_ij
        assert isinstance(blk, MaskedDenseBlock) and blk.missing == "nan" and blk.is_masked_dense
        assert tuple(blk.shape) == An.shape and blk.dtype == torch.float32 and blk.device.type == "cpu"
        assert blk.n_observed == int(mask.sum())
        assert _is_masked(blk) and not _is_sparse(blk)
        assert np.array_equal(np.isnan(blk.tensor.numpy()), ~mask)                    # the data stay as handed over: no mask array
        assert not nmf._whole_fit_ok(nmf._ops())
        W, H, err = nmf.fit()
        assert np.isfinite(np.asarray(W)).all() and np.isfinite(np.asarray(H)).all() and np.isfinite(err)
    assert isinstance(nmf.fit()[0], torch.Tensor)                                      # tensor in, tensors out


def test_dense_data_without_missing_are_not_scanned_for_nan():
    """no params.missing: the NaN-holding array is an ordinary dense block (a tensor, not a MaskedDenseBlock), exactly as before"""
    from pydnmfk_amd.dist_nmf import _is_masked
    from pydnmfk_amd.pyDNMF import PyNMF
    An, mask, W0, H0, k = _problem()
    nmf = PyNMF(An, factors=[W0, H0], params=_args(k, 3, "fro", missing=None), ops=M.MaskedOracleOps())
    assert isinstance(nmf.A_ij, torch.Tensor) and not _is_masked(nmf.A_ij) and not nmf._masked_dense
    assert torch.isnan(nmf.A_ij).sum() == (~mask).sum()


def test_refusals_name_missing_and_the_combination():
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D, nmf_algorithms_2D
    from pydnmfk_amd.masked import MaskedDenseBlock
    from pydnmfk_amd.pyDNMF import PyNMF
    from pydnmfk_amd.pyDNMFk import PyNMFk
    An, mask, W0, H0, k = _problem()
    ops = D.MaskedDenseOracleOps()
    for method in ("hals", "bcd"):
        with pytest.raises(NotImplementedError, match="missing='nan'.*%s" % method):
            PyNMF(An, params=_args(k, 3, "fro", method=method), ops=ops)
    with pytest.raises(NotImplementedError, match="missing='nan'.*2D grid"):
        PyNMF(An, params=_args(k, 3, "fro", grid=(2, 2)), ops=ops)
    with pytest.raises(NotImplementedError, match="missing='nan'.*prune"):
        PyNMF(An, factors=[W0, H0], params=_args(k, 3, "fro", prune=True), ops=ops)
    a = _args(k, 3, "fro")
    a.init = "nnsvd"
    with pytest.raises(NotImplementedError, match="missing='nan'.*nnsvd"):
        PyNMF(An, params=a, ops=ops)
    with pytest.raises(NotImplementedError, match="missing='nan'.*float64"):
        PyNMF(An.astype(np.float64), params=_args(k, 3, "fro"), ops=ops)
    with pytest.raises(NotImplementedError, match="missing='nan'.*bfloat16"):
        PyNMF(torch.from_numpy(An).to(torch.bfloat16), params=_args(k, 3, "fro"), ops=ops)
    a = _args(k, 3, "fro")
    a.precision = "bfloat16"
    with pytest.raises(NotImplementedError, match="missing='nan'.*bfloat16"):
        PyNMF(An, params=a, ops=ops)
    a = _args(k, 3, "fro")
    a.gemm = "bf16x6"
    with pytest.raises(NotImplementedError, match="missing='nan'.*bf16x6"):
        PyNMF(An, params=a, ops=ops)
    from pydnmfk_amd.engine import ops_for
    with pytest.raises(NotImplementedError, match="missing='nan'.*bf16x6"):
        ops_for(a, torch.float32, masked=True)
    big = np.full((4, 200), np.nan, dtype=np.float32)
    with pytest.raises(NotImplementedError, match="missing='nan'.*k = 129"):
        PyNMF(big, params=_args(129, 3, "fro"), ops=ops)
    with pytest.raises(NotImplementedError, match="PyNMFk.*missing='nan'"):
        PyNMFk(An, params=_args(k, 3, "fro"), ops=ops)
    # the choreography dispatches on the block: HALS / BCD and the 2D grid are refused there too, whatever params say
    blk = MaskedDenseBlock(torch.from_numpy(An))
    for method in ("hals", "bcd"):
        a = _args(k, 3, "fro", method=method, missing=None)
        a.m, a.n, a.eps = 24, 12, M.EPS
        with pytest.raises(NotImplementedError, match="missing='nan'.*%s" % method):
            nmf_algorithms_1D(blk, torch.from_numpy(W0.copy()), torch.from_numpy(H0.copy()), params=a, ops=ops).update()
    a = _args(k, 3, "fro", grid=(2, 2), missing=None)
    a.m, a.n, a.eps = 24, 12, M.EPS
    with pytest.raises(NotImplementedError, match="missing='nan'.*2D grid"):
        nmf_algorithms_2D(blk, torch.from_numpy(W0.copy()), torch.from_numpy(H0.copy()), params=a, ops=ops)
    # an operator set without the masked operations is named, not tripped over
    from tests._ops_double import OracleOps
    a = _args(k, 3, "fro")
    a.m, a.n, a.eps = 24, 12, M.EPS
    with pytest.raises(NotImplementedError, match="missing='nan'"):
        nmf_algorithms_1D(blk, torch.from_numpy(W0.copy()), torch.from_numpy(H0.copy()), params=a, ops=OracleOps()).update()
    # a block is float32, 2-D
    with pytest.raises(NotImplementedError, match="missing='nan'.*float64"):
        MaskedDenseBlock(torch.from_numpy(An.astype(np.float64)))


def test_what_stays_as_it_is():
    from pydnmfk_amd import sparse
    from pydnmfk_amd.pyDNMF import PyNMF
    from pydnmfk_amd.sparse import SparseBlock
    A, mask, W0, H0, k = M.small_problem()
    S = M.observed(A, mask)
    ops = M.MaskedOracleOps()
    with pytest.raises(NotImplementedError, match="missing.*dense"):                  # 'unstored' keeps its refusal of dense input
        PyNMF(np.where(mask, A, 0).astype(np.float32), params=M.args_for(_args(k, 3, "fro").comm, 1, 1, k, 3, "fro"), ops=ops)
    rows, col, val = M.coo_of(S)
    coo = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, col])), torch.from_numpy(val), size=S.shape)
    for data in (S, coo, SparseBlock.from_any(S, "cpu"), SparseBlock.from_any(S, "cpu", keep_zeros=True, missing="unstored")):
        with pytest.raises(ValueError, match="missing"):                              # 'nan' with sparse input stays a ValueError
            PyNMF(data, params=_args(k, 3, "fro"), ops=ops)
    assert sparse.MISSING == (None, "unstored")                                       # the sparse block's own set of meanings
    with pytest.raises(ValueError, match="missing"):
        SparseBlock.from_any(S, "cpu", missing="nan")
    with pytest.raises(ValueError, match="missing"):
        PyNMF(D.nan_marked(A, mask), params=_args(k, 3, "fro", missing="NaN"), ops=ops)      # (an unknown value)


# ---- 2. the oracle operator set through PyNMF
@pytest.fixture(scope="module")
def reference_fits():
    return M.reference_fits()


@pytest.fixture(scope="module")
def one_rank_fits():
    return D.run_grid((1, 1), use_hip=False)


def _close(got, want, what):
    for combo, (Wr, Hr, err_r) in want.items():
        W, H, err = got[combo]
        dw, dh, de = rel_fro(W, Wr), rel_fro(H, Hr), abs(err - err_r) / err_r
        print("masked dense %s %s W_update=%s: dW=%.2e dH=%.2e derr=%.2e (err %.6g)" % ((what,) + combo + (dw, dh, de, err_r)))
        assert dw <= 1e-5 and dh <= 1e-5 and de <= 1e-5, (what, combo, dw, dh, de)     # (the bounds of tests/test_masked_cpu.py)


def test_one_rank_against_the_float64_fit(one_rank_fits, reference_fits):
    """small_problem() with NaN where its mask is false: 20 iterations, fro and kl, W_update on and off, equal to the float64 numpy fit
    of the same observations; the factor row / column without an observation ends as eps-clamped then normalised, as for CSR"""
    _close(one_rank_fits, reference_fits, "1x1 / float64")


@pytest.mark.parametrize("grid", [(2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_grids_against_the_one_rank_fit(grid, one_rank_fits):
    _close(D.run_grid(grid, use_hip=False), one_rank_fits, "%dx%d / 1x1" % grid)


def test_the_masked_fit_differs_from_the_zero_filled_fit():
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests._ops_double import OracleOps
    A, mask, W0, H0, k = M.small_problem()
    Wm, Hm, em = PyNMF(D.nan_marked(A, mask), factors=[W0, H0], params=_args(k, 20, "fro"), ops=D.MaskedDenseOracleOps()).fit()
    Wz, Hz, ez = PyNMF(np.where(mask, A, 0).astype(np.float32), factors=[W0, H0], params=_args(k, 20, "fro", missing=None), ops=OracleOps()).fit()
    assert rel_fro(Wm, Wz) > 1e-2 and em < ez


@pytest.mark.parametrize("name", M.FULL_GOLDENS)
def test_block_without_a_nan_meets_the_reference_golden(name):
    from tests._sparse import judge_with_run_case
    out = D.full_case(name, D.MaskedDenseOracleOps())
    print("masked dense full %s:" % name, {k_: tuple("%.2e" % v for v in vals) for k_, vals in out.items()})
    judge_with_run_case(name, [(0, out, None)])


# ---- 3. main.py --missing nan
def test_main_accepts_missing_nan_for_dense_file_types_and_refuses_spnpz(tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import main as cli
    finally:
        sys.path.remove(ROOT)
    An = _problem()[0]
    np.save(os.path.join(str(tmp_path), "gaps.npy"), An)
    base = ["--p_r", "1", "--p_c", "1", "--fpath", str(tmp_path) + "/", "--fname", "gaps", "--k", "3", "--itr", "5", "--norm", "fro"]
    ap = cli.build_parser()
    assert "nan" in ap.format_help() and "unstored" in ap.format_help()
    for ftype in ("npy", "mat", "csv", "txt", "folder"):
        args = ap.parse_args(base + ["--ftype", ftype, "--missing", "nan"])
        cli.check_missing_flag(args)                                                 # accepted
        assert args.missing == "nan"
    cli.check_missing_flag(ap.parse_args(base + ["--ftype", "spnpz", "--missing", "unstored"]))
    cli.check_missing_flag(ap.parse_args(base + ["--ftype", "npy"]))
    with pytest.raises(SystemExit, match="missing"):
        cli.check_missing_flag(ap.parse_args(base + ["--ftype", "npy", "--missing", "zero"]))
    with pytest.raises(SystemExit, match="missing nan.*pyDNMF"):
        cli.check_missing_flag(ap.parse_args(base + ["--ftype", "npy", "--missing", "nan", "--process", "pyDNMFk"]))
    # the file as main.py reads it, through PyNMF on the oracle operator set
    from pydnmfk_amd.data_io import data_read
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMF import PyNMF
    args = ap.parse_args(base + ["--ftype", "npy", "--missing", "nan"])
    comms = MPI_comm(None, 1, 1)
    args.size, args.rank, args.comm1, args.comm = comms.size, comms.rank, comms.comm, comms
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    A_ij = data_read(args).read()
    assert np.array_equal(np.isnan(A_ij), np.isnan(An))
    args.rng, args.results_paths = "numpy", str(tmp_path) + "/"
    np.random.seed(3)
    W, H, err = PyNMF(A_ij, params=args, ops=D.MaskedDenseOracleOps()).fit()
    assert W.shape == (24, 3) and H.shape == (3, 12) and np.isfinite(err) and 0 < err < 1
    # the whole program: the refusal comes from the flags alone, before a device is touched
    res = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + base + ["--ftype", "spnpz", "--missing", "nan"],
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert res.returncode != 0 and "--missing nan" in res.stderr and "spnpz" in res.stderr, res.stderr[-2000:]


# ---- 4. the exact operands of the GPU test stay exact under a mask (float64 proof)
def _exact_case(shape):
    """(ranks, problem builder) of a shape of EXACT_SHAPES or EXACT_LOOP_SHAPES"""
    if shape in D.EXACT_SHAPES:
        return D.EXACT_KS, D.exact_problem
    return D.loop_case(shape)["ks"], D.loop_problem


@pytest.mark.parametrize("shape", D.EXACT_SHAPES + D.EXACT_LOOP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_masked_exact_operands_are_integers_below_2_24(shape):
    """all terms are non-negative, so a masked sum is at most the unmasked sum the generator already bounds -- asserted here, not
    assumed: every masked `fro` numerator and denominator (and the `kl` denominators) is an integer below 2^24, hence exact in float32
    in any summation order.  The shapes of EXACT_LOOP_CASES (more tiles per split, more row blocks per chunk: longer partial sums in
    one accumulator) and the 0 / 1 generator of the tall one included."""
    m, n = shape
    ks, problem = _exact_case(shape)
    for k in ks:
        A, mask, W, H, ref = problem(m, n, k)
        assert (A >= 0).all() and (W >= 0).all() and (H >= 0).all()
        assert 0.4 < mask.mean() < 0.6
        assert (ref["row_obs"] == 0).any() and (ref["col_obs"] == 0).any() and (ref["row_obs"] == 1).sum() >= 3 and (ref["col_obs"] == 1).sum() >= 1
        for got, full, what in zip(ref["fro"] + ref["kl"][1::2], ref["unmasked_fro"] + (None, None),
                                   ("num_w", "den_w", "num_h", "den_h", "klden_w", "klden_h")):
            assert np.array_equal(got, np.round(got)) and got.min() >= 0, (shape, k, what)
            assert got.max() < 2.0 ** 24, (shape, k, what, got.max())
            if full is not None:
                assert (got <= full).all() and full.max() < 2.0 ** 24, (shape, k, what)
            assert np.array_equal(got.astype(np.float32).astype(np.float64), got), (shape, k, what)
        # every model value <W_r, H_c> is an integer of at most 9 k: the first product is exact as well
        Dm = W.astype(np.float64) @ H.astype(np.float64)
        assert np.array_equal(Dm, np.round(Dm)) and Dm.max() <= 9 * k
        if problem is D.loop_problem and D.loop_case(shape)["gen"] == "01":
            assert set(np.unique(W)) <= {0.0, 1.0} and set(np.unique(H)) <= {0.0, 1.0} and 1 <= Dm.min() and Dm.max() <= k
        print("exact operands %dx%d k=%d: largest unmasked sum %d, largest masked sum %d" % (m, n, k, max(x.max() for x in ref["unmasked_fro"]),
                                                                                         max(x.max() for x in ref["fro"])))


@pytest.mark.parametrize("case", D.EXACT_LOOP_CASES, ids=lambda c: "%dx%d" % c["shape"])
def test_exact_residual_block_has_exact_per_lane_partials(case):
    """The block W H + r, r in {0, 1, 2}, NaN where not observed: its entries are integers below 2^24 (exact in float32), the model
    value the kernel forms is the same integer (the proof above), so every difference is exactly r and every squared difference at
    most 4.  A lane of masked_resid_kernel adds 64 of them in float32 (16 rows x 4 columns of its tile): at most 256, far below
    2^24, whatever the order.  From there on the sums are float64: the total, an integer of at most 4 m n, is below 2^53.  The sum of
    squares of the data block itself (`sqnorm`) is an integer of at most 49 m n in float64 throughout."""
    m, n = case["shape"]
    for k in case["ks"]:
        A, mask, W, H, _ = D.loop_problem(m, n, k)
        blk, r = D.exact_resid_block(A, mask, W, H)
        assert set(np.unique(r)) == {0, 1, 2} and np.array_equal(np.isnan(blk), ~mask)
        Dm = W.astype(np.float64) @ H.astype(np.float64)
        assert np.array_equal(blk[mask].astype(np.float64), (Dm + r)[mask]) and (Dm + r).max() < 2.0 ** 24      # stored without rounding
        d2 = (blk[mask].astype(np.float64) - Dm[mask]) ** 2
        assert d2.max() <= 4 and 64 * d2.max() < 2.0 ** 24
        assert float(d2.sum()) == float((mask * r ** 2).sum()) <= 4.0 * m * n < 2.0 ** 53
        assert 49.0 * m * n < 2.0 ** 53 and float((A.astype(np.float64) ** 2)[mask].sum()) == float(np.sum((mask * A.astype(np.int64) ** 2)))
