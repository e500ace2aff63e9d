"""Dense data whose missing entries are NaN (`params.missing = 'nan'`) on the GPU (csrc/dnmf_masked.h through engine.HipMaskedOps):
the masked MFMA passes against float64 and against the CSR masked kernels, exact operands element by element on padded views,
single steps along a float64 trajectory, the reference's goldens on blocks without a NaN, 1D grids, recovery of held-out entries,
bit-reproducibility."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

from tests import _exact as E  # noqa: E402
from tests import _masked as M  # noqa: E402
from tests import _masked_dense as D  # noqa: E402
from tests._golden import rel_fro  # noqa: E402

EPS = M.EPS
KS = (1, 3, 16, 17, 32, 33, 64, 100, 128)


def _ops():
    from pydnmfk_amd.engine import HIP_MASKED_OPS
    return HIP_MASKED_OPS


def _block(An):
    from pydnmfk_amd.masked import MaskedDenseBlock
    return MaskedDenseBlock(torch.from_numpy(np.ascontiguousarray(An)).cuda())


def _args(k, itr, norm, W_update=True, missing="nan"):
    from pydnmfk_amd.dist_comm import MPI_comm
    return D.args_for(MPI_comm(None, 1, 1), 1, 1, k, itr, norm, W_update, missing=missing)


# ---- 1. the kernels against float64 (and 2. against the CSR masked kernels on the same observations)
def _check_kernels(tag, A, mask, blk, csr, W, H, worst):
    from pydnmfk_amd.engine import HIP_CSR_OPS
    from tests.test_gpu_masked import _pairs64, _rel, _ulp_apart
    ops = _ops()
    m, n = A.shape
    k = W.shape[1]
    ref, ref_r = _pairs64(A, mask, W, H)
    Wd, Hd = torch.from_numpy(W).cuda(), torch.from_numpy(H).cuda()
    empty_rows, empty_cols = mask.sum(1) == 0, mask.sum(0) == 0
    for norm, bound in (("fro", 2e-6), ("kl", 1e-5)):
        bw, bh = torch.full((2 * m * k,), np.nan, device="cuda"), torch.full((2 * k * n,), np.nan, device="cuda")
        nw, dw = ops.masked_aht_pair(blk, Wd, Hd, EPS, norm, bw)
        nh, dh = ops.masked_wta_pair(blk, Wd, Hd, EPS, norm, bh)
        assert nw.data_ptr() == bw.data_ptr() and dw.data_ptr() == bw.data_ptr() + 4 * m * k          # ONE contiguous [num | den]
        assert nh.data_ptr() == bh.data_ptr() and dh.data_ptr() == bh.data_ptr() + 4 * k * n
        got = [t.cpu().numpy() for t in (nw, dw, nh, dh)]
        d = [_rel(g, r) for g, r in zip(got, ref[norm])]
        print("masked dense %-20s %s k=%3d obs=%6d  W: num %.2e den %.2e | H: num %.2e den %.2e" % (tag, norm, k, blk.n_observed, *d))
        worst[norm] = max(worst.get(norm, 0.0), *d)
        for g in got:
            assert np.isfinite(g).all(), (tag, norm)                  # every output element was written, no NaN came through
        for g in got[:2]:
            assert not g[empty_rows].any(), (tag, norm)               # exact zeros, not small values
        for g in got[2:]:
            assert not g[:, empty_cols].any(), (tag, norm)
        assert max(d) <= bound, (tag, norm, k, d)
        # two independent kernels, one answer: the CSR masked passes on the same observations, within the sum of the two bounds
        cw, ch = torch.full((2 * m * k,), np.nan, device="cuda"), torch.full((2 * k * n,), np.nan, device="cuda")
        c = [t.cpu().numpy() for t in HIP_CSR_OPS.masked_aht_pair(csr, Wd, Hd, EPS, norm, cw) + HIP_CSR_OPS.masked_wta_pair(csr, Wd, Hd, EPS, norm, ch)]
        dc = [_rel(g, x.astype(np.float64)) for g, x in zip(got, c)]
        worst[norm + "/csr"] = max(worst.get(norm + "/csr", 0.0), *dc)
        assert max(dc) <= 2 * bound, (tag, norm, k, "against CSR", dc)
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
    worst["resid"] = max(worst.get("resid", 0.0), dr)
    assert dr <= 1e-5, (tag, k, r, ref_r)
    sq = float(ops.sqnorm(blk).cpu())
    sq_ref = float(np.sum((A.astype(np.float64) ** 2)[mask]))
    assert abs(sq - sq_ref) <= 1e-12 * max(sq_ref, 1.0) and blk._sqnorm is not None, (tag, sq, sq_ref)
    assert float(blk._sqnorm[1].cpu()) == blk.n_observed                             # the kernel's own count of observed entries


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (129, 33), (300, 257)], ids=lambda s: "%dx%d" % s)
def test_masked_dense_kernels_against_float64_and_csr(shape):
    """the smallest shapes that cross one 128-row slab, one 32-column tile and each KP boundary (k = 32 | 33, 64 | 100); all-missing
    (density 0) and all-observed (1.0) blocks included"""
    from pydnmfk_amd.sparse import SparseBlock
    from tests.test_gpu_masked import _observed_block
    rs = np.random.RandomState(700 + shape[0])
    m, n = shape
    worst = {}
    for density in (0.0, 0.05, 0.5, 1.0):
        A, mask = _observed_block(rs, m, n, density)
        blk = _block(D.nan_marked(A, mask))
        csr = SparseBlock.from_any(M.observed(A, mask), torch.device("cuda", 0), keep_zeros=True, missing="unstored")
        assert blk.n_observed == int(mask.sum()) == csr.nnz
        for k in KS:
            W, H = (rs.rand(m, k) + 0.01).astype(np.float32), (rs.rand(k, n) + 0.01).astype(np.float32)
            _check_kernels("%dx%d d=%g" % (m, n, density), A, mask, blk, csr, W, H, worst)
    print("masked dense %dx%d maxima:" % shape, {k_: "%.2e" % v for k_, v in sorted(worst.items())})


# ---- 3. exact operands, element by element, on padded views
def _pairs_on_views(blk, Wp, Hp, k, norm, aligned=True):
    """both pairs of one objective into poisoned, pitched output views: (num_w, den_w, num_h, den_h) as numpy, after the check that
    nothing outside a view was written and no NaN came through"""
    ops = _ops()
    m, n = blk.shape
    out = []
    for side, (r, c) in (("w", (m, k)), ("h", (k, n))):
        num, den = E.Poisoned.out(torch, r, c, torch.float32, aligned=aligned), E.Poisoned.out(torch, r, c, torch.float32, aligned=aligned)
        assert num.ld == den.ld > c
        ops.masked_pair_into(side, blk, Wp.view, Hp.view, EPS, norm, num.view, den.view)
        out += [num.check("%s %s num k=%d" % (norm, side, k)), den.check("%s %s den k=%d" % (norm, side, k))]   # nothing outside, no NaN
    return tuple(out)


def _exact_pair_checks(A, mask, W, H, ref, aligned=True):
    """the checks of test_masked_dense_exact_operands on one problem; returns the views, the block and {norm: the four arrays}.
    aligned=False: every view starts at an odd element and has an odd pitch (tests/_exact.py::Poisoned)"""
    from pydnmfk_amd.masked import MaskedDenseBlock
    m, n = A.shape
    k = W.shape[1]
    Ap = E.Poisoned(torch, D.nan_marked(A, mask), aligned=aligned)
    Wp, Hp = E.Poisoned(torch, W, aligned=aligned), E.Poisoned(torch, H, aligned=aligned)
    assert Ap.ld > n and Wp.ld > k and Hp.ld > n and not Ap.view.is_contiguous()
    blk = MaskedDenseBlock(Ap.view)
    got = {}
    for norm in ("fro", "kl"):
        nw, dw, nh, dh = got[norm] = _pairs_on_views(blk, Wp, Hp, k, norm, aligned)
        rnw, rdw, rnh, rdh = ref[norm]
        E.assert_ulp(dw, rdw, 0, "%s den_w k=%d" % (norm, k))
        E.assert_ulp(dh, rdh, 0, "%s den_h k=%d" % (norm, k))
        if norm == "fro":
            E.assert_ulp(nw, rnw, 0, "fro num_w k=%d" % k)
            E.assert_ulp(nh, rnh, 0, "fro num_h k=%d" % k)
        else:
            one_r, one_c = ref["row_obs"] == 1, ref["col_obs"] == 1
            assert one_r.sum() >= 3 and one_c.sum() >= 1
            E.assert_ulp(nw[one_r], rnw[one_r], 5, "kl num_w (single-observation rows) k=%d" % k)
            E.assert_ulp(nh[:, one_c], rnh[:, one_c], 5, "kl num_h (single-observation columns) k=%d" % k)
            for g, r_ in ((nw, rnw), (nh, rnh)):                                    # the rest: test 1's bound
                assert np.linalg.norm(g - r_) <= 1e-5 * np.linalg.norm(r_), (norm, k)
        assert not nw[ref["row_obs"] == 0].any() and not dw[ref["row_obs"] == 0].any()
        assert not nh[:, ref["col_obs"] == 0].any() and not dh[:, ref["col_obs"] == 0].any()
    _operands_not_written(Ap, Wp, Hp)
    return Ap, Wp, Hp, blk, got


def _operands_not_written(Ap, Wp, Hp):
    for p_, what in ((Ap, "A"), (Wp, "W"), (Hp, "H")):
        b = p_.buf.cpu().numpy()
        assert np.isnan(b[~p_.mask]).all(), what


@pytest.mark.parametrize("shape", D.EXACT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_masked_dense_exact_operands(shape):
    """tests/_exact.py::products under a 50 % mask written as NaN (tests/test_masked_dense_cpu.py proves every masked sum an integer
    below 2^24): the `fro` pairs and the `kl` denominators bit for bit, whatever the split, chunk and tile order.  W, H and the outputs
    sit in poisoned buffers (NaN around the operands, pitch larger than the width), A is a strided view with NaN around it as well.
    The `kl` numerators are held per element where the row (column) has ONE observation: the sum is then the single term
    a * rcp(s + eps) * f.  v_rcp_f32 is within 1 ulp (relative error at most 2^-23); the sum s + eps, the product with a and the
    MFMA's multiply-add round once each (2^-24 each): at most 5 * 2^-24 relative in all, and one ulp of the result is at least 2^-24
    of it -- hence 5 ulp.  Elsewhere the numerators fall under test 1's bound.  (132, 96) adds the 16-byte vector paths on padded
    views to the issue's two shapes, whose widths are no multiple of 4.)"""
    m, n = shape
    for k in D.EXACT_KS:
        _exact_pair_checks(*D.exact_problem(m, n, k))


# ---- 3b. the same where a workgroup walks several tiles, a wave several row blocks, the reduce a second trip
def _takes_vector_kernels(Ap, Wp, Hp, k):
    """the library's own condition for its FAST kernels (csrc/dnmf_masked.hip::masked_fast), on the views handed over"""
    n = Ap.cols
    return all(p_.view.data_ptr() % 16 == 0 and p_.ld % 4 == 0 for p_ in (Ap, Wp, Hp)) and n % 4 == 0 and k % 4 == 0


def _assert_within_an_ulp(got, exp, what):
    from tests.test_gpu_masked import _ulp_apart
    ok = _ulp_apart(got, exp)
    if not ok.all():
        idx = tuple(int(i) for i in np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d elements more than an ulp from x * (num / (den + eps)); first at %s: got %r, expected %r"
                             % (what, int((~ok).sum()), ok.size, idx, got[idx].item(), exp[idx].item()))


@pytest.mark.parametrize("shape", D.EXACT_LOOP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_masked_dense_exact_operands_in_the_loops(shape):
    """The checks of test_masked_dense_exact_operands at the shapes of tests/_masked_dense.py::EXACT_LOOP_CASES -- the smallest at
    which dnmf_masked_plan (asserted in tests/test_capi_masked.py) gives a workgroup of masked_uht_kernel three tiles (both LDS
    buffers, the prefetch, a ragged last tile that is not the first), a wave of masked_wtu_kernel two row blocks (and the last chunk
    one), and masked_reduce_kernel a second grid-stride trip -- generic and 16-byte vector kernels.  Then each pair form once more on
    the same inputs: bit-identical (partials are added in a fixed order, no float atomics)."""
    case = D.loop_case(shape)
    m, n = shape
    for k in case["ks"]:
        A, mask, W, H, ref = D.loop_problem(m, n, k)
        Ap, Wp, Hp, blk, got = _exact_pair_checks(A, mask, W, H, ref)
        assert _takes_vector_kernels(Ap, Wp, Hp, k) == (case["fast"] and k % 4 == 0), (shape, k)
        for norm in ("fro", "kl"):
            again = _pairs_on_views(blk, Wp, Hp, k, norm)
            for a, b, what in zip(got[norm], again, ("num_w", "den_w", "num_h", "den_h")):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (shape, k, norm, what, "second call differs")


@pytest.mark.parametrize("shape", [(70, 2085), (2130, 70)], ids=lambda s: "%dx%d" % s)
def test_masked_dense_exact_operands_in_the_loops_at_odd_base_and_pitch(shape):
    """The tile loop (70 x 2085) and the row-block loop (2130 x 70) once more with every operand and output view starting three
    elements into its buffer at a pitch of its width + 3: no view is 16-byte aligned and rows fall at every 4-byte offset, at any
    rank -- the per-element loads and stores of the generic kernels inside the loops, whatever k.  The same checks, the same bounds."""
    case = D.loop_case(shape)
    m, n = shape
    for k in case["ks"]:
        A, mask, W, H, ref = D.loop_problem(m, n, k)
        Ap, Wp, Hp, _, _ = _exact_pair_checks(A, mask, W, H, ref, aligned=False)
        assert all(p_.view.data_ptr() % 16 and p_.ld == p_.cols + 3 for p_ in (Ap, Wp, Hp)) and not _takes_vector_kernels(Ap, Wp, Hp, k)


@pytest.mark.parametrize("shape", D.EXACT_LOOP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_masked_dense_fused_endings_on_padded_views_in_the_loops(shape):
    """masked_update_w, masked_update_h (clamp off and on) at the same shapes with the updated factor, the other factor and A all
    poisoned, pitched views: each result within an ulp of x * (num / (den + eps)) evaluated in float32 from the pair the pair-writing
    ending just wrote on the same views (the helper and bound of tests/test_gpu_masked.py, as test 1 has them on contiguous tensors);
    nothing outside the view changes, no NaN comes through."""
    from pydnmfk_amd.masked import MaskedDenseBlock
    ops = _ops()
    case = D.loop_case(shape)
    m, n = shape
    e = np.float32(EPS)
    for k in case["ks"]:
        A, mask, W, H, _ = D.loop_problem(m, n, k)
        Ap, Wp, Hp = E.Poisoned(torch, D.nan_marked(A, mask)), E.Poisoned(torch, W), E.Poisoned(torch, H)
        blk = MaskedDenseBlock(Ap.view)
        for norm in ("fro", "kl"):
            nw, dw, nh, dh = _pairs_on_views(blk, Wp, Hp, k, norm)
            expW, expH = W * (nw / (dw + e)), H * (nh / (dh + e))
            W1, H1, H2 = E.Poisoned(torch, W), E.Poisoned(torch, H), E.Poisoned(torch, H)
            ops.masked_update_w(blk, W1.view, Hp.view, EPS, norm)
            ops.masked_update_h(blk, Wp.view, H1.view, EPS, norm)
            ops.masked_update_h(blk, Wp.view, H2.view, EPS, norm, clamp=True)
            tag = "%dx%d %s k=%d " % (m, n, norm, k)
            _assert_within_an_ulp(W1.check(tag + "fused W"), expW, tag + "fused W")
            _assert_within_an_ulp(H1.check(tag + "fused H"), expH, tag + "fused H")
            _assert_within_an_ulp(H2.check(tag + "fused H, clamped"), np.maximum(expH, e), tag + "fused H, clamped")
        _operands_not_written(Ap, Wp, Hp)


@pytest.mark.parametrize("shape", D.EXACT_LOOP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_masked_dense_exact_residual_in_the_loops(shape):
    """The block W H + r, r in {0, 1, 2} at the observed positions (tests/test_masked_dense_cpu.py proves the per-lane float32
    partials exact): the masked residual equals sum(mask * r^2) as a float64, on poisoned views.  The sum of squares of the exact
    problem's own block equals the integer sum, and the kernel's count of observed entries the mask's."""
    from pydnmfk_amd.masked import MaskedDenseBlock
    ops = _ops()
    case = D.loop_case(shape)
    m, n = shape
    for k in case["ks"]:
        A, mask, W, H, _ = D.loop_problem(m, n, k)
        Rn, r = D.exact_resid_block(A, mask, W, H)
        Rp, Wp, Hp = E.Poisoned(torch, Rn), E.Poisoned(torch, W), E.Poisoned(torch, H)
        got = float(ops.resid_sqnorm(MaskedDenseBlock(Rp.view), Wp.view, Hp.view).cpu())
        want = float((mask * r ** 2).sum())
        assert got == want, (shape, k, got, want)
        _operands_not_written(Rp, Wp, Hp)
    A, mask, _, _, _ = D.loop_problem(m, n, case["ks"][-1])
    Ap = E.Poisoned(torch, D.nan_marked(A, mask))
    blk = MaskedDenseBlock(Ap.view)
    sq = float(ops.sqnorm(blk).cpu())
    assert sq == float((A.astype(np.int64) ** 2)[mask].sum()), (shape, sq)
    assert float(blk._sqnorm[1].cpu()) == float(mask.sum()) == blk.n_observed
    assert np.isnan(Ap.buf.cpu().numpy()[~Ap.mask]).all()


# ---- 4. single steps along a float64 trajectory, through PyNMF
def _traj_problem():
    rs = np.random.RandomState(101)
    m, n, k = 300, 200, 32
    A = (rs.rand(m, n) + 0.05).astype(np.float32)
    mask = rs.rand(m, n) < 0.5
    W0, H0 = rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)
    return A, mask, W0, H0, k


@pytest.mark.parametrize("norm", ["fro", "kl"])
def test_masked_dense_steps_along_a_float64_trajectory(norm):
    """From the helper's float64 states after t = 0, 5, 19 steps (cast to float32): ONE masked step on the GPU against the helper's
    float64 step; bound max(tol_step, 2 d_ref), d_ref = distance of the helper's float32 step from its float64 step."""
    from pydnmfk_amd.pyDNMF import PyNMF
    from tests.test_gpu_parity import _tols
    A, mask, W0, H0, k = _traj_problem()
    tol_step = _tols({"method": "mu"})[0]
    An = D.nan_marked(A, mask)
    csr = D.coo_of_dense(An)
    for t in (0, 5, 19):
        Wt, Ht = M.iterate(csr, A.shape, W0.astype(np.float64), H0.astype(np.float64), t, norm)
        Wt, Ht = Wt.astype(np.float32), Ht.astype(np.float32)
        W64, H64, _ = M.fit(csr, A.shape, Wt, Ht, 1, norm, dtype=np.float64)
        W32, H32, _ = M.fit(csr, A.shape, Wt, Ht, 1, norm, dtype=np.float32)
        nmf = PyNMF(An, factors=[Wt, Ht], params=_args(k, 1, norm))
        assert nmf.A_ij.missing == "nan" and nmf._ops().name == "hip-masked"
        Wg, Hg, _ = nmf.fit()
        for nm, g, r32, r64 in (("W", Wg, W32, W64), ("H", Hg, H32, H64)):
            d_ref, d_gpu = rel_fro(r32, r64), rel_fro(g, r64)
            print("masked dense trajectory %s t=%2d %s: d_ref=%.2e gpu=%.2e bound=%.2e" % (norm, t, nm, d_ref, d_gpu, max(tol_step, 2 * d_ref)))
            assert d_gpu <= max(tol_step, 2 * d_ref), (norm, t, nm, d_gpu, d_ref)


# ---- 5. a block without a NaN is the reference
@pytest.mark.parametrize("name", M.FULL_GOLDENS)
def test_block_without_a_nan_meets_the_reference_golden_on_the_gpu(name):
    from tests._sparse import judge_with_run_case
    out = D.full_case(name, None)
    print("masked dense full %s (gpu):" % name, {k_: tuple("%.2e" % v for v in vals) for k_, vals in out.items()})
    judge_with_run_case(name, [(0, out, None)])


# ---- 6. 1D grids, two processes on the one GPU
@pytest.fixture(scope="module")
def one_rank_gpu_fits():
    return D.run_grid((1, 1), use_hip=True)


@pytest.mark.parametrize("grid", [(2, 1), (1, 2)], ids=lambda g: "%dx%d" % g)
def test_masked_dense_grids_match_the_one_rank_gpu_fit(grid, one_rank_gpu_fits):
    got = D.run_grid(grid, use_hip=True, timeout=300)
    for combo, (Wr, Hr, err_r) in one_rank_gpu_fits.items():                          # W_update on and off, fro and kl
        W, H, err = got[combo]
        dw, dh, de = rel_fro(W, Wr), rel_fro(H, Hr), abs(err - err_r) / err_r
        print("masked dense gpu grid %dx%d %s W_update=%s: dW=%.2e dH=%.2e derr=%.2e" % (grid + combo + (dw, dh, de)))
        assert dw <= 1e-5 and dh <= 1e-5 and de <= 1e-5, (grid, combo, dw, dh, de)


def test_one_rank_gpu_fit_matches_the_float64_fit(one_rank_gpu_fits):
    for combo, (Wr, Hr, err_r) in M.reference_fits().items():
        W, H, err = one_rank_gpu_fits[combo]
        dw, dh, de = rel_fro(W, Wr), rel_fro(H, Hr), abs(err - err_r) / err_r
        print("masked dense gpu 1x1 %s W_update=%s against float64: dW=%.2e dH=%.2e derr=%.2e" % (combo + (dw, dh, de)))
        assert dw <= 1e-4 and dh <= 1e-4 and de <= 1e-5, (combo, dw, dh, de)


# ---- 7. recovery of held-out entries
def test_recovery_of_held_out_entries_from_nan_marked_data():
    """planted rank 4, 300 x 200, 30 % observed, 200 MU/FRO iterations: the NaN-marked fit predicts the entries it never saw, the
    zero-filled dense fit of the same observations does not"""
    from pydnmfk_amd.pyDNMF import PyNMF
    rs = np.random.RandomState(4)
    m, n, k = 300, 200, 4
    A = (rs.rand(m, k) @ rs.rand(k, n)).astype(np.float32)
    mask = rs.rand(m, n) < 0.3
    W0, H0 = rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)
    An = D.nan_marked(A, mask)
    held = ~mask

    def held_out(W, H):
        R = (A.astype(np.float64) - np.asarray(W, dtype=np.float64) @ np.asarray(H, dtype=np.float64))[held]
        return float(np.linalg.norm(R) / np.linalg.norm(A.astype(np.float64)[held]))

    Wr, Hr, _ = M.fit(D.coo_of_dense(An), A.shape, W0, H0, 200, "fro")
    Wg, Hg, _ = PyNMF(An, factors=[W0, H0], params=_args(k, 200, "fro")).fit()
    Wz, Hz, _ = PyNMF(np.where(mask, A, 0).astype(np.float32), factors=[W0, H0], params=_args(k, 200, "fro", missing=None)).fit()
    e_ref, e_gpu, e_zero = held_out(Wr, Hr), held_out(Wg, Hg), held_out(Wz, Hz)
    print("recovery (dense, NaN-marked): held-out error float64 helper %.3e, gpu masked %.3e, gpu zero-filled %.3e" % (e_ref, e_gpu, e_zero))
    assert e_gpu <= 2 * e_ref and e_gpu <= 0.05
    assert e_zero >= 0.5


# ---- 8. bit-reproducible
def test_masked_dense_bit_reproducible():
    """300 x 257 at 50 % observed, k = 33, 30 steps (fro and kl), twice in this process: W and H identical bit for bit -- the products
    add their partials in a fixed order and use no float atomics"""
    from pydnmfk_amd.pyDNMF import PyNMF
    rs = np.random.RandomState(8)
    m, n, k = 300, 257, 33
    A = (rs.rand(m, n) + 0.05).astype(np.float32)
    An = D.nan_marked(A, rs.rand(m, n) < 0.5)
    W0, H0 = rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)
    for norm in ("fro", "kl"):
        runs = [PyNMF(An, factors=[W0, H0], params=_args(k, 30, norm)).fit() for _ in range(2)]
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), norm
        assert np.isfinite(runs[0][0]).all() and np.isfinite(runs[0][1]).all()
