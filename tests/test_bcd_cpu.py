"""method='bcd' (accelerated block coordinate descent, Frobenius): the choreography of nmf_algorithms_{1D,2D}.FRO_BCD_update and
PyNMF.fit run under gloo on every BCD fixture's grid against the reference's outputs (tests/golden/bcd_*.npz).  The arithmetic is
the numpy checker of tests/_bcd.py -- these tests pin the sequencing, the exchanges and the restart logic, not the HIP kernels
(tests/test_gpu_bcd.py)."""
import numpy as np
import pytest
import torch

from tests._bcd import BcdOracleOps, bcd_case_names, check_tolerances, run_bcd


@pytest.mark.parametrize("name", bcd_case_names())
def test_bcd_choreography_matches_reference(name):
    check_tolerances(name, run_bcd(name, use_hip=False))


def test_bcd_fixtures_cover_the_grids():
    names = bcd_case_names()
    for want in ("t24x12_1x1", "t24x12_1x2", "t24x12_2x1", "t24x12_2x2", "r25x13_3x1", "swim_1x1", "lr200x136k64_1x1",
                 "lr200x136k64_1x2", "lr150x140k128_1x1"):
        assert want in names


def _one_rank_params(itr, method="bcd", norm="fro"):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.utils import parse
    comms = MPI_comm(None, 1, 1)
    args = parse()
    args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, 1, 1, 2
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    args.itr, args.init, args.verbose, args.prune, args.norm, args.method = itr, "rand", False, False, norm, method
    return args


def test_bcd_restart_restores_the_last_accepted_pair():
    """A rejected iteration (objective not lower) restarts the extrapolation from W_old / H_old and puts back the products of H_old,
    while W, H keep the rejected iterate (dist_nmf.py:1026-1031): forced here with an objective that can never decrease."""
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF

    class NeverLower(BcdOracleOps):
        def resid_sqnorm(self, A, W, H):
            return torch.tensor([float("inf")], dtype=torch.float64)

    rs = np.random.RandomState(3)
    A = (rs.rand(12, 2) @ rs.rand(2, 9)).astype(np.float32)
    W0, H0 = rs.rand(12, 2).astype(np.float32), rs.rand(2, 9).astype(np.float32)
    ops = NeverLower()
    nmf = PyNMF(A, factors=[W0, H0], params=_one_rank_params(3), ops=ops)
    alg = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=ops)
    W, H = alg.update()
    st = alg._bcd_st.numpy()
    assert st[9] == 0 and st[4] == 1.0                        # the last decision was a restart; t_old never advanced
    # every iteration restarted from the same (W_old, H_old, A H_old^T, H_old H_old^T): the three iterates are equal
    nmf1 = PyNMF(A, factors=[W0, H0], params=_one_rank_params(1), ops=ops)
    W1, H1 = nmf_algorithms_1D(nmf1.A_ij, nmf1.W_i, nmf1.H_j, params=nmf1.params, ops=ops).update()
    np.testing.assert_array_equal(W.numpy(), W1.numpy())
    np.testing.assert_array_equal(H.numpy(), H1.numpy())


def test_bcd_kl_is_refused_with_the_reference_message():
    from pydnmfk_amd.pyDNMF import PyNMF
    rs = np.random.RandomState(0)
    A = rs.rand(8, 6).astype(np.float32)
    with pytest.raises(Exception, match="Choose \\(mu\\)"):
        PyNMF(A, factors=[rs.rand(8, 2), rs.rand(2, 6)], params=_one_rank_params(2, norm="kl"), ops=BcdOracleOps()).fit()


def test_bcd_refuses_float64_operator_sets():
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    from pydnmfk_amd.pyDNMF import PyNMF
    rs = np.random.RandomState(0)
    A = rs.rand(8, 6)
    nmf = PyNMF(A, factors=[rs.rand(8, 2), rs.rand(2, 6)], params=_one_rank_params(2), ops=BcdOracleOps())
    assert nmf.A_ij.dtype == torch.float64
    with pytest.raises(NotImplementedError, match="bcd"):
        nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update()
