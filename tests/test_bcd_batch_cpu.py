"""Batched method='bcd' fits, the part that needs no GPU: the workspace query of a batch, the argument checks of
dnmf_bcd_fro_fit with batch > 1 (before any HIP call) and the routing of PyNMF.fit_batch (same-shape BCD fits become ONE whole-fit
call on stacks; anything else stays one fit after another).  The kernels: tests/test_gpu_bcd_batch.py."""
import numpy as np
import pytest
import torch


@pytest.mark.parametrize("m,n", [(131, 203), (1024, 256), (2049, 515)])
def test_batch_workspace_is_batch_slices(m, n):
    from pydnmfk_amd._lib import lib
    for k in (1, 17, 33, 65, 129, 256):                     # across the dnmf_kp boundaries
        one = lib.dnmf_bcd_ws_bytes(m, n, k)
        assert one > 0 and one % 16 == 0                     # (a slice is a stride of the workspace family: 16-byte multiples)
        assert lib.dnmf_bcd_ws_bytes_fit(m, n, k, 1) == one
        for B in (2, 5, 20):
            assert lib.dnmf_bcd_ws_bytes_fit(m, n, k, B) == B * one
    assert lib.dnmf_bcd_ws_bytes_fit(m, n, 4, 0) == 0 and lib.dnmf_bcd_ws_bytes_fit(m, n, 4, -3) == 0
    assert lib.dnmf_bcd_ws_bytes_fit(0, n, 4, 2) == 0 and lib.dnmf_bcd_ws_bytes_fit(m, 0, 4, 2) == 0
    assert lib.dnmf_bcd_ws_bytes_fit(m, n, 257, 2) == 0 and lib.dnmf_bcd_ws_bytes_fit(m, n, 0, 2) == 0


def test_batched_fit_arguments_are_checked_before_any_gpu_call():
    from pydnmfk_amd._lib import lib
    rc = lib.dnmf_bcd_fro_fit(None, 8, 8, 8, None, 4, None, 8, 4, 1e-7, 1, 3, 2, 64, 32, 32, None, None, 0, None)
    msg = lib.dnmf_last_error()
    assert rc == -1 and b"bcd_fro_fit" in msg
    assert b"not provided" not in msg and b"one by one" not in msg
    assert lib.dnmf_bcd_fro_fit(None, 8, 8, 8, None, 4, None, 8, 4, 1e-7, 1, 3, 0, 64, 32, 32, None, None, 0, None) == -1
    assert b"bcd_fro_fit" in lib.dnmf_last_error()


class _StubOps:
    """What PyNMF._whole_fit_ok asks of the product's operator set (name 'hip', a `fit` method), recording the whole-fit calls
    instead of running them: {sum (A - W H)^2, sum A^2} = {0, 1} (a zero denominator would divide by zero in relative_err), factors
    left as they are."""
    name = "hip"

    def __init__(self):
        self.calls = []

    def fit(self, method, norm, A, W, H, eps, w_update, itr, column_sweep=False):
        self.calls.append((method, norm, tuple(A.shape), tuple(W.shape), tuple(H.shape), int(itr)))
        sq = torch.zeros(A.shape[0] if A.dim() == 3 else 1, 2, dtype=torch.float64)
        sq[:, 1] = 1.0
        return sq


def _params(k, itr):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.utils import parse
    comms = MPI_comm(None, 1, 1)
    args = parse()
    args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, 1, 1, k
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    args.itr, args.init, args.verbose, args.prune, args.norm, args.method = itr, "rand", False, False, "fro", "bcd"
    return args


def _fits(ops, shapes, k=3, itr=7):
    from pydnmfk_amd.pyDNMF import PyNMF
    rs = np.random.RandomState(5)
    out = []
    for m, n in shapes:
        A = torch.from_numpy(rs.rand(m, n).astype(np.float32))
        f = [torch.from_numpy(rs.rand(m, k).astype(np.float32)), torch.from_numpy(rs.rand(k, n).astype(np.float32))]
        out.append(PyNMF(A, factors=f, params=_params(k, itr), ops=ops))
    return out


def test_fit_batch_sends_same_shape_bcd_fits_as_one_call():
    from pydnmfk_amd.pyDNMF import PyNMF
    ops = _StubOps()
    fits = _fits(ops, [(24, 12)] * 3)
    assert all(f._whole_fit_ok(ops) for f in fits)
    W0 = [f.W_i.clone() for f in fits]
    res = PyNMF.fit_batch(fits)
    assert ops.calls == [("bcd", "fro", (3, 24, 12), (3, 24, 3), (3, 3, 12), 7)]
    assert len(res) == 3 and fits[0]._stack.shape[0] == 3
    for b, (f, (W, H, err)) in enumerate(zip(fits, res)):
        assert f.A_ij.data_ptr() == fits[0]._stack[b].data_ptr()
        assert torch.equal(W, W0[b]) and err == 0.0          # (the stub leaves the factors: problem b came back as problem b)


def test_fit_batch_keeps_mixed_shapes_as_single_fits():
    from pydnmfk_amd.pyDNMF import PyNMF
    ops = _StubOps()
    fits = _fits(ops, [(24, 12), (24, 12), (20, 12)])
    res = PyNMF.fit_batch(fits)
    assert len(res) == 3 and len(ops.calls) == 3
    assert all(c[:2] == ("bcd", "fro") and len(c[2]) == 2 for c in ops.calls)          # matrices, no stack
    assert [c[2] for c in ops.calls] == [(24, 12), (24, 12), (20, 12)]
