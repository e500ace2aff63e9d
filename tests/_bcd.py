"""BCD test infrastructure (method='bcd', norm='fro'): the fixtures of tests/golden/make_golden_bcd.py, a checker back end for the
BCD primitives, and a multi-process runner (gloo) shared by tests/test_bcd_cpu.py and tests/test_gpu_bcd.py.

The fixtures are named bcd_<dataset>_<grid>.npz (not case_*: tests/_golden.case_names() and the suites that parametrize over it
know only MU / HALS), and hold per rank `step<N>` (one bare update() with params.itr = N) and `fit<N>` (PyNMF.fit with itr = N)."""
import glob
import json
import os
import traceback

import numpy as np
import torch

from tests._golden import GOLDEN, rel_fro
from tests._ops_double import OracleOps, _n


def bcd_case_names(grid=None):
    names = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "bcd_*.npz")))
    return [nm for nm in names if grid is None or nm.endswith("_%dx%d" % tuple(grid))]


def load_bcd(name):
    z = np.load(os.path.join(GOLDEN, "bcd_%s.npz" % name))
    meta = json.loads(str(z["meta"]))
    d = np.load(os.path.join(GOLDEN, "data_%s.npz" % meta["dataset"]))
    A = np.ascontiguousarray(d["A"].astype(np.float32))
    return meta, A, d["W0"].astype(np.float32), d["H0"].astype(np.float32), z


# slots of the device state block (csrc/dnmf_bcd.h BcdSlot)
XN, SW, SH, OBJ_OLD, T_OLD, LW, LW_OLD, LH, LH_OLD, ACC, WW, WH, OBJ, T = range(14)


class BcdOracleOps(OracleOps):
    """OracleOps plus the BCD primitives in numpy: products summed in float64 and rounded to float32, element-wise steps in float32
    as numpy evaluates the reference's expressions (dist_nmf.py:940-1047)."""
    name = "oracle-double"

    def bcd_state(self, like):
        return torch.zeros(16, dtype=torch.float64)

    def bcd_state_init(self, st, sq):
        s, q = st.numpy(), sq.numpy()
        s[:] = 0
        s[XN], s[SW], s[SH] = q[0], q[1], q[2]
        s[OBJ_OLD], s[T_OLD], s[LW], s[LH] = 0.5 * q[0], 1.0, 1.0, 1.0

    def bcd_init_factor(self, X0, Xold, Xm, st, which):
        s = st.numpy()
        a, b = np.float32(np.sqrt(s[SW + which])), np.float32(np.sqrt(np.sqrt(s[XN])))
        v = _n(X0) / a * b
        _n(Xold)[...] = v
        _n(Xm)[...] = v

    def bcd_lipschitz(self, G, k, st, which):
        s = st.numpy()
        slot = LW if which == 0 else LH
        s[slot + 1] = s[slot]
        s[slot] = float(np.float32(np.sqrt((_n(G)[:k, :k].astype(np.float64) ** 2).sum())))

    def bcd_update_w(self, Wm, AH, G, st, W, s):
        k = W.shape[1]
        L = np.float32(st.numpy()[LW])
        prod = (_n(Wm).astype(np.float64) @ _n(G)[:k, :k].astype(np.float64)).astype(np.float32)
        y = np.maximum(np.float32(0), _n(Wm) - (prod - _n(AH)) / L)
        _n(W)[...] = y
        _n(s)[:k] = y.astype(np.float64).sum(0).astype(np.float32)

    def bcd_scale_cols(self, W, s):
        w = _n(W)
        w /= _n(s)[None, : w.shape[1]]

    def bcd_update_h(self, Hm, AtW, G, st, H):
        k = H.shape[0]
        L = np.float32(st.numpy()[LH])
        prod = (_n(G)[:k, :k].astype(np.float64) @ _n(Hm).astype(np.float64)).astype(np.float32)
        _n(H)[...] = np.maximum(np.float32(0), _n(Hm) - (prod - _n(AtW)) / L)

    def bcd_decide(self, st, sq):
        s = st.numpy()
        obj = 0.5 * float(sq.numpy()[0])
        t_old = s[T_OLD]
        t = (1 + np.sqrt(1 + 4 * t_old * t_old)) / 2
        s[OBJ], s[T] = obj, t
        if obj >= s[OBJ_OLD]:
            s[ACC] = 0
            return
        w = (t_old - 1) / t
        s[ACC] = 1
        s[WW] = min(w, float(np.sqrt(np.float32(s[LW_OLD]) / np.float32(s[LW]))))
        s[WH] = min(w, float(np.sqrt(np.float32(s[LH_OLD]) / np.float32(s[LH]))))
        s[T_OLD], s[OBJ_OLD] = t, obj

    def bcd_extrapolate(self, W, Wold, Wm, H, Hold, Hm, AH, AHk, G, Gk, st):
        s = st.numpy()
        if s[ACC]:
            for x, o, p, slot in ((W, Wold, Wm, WW), (H, Hold, Hm, WH)):
                x_, o_ = _n(x), _n(o)
                _n(p)[...] = x_ + np.float32(s[slot]) * (x_ - o_)
                o_[...] = x_
            _n(AHk)[...] = _n(AH)
            _n(Gk)[...] = _n(G)
        else:
            _n(Wm)[...] = _n(Wold)
            _n(Hm)[...] = _n(Hold)
            _n(AH)[...] = _n(AHk)
            _n(G)[...] = _n(Gk)


def _params(comms, meta, itr, extra=None):
    from pydnmfk_amd.utils import parse
    args = parse()
    p_r, p_c = meta["grid"]
    args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, p_r, p_c, meta["k"]
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    args.itr, args.init, args.verbose, args.prune = itr, "rand", False, False
    args.norm, args.method, args.W_update = "fro", "bcd", True
    for key, val in (extra or {}).items():
        setattr(args, key, val)
    return args


def run_bcd_rank(rank, world, port, name, q, use_hip, extra=None):
    """Every step<N> and fit<N> of fixture `name` on this rank; puts {key: (rel W, rel H, |d err|)} on `q`."""
    try:
        import torch.distributed as dist
        from oracle import nmf_oracle as orc
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.dist_nmf import nmf_algorithms_1D, nmf_algorithms_2D
        from pydnmfk_amd.pyDNMF import PyNMF
        from pydnmfk_amd.utils import determine_block_params

        torch.set_num_threads(1)
        if use_hip:
            torch.cuda.set_device(0)
        ops = None if use_hip else BcdOracleOps()
        if world > 1:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        meta, A, W0, H0, z = load_bcd(name)
        p_r, p_c = meta["grid"]
        comms = MPI_comm(None, p_r, p_c)
        s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
        assert [s[0], e[0] + 1, s[1], e[1] + 1] == list(z["r%d_A_range" % rank])
        A_ij = A[s[0]:e[0] + 1, s[1]:e[1] + 1]
        (w0, w1), (h0, h1) = orc.factor_ranges(rank, p_r, p_c, meta["m"], meta["n"])
        out = {}
        for N in meta["steps"]:
            nmf = PyNMF(A_ij, factors=[W0[w0:w1], H0[:, h0:h1]], params=_params(comms, meta, N, extra), ops=ops)
            if nmf.topo == "2d":
                W1, H1 = nmf_algorithms_2D(nmf.A_ij, nmf.W_ij, nmf.H_ij, params=nmf.params, ops=nmf._ops()).update()
            else:
                W1, H1 = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update()
            out["step%d" % N] = (rel_fro(W1.cpu().numpy(), z["r%d_step%d_W" % (rank, N)]),
                                 rel_fro(H1.cpu().numpy(), z["r%d_step%d_H" % (rank, N)]), 0.0)
        for N in meta["itrs"]:
            W, H, err = PyNMF(A_ij, factors=[W0[w0:w1], H0[:, h0:h1]], params=_params(comms, meta, N, extra), ops=ops).fit()
            ref_W, ref_H = z["r%d_fit%d_W" % (rank, N)], z["r%d_fit%d_H" % (rank, N)]
            assert W.shape == ref_W.shape and H.shape == ref_H.shape
            assert W.dtype == ref_W.dtype and H.dtype == ref_H.dtype, (W.dtype, ref_W.dtype, H.dtype, ref_H.dtype)
            out["fit%d" % N] = (rel_fro(W, ref_W), rel_fro(H, ref_H), abs(err - float(z["r0_fit%d_err" % N])))
        q.put((rank, out, None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_bcd(name, use_hip=False, timeout=240, extra=None):
    """Runs the fixture on its grid (one process per rank, gloo) and returns {rank: {key: (dW, dH, derr)}}; raises on a rank's error."""
    import torch.multiprocessing as mp
    from tests._mp import collect, free_port
    meta = load_bcd(name)[0]
    world = meta["grid"][0] * meta["grid"][1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run_bcd_rank, args=(r, world, port, name, q, use_hip, extra)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(procs, q, timeout)
    out = {}
    for rank, o, err in res:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
        out[rank] = o
    return out


def check_tolerances(name, res):
    """steps: rel-Fro <= 1e-5 N on W and H; fits: <= 1e-4 and |d err| <= 1e-5 (a restart decided differently on a near tie would show as far larger)"""
    for rank, o in res.items():
        for key, (dw, dh, de) in o.items():
            tol = 1e-5 * int(key[4:]) if key.startswith("step") else 1e-4
            assert dw <= tol and dh <= tol and de <= 1e-5, (name, rank, key, dw, dh, de)


def run_acceptance_rank(rank, world, port, grid, itr, q):
    """The reference's own acceptance (tests/test_dist_nmf_1d.py:39-47): t24x12 from the fixture's initial factors, method='bcd',
    `itr` iterations on `grid`; puts the relative error."""
    try:
        import torch.distributed as dist
        from oracle import nmf_oracle as orc
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        from pydnmfk_amd.utils import determine_block_params
        torch.set_num_threads(1)
        torch.cuda.set_device(0)
        if world > 1:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        meta, A, W0, H0, _ = load_bcd("t24x12_1x1")
        meta = dict(meta, grid=list(grid))
        comms = MPI_comm(None, *grid)
        s, e = determine_block_params(rank, tuple(grid), A.shape).determine_block_index_range_asymm()
        (w0, w1), (h0, h1) = orc.factor_ranges(rank, grid[0], grid[1], meta["m"], meta["n"])
        _, _, err = PyNMF(A[s[0]:e[0] + 1, s[1]:e[1] + 1], factors=[W0[w0:w1], H0[:, h0:h1]], params=_params(comms, meta, itr)).fit()
        q.put((rank, err, None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_acceptance(grid, itr, timeout=240):
    import torch.multiprocessing as mp
    from tests._mp import collect, free_port
    world = grid[0] * grid[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run_acceptance_rank, args=(r, world, port, grid, itr, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(procs, q, timeout)
    for rank, err, tb in res:
        assert tb is None, "rank %d failed:\n%s" % (rank, tb)
    return [err for _, err, _ in res]
