"""Multi-process harness shared by the CPU choreography tests (gloo, checker back end) and the GPU multi-rank
tests (gloo transport, real HIP kernels, every rank on cuda:0 of a one-GPU box)."""
import os
import socket
import traceback

import torch
import torch.multiprocessing as mp

from tests._golden import load_case, rel_fro


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def collect(procs, q, timeout):
    """One result per rank from `q` (each within `timeout`), then the ranks joined.  A rank that is still alive when this returns or
    raises is terminated: a rank stuck in a collective whose peer has gone would otherwise outlive the test and, being a
    non-daemonic child, keep the interpreter from exiting.  A missing result fails with every rank's state and what the others sent."""
    import queue
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=timeout))
        for p in procs:
            p.join(timeout=60)
    except queue.Empty:
        state = ["alive" if getattr(p, "exitcode", 0) is None else "exit code %r" % getattr(p, "exitcode", 0) for p in procs]
        sent = "\n".join("rank %d sent:\n%s" % (r[0], r[-1]) for r in res if r[-1] is not None)
        raise AssertionError("%d of %d ranks sent a result within %g s; ranks: %s\n%s" % (len(res), len(procs), timeout, ", ".join(state), sent))
    finally:
        for p in procs:
            if getattr(p, "is_alive", lambda: False)():
                p.terminate()
                p.join(timeout=10)
                if p.is_alive():
                    p.kill()
                    p.join(timeout=10)
    return res


def run_case_rank(rank, world, port, name, q, use_hip, extra=None):
    try:
        import torch.distributed as dist
        from oracle import nmf_oracle as orc
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        from pydnmfk_amd.utils import determine_block_params, parse

        torch.set_num_threads(1)
        if use_hip:
            torch.cuda.set_device(0)
            ops = None                      # product default: HIP kernels
        else:
            from tests._ops_double import OracleOps
            ops = OracleOps()
        if world > 1:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        meta, A, W0, H0, z = load_case(name)
        p_r, p_c = meta["grid"]
        comms = MPI_comm(None, p_r, p_c)
        out = {}
        if not meta.get("prune", False):
            # one bare update() from the fixture's initial factors (what make_golden.py captured as step1): pins every
            # method -- HALS included -- per step, where the fits below carry the looser multi-iteration budget
            from pydnmfk_amd.dist_nmf import nmf_algorithms_1D, nmf_algorithms_2D
            args = parse()
            args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, p_r, p_c, meta["k"]
            args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
            args.itr, args.init, args.verbose, args.prune = 1, "rand", False, False
            args.norm, args.method, args.W_update = meta["norm"], meta.get("method", "mu"), meta["W_update"]
            for key, val in (extra or {}).items():
                setattr(args, key, val)
            s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
            (w0, w1), (h0, h1) = orc.factor_ranges(rank, p_r, p_c, meta["m"], meta["n"])
            nmf = PyNMF(A[s[0]:e[0] + 1, s[1]:e[1] + 1], factors=[W0[w0:w1], H0[:, h0:h1]], params=args, ops=ops)
            if nmf.topo == "2d":
                W1, H1 = nmf_algorithms_2D(nmf.A_ij, nmf.W_ij, nmf.H_ij, params=nmf.params, ops=nmf._ops()).update()
            else:
                W1, H1 = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update()
            out["step1"] = (rel_fro(W1.cpu().numpy(), z["r%d_step1_W" % rank]), rel_fro(H1.cpu().numpy(), z["r%d_step1_H" % rank]), 0.0)
        for itr in meta["itrs"]:
            args = parse()
            args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, p_r, p_c, meta["k"]
            args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
            args.itr, args.init, args.verbose, args.prune = itr, "rand", False, meta.get("prune", False)
            args.norm, args.method, args.W_update = meta["norm"], meta.get("method", "mu"), meta["W_update"]
            for key, val in (extra or {}).items():
                setattr(args, key, val)
            s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
            assert [s[0], e[0] + 1, s[1], e[1] + 1] == list(z["r%d_A_range" % rank])
            A_ij = A[s[0]:e[0] + 1, s[1]:e[1] + 1]
            (w0, w1), (h0, h1) = orc.factor_ranges(rank, p_r, p_c, meta["m"], meta["n"])
            W, H, err = PyNMF(A_ij, factors=[W0[w0:w1], H0[:, h0:h1]], params=args, ops=ops).fit()
            assert (args.m, args.n) == (meta["m"], meta["n"])
            assert [args.m_loc, args.n_loc] == list(z["r%d_m_loc_n_loc" % rank])
            assert tuple(W.shape) == z["r%d_fit%d_W" % (rank, itr)].shape
            assert W.dtype == z["r%d_fit%d_W" % (rank, itr)].dtype and H.dtype == z["r%d_fit%d_H" % (rank, itr)].dtype
            out[itr] = (rel_fro(W, z["r%d_fit%d_W" % (rank, itr)]), rel_fro(H, z["r%d_fit%d_H" % (rank, itr)]),
                        abs(err - float(z["r0_fit%d_err" % itr])))
            import pydnmfk_amd.engine as _eng
            # (ranks stacked on ONE GPU share it: a persistent kernel may lose its residency, and PyNMF then fits again on the launch chains
            # -- round 6 -- which is a correct fit with other counts; the counts are asserted for undisturbed fits)
            recovered = bool(getattr(_eng, "_downgraded", False))
            if (extra or {}).get("exchange") in ("native", "native-hosted") and not recovered:      # the fit really ran inside the library
                assert getattr(args, "_native_comm", None) is not None and args._native_comm.steps == itr, \
                    (itr, getattr(getattr(args, "_native_comm", None), "steps", None))
                if (extra or {}).get("direct_allreduce"):                         # ... with its world allreduce over the peer regions
                    assert getattr(args._native_comm, "direct_ready", False) and not args._native_comm.direct_timed_out()
                    if meta.get("method") == "hals" and p_r > 1 and meta["W_update"]:
                        # ... and every W sweep as ONE persistent launch across the ranks (csrc/dnmf_hals.h, HalsPeers)
                        assert args._native_comm.hals_xsweeps() == itr, (itr, args._native_comm.hals_xsweeps())
        q.put((rank, out, None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_case(name, use_hip=False, timeout=240, extra=None, tols=None):
    """`tols` = (per step, per fit, error) overrides the float32 budgets (the float64 goldens: 1e-10 / 1e-8 / 1e-9)"""
    meta = load_case(name)[0]
    world = meta["grid"][0] * meta["grid"][1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run_case_rank, args=(r, world, port, name, q, use_hip, extra)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(procs, q, timeout)
    for rank, out, err in res:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
        hals = meta.get("method") == "hals"
        for itr, (dw, dh, de) in out.items():
            if itr == "step1":
                tol = 5e-5 if hals else 1e-5
            else:
                tol = 2e-3 if hals else 1e-4      # HALS cancels: see tests/test_oracle_golden.py::test_fit
            tol_e = 1e-5
            if tols is not None:
                tol, tol_e = (tols[0] if itr == "step1" else tols[1]), tols[2]
            assert dw <= tol and dh <= tol and de <= tol_e, (name, rank, itr, dw, dh, de)


def run_bf16_rank(rank, world, port, grid, method, q, use_hip, cfg=None):
    """PyNMF with params.precision = 'bfloat16' on a p_r x p_c grid == the oracle's grid simulation on float(bf16(A)).
    `cfg` = {"shape": (m, n, k, itr), "precision": ..., "gemm": ...} varies the problem (default: the bf16 case)."""
    try:
        import numpy as np
        import torch.distributed as dist
        from oracle import nmf_oracle as orc
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        from pydnmfk_amd.utils import determine_block_params, parse

        torch.set_num_threads(1)
        if use_hip:
            torch.cuda.set_device(0)
            ops = None
        else:
            from tests._ops_double import OracleOps
            ops = OracleOps()
        if world > 1:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        p_r, p_c = grid
        cfg = cfg or {}
        m, n, k, itr = cfg.get("shape", (50, 38, 4, 12))
        precision = cfg.get("precision", "bfloat16")
        rs = np.random.RandomState(11)
        A = np.abs(rs.rand(m, k) @ rs.rand(k, n) + 0.05 * rs.randn(m, n)).astype(np.float32)
        W0, H0 = rs.rand(m, k).astype(np.float32), rs.rand(k, n).astype(np.float32)
        Ar = torch.from_numpy(A).to(torch.bfloat16).float().numpy() if precision == "bfloat16" else A
        norm = cfg.get("norm", "fro")
        Wr, Hr, err_r = orc.SimGrid(Ar, W0, H0, p_r, p_c, norm=norm, W_update=True, method=method).fit(itr)
        comms = MPI_comm(None, p_r, p_c)
        args = parse()
        args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, p_r, p_c, k
        args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
        args.itr, args.init, args.verbose, args.prune = itr, "rand", False, False
        args.norm, args.method, args.W_update, args.precision = norm, method, True, precision
        if cfg.get("gemm"):
            args.gemm = cfg["gemm"]
        if cfg.get("overlap_min_cols"):
            args.overlap_min_cols = cfg["overlap_min_cols"]
        if cfg.get("exchange"):
            args.exchange = cfg["exchange"]
        s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
        (w0, w1), (h0, h1) = orc.factor_ranges(rank, p_r, p_c, m, n)
        nmf = PyNMF(A[s[0]:e[0] + 1, s[1]:e[1] + 1], factors=[W0[w0:w1], H0[:, h0:h1]], params=args, ops=ops)
        assert nmf.A_ij.dtype == (torch.bfloat16 if precision == "bfloat16" else torch.float32)
        if cfg.get("gemm") and use_hip:
            assert nmf._ops().name == "hip-" + cfg["gemm"]
        W, H, err = nmf.fit()
        import pydnmfk_amd.engine as _eng
        if cfg.get("exchange") and not getattr(_eng, "_downgraded", False):   # every iteration ran inside the library (undisturbed fits: see run_case_rank)
            assert getattr(args, "_native_comm", None) is not None and args._native_comm.steps == itr, getattr(args, "_native_comm", None)
        q.put((rank, (rel_fro(W, Wr[rank]), rel_fro(H, Hr[rank]), abs(err - err_r)), None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_bf16(grid, method, use_hip=False, timeout=240, cfg=None):
    world = grid[0] * grid[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run_bf16_rank, args=(r, world, port, grid, method, q, use_hip, cfg)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(procs, q, timeout)
    tol = 2e-3 if method == "hals" else 1e-4
    for rank, out, err in res:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
        dw, dh, de = out
        assert dw <= tol and dh <= tol and de <= 1e-5, (grid, method, rank, dw, dh, de)


def run_swim_nmfk_rank(rank, world, port, cfg, q, use_hip):
    """examples/dist_pynmfk_2d_Swim.py of the reference: swim.mat on a 2 x 2 grid, KL / MU, rand init, noise 0.016,
    sill_thr 0.6, the default 20 perturbations; `cfg` = (start_k, end_k, itr[, gemm[, perturbations]])."""
    try:
        import time
        import numpy as np
        import torch.distributed as dist
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMFk import PyNMFk
        from pydnmfk_amd.utils import determine_block_params, parse

        torch.set_num_threads(1)
        if use_hip:
            torch.cuda.set_device(0)
            ops = None
        else:
            from tests._ops_double import OracleOps
            ops = OracleOps()
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import tempfile
        from tests._golden import GOLDEN
        A = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "data_swim.npz"))["A"].astype(np.float32))
        p_r, p_c = 2, 2
        comms = MPI_comm(None, p_r, p_c)
        args = parse()
        args.size, args.rank, args.comm, args.p_r, args.p_c = world, rank, comms, p_r, p_c
        args.row_comm, args.col_comm, args.comm1 = comms.cart_1d_row(), comms.cart_1d_column(), comms.comm
        args.fpath, args.fname, args.ftype = "../data/", "swim", "mat"
        args.start_k, args.end_k, args.sill_thr, args.itr, args.init = cfg[0], cfg[1], 0.6, cfg[2], "rand"
        args.noise_var, args.verbose, args.norm, args.method, args.checkpoint = 0.016, False, "kl", "mu", False
        args.precision = np.float32
        if len(cfg) > 3:
            args.gemm = cfg[3]
        if len(cfg) > 4:
            args.perturbations = cfg[4]
        if os.environ.get("DNMF_TEST_EXCHANGE"):          # ad-hoc: the same sweep with library-sequenced steps (native-hosted)
            args.exchange = os.environ["DNMF_TEST_EXCHANGE"]
        tmp = [tempfile.mkdtemp() if rank == 0 else None]
        dist.broadcast_object_list(tmp, src=0)
        args.results_path = tmp[0] + "/"
        s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
        A_ij = A[s[0]:e[0] + 1, s[1]:e[1] + 1].astype(args.precision)
        t0 = time.time()
        nmfk = PyNMFk(A_ij, factors=None, params=args, ops=ops)
        nopt = nmfk.fit()
        sil = {k: float(np.min(v["clusterSilhouetteCoefficients"])) for k, v in nmfk.stats.items()}
        if os.environ.get("DNMF_TEST_EXCHANGE"):
            assert getattr(args, "_native_comm", None) is not None and args._native_comm.steps > 0
        q.put((rank, (int(nopt), sil, time.time() - t0), None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_swim_nmfk(cfg, use_hip=True, timeout=3600):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run_swim_nmfk_rank, args=(r, 4, port, cfg, q, use_hip)) for r in range(4)]
    for p in procs:
        p.start()
    res = collect(procs, q, timeout)
    for rank, out, err in res:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
    return [out for _, out, _ in sorted(res, key=lambda r: r[0])]


def run_nmfk_golden_rank(rank, world, port, fixture, q, use_hip, extra):
    """PyNMFk on the problem, grid and parameters of a reference-generated NMFk fixture (tests/golden/make_golden_nmfk.py:
    nmfk_2x1.npz, nmfk_hals_1x1.npz, nmfk_hals_2x1.npz).  numpy input: every rank consumes the reference's numpy stream
    (every MPI rank of the reference seeds its own process-global generator alike, pyDNMFk.py:31-32)."""
    try:
        import json
        import tempfile
        import numpy as np
        import torch.distributed as dist
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMFk import PyNMFk
        from pydnmfk_amd.utils import determine_block_params, parse
        from tests._golden import GOLDEN

        torch.set_num_threads(1)
        if use_hip:
            torch.cuda.set_device(0)
            ops = None
        else:
            from tests._ops_double import OracleOps
            ops = OracleOps()
        if world > 1:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        z = np.load(os.path.join(GOLDEN, fixture))
        meta = json.loads(str(z["meta"]))
        A = z["A"]
        p_r, p_c = meta["grid"]
        args = parse()
        if (extra or {}).get("nmfk_split") == "perturbations":
            # a 1 x 1 fixture on `world` ranks that SHARE its perturbations: every rank holds the whole matrix
            # (pydnmfk_amd/pyDNMFk.py, params.nmfk_split), the job's communicator is the world
            from pydnmfk_amd.dist_comm import COMM_WORLD, SoloGrid
            assert (p_r, p_c) == (1, 1)
            comms = SoloGrid(rank)
            args.size, args.rank, args.comm1, args.comm, args.p_r, args.p_c = world, rank, COMM_WORLD(), comms, 1, 1
        else:
            comms = MPI_comm(None, p_r, p_c)
            args.size, args.rank, args.comm1, args.comm, args.p_r, args.p_c = world, rank, comms.comm, comms, p_r, p_c
        args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
        tmp = [tempfile.mkdtemp() if rank == 0 else None]
        if world > 1:
            dist.broadcast_object_list(tmp, src=0)
        args.fpath, args.fname, args.ftype = tmp[0] + "/", "synth", "npy"
        args.start_k, args.end_k, args.step_k = meta["start_k"], meta["end_k"], 1
        args.sill_thr, args.itr, args.init, args.verbose = meta["sill_thr"], meta["itr"], "rand", False
        args.norm, args.method, args.prune = meta["norm"], meta["method"], False
        args.perturbations, args.noise_var, args.checkpoint = meta["perturbations"], meta["noise_var"], False
        args.results_path = tmp[0] + "/results/"
        for key, val in (extra or {}).items():
            setattr(args, key, val)
        s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
        A_ij = np.ascontiguousarray(A[s[0]:e[0] + 1, s[1]:e[1] + 1])
        nmfk = PyNMFk(A_ij, factors=None, params=args, ops=ops)
        nopt = nmfk.fit()
        stats = {k: {key: np.asarray(val) for key, val in st.items()} for k, st in nmfk.stats.items()}
        if (extra or {}).get("exchange") in ("native", "native-hosted"):
            assert getattr(args, "_native_comm", None) is not None and args._native_comm.steps > 0
        q.put((rank, (int(nopt), stats), None))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_nmfk_golden(fixture, use_hip=False, timeout=600, extra=None, world=None):
    """-> [(nopt, {k: statistics}) per rank].  `world`: ranks of the job when they SHARE the perturbations of a 1 x 1 fixture
    (extra = {"nmfk_split": "perturbations"}); default: the fixture's grid."""
    import json
    import numpy as np
    from tests._golden import GOLDEN
    grid = json.loads(str(np.load(os.path.join(GOLDEN, fixture))["meta"]))["grid"]
    world = world or grid[0] * grid[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run_nmfk_golden_rank, args=(r, world, port, fixture, q, use_hip, extra)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(procs, q, timeout)
    for rank, out, err in res:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
    return [out for _, out, _ in sorted(res, key=lambda r: r[0])]


def run_exact_rank(rank, world, port, grid, shape, q, exchange=None):
    """One MU/Frobenius step of PyNMF's update() on a p_r x p_c grid with the exact operands of tests/_exact.py (fro_step): every
    partial sum that crosses ranks is exact, so each rank's block of the new W must EQUAL the whole-matrix reference and its block of
    the new H be within 3 ulps of the float64 quotient, element by element.  `exchange`: None (the Python choreography) or
    'native-hosted' (the step sequenced inside the library, collectives handed to gloo)."""
    try:
        import torch.distributed as dist
        from oracle import nmf_oracle as orc
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.dist_nmf import nmf_algorithms_1D, nmf_algorithms_2D
        from pydnmfk_amd.pyDNMF import PyNMF
        from pydnmfk_amd.utils import determine_block_params, parse
        from tests import _exact as ex

        torch.set_num_threads(1)
        torch.cuda.set_device(0)
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        p_r, p_c = grid
        m, n, k = shape
        A, W0, H0, Wn, Hq = ex.fro_step(m, n, k)
        comms = MPI_comm(None, p_r, p_c)
        args = parse()
        args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, p_r, p_c, k
        args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
        args.itr, args.init, args.verbose, args.prune = 1, "rand", False, False
        args.norm, args.method, args.W_update = "fro", "mu", True
        if exchange:
            args.exchange = exchange
        s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
        (w0, w1), (h0, h1) = orc.factor_ranges(rank, p_r, p_c, m, n)
        nmf = PyNMF(A[s[0]:e[0] + 1, s[1]:e[1] + 1], factors=[W0[w0:w1], H0[:, h0:h1]], params=args, ops=None)
        if nmf.topo == "2d":
            W1, H1 = nmf_algorithms_2D(nmf.A_ij, nmf.W_ij, nmf.H_ij, params=nmf.params, ops=nmf._ops()).update()
        else:
            W1, H1 = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update()
        import pydnmfk_amd.engine as _eng
        if exchange and not getattr(_eng, "_downgraded", False):         # the step really ran inside the library
            assert getattr(args, "_native_comm", None) is not None and args._native_comm.steps == 1, getattr(args, "_native_comm", None)
        ex.assert_ulp(W1.cpu().numpy(), Wn[w0:w1], 0, "rank %d W rows %d:%d (exact)" % (rank, w0, w1))
        ex.assert_ulp(H1.cpu().numpy(), Hq[:, h0:h1], 3, "rank %d H columns %d:%d" % (rank, h0, h1))
        q.put((rank, None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc()))


def run_exact(grid, shape, exchange=None, timeout=240):
    world = grid[0] * grid[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run_exact_rank, args=(r, world, port, grid, shape, q, exchange)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(procs, q, timeout)
    for rank, err in res:
        assert err is None, "rank %d failed:\n%s" % (rank, err)


# ---------------------------------------------------------------------------------------------------------- exact operands on a grid
# Modes of one exact case: what is set on the params bag before the step (tests/_exact.py, GRID_EXACT lists the modes of every grid)
EXACT_MODES = {
    "choreography": {},
    "overlap4": {"overlap_chunks": 4, "overlap_min_cols": 64},
    "native-hosted": {"exchange": "native-hosted"},
    "overlap4-native": {"exchange": "native-hosted", "overlap_chunks": 4, "overlap_min_cols": 64},
    "direct": {"exchange": "native-hosted", "direct_allreduce": True},
}


_EXACT_CLAMPS = {"fro": (False, True), "fro_bf16": (False, True)}      # the kinds that run with and without the clamp


def _exact_problem(kind, shape):
    """-> (A, W0, H0, w_update, variants, expected): the operands of a case kind on the WHOLE matrix and what the step must give;
    `variants`: the values of `clamp` the step runs with"""
    from tests import _exact as ex
    m, n, k = shape
    if kind in ("fro", "fro_bf16"):
        A, W, H, Wn, Hq = ex.fro_step(m, n, k)
        assert ex.is_bf16(A).all(), "%s: an entry of A is no bfloat16 number" % (shape,)
        return A, W, H, True, _EXACT_CLAMPS[kind], {"Wn": Wn, "Hq": Hq}
    if kind in ("kl_wfixed", "kl_w"):
        A, W, H, U = ex.kl(m, n, k)
        _, _, _, _, Wq, Hq = ex.kl_refs(A, W, H, U)
        return A, W, H, kind == "kl_w", (False,), {"Wq": Wq, "Hq": Hq}
    if kind == "kl_fixed":
        A, W, H = ex.kl_fixed(m, n, k)
        return A, W, H, True, (False,), {}
    if kind in ("hals", "hals_bf16"):
        P = ex.hals_step_problem(m, n, k, bf16=(kind == "hals_bf16"))
        if kind == "hals_bf16":
            assert ex.is_bf16(P["A"]).all()
        return P["A"], P["W_old"], P["H_old"], True, (False,), P
    if kind == "hals_wfixed":
        A, W, H, Hn = ex.hals_h_step_problem(m, n, k)
        return A, W, H, False, (False,), {"Hn": Hn}
    raise ValueError("unknown exact case kind %r" % (kind,))


def _exact_check(kind, clamp, exp, W0, H0, A, W1, H1, w, h, gathered, what):
    """the assertions of a case kind on this rank's slices (rows w[0]:w[1] of W, columns h[0]:h[1] of H); `gathered` (kl_w): every rank's
    (first row, last row + 1, new W slice)"""
    import numpy as np
    from tests import _exact as ex
    eps32 = np.float32(np.finfo(np.float32).eps)
    (w0, w1), (h0, h1) = w, h
    ws, hs = "%s: W rows %d:%d" % (what, w0, w1), "%s: H columns %d:%d" % (what, h0, h1)
    if kind in ("fro", "fro_bf16"):
        Wn, Hq = (np.maximum(exp["Wn"], eps32), np.maximum(exp["Hq"], eps32)) if clamp else (exp["Wn"], exp["Hq"])
        ex.assert_ulp(W1, Wn[w0:w1], 0, ws + " (exact)")
        ex.assert_ulp(H1, Hq[:, h0:h1], 3, hs)
    elif kind == "kl_wfixed":
        ex.assert_ulp(W1, W0[w0:w1].astype(np.float64), 0, ws + " (W fixed)")
        ex.assert_ulp(H1, exp["Hq"][:, h0:h1], 2, hs)                      # kl_update_h: one IEEE division and one product
    elif kind == "kl_w":
        ex.assert_ulp(W1, exp["Wq"][w0:w1], 2, ws)                         # kl_update_w: the same
        # H after W moved: its quotient U is no longer exact -- 1e-5 of each element against the float64 step from the gathered new W
        Wn = np.zeros(W0.shape)
        for a, b, blk in gathered:
            Wn[a:b] = blk
        H64 = H0.astype(np.float64)
        Un = A.astype(np.float64) / (Wn @ H64 + float(eps32))
        Hn = (H64 * (Wn.T @ Un) / (Wn.sum(0) + float(eps32))[:, None])[:, h0:h1]
        bad = ~(np.abs(H1 - Hn) <= 1e-5 * np.abs(Hn))
        assert not bad.any(), "%s: off by more than 1e-5 first at %s: got %r, float64 %r" % (
            hs, tuple(np.argwhere(bad)[0]), H1[tuple(np.argwhere(bad)[0])], Hn[tuple(np.argwhere(bad)[0])])
    elif kind == "kl_fixed":
        ex.assert_ulp(W1, W0[w0:w1].astype(np.float64), 0, ws + " (fixed point)")
        ex.assert_ulp(H1, H0[:, h0:h1].astype(np.float64), 0, hs + " (fixed point)")
    elif kind in ("hals", "hals_bf16"):
        ex.assert_ulp(W1, exp["W_new"][w0:w1], 0, ws + " (exact)", tile=(ex.HALS_ROWS, 4))
        # the H sweep on the new W cannot be exact: the derived forward bound of the generator, which its docstring calls loose from k of about 16 on
        Hn, He = exp["H_new"][:, h0:h1], exp["H_err"][:, h0:h1]
        assert np.isfinite(H1).all() and (H1 >= ex.HALS_EPS_A).all(), hs + ": not finite or below eps"
        bad = np.abs(H1 - Hn) > He
        assert not bad.any(), "%s: at %s got %r, expected %r within %g" % (
            hs, tuple(np.argwhere(bad)[0]), H1[tuple(np.argwhere(bad)[0])], Hn[tuple(np.argwhere(bad)[0])], He[tuple(np.argwhere(bad)[0])])
    elif kind == "hals_wfixed":
        ex.assert_ulp(W1, W0[w0:w1].astype(np.float64), 0, ws + " (W fixed)")
        ex.assert_ulp(H1, exp["Hn"][:, h0:h1], 0, hs + " (exact)")


def run_exact_cases_rank(rank, world, port, grid, cases, q, use_hip):
    """Every case of `cases` = [(kind, (m, n, k), modes), ...] in every one of its modes on this rank of ONE process group: one update()
    of nmf_algorithms_1D / _2D through PyNMF per (case, mode, clamp), this rank's slices against the whole-matrix answer (`_exact_check`).
    A failed assertion is recorded with rank, case and mode and the loop goes on (the ranks stay in step); anything else ends the rank."""
    try:
        import numpy as np
        import torch.distributed as dist
        from oracle import nmf_oracle as orc
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.dist_nmf import nmf_algorithms_1D, nmf_algorithms_2D
        from pydnmfk_amd.pyDNMF import PyNMF
        from pydnmfk_amd.utils import determine_block_params, parse
        from tests import _exact as ex

        torch.set_num_threads(1)
        if use_hip:
            torch.cuda.set_device(0)
            ops = None
        else:
            from tests._ops_double import OracleOps
            ops = OracleOps()
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        p_r, p_c = grid
        comms = MPI_comm(None, p_r, p_c)
        kmax = max(shape[2] for _, shape, _ in cases)
        shared = {}                         # the library's communicators of this process: one hosted, one with the peer regions on top
        failures = []
        done = {"steps": 0, "library": 0, "direct": 0, "xsweeps": 0, "downgraded": False}     # what really ran, for the parent to count
        for kind, shape, modes in cases:
            m, n, k = shape
            A, W0, H0, w_update, variants, exp = _exact_problem(kind, shape)
            hals = kind.startswith("hals")
            s, e = determine_block_params(rank, (p_r, p_c), A.shape).determine_block_index_range_asymm()
            w, h = orc.factor_ranges(rank, p_r, p_c, m, n)
            for mode in modes:
                extra = EXACT_MODES[mode]
                if extra and not use_hip and "exchange" in extra:
                    raise ValueError("mode %r needs the library: not a mode of the CPU tier" % mode)
                for clamp in variants:
                    what = "rank %d, %s %d x %d k = %d on %d x %d, mode %s%s" % (rank, kind, m, n, k, p_r, p_c, mode, ", clamp" if clamp else "")
                    args = parse()
                    args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, p_r, p_c, k
                    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
                    args.itr, args.init, args.verbose, args.prune = 1, "rand", False, False
                    args.norm, args.method, args.W_update = ("kl" if kind.startswith("kl") else "fro"), ("hals" if hals else "mu"), w_update
                    if kind.endswith("bf16"):
                        args.precision = "bfloat16"
                    for key, val in extra.items():
                        setattr(args, key, val)
                    native, direct = "exchange" in extra, bool(extra.get("direct_allreduce"))
                    if direct:
                        args.end_k = kmax           # the peer regions are sized once per process: for the largest rank of the list, as an NMFk sweep sizes them
                    if native and shared.get(direct) is not None:
                        args._native_comm = shared[direct]
                    nmf = PyNMF(A[s[0]:e[0] + 1, s[1]:e[1] + 1], factors=[W0[w[0]:w[1]], H0[:, h[0]:h[1]]], params=args, ops=ops)
                    assert nmf.A_ij.dtype == (torch.bfloat16 if kind.endswith("bf16") else torch.float32), what
                    if hals:
                        nmf.params.eps = ex.HALS_EPS_A
                    nc = shared.get(direct) if native else None
                    steps0 = nc.steps if nc is not None else 0
                    sweeps0 = nc.hals_xsweeps() if nc is not None and direct else 0
                    if nc is not None:
                        nc.fit_begin()              # (what PyNMF.fit does on every rank before the first step on new data)
                    if nmf.topo == "2d":
                        W1, H1 = nmf_algorithms_2D(nmf.A_ij, nmf.W_ij, nmf.H_ij, params=nmf.params, ops=nmf._ops()).update(clamp=clamp)
                    else:
                        W1, H1 = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params, ops=nmf._ops()).update(clamp=clamp)
                    W1, H1 = W1.cpu().numpy(), H1.cpu().numpy()
                    done["steps"] += 1
                    gathered = comms.comm.allgather((w[0], w[1], W1)) if kind == "kl_w" else None    # (a collective: before anything can raise)
                    try:
                        if native:
                            import pydnmfk_amd.engine as _eng
                            nc = shared[direct] = getattr(args, "_native_comm", None)
                            done["downgraded"] = bool(getattr(_eng, "_downgraded", False))
                            done["library"] += int(nc is not None and nc.steps == steps0 + 1)
                            if not getattr(_eng, "_downgraded", False):     # the step really ran inside the library
                                assert nc is not None and nc.steps == steps0 + 1, "the library's step was not taken (%r)" % (nc,)
                            if direct:                                      # ... with its world allreduce over the peer regions
                                assert nc is not None and getattr(nc, "direct_ready", False) and not nc.direct_timed_out(), "no direct allreduce"
                                done["direct"] += 1
                                done["xsweeps"] += nc.hals_xsweeps() - sweeps0
                                if kind in ("hals", "hals_bf16") and p_r > 1 and p_c == 1 and not getattr(_eng, "_downgraded", False):
                                    # ... and the W sweep as ONE persistent launch across the ranks (csrc/dnmf_hals.h, HalsPeers)
                                    assert nc.hals_xsweeps() == sweeps0 + 1, "%d cross-rank sweeps" % (nc.hals_xsweeps() - sweeps0)
                        _exact_check(kind, clamp, exp, W0, H0, A, W1, H1, w, h, gathered, what)
                    except AssertionError:
                        failures.append("%s\n%s" % (what, traceback.format_exc()))
        q.put((rank, done, "\n".join(failures) or None))
        dist.barrier()
        for nc in shared.values():
            if nc is not None:
                nc.close()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_exact_cases(grid, cases, use_hip=True, timeout=240):
    """All of `cases` = [(kind, (m, n, k), modes), ...] on ONE process group of grid[0] x grid[1] ranks (gloo; with `use_hip` every rank on
    cuda:0 and the HIP kernels, without it the checker back end of tests/_ops_double.py and no GPU): a GPU process takes seconds to
    start, a step milliseconds.  kinds: `_exact_problem`; modes: EXACT_MODES; what each rank's slice must satisfy: `_exact_check`."""
    world = grid[0] * grid[1]
    assert 1 < world <= 8, "at most 8 ranks"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run_exact_cases_rank, args=(r, world, port, grid, cases, q, use_hip)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(procs, q, timeout)
    bad = ["rank %d failed:\n%s" % (rank, err) for rank, _, err in sorted(res, key=lambda r: r[0]) if err is not None]
    assert not bad, "\n".join(bad)
    # every rank ran every (case, mode, clamp), and every mode that names the library ran inside it (unless the engine fell back
    # to its launch chains on a shared GPU: run_case_rank)
    steps = sum(len(modes) * len(_EXACT_CLAMPS.get(kind, (False,))) for kind, _, modes in cases)
    lib = sum(len([mo for mo in modes if "exchange" in EXACT_MODES[mo]]) * len(_EXACT_CLAMPS.get(kind, (False,))) for kind, _, modes in cases)
    for rank, done, _ in res:
        assert done["steps"] == steps and (done["library"] == lib or done["downgraded"]), (rank, done, steps, lib)
    return [done for _, done, _ in sorted(res, key=lambda r: r[0])]
