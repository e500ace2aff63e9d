"""bench.py as the driver (and a person) launches it: `python bench.py --gpus N` starts its own N ranks, N > 1 lines carry
the exchange diagnostics.  CPU tier: the launcher refuses cleanly without GPUs.  GPU tier: two ranks stacked on the one
GPU over the host-staged gloo transport (RCCL refuses two ranks on one device) -- the whole N > 1 code path of bench.py
except the RCCL calls themselves, which tests/test_gpu_rccl.py covers on a one-rank group."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, timeout=900):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)


def _json_line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_count_gpus_needs_no_hip():
    sys.path.insert(0, ROOT)
    import bench
    n = bench.count_gpus()
    assert isinstance(n, int) and n >= 0


def test_plain_run_leaves_the_extras_to_full():
    """`bench.py` without --full times the steps and nothing else; --full measures every extra unless its --no-* flag says no."""
    sys.path.insert(0, ROOT)
    import bench
    plain = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert not plain.full and plain.steps == 7 and plain.warmup == 2 and plain.dump_outputs is None
    assert all(getattr(plain, key) for key in bench.LEAN_SKIPS)
    full = bench.parse_args(["--full"])
    assert full.full and not any(getattr(full, key) for key in bench.LEAN_SKIPS)
    part = bench.parse_args(["--full", "--no-cpu-baseline", "--dump-outputs", "out"])
    assert part.no_cpu_baseline and not part.no_kernel_timing and part.dump_outputs == "out"


def test_dump_outputs_samples_within_budget(tmp_path):
    """--dump-outputs: float32 / float64 files; an array over its share of the budget becomes a fixed, sorted sample of its rows
    (or columns) with the kept indices beside it -- the same on every run."""
    import numpy as np
    torch = pytest.importorskip("torch")
    sys.path.insert(0, ROOT)
    from benchlib.common import dump_outputs
    g = torch.Generator().manual_seed(5)
    W = torch.rand(5000, 16, generator=g)
    H = torch.rand(16, 300, generator=g, dtype=torch.float64)
    budget = 3 * 4 * 16 * 1000                                   # a third each: W keeps 1000 of its 5000 rows, H fits whole
    for d in ("a", "b"):
        dump_outputs(str(tmp_path / d), [("W", W, 0), ("H", H.to(torch.float64), 1), ("B", W[:8].to(torch.bfloat16), 0)], budget=budget)
    w, wi, h, b = (np.load(str(tmp_path / "a" / f)) for f in ("W.npy", "W_index.npy", "H.npy", "B.npy"))
    assert w.dtype == np.float32 and w.shape == (1000, 16) and wi.dtype == np.float64 and wi.shape == (1000,)
    assert np.all(np.diff(wi) > 0) and np.array_equal(w, W.numpy()[wi.astype(np.int64)])
    assert h.dtype == np.float64 and np.array_equal(h, H.numpy()) and not (tmp_path / "a" / "H_index.npy").exists()
    assert b.dtype == np.float32 and b.shape == (8, 16)
    for f in ("W.npy", "W_index.npy", "H.npy", "B.npy"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK), reason="a GPU is present")
def test_launcher_refuses_without_gpus():
    """No GPU in this container: `--gpus 2` must end with ONE line saying why and a non-zero exit, before any rank starts."""
    r = _run(["--gpus", "2", "--steps", "2"], timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr)
    err = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(err) == 1 and "--gpus 2" in err[0] and "GPU" in err[0], r.stderr
    assert r.stdout.strip() == ""


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [1024, 4096])
def test_two_ranks_on_one_gpu_gloo(cols):
    r = _run(["--gpus", "2", "--rows", "8192", "--cols", str(cols), "--steps", "5", "--warmup", "2", "--backend", "gloo",
              "--full", "--no-cpu-baseline"], env_extra={"DNMF_BENCH_OVERSUBSCRIBE": "1"})
    assert r.returncode == 0, r.stderr[-4000:]
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 2 and out["steps"] == 5 and out["warmup"] == 2
    assert out["scaling"] == "strong" and out["value"] > 0 and out["config"]["rows_per_gpu"] == 4096
    mg = out["multi_gpu"]
    assert mg["rccl_ranks_seen"] == 2 and mg["backend"] == "gloo"
    assert len(mg["compute_only_ms_per_rank"]) == 2 and all(v > 0 for v in mg["compute_only_ms_per_rank"])
    assert abs(mg["exposed_comm_ms"] - (mg["full_step_ms"] - mg["compute_only_ms"])) < 1e-9
    assert set(mg["exchange_ab_ms_per_step"]) == {"torch/chunks=1", "torch/chunks=2", "torch/chunks=4"}
    assert mg["overlap_chunks_used"] in (1, 2, 4) and mg["exchange_used"] == "torch"
    assert mg["allreduce_alone_ms"] > 0 and mg["allreduce_bytes"] == 4 * (64 * cols + 64 * 64)
    assert out["roofline"]["bound"] == "mfma" and "cpu_baseline" not in out


@pytest.mark.gpu
def test_launcher_refuses_more_ranks_than_gpus_over_rccl():
    """One GPU on the box: `--gpus 2` over RCCL must be refused by the parent (one line, exit 2), not fail inside RCCL."""
    sys.path.insert(0, ROOT)
    import bench
    ng = bench.count_gpus() + 1            # one more than the node has (the box of the GPU tier has one; any node works)
    r = _run(["--gpus", str(ng), "--steps", "2"], timeout=120)
    assert r.returncode == 2 and ("--gpus %d" % ng) in r.stderr, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_single_gpu_line_small():
    r = _run(["--rows", "8192", "--cols", "1024", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--no-sustained"])
    assert r.returncode == 0, r.stderr[-4000:]
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 1 and "multi_gpu" not in out and out["value"] > 0


@pytest.mark.gpu
def test_plain_line_is_lean_and_dumps_the_same_outputs(tmp_path):
    """A plain run: the headline keys, exactly --steps timed steps, none of the --full extras; --dump-outputs writes the factors of
    the last timed step (W sampled: over its share of the budget), and a second run with the same arguments writes the same bytes."""
    import numpy as np
    args = ["--rows", "131072", "--cols", "1024", "--steps", "6", "--warmup", "2"]
    outs = []
    for d in ("a", "b"):
        r = _run(args + ["--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-4000:]
        outs.append(_json_line(r.stdout))
    out = outs[0]
    assert out["metric"] == "mu_iterations_per_sec" and out["unit"] == "iter/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["steps"] == 6 and out["value"] > 0
    assert abs(out["ms_per_step"] - 1e3 / out["value"]) < 1e-6 * out["ms_per_step"]
    for key in ("roofline", "rooflines", "kernels", "held_clock_ghz", "sustained", "bf16x6", "bf16_stored_x", "cpu_baseline",
                "reference_example_swim", "configs"):
        assert key not in out, key
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == ["H.npy", "W.npy", "W_index.npy"]
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in files) <= 64e6
    w, wi, h = (np.load(str(tmp_path / "a" / f)) for f in ("W.npy", "W_index.npy", "H.npy"))
    assert w.dtype == h.dtype == np.float32 and h.shape == (64, 1024) and w.shape == (wi.size, 64) and 0 < wi.size < 131072
    assert np.isfinite(w).all() and np.isfinite(h).all() and (w >= 0).all() and (h >= 0).all() and h.max() > 0
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f


@pytest.mark.gpu
def test_emulated_rank_runs_the_rccl_exchange_paths():
    """`--emulate-ranks 8` on the one GPU: one rank's share of the 8-GPU row grid with the REAL RCCL calls on a one-rank
    group -- both exchange transports (torch.distributed and the library's own communicator) x 1 / 2 / 4 overlap chunks are
    timed in the warm-up, i.e. every line of bench.py's N > 1 path runs over RCCL before a multi-GPU node ever sees it."""
    r = _run(["--emulate-ranks", "8", "--rows", "65536", "--cols", "4096", "--steps", "10", "--warmup", "2", "--full", "--no-kernel-timing"])
    assert r.returncode == 0, r.stderr[-4000:]
    out = _json_line(r.stdout)
    mg = out["multi_gpu"]
    assert out["n_gpus"] == 1 and "EMULATED" in out["config"]["workload"] and out["config"]["rows_per_gpu"] == 8192
    assert mg["backend"] == "nccl" and "native_exchange_unavailable" not in mg
    assert set(mg["exchange_ab_ms_per_step"]) == {"%s/chunks=%d" % (t, c) for t in ("torch", "native") for c in (1, 2, 4)}
    assert mg["exchange_used"] in ("torch", "native") and mg["overlap_chunks_used"] in (1, 2, 4)
    assert mg["compute_only_ms"] > 0 and mg["allreduce_alone_ms"] > 0


# ---- round 4: every BASELINE configuration is launchable as typed
@pytest.mark.gpu
def test_config4_emulated_rank_of_the_4x2_grid():
    """`--config 4 --emulate-ranks 8` on the one GPU: rank 0 of the 4 x 2 grid steps its own block through nmf_algorithms_2D
    with the real collective calls on one-rank groups; the line names the configuration and carries the KL roofline."""
    r = _run(["--config", "4", "--emulate-ranks", "8", "--rows", "8192", "--cols", "4096", "--steps", "4", "--warmup", "1",
              "--full", "--no-cpu-baseline"])
    assert r.returncode == 0, r.stderr[-4000:]
    out = _json_line(r.stdout)
    assert out["metric"] == "mu_iterations_per_sec" and out["n_gpus"] == 1 and out["value"] > 0
    assert "BASELINE config 4" in out["config"]["workload"] and "EMULATED" in out["config"]["workload"]
    assert out["config"]["block_per_gpu"] == [2048, 2048] and out["config"]["k"] == 128
    mg = out["multi_gpu"]
    # both arms of the exchange A/B ran: torch.distributed between the launches, and the whole step inside the library
    # (dnmf_mu_kl_step_2d over dnmf_comm_create_emulated); the faster one is used for the timed region
    assert mg["grid"] == [4, 2] and mg["rccl_ranks_seen"] == 1 and mg["exchange_used"] in ("torch", "native")
    assert set(mg["exchange_ab_ms_per_step"]) == {"torch", "native"} and all(v > 0 for v in mg["exchange_ab_ms_per_step"].values())
    assert mg["compute_only_ms"] > 0 and abs(mg["exposed_comm_ms"] - (mg["full_step_ms"] - mg["compute_only_ms"])) < 1e-9
    rf = out["roofline"]
    assert rf["bound"] == "mfma" and rf["kernel"].startswith("kl_uht_pipe_kernel<KT=4>") and 0 < rf["frac"] < 1
    assert rf["flops_per_launch"] == 4.0 * 2048 * 2048 * 128 and "cpu_baseline" not in out


@pytest.mark.gpu
def test_config4_on_a_2x2_grid_stacked_on_one_gpu():
    """`--config 4 --gpus 4` over gloo with the four ranks stacked on the one GPU: the whole N > 1 path of config 4 (2 x 2
    grid, sub-communicators, allgather / reduce-scatter between the kernels, compute-only leg)."""
    r = _run(["--config", "4", "--gpus", "4", "--backend", "gloo", "--rows", "2048", "--cols", "1024", "--rank", "32", "--steps", "3",
              "--warmup", "1", "--full", "--no-kernel-timing"], env_extra={"DNMF_BENCH_OVERSUBSCRIBE": "1"})
    assert r.returncode == 0, r.stderr[-4000:]
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 4 and out["scaling"] == "strong" and out["config"]["block_per_gpu"] == [1024, 512]
    mg = out["multi_gpu"]
    assert mg["grid"] == [2, 2] and mg["rccl_ranks_seen"] == 4 and len(mg["compute_only_ms_per_rank"]) == 4
    assert "2D grid p_r=2 p_c=2" in out["config"]["workload"]


@pytest.mark.gpu
def test_config5_sweep_line_small():
    """`--config 5` cut down (k = 2..5, 3 perturbations x 20 HALS iterations on 4096 x 512): one sweep = one step, fits/s."""
    r = _run(["--config", "5", "--rows", "4096", "--cols", "512", "--end-k", "5", "--perturbations", "3", "--itr", "20",
              "--full", "--no-cpu-baseline"])
    assert r.returncode == 0, r.stderr[-4000:]
    out = _json_line(r.stdout)
    assert out["metric"] == "nmfk_fits_per_sec" and out["unit"] == "fits/s" and out["fits_per_step"] == 12 and out["value"] > 0
    assert "BASELINE config 5" in out["config"]["workload"] and out["dtype"].startswith("bf16")
    assert out["roofline"]["bound"] == "hbm" and out["roofline"]["kernel"].startswith("nt16_kernel<bf16 X>")


@pytest.mark.gpu
def test_config5_two_ranks_share_the_perturbations():
    """`--config 5 --gpus 2` (gloo, both ranks on the one GPU): the ranks hold the whole X and share the perturbation fits
    (params.nmfk_split = 'perturbations'); the planted rank must come back, and the single-rank sweep must agree on it."""
    common = ["--config", "5", "--rows", "4096", "--cols", "512", "--end-k", "8", "--perturbations", "4", "--itr", "60",
              "--no-cpu-baseline", "--no-kernel-timing"]
    r = _run(common + ["--gpus", "2", "--backend", "gloo"], env_extra={"DNMF_BENCH_OVERSUBSCRIBE": "1"})
    assert r.returncode == 0, r.stderr[-4000:]
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 2 and out["fits_per_step"] == 28 and out["value"] > 0
    assert out["config"]["parallelism"].startswith("perturbations over 2 ranks") and out["config"]["block_per_gpu"] == [4096, 512]
    one = _json_line(_run(common).stdout)
    assert out["estimated_k"] == one["estimated_k"] == 6


@pytest.mark.gpu
def test_config2_line_small_steps():
    r = _run(["--config", "2", "--steps", "20", "--warmup", "3", "--full", "--no-cpu-baseline", "--no-sustained"])
    assert r.returncode == 0, r.stderr[-4000:]
    out = _json_line(r.stdout)
    assert "BASELINE config 2" in out["config"]["workload"] and (out["config"]["m"], out["config"]["n"], out["config"]["k"]) == (65536, 4096, 32)
    assert out["roofline"]["bound"] == "mfma" and out["value"] > 500


@pytest.mark.gpu
def test_three_exchange_arms_over_gloo_with_a_hosted_library_communicator():
    """The warm-up A/B of an N > 1 run with all THREE arms -- torch.distributed between the launches, the library-sequenced step, and
    the library-sequenced step with its packed allreduce over IPC peer buffers (`native-direct`) -- on two ranks stacked on the
    one GPU: the library's communicator is a hosted one over gloo here (DNMF_BENCH_HOSTED=1; on a node it is RCCL)."""
    r = _run(["--gpus", "2", "--backend", "gloo", "--rows", "8192", "--cols", "1024", "--steps", "6", "--warmup", "2", "--no-kernel-timing",
              "--no-sustained"], env_extra={"DNMF_BENCH_OVERSUBSCRIBE": "1", "DNMF_BENCH_HOSTED": "1"})
    assert r.returncode == 0, r.stderr[-4000:]
    mg = _json_line(r.stdout)["multi_gpu"]
    assert set(mg["exchange_ab_ms_per_step"]) == {"%s/chunks=%d" % (t, c) for t in ("torch", "native", "native-direct") for c in (1, 2, 4)}
    assert mg["direct_vs_rccl_max_rel_diff"] < 1e-5 and mg["exchange_used"] in ("torch", "native", "native-direct")
    assert mg["native_transport"] == "hosted over gloo"
