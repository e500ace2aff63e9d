"""ms per MU/FRO and MU/KL step on a sparse data block (engine.HipCsrOps, csrc/dnmf_csr.h), per kernel and per step, next to the
dense step of the same build on the densified matrix where that fits.

    python tools/sparsebench.py [--json out.json] [--quick]
    python tools/sparsebench.py --nmfk [--json out.json]        # NMFk on a sparse block: the two kernels and one small sweep

Matrices: uniformly placed entries and power-law rows AND columns (Zipf exponent 1 over a random permutation), values uniform in
[0.05, 1.05).  k = 16 and 64.  Every figure is the median (min / max next to it) of --steps timed steps after --warmup steps, each
step timed with its own pair of events.  Per kernel: time, stored entries per second, and effective bytes per second counting
8 nnz + 4 k nnz for a gather pass.  The dense path is untouched by the sparse work, so the dense figure of this build is the
parent's.  Sanity condition (checked here): at 1 % density on 65536 x 4096, k = 64, the sparse MU/FRO step is not slower than
the dense step on the same data.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pydnmfk_amd.engine import HIP_CSR_OPS, HIP_OPS  # noqa: E402
from pydnmfk_amd.sparse import SparseBlock  # noqa: E402

EPS = 1.1920929e-07


def _args(m, n, k, norm):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.utils import parse
    comms = MPI_comm(None, 1, 1)
    a = parse()
    a.comm1, a.comm, a.p_r, a.p_c, a.k = comms.comm, comms, 1, 1, k
    a.row_comm, a.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    a.itr, a.init, a.verbose, a.prune, a.norm, a.method, a.W_update = 1, "rand", False, False, norm, "mu", True
    a.m, a.n, a.eps = m, n, EPS
    return a


def make_block(m, n, nnz, kind, seed=0):
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    if kind == "uniform":
        rows = torch.randint(0, m, (nnz,), device=dev, generator=g)
        cols = torch.randint(0, n, (nnz,), device=dev, generator=g)
    else:                                                           # power law: P(index of rank r) ~ 1 / r
        def zipf(size):
            w = 1.0 / torch.arange(1, size + 1, device=dev, dtype=torch.float64)
            idx = torch.multinomial(w.float(), nnz, replacement=True, generator=g)
            return torch.randperm(size, device=dev, generator=g)[idx]
        rows, cols = zipf(m), zipf(n)
    vals = torch.rand(nnz, device=dev, generator=g) + 0.05
    return SparseBlock.from_coo(rows, cols, vals, (m, n))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def bench_block(blk, k, steps, warmup, dense=False):
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    m, n = blk.shape
    dev = blk.device
    ops = HIP_CSR_OPS
    W, H = torch.rand(m, k, device=dev), torch.rand(k, n, device=dev)
    AH, AtW = torch.empty(m, k, device=dev), torch.empty(k, n, device=dev)
    out = {"m": m, "n": n, "k": k, "nnz": blk.nnz, "density": blk.nnz / (m * n), "long_rows": blk.n_long, "long_cols": blk.t_n_long}
    gather_bytes = 8.0 * blk.nnz + 4.0 * k * blk.nnz
    for name, fn in (("aht", lambda: ops.aht(blk, H, AH)), ("wta", lambda: ops.wta(blk, W, AtW)),
                     ("kl_uht", lambda: ops.kl_uht(blk, W, H, EPS, AH)), ("kl_wtu", lambda: ops.kl_wtu(blk, W, H, EPS, AtW)),
                     ("resid_sqnorm", lambda: ops.resid_sqnorm(blk, W, H))):
        t = timed(fn, steps, warmup)
        t["entries_per_s"] = blk.nnz / (t["median_ms"] * 1e-3)
        t["eff_GBps"] = gather_bytes / (t["median_ms"] * 1e-3) / 1e9
        out[name] = t
    for norm in ("fro", "kl"):
        a = _args(m, n, k, norm)
        W.uniform_(); H.uniform_()
        out["step_" + norm] = timed(lambda: nmf_algorithms_1D(blk, W, H, params=a, ops=ops).update(), steps, warmup)
    if dense:
        A = blk.to_dense()
        for norm in ("fro", "kl"):
            a = _args(m, n, k, norm)
            W.uniform_(); H.uniform_()
            out["dense_step_" + norm] = timed(lambda: nmf_algorithms_1D(A, W, H, params=a, ops=HIP_OPS).update(), steps, warmup)
        del A
    return out


def bench_nmfk(steps, warmup):
    """--nmfk: the perturbed copy (both images) and the per-column error of a sparse block, per call, under both meanings of an
    unstored entry, and the wall time of one small sweep through PyNMFk.  Reported only: nothing here is a pass / fail condition."""
    import tempfile
    import time
    from pydnmfk_amd.pyDNMFk import PyNMFk
    ops = HIP_CSR_OPS
    rows = []
    for kind, m, n, nnz in (("uniform 0.01", 65536, 4096, int(0.01 * 65536 * 4096)), ("powerlaw", 2 ** 20, 2 ** 16, 20_000_000)):
        blk = make_block(m, n, nnz, "uniform" if kind.startswith("uniform") else "powerlaw")
        r = {"kind": kind, "m": m, "n": n, "nnz": blk.nnz, "long_cols": blk.t_n_long}
        r["perturb_uniform"] = timed(lambda: ops.perturb_uniform(blk, 0.03, 1000), steps, warmup)
        for k in (16, 64, 256):
            W, H = torch.rand(m, k, device=blk.device), torch.rand(k, n, device=blk.device)
            for missing in (None, "unstored"):
                blk.missing = missing
                r["column_err k=%d %s" % (k, missing or "zero")] = timed(lambda: ops.column_err_sums(blk, W, H), steps, warmup)
            blk.missing = None
            del W, H
        rows.append(r)
        del blk
    blk = make_block(8192, 1024, int(0.02 * 8192 * 1024), "uniform")
    a = _args(8192, 1024, 2, "fro")
    a.fpath, a.fname, a.ftype, a.results_path = "", "sparsebench", None, tempfile.mkdtemp() + "/"
    a.start_k, a.end_k, a.step_k, a.perturbations, a.noise_var, a.itr, a.checkpoint, a.rng = 2, 4, 1, 8, 0.03, 100, False, "device"
    torch.cuda.synchronize()
    t0 = time.time()
    nopt = PyNMFk(blk, params=a).fit()
    torch.cuda.synchronize()
    sweep = {"m": 8192, "n": 1024, "nnz": blk.nnz, "k": "2..4", "perturbations": 8, "itr": 100, "seconds": time.time() - t0, "nopt": int(nopt)}
    print("| matrix | m x n | nnz | long columns | perturb (both images) ms | " + " | ".join(
        "col err k=%d %s ms" % (k, w) for k in (16, 64, 256) for w in ("zero", "unstored")) + " |")
    print("|---|---|---|---|---|" + "---|" * 6)
    for r in rows:
        print("| %s | %d x %d | %d | %d | %.3f | " % (r["kind"], r["m"], r["n"], r["nnz"], r["long_cols"], r["perturb_uniform"]["median_ms"])
              + " | ".join("%.3f" % r["column_err k=%d %s" % (k, w)]["median_ms"] for k in (16, 64, 256) for w in ("zero", "unstored")) + " |")
    print("sweep: %(m)d x %(n)d, nnz %(nnz)d, k = %(k)s, %(perturbations)d perturbations x %(itr)d iterations (mu / fro, rng = device): "
          "%(seconds).2f s, estimate %(nopt)d" % sweep)
    return {"rows": rows, "sweep": sweep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nmfk", action="store_true", help="time the two kernels of NMFk on a sparse block and one small sweep (reported only)")
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the crossover table only")
    opt = ap.parse_args()
    torch.cuda.set_device(0)
    if opt.nmfk:
        res = bench_nmfk(opt.steps, opt.warmup)
        if opt.json:
            with open(opt.json, "w") as f:
                json.dump(res, f, indent=1)
        return 0
    rows = []
    m, n = 65536, 4096
    for dens in (0.001, 0.01, 0.05, 0.2):
        blk = make_block(m, n, int(dens * m * n), "uniform")
        for k in (16, 64):
            r = bench_block(blk, k, opt.steps, opt.warmup, dense=True)
            r["kind"] = "uniform %g" % dens
            rows.append(r)
        del blk
    if not opt.quick:
        for kind in ("uniform", "powerlaw"):
            blk = make_block(2 ** 20, 2 ** 16, 20_000_000, kind)
            for k in (16, 64):
                r = bench_block(blk, k, opt.steps, opt.warmup)
                r["kind"] = kind
                rows.append(r)
            del blk
    print("| matrix | m x n | nnz | k | aht ms | wta ms | kl_uht ms | kl_wtu ms | resid ms | Gentries/s (aht) | GB/s (aht) | sparse FRO step ms (min-max) | "
          "sparse KL step ms | dense FRO step ms | dense KL step ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        d = lambda key: ("%.3f" % r[key]["median_ms"]) if key in r else "-"      # noqa: E731
        print("| %s | %d x %d | %d | %d | %s | %s | %s | %s | %s | %.2f | %.0f | %s (%.3f-%.3f) | %s | %s | %s |" % (
            r["kind"], r["m"], r["n"], r["nnz"], r["k"], d("aht"), d("wta"), d("kl_uht"), d("kl_wtu"), d("resid_sqnorm"),
            r["aht"]["entries_per_s"] / 1e9, r["aht"]["eff_GBps"], d("step_fro"), r["step_fro"]["min_ms"], r["step_fro"]["max_ms"],
            d("step_kl"), d("dense_step_fro"), d("dense_step_kl")))
    sane = [r for r in rows if r["kind"] == "uniform 0.01" and r["k"] == 64][0]
    ok = sane["step_fro"]["median_ms"] <= sane["dense_step_fro"]["median_ms"]
    print("sanity (1 %% density, 65536 x 4096, k = 64): sparse MU/FRO step %.3f ms, dense %.3f ms -> %s" % (
        sane["step_fro"]["median_ms"], sane["dense_step_fro"]["median_ms"], "OK" if ok else "SPARSE IS SLOWER"))
    if opt.json:
        with open(opt.json, "w") as f:
            json.dump({"rows": rows, "sanity_ok": ok}, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
