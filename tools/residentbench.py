"""Whole Itakura-Saito fits and a whole NMFk sweep under `params.fit_loop = 'resident'` (csrc/dnmf_resident.h: one workgroup per
problem, a batch in one launch) next to the default path of the SAME build (dnmf_is_mu_fit: a chain of launches per step, one problem
per call) on the same data.

    python tools/residentbench.py [--md out.md] [--json out.json] [--reps 7] [--itr 300] [--rows all|plain|weighted]

One MI355X.  Fits: 120 x 90 at k = 3, 16 and 1024 x 256 at k = 16, 32, each as one problem and as 20 problems of that shape (the
perturbations of a sweep); A uniform in [0.05, 1.05), factors uniform, `--itr` steps.  A batch on the default path is its fits one by
one, which is what PyNMFk does there.  The two paths alternate, `--reps` times after one untimed round of each; a time is the host
clock around the call(s) and a device synchronise (launch overhead is what is being compared); the figures are medians (min - max).
Before the timing the two paths' factors are compared once (relative Frobenius distance).  A shape that one workgroup does not hold
is reported as such.  Sweep: the 120 x 90 rank-3 problem below, k = 1..5, 6 perturbations, 300 iterations, both paths alternating.
`--rows weighted` (part of the default `all`): the same under `params.weights` -- 120 x 90 at k = 3, 16 under norms kl and is, one V with
30 % zero weights for every problem of a batch, against dnmf_weighted_mu_fit one by one -- and the sweep under those weights.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pydnmfk_amd.engine import HIP_OPS, stack_alloc  # noqa: E402

EPS = float(np.finfo(np.float32).eps)
SHAPES = ((120, 90, 3), (120, 90, 16), (1024, 256, 16), (1024, 256, 32))
BATCHES = (1, 20)
WEIGHTED_SHAPES, WEIGHTED_NORMS = ((120, 90, 3), (120, 90, 16)), ("kl", "is")      # the rows under params.weights


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def _weights(m, n, dev, seed=11):
    """weights in [0.25, 4), 30 % of them zero: one matrix for every problem of a batch, as in a sweep"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    v = 0.25 + 3.75 * torch.rand(m, n, device=dev, generator=g)
    return torch.where(torch.rand(m, n, device=dev, generator=g) < 0.3, torch.zeros_like(v), v)


def bench_fits(m, n, k, batch, itr, reps, seed=0, norm="is", weighted=False):
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    A, W0, H0 = stack_alloc(batch, m, n, torch.float32, dev), stack_alloc(batch, m, k, torch.float32, dev), stack_alloc(batch, k, n, torch.float32, dev)
    A.copy_(torch.rand(batch, m, n, device=dev, generator=g) + 0.05)
    W0.copy_(torch.rand(batch, m, k, device=dev, generator=g) + 0.01)
    H0.copy_(torch.rand(batch, k, n, device=dev, generator=g) + 0.01)
    W, H = torch.empty_like(W0), torch.empty_like(H0)
    V = _weights(m, n, dev) if weighted else None
    out = {"m": m, "n": n, "k": k, "batch": batch, "itr": itr, "norm": norm, "weighted": weighted}
    why = HIP_OPS.resident_refusal(m, n, k)
    if why:
        out["not_eligible"] = why
        return out

    def reset():
        W.copy_(W0)
        H.copy_(H0)

    def default():
        for b in range(batch):
            if weighted:                     # (dnmf_weighted_mu_fit: what a weighted fit runs without fit_loop='resident')
                HIP_OPS.weighted_fit(A[b], V, W[b], H[b], EPS, norm, 0.0, True, itr)
            else:
                HIP_OPS.is_fit(A[b], W[b], H[b], EPS, True, itr)

    def resident():
        HIP_OPS.resident_fit(norm, 0.0, A, W, H, EPS, True, itr, V=V)
    reset(); default(); Wd, Hd = W.clone(), H.clone()
    reset(); resident()
    out["dW"] = float((W - Wd).norm() / Wd.norm())
    out["dH"] = float((H - Hd).norm() / Hd.norm())
    ts = {"default": [], "resident": []}
    for _ in range(reps):
        for name, fn in (("default", default), ("resident", resident)):
            reset()
            ts[name].append(_wall(fn))
    out.update({name: _stats(v) for name, v in ts.items()})
    out["speedup"] = out["default"]["median_ms"] / out["resident"]["median_ms"]
    return out


def _planted(seed=1):
    """120 x 90, rank 3, strictly positive float32: three bumps times column scales over three decades, gamma noise"""
    rs = np.random.RandomState(seed)
    m, n, k = 120, 90, 3
    x = np.arange(m)[:, None]
    Wt = np.exp(-0.5 * ((x - m * (np.arange(k)[None, :] + 0.5) / k) / (m / 10.0)) ** 2) + 0.05
    S = (Wt @ (rs.rand(k, n) + 0.05)) * 10.0 ** (-3.0 * rs.rand(n))[None, :]
    return (S * rs.gamma(10.0, 0.1, size=(m, n))).astype(np.float32)


def bench_sweep(reps, weighted=False):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMFk import PyNMFk
    from pydnmfk_amd.utils import parse
    A = _planted()                           # (numpy input: the perturbations and initial factors are numpy's draws, seeded per sweep)
    V = _weights(120, 90, torch.device("cuda", torch.cuda.current_device())).cpu().numpy() if weighted else None
    ts, nopt = {"default": [], "resident": []}, {}
    with tempfile.TemporaryDirectory() as tmp:
        def sweep(name):
            comms = MPI_comm(None, 1, 1)
            args = parse()
            args.comm1, args.comm, args.p_r, args.p_c = comms.comm, comms, 1, 1
            args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
            args.fpath, args.fname, args.ftype, args.results_path = tmp + "/", "synth", "npy", tmp + "/results-%s/" % name
            args.start_k, args.end_k, args.step_k, args.sill_thr, args.itr, args.init, args.verbose = 1, 5, 1, 0.8, 300, "rand", False
            args.norm, args.method, args.prune, args.perturbations, args.noise_var, args.checkpoint = "is", "mu", False, 6, 0.03, False
            if name == "resident":
                args.fit_loop = "resident"
            if weighted:
                args.weights = V
            np.random.seed(0)
            nopt[name] = PyNMFk(A, params=args).fit()
        for r in range(reps + 1):
            for name in ("default", "resident"):
                t = _wall(lambda: sweep(name))
                if r:
                    ts[name].append(t)
    out = {name: _stats(v) for name, v in ts.items()}
    out["nopt"] = nopt
    out["speedup"] = out["default"]["median_ms"] / out["resident"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--itr", type=int, default=300)
    ap.add_argument("--rows", choices=("all", "plain", "weighted"), default="all")
    opt = ap.parse_args()
    torch.cuda.set_device(0)
    t = lambda s: "%.2f (%.2f - %.2f)" % (s["median_ms"], s["min_ms"], s["max_ms"])      # noqa: E731
    lines, results = [], {}
    if opt.rows != "weighted":
        rows = [bench_fits(m, n, k, b, opt.itr, opt.reps) for m, n, k in SHAPES for b in BATCHES]
        sweep = bench_sweep(opt.reps)
        results.update(fits=rows, sweep=sweep)
        lines += ["| m x n | k | problems | default ms (min - max) | resident ms (min - max) | default / resident | dW | dH |", "|---|---|---|---|---|---|---|---|"]
        for r in rows:
            head = "| %d x %d | %d | %d |" % (r["m"], r["n"], r["k"], r["batch"])
            if "not_eligible" in r:
                lines.append(head + " - | not eligible: beyond one workgroup's LDS | - | - | - |")
            else:
                lines.append(head + " %s | %s | %.2f | %.1e | %.1e |" % (t(r["default"]), t(r["resident"]), r["speedup"], r["dW"], r["dH"]))
        lines += ["", "Sweep (120 x 90, norm='is', k = 1..5, 6 perturbations, 300 iterations; estimates %s):" % (sweep["nopt"],), "",
                  "| default ms (min - max) | resident ms (min - max) | default / resident |", "|---|---|---|",
                  "| %s | %s | %.2f |" % (t(sweep["default"]), t(sweep["resident"]), sweep["speedup"]), ""]
    if opt.rows != "plain":
        # under params.weights (30 % zero weights, one V per batch): the default path is dnmf_weighted_mu_fit, fits one by one
        rows = [bench_fits(m, n, k, b, opt.itr, opt.reps, norm=norm, weighted=True)
                for norm in WEIGHTED_NORMS for m, n, k in WEIGHTED_SHAPES for b in BATCHES]
        sweep = bench_sweep(opt.reps, weighted=True)
        results.update(weighted_fits=rows, weighted_sweep=sweep)
        lines += ["| norm | m x n | k | problems | default ms (min - max) | resident ms (min - max) | default / resident | dW | dH |",
                  "|---|---|---|---|---|---|---|---|---|"]
        lines += ["| %s | %d x %d | %d | %d | %s | %s | %.2f | %.1e | %.1e |" % (r["norm"], r["m"], r["n"], r["k"], r["batch"], t(r["default"]),
                                                                                 t(r["resident"]), r["speedup"], r["dW"], r["dH"]) for r in rows]
        lines += ["", "Weighted sweep (120 x 90, norm='is', 30 %% zero weights, k = 1..5, 6 perturbations, 300 iterations; estimates %s):"
                  % (sweep["nopt"],), "", "| default ms (min - max) | resident ms (min - max) | default / resident |", "|---|---|---|",
                  "| %s | %s | %.2f |" % (t(sweep["default"]), t(sweep["resident"]), sweep["speedup"]), ""]
    text = "\n".join(lines[:-1])
    print(text)
    for path, body in ((opt.md, text + "\n"), (opt.json, json.dumps(results, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(body)
    return 0


if __name__ == "__main__":
    sys.exit(main())
