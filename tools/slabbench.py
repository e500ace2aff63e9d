"""Whole pair-rule fits under `params.fit_loop = 'slab'` (csrc/dnmf_slab.h: every step two launches for ALL problems of a batch) next to
the default path of the SAME build (dnmf_is_mu_fit / dnmf_weighted_mu_fit: a chain of launches per step, one problem per call) and,
where one workgroup holds the problem, next to `fit_loop = 'resident'`, on the same data.

    python tools/slabbench.py [--md out.md] [--json out.json] [--reps 7] [--itr 300]

One MI355X.  Shapes 1024 x 256 at k = 16, 32 and 4096 x 1024 at k = 16, 64, each as one problem and as 20 problems of that shape (the
perturbations of one rank of a sweep), under norm 'is' and under norm 'kl' with weights of which 30 % are zero (one V for the batch); A
uniform in [0.05, 1.05), factors uniform, `--itr` steps.  A batch on the default path is its fits one by one, which is what PyNMFk
does there.  The paths alternate, `--reps` times after one untimed round of each; a time is the host clock around the call(s) and a
device synchronise; the figures are medians (min - max).  Before the timing the slab factors are compared once with the default
path's (relative Frobenius distance).  The last two columns split a slab step into its phases: the H phase is a fit with W fixed
(H-phase launches alone) over its steps, the W phase the difference to the full fit, both from device events on one problem batch.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pydnmfk_amd.engine import HIP_OPS, stack_alloc  # noqa: E402

EPS = float(np.finfo(np.float32).eps)
SHAPES = ((1024, 256, 16), (1024, 256, 32), (4096, 1024, 16), (4096, 1024, 64))
BATCHES = (1, 20)
CASES = (("is", False), ("kl", True))


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _stats(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def _weights(m, n, dev, seed=11):
    """weights in [0.25, 4), 30 % of them zero: one matrix for every problem of a batch, as in a sweep"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    v = 0.25 + 3.75 * torch.rand(m, n, device=dev, generator=g)
    return torch.where(torch.rand(m, n, device=dev, generator=g) < 0.3, torch.zeros_like(v), v)


def bench_fits(m, n, k, batch, itr, reps, norm, weighted, seed=0):
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

    def reset():
        W.copy_(W0)
        H.copy_(H0)

    def default():
        for b in range(batch):
            if weighted:
                HIP_OPS.weighted_fit(A[b], V, W[b], H[b], EPS, norm, 0.0, True, itr)
            else:
                HIP_OPS.is_fit(A[b], W[b], H[b], EPS, True, itr)

    paths = {"default": default, "slab": lambda: HIP_OPS.slab_fit(norm, 0.0, A, W, H, EPS, True, itr, V=V)}
    if HIP_OPS.resident_refusal(m, n, k) is None:
        paths["resident"] = lambda: HIP_OPS.resident_fit(norm, 0.0, A, W, H, EPS, True, itr, V=V)
    reset(); default(); Wd, Hd = W.clone(), H.clone()
    reset(); paths["slab"]()
    out["dW"] = float((W - Wd).norm() / Wd.norm())
    out["dH"] = float((H - Hd).norm() / Hd.norm())
    if "resident" in paths:
        reset(); paths["resident"]()
    ts = {name: [] for name in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            reset()
            ts[name].append(_wall(fn))
    out.update({name: _stats(v) for name, v in ts.items()})
    out["speedup"] = out["default"]["median_ms"] / out["slab"]["median_ms"]
    out["ranges_apart"] = out["slab"]["max_ms"] < out["default"]["min_ms"]
    # the two phases of a slab step, per step and for the whole batch (device events; the finish is in both fits and cancels in the W figure)
    full, fixed = [], []
    for _ in range(3):
        reset(); full.append(_device_ms(paths["slab"]))
        reset(); fixed.append(_device_ms(lambda: HIP_OPS.slab_fit(norm, 0.0, A, W, H, EPS, False, itr, V=V)))
    out["h_phase_us"] = 1e3 * sorted(fixed)[1] / itr
    out["w_phase_us"] = 1e3 * (sorted(full)[1] - sorted(fixed)[1]) / itr
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--itr", type=int, default=300)
    opt = ap.parse_args()
    torch.cuda.set_device(0)
    t = lambda s: "%.2f (%.2f - %.2f)" % (s["median_ms"], s["min_ms"], s["max_ms"])      # noqa: E731
    rows = []
    lines = ["| norm | m x n | k | problems | default ms (min - max) | resident ms (min - max) | slab ms (min - max) | default / slab | ranges apart | dW | dH "
             "| W phase us/step | H phase us/step |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for norm, weighted in CASES:
        for m, n, k in SHAPES:
            for b in BATCHES:
                r = bench_fits(m, n, k, b, opt.itr, opt.reps, norm, weighted)
                rows.append(r)
                lines.append("| %s | %d x %d | %d | %d | %s | %s | %s | %.2f | %s | %.1e | %.1e | %.1f | %.1f |" % (
                    norm + (" weighted" if weighted else ""), m, n, k, b, t(r["default"]), t(r["resident"]) if "resident" in r else "not eligible",
                    t(r["slab"]), r["speedup"], "yes" if r["ranges_apart"] else "no", r["dW"], r["dH"], r["w_phase_us"], r["h_phase_us"]))
                print(lines[-1], flush=True)
    text = "\n".join(lines)
    for path, body in ((opt.md, text + "\n"), (opt.json, json.dumps(rows, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(body)
    return 0


if __name__ == "__main__":
    sys.exit(main())
