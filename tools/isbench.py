"""ms per Itakura-Saito MU step (engine.HipOps.is_*, csrc/dnmf_is.h) next to the MU/KL step of the SAME build on the same data.

    python tools/isbench.py [--json out.json] [--steps 20] [--warmup 5] [--only m,n,k]

One MI355X; 32768 x 16384 at k = 5, 32, 64, 128 and 65536 x 4096 at k = 64; A uniform in [0.05, 1.05), factors uniform.  A step is
one `nmf_algorithms_1D(...).update()` on one rank (both factors, the fused endings).  The two steps are timed back to back -- IS,
then KL, `--steps` times after `--warmup` of each -- every step with its own pair of HIP events; the figures are medians (min / max
next to them).  The two sides of the IS step, the divergence and the per-column divergence of an NMFk sweep (dnmf_is_column_div,
once per k of a sweep) are timed on their own as well.  By arithmetic an IS side is 6 m n k flop against KL's
4 m n k on the same bytes: the figure to hold the ratio against is 1.5 where the fp32 MFMA bounds the step and 1 at k <= 16.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pydnmfk_amd.engine import HIP_OPS  # noqa: E402
from tools.sparsebench import EPS, _args  # noqa: E402

SHAPES = ((32768, 16384, 5), (32768, 16384, 32), (32768, 16384, 64), (32768, 16384, 128), (65536, 4096, 64))


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def bench(m, n, k, steps, warmup, seed=0):
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    A = torch.rand(m, n, device=dev, generator=g) + 0.05
    W, H = torch.rand(m, k, device=dev, generator=g) + 0.01, torch.rand(k, n, device=dev, generator=g) + 0.01
    fns = {
        "is_step": lambda a=_args(m, n, k, "is"): nmf_algorithms_1D(A, W, H, params=a, ops=HIP_OPS).update(),
        "kl_step": lambda a=_args(m, n, k, "kl"): nmf_algorithms_1D(A, W, H, params=a, ops=HIP_OPS).update(),
        "is_update_w": lambda: HIP_OPS.is_update_w(A, W, H, EPS),
        "is_update_h": lambda: HIP_OPS.is_update_h(A, W, H, EPS),
        "is_divergence": lambda: HIP_OPS.is_divergence(A, W, H, EPS),
        "is_column_div": lambda: HIP_OPS.is_column_div(A, W, H, EPS),
    }
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(steps):
        for name, fn in fns.items():                       # back to back: IS step, KL step, then the pieces
            ts[name].append(_event_ms(fn))
    out = {"m": m, "n": n, "k": k}
    out.update({name: _stats(v) for name, v in ts.items()})
    out["ratio_is_over_kl"] = out["is_step"]["median_ms"] / out["kl_step"]["median_ms"]
    out["is_tflops"] = 2 * 6.0 * m * n * max(k, 32 if k <= 32 else (64 if k <= 64 else 128)) / (out["is_step"]["median_ms"] * 1e9)
    assert torch.isfinite(W).all() and torch.isfinite(H).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", help="m,n,k: one shape (a profiler run)")
    opt = ap.parse_args()
    torch.cuda.set_device(0)
    shapes = (tuple(int(x) for x in opt.only.split(",")),) if opt.only else SHAPES
    rows = [bench(m, n, k, opt.steps, opt.warmup) for m, n, k in shapes]
    print("| m x n | k | IS step ms (min-max) | KL step ms (min-max) | IS / KL | IS W side ms | IS H side ms | divergence ms | per-column divergence ms | "
          "IS step, padded-rank TFLOP/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        t = lambda key: "%.3f (%.3f-%.3f)" % (r[key]["median_ms"], r[key]["min_ms"], r[key]["max_ms"])      # noqa: E731
        print("| %d x %d | %d | %s | %s | %.2f | %.3f | %.3f | %.3f | %.3f | %.1f |" % (
            r["m"], r["n"], r["k"], t("is_step"), t("kl_step"), r["ratio_is_over_kl"], r["is_update_w"]["median_ms"],
            r["is_update_h"]["median_ms"], r["is_divergence"]["median_ms"], r["is_column_div"]["median_ms"], r["is_tflops"]))
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
