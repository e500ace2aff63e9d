"""ms per Huber MU step (engine.HipOps.huber_*, csrc/dnmf_huber.h) next to the beta-divergence step of the SAME build on the same data.

    python tools/huberbench.py [--json out.json] [--steps 20] [--warmup 5] [--delta 0.25] [--beta 0.5] [--only m,n,k]

The method of tools/betabench.py: one MI355X; 32768 x 16384 at k = 32, 64, 128; A uniform in [0.05, 1.05) with one entry in fifty replaced
by a spike of 50, factors uniform.  A step is one `nmf_algorithms_1D(...).update()` on one rank (both factors, the fused endings).  The
two steps are timed back to back -- Huber, then beta, `--steps` times after `--warmup` of each -- every step with its own pair of HIP
events; the figures are medians (min / max next to them).  The two sides of both steps and the two objectives are timed on their own as
well.  Both steps run the same pair kernels with the same launch plans on the same bytes; the Huber step's element-wise work is seven
vector instructions per element (v_add, v_sub, v_rcp, v_mul, v_min, two v_mul) where the beta step has six (v_add, v_log, v_mul, v_exp, two
v_mul).  The cost does not depend on delta.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pydnmfk_amd.engine import HIP_OPS  # noqa: E402
from tools.isbench import _event_ms, _stats  # noqa: E402
from tools.sparsebench import EPS, _args  # noqa: E402

SHAPES = ((32768, 16384, 32), (32768, 16384, 64), (32768, 16384, 128))
PIECES = (("step", "step"), ("update_w", "update_w"), ("update_h", "update_h"), ("loss", "divergence"))


def bench(m, n, k, delta, beta, steps, warmup, seed=0):
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    A = torch.rand(m, n, device=dev, generator=g) + 0.05
    A[torch.rand(m, n, device=dev, generator=g) < 0.02] = 50.0
    W, H = torch.rand(m, k, device=dev, generator=g) + 0.01, torch.rand(k, n, device=dev, generator=g) + 0.01
    a_huber, a_beta = _args(m, n, k, "huber"), _args(m, n, k, "beta")
    a_huber.delta, a_beta.beta = delta, beta
    fns = {
        "huber_step": lambda: nmf_algorithms_1D(A, W, H, params=a_huber, ops=HIP_OPS).update(),
        "beta_step": lambda: nmf_algorithms_1D(A, W, H, params=a_beta, ops=HIP_OPS).update(),
        "huber_update_w": lambda: HIP_OPS.huber_update_w(A, W, H, EPS, delta),
        "beta_update_w": lambda: HIP_OPS.beta_update_w(A, W, H, EPS, beta),
        "huber_update_h": lambda: HIP_OPS.huber_update_h(A, W, H, EPS, delta),
        "beta_update_h": lambda: HIP_OPS.beta_update_h(A, W, H, EPS, beta),
        "huber_loss": lambda: HIP_OPS.huber_loss(A, W, H, EPS, delta),
        "beta_divergence": lambda: HIP_OPS.beta_divergence(A, W, H, EPS, beta),
    }
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(steps):
        for name, fn in fns.items():                       # back to back: Huber step, beta step, then the pieces in pairs
            ts[name].append(_event_ms(fn))
    out = {"m": m, "n": n, "k": k, "delta": delta, "beta": beta}
    out.update({name: _stats(v) for name, v in ts.items()})
    for hub, bet in PIECES:
        out["ratio_" + hub] = out["huber_" + hub]["median_ms"] / out["beta_" + bet]["median_ms"]
    assert torch.isfinite(W).all() and torch.isfinite(H).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--delta", type=float, default=0.25)
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--only", help="m,n,k: one shape (a profiler run)")
    opt = ap.parse_args()
    torch.cuda.set_device(0)
    shapes = (tuple(int(x) for x in opt.only.split(",")),) if opt.only else SHAPES
    rows = [bench(m, n, k, opt.delta, opt.beta, opt.steps, opt.warmup) for m, n, k in shapes]
    print("| m x n | k | Huber step ms (min-max) | beta step ms (min-max) | Huber / beta | W side: Huber ms | beta ms | ratio | H side: Huber ms | beta ms | "
          "ratio | objective: Huber ms | beta ms | ratio |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        t = lambda key: "%.3f (%.3f-%.3f)" % (r[key]["median_ms"], r[key]["min_ms"], r[key]["max_ms"])      # noqa: E731
        cells = ["%.3f | %.3f | %.2f" % (r["huber_" + hub]["median_ms"], r["beta_" + bet]["median_ms"], r["ratio_" + hub]) for hub, bet in PIECES[1:]]
        print("| %d x %d | %d | %s | %s | %.2f | %s |" % (r["m"], r["n"], r["k"], t("huber_step"), t("beta_step"), r["ratio_step"], " | ".join(cells)))
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
