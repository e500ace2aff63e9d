"""ms per beta-divergence MU step (engine.HipOps.beta_*, csrc/dnmf_beta.h) next to the Itakura-Saito step of the SAME build on the same data.

    python tools/betabench.py [--json out.json] [--steps 20] [--warmup 5] [--beta 0.5] [--only m,n,k]

One MI355X; 32768 x 16384 at k = 32, 64, 128 and 65536 x 4096 at k = 64; A uniform in [0.05, 1.05), factors uniform.  A step is one
`nmf_algorithms_1D(...).update()` on one rank (both factors, the fused endings).  The two steps are timed back to back -- beta, then IS,
`--steps` times after `--warmup` of each -- every step with its own pair of HIP events; the figures are medians (min / max next to
them).  The two sides of both steps, the divergence and the per-column sums of an NMFk sweep (dnmf_beta_column_div next to
dnmf_is_column_div, once per k of a sweep) are timed on their own as well.  Both steps run the same pair kernels with the
same launch plans on the same bytes; the beta step's element-wise work is six vector instructions per element (v_add, v_log, v_mul,
v_exp, two v_mul) where the IS step has four (v_add, v_rcp, two v_mul): the ratio shows what the extra transcendental pair costs.
The cost does not depend on the value of beta (the ending's powf runs over m k + k n elements, and not at all for 1 <= beta <= 2).
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

SHAPES = ((32768, 16384, 32), (32768, 16384, 64), (32768, 16384, 128), (65536, 4096, 64))


def bench(m, n, k, beta, steps, warmup, seed=0):
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    A = torch.rand(m, n, device=dev, generator=g) + 0.05
    W, H = torch.rand(m, k, device=dev, generator=g) + 0.01, torch.rand(k, n, device=dev, generator=g) + 0.01
    a_beta = _args(m, n, k, "beta")
    a_beta.beta = beta
    fns = {
        "beta_step": lambda: nmf_algorithms_1D(A, W, H, params=a_beta, ops=HIP_OPS).update(),
        "is_step": lambda a=_args(m, n, k, "is"): nmf_algorithms_1D(A, W, H, params=a, ops=HIP_OPS).update(),
        "beta_update_w": lambda: HIP_OPS.beta_update_w(A, W, H, EPS, beta),
        "is_update_w": lambda: HIP_OPS.is_update_w(A, W, H, EPS),
        "beta_update_h": lambda: HIP_OPS.beta_update_h(A, W, H, EPS, beta),
        "is_update_h": lambda: HIP_OPS.is_update_h(A, W, H, EPS),
        "beta_divergence": lambda: HIP_OPS.beta_divergence(A, W, H, EPS, beta),
        "is_divergence": lambda: HIP_OPS.is_divergence(A, W, H, EPS),
        "beta_column_div": lambda: HIP_OPS.beta_column_div(A, W, H, EPS, beta),
        "is_column_div": lambda: HIP_OPS.is_column_div(A, W, H, EPS),
    }
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(steps):
        for name, fn in fns.items():                       # back to back: beta step, IS step, then the pieces in pairs
            ts[name].append(_event_ms(fn))
    out = {"m": m, "n": n, "k": k, "beta": beta}
    out.update({name: _stats(v) for name, v in ts.items()})
    for what in ("step", "update_w", "update_h", "divergence", "column_div"):
        out["ratio_%s" % what] = out["beta_" + what]["median_ms"] / out["is_" + what]["median_ms"]
    assert torch.isfinite(W).all() and torch.isfinite(H).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--only", help="m,n,k: one shape (a profiler run)")
    opt = ap.parse_args()
    torch.cuda.set_device(0)
    shapes = (tuple(int(x) for x in opt.only.split(",")),) if opt.only else SHAPES
    rows = [bench(m, n, k, opt.beta, opt.steps, opt.warmup) for m, n, k in shapes]
    print("| m x n | k | beta | beta step ms (min-max) | IS step ms (min-max) | beta / IS | W side: beta ms | IS ms | ratio | H side: beta ms | IS ms | ratio | "
          "divergence: beta ms | IS ms | per-column: beta ms | IS ms | ratio |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        t = lambda key: "%.3f (%.3f-%.3f)" % (r[key]["median_ms"], r[key]["min_ms"], r[key]["max_ms"])      # noqa: E731
        md = lambda key: r[key]["median_ms"]                                                                 # noqa: E731
        print("| %d x %d | %d | %g | %s | %s | %.2f | %.3f | %.3f | %.2f | %.3f | %.3f | %.2f | %.3f | %.3f | %.3f | %.3f | %.2f |" % (
            r["m"], r["n"], r["k"], r["beta"], t("beta_step"), t("is_step"), r["ratio_step"], md("beta_update_w"), md("is_update_w"),
            r["ratio_update_w"], md("beta_update_h"), md("is_update_h"), r["ratio_update_h"], md("beta_divergence"), md("is_divergence"),
            md("beta_column_div"), md("is_column_div"), r["ratio_column_div"]))
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
