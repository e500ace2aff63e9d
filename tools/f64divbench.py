"""ms per float64 Itakura-Saito / beta-divergence MU step (engine.HipOpsF64.is_* / beta_*, csrc/dnmf_f64_div.h) next to the float64 MU/KL
step of the SAME build on the same data.

    python tools/f64divbench.py [--md out.md] [--json out.json] [--steps 12] [--warmup 4] [--half 0.5] [--general 0.3] [--only m,n,k]

One MI355X; 65536 x 4096 at k = 32 and 64; A uniform in [0.05, 1.05), factors uniform, float64.  A step is one
`nmf_algorithms_1D(...).update()` on one rank (both factors, the fused endings).  The four steps -- KL, IS, beta with 2 (beta - 2) an
integer (multiplies, a refined reciprocal and reciprocal square root), beta in general (the double-precision pow) -- are timed back to
back, `--steps` times after `--warmup` of each, every step with its own pair of HIP events; the figures are medians with the range
next to them.  A timing tool, not a gate: the arithmetic of a pair is 1.5 times the KL step's (three products a side where KL has two),
and the fp64 element-wise step, which does not overlap with the fp64 MFMAs on gfx950, adds to that.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pydnmfk_amd.engine import HIP_OPS_F64  # noqa: E402
from tools.isbench import _event_ms, _stats  # noqa: E402
from tools.sparsebench import _args  # noqa: E402

SHAPES = ((65536, 4096, 32), (65536, 4096, 64))
EPS64 = 2.220446049250313e-16
STEPS = ("kl", "is", "beta_half", "beta_general")


def bench(m, n, k, half, general, steps, warmup, seed=0):
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    A = torch.rand(m, n, device=dev, generator=g, dtype=torch.float64) + 0.05
    W = torch.rand(m, k, device=dev, generator=g, dtype=torch.float64) + 0.01
    H = torch.rand(k, n, device=dev, generator=g, dtype=torch.float64) + 0.01

    def args(norm, beta=None):
        a = _args(m, n, k, norm)
        a.eps, a.beta = EPS64, beta
        return a
    params = {"kl": args("kl"), "is": args("is"), "beta_half": args("beta", half), "beta_general": args("beta", general)}
    fns = {name: (lambda a=a: nmf_algorithms_1D(A, W, H, params=a, ops=HIP_OPS_F64).update()) for name, a in params.items()}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(steps):
        for name, fn in fns.items():
            ts[name].append(_event_ms(fn))
    assert torch.isfinite(W).all() and torch.isfinite(H).all()
    out = {"m": m, "n": n, "k": k, "beta_half_value": half, "beta_general_value": general}
    out.update({name: _stats(v) for name, v in ts.items()})
    return out


def table(rows):
    lines = ["| m x n | k | KL step ms (min-max) | IS step ms (min-max) | IS / KL | beta = %g ms (min-max) | / KL | beta = %g ms (min-max) | / KL | general / half |"
             % (rows[0]["beta_half_value"], rows[0]["beta_general_value"]), "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        t = lambda key: "%.3f (%.3f-%.3f)" % (r[key]["median_ms"], r[key]["min_ms"], r[key]["max_ms"])      # noqa: E731
        md = lambda key: r[key]["median_ms"]                                                                 # noqa: E731
        lines.append("| %d x %d | %d | %s | %s | %.2f | %s | %.2f | %s | %.2f | %.2f |" % (
            r["m"], r["n"], r["k"], t("kl"), t("is"), md("is") / md("kl"), t("beta_half"), md("beta_half") / md("kl"), t("beta_general"),
            md("beta_general") / md("kl"), md("beta_general") / md("beta_half")))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--half", type=float, default=0.5)
    ap.add_argument("--general", type=float, default=0.3)
    ap.add_argument("--only", help="m,n,k: one shape")
    opt = ap.parse_args()
    torch.cuda.set_device(0)
    shapes = (tuple(int(x) for x in opt.only.split(",")),) if opt.only else SHAPES
    rows = [bench(m, n, k, opt.half, opt.general, opt.steps, opt.warmup) for m, n, k in shapes]
    text = table(rows)
    print(text)
    for path, body in ((opt.md, "# float64 IS / beta step times (tools/f64divbench.py, one MI355X, %d steps after %d warm-up)\n\n%s\n"
                        % (opt.steps, opt.warmup, text)), (opt.json, json.dumps({"rows": rows}, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(body)
    return 0


if __name__ == "__main__":
    sys.exit(main())
