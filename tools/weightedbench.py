"""ms per weighted MU step (engine.HipOps.weighted_*, csrc/dnmf_weighted.h) next to the unweighted step of the SAME mode and build on the same data.

    python tools/weightedbench.py [--md out.md] [--json out.json] [--steps 20] [--warmup 5] [--only m,n,k]

One MI355X; 32768 x 16384 at k = 32, 64, 128 and 65536 x 4096 at k = 64; A uniform in [0.05, 1.05), weights uniform in [0.25, 4) with a
quarter of them zero, factors uniform.  A step is update_w then update_h with the fused endings on one rank.  Modes: kl (the unweighted
twin is the masked KL step, the PAIR_KL kernels, on the same NaN-free data) and beta = 0.5 (the twin is the beta step).  The two steps
are timed back to back -- weighted, then unweighted, `--steps` times after `--warmup` of each -- every step with its own pair of HIP
events; the figures are medians (min / max next to them).  Both run the mode's launch plan; the weighted step reads 4 m n more bytes
per side (V beside A), so the byte ratio of a side is (2 A-sized reads) / (1): at most 2, reached only where a side is bound by HBM.
A second table times dnmf_weighted_column_div (beta = 0.5) next to dnmf_beta_column_div on the same A, W, H, in the same rounds.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pydnmfk_amd.engine import HIP_MASKED_OPS, HIP_OPS  # noqa: E402
from pydnmfk_amd.masked import MaskedDenseBlock  # noqa: E402
from tools.isbench import _event_ms, _stats  # noqa: E402
from tools.sparsebench import EPS  # noqa: E402

SHAPES = ((32768, 16384, 32), (32768, 16384, 64), (32768, 16384, 128), (65536, 4096, 64))
MODES = (("kl", 0.0), ("beta", 0.5))


def bench(m, n, k, steps, warmup, seed=0):
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    A = torch.rand(m, n, device=dev, generator=g) + 0.05
    V = torch.where(torch.rand(m, n, device=dev, generator=g) < 0.25, 0.0, 0.25 + 3.75 * torch.rand(m, n, device=dev, generator=g))
    W, H = torch.rand(m, k, device=dev, generator=g) + 0.01, torch.rand(k, n, device=dev, generator=g) + 0.01
    blk = MaskedDenseBlock(A)
    fns = {}
    for norm, beta in MODES:
        def weighted(side, norm=norm, beta=beta):
            return (lambda: HIP_OPS.weighted_update_w(A, V, W, H, EPS, norm, beta)) if side == "w" else \
                (lambda: HIP_OPS.weighted_update_h(A, V, W, H, EPS, norm, beta))

        def plain(side, norm=norm, beta=beta):
            if norm == "kl":
                return (lambda: HIP_MASKED_OPS.masked_update_w(blk, W, H, EPS, "kl")) if side == "w" else \
                    (lambda: HIP_MASKED_OPS.masked_update_h(blk, W, H, EPS, "kl"))
            return (lambda: HIP_OPS.beta_update_w(A, W, H, EPS, beta)) if side == "w" else (lambda: HIP_OPS.beta_update_h(A, W, H, EPS, beta))
        for kind, make in (("weighted", weighted), ("plain", plain)):
            w, h = make("w"), make("h")
            fns["%s_%s_step" % (norm, kind)] = lambda w=w, h=h: (w(), h())
            fns["%s_%s_w" % (norm, kind)], fns["%s_%s_h" % (norm, kind)] = w, h
    # the per-column pair of an NMFk sweep under weights next to dnmf_beta_column_div of the same build on the same A, W, H (beta = 0.5:
    # the general form): twice the A-sized bytes at the same flops
    fns["coldiv_weighted"] = lambda: HIP_OPS.weighted_column_div(A, V, W, H, EPS, "beta", 0.5)
    fns["coldiv_plain"] = lambda: HIP_OPS.beta_column_div(A, W, H, EPS, 0.5)
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(steps):
        for name, fn in fns.items():                       # back to back: weighted step, unweighted step, then the sides in pairs
            ts[name].append(_event_ms(fn))
    out = {"m": m, "n": n, "k": k}
    out.update({name: _stats(v) for name, v in ts.items()})
    for norm, _ in MODES:
        for what in ("step", "w", "h"):
            out["ratio_%s_%s" % (norm, what)] = out["%s_weighted_%s" % (norm, what)]["median_ms"] / out["%s_plain_%s" % (norm, what)]["median_ms"]
    out["ratio_coldiv"] = out["coldiv_weighted"]["median_ms"] / out["coldiv_plain"]["median_ms"]
    assert torch.isfinite(W).all() and torch.isfinite(H).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--md")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", help="m,n,k: one shape (a profiler run)")
    opt = ap.parse_args()
    torch.cuda.set_device(0)
    shapes = (tuple(int(x) for x in opt.only.split(",")),) if opt.only else SHAPES
    rows = [bench(m, n, k, opt.steps, opt.warmup) for m, n, k in shapes]
    lines = ["| m x n | k | mode | weighted step ms (min-max) | unweighted step ms (min-max) | ratio | W side: weighted ms | unweighted ms | ratio | "
             "H side: weighted ms | unweighted ms | ratio |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for norm, beta in MODES:
            t = lambda key: "%.3f (%.3f-%.3f)" % (r[key]["median_ms"], r[key]["min_ms"], r[key]["max_ms"])      # noqa: E731
            md = lambda key: r[key]["median_ms"]                                                                 # noqa: E731
            lines.append("| %d x %d | %d | %s | %s | %s | %.2f | %.3f | %.3f | %.2f | %.3f | %.3f | %.2f |" % (
                r["m"], r["n"], r["k"], norm if norm != "beta" else "beta=%g" % beta, t(norm + "_weighted_step"), t(norm + "_plain_step"),
                r["ratio_%s_step" % norm], md(norm + "_weighted_w"), md(norm + "_plain_w"), r["ratio_%s_w" % norm], md(norm + "_weighted_h"),
                md(norm + "_plain_h"), r["ratio_%s_h" % norm]))
    lines += ["", "| m x n | k | dnmf_weighted_column_div ms (min-max) | dnmf_beta_column_div ms (min-max) | ratio |", "|---|---|---|---|---|"]
    for r in rows:
        t = lambda key: "%.3f (%.3f-%.3f)" % (r[key]["median_ms"], r[key]["min_ms"], r[key]["max_ms"])          # noqa: E731
        lines.append("| %d x %d | %d | %s | %s | %.2f |" % (r["m"], r["n"], r["k"], t("coldiv_weighted"), t("coldiv_plain"), r["ratio_coldiv"]))
    print("\n".join(lines))
    for path, text in ((opt.md, "\n".join(lines) + "\n"), (opt.json, json.dumps({"rows": rows}, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
