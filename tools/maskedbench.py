"""ms per masked MU step on DENSE data whose missing entries are NaN (engine.HipMaskedOps, csrc/dnmf_masked.h), next to the two ways
the same data could be run before: the CSR masked step on the same observations (engine.HipCsrOps, missing='unstored') and the
unmasked dense KL step on the zero-filled matrix (the structural cousin: the same two products with one output).

    python tools/maskedbench.py [--json out.json]

One MI355X, 8192 x 4096, k = 32 and 64, 10 % / 50 % / 90 % observed, values uniform in [0.05, 1.05).  Every figure is the median
(min / max next to it) of --steps timed steps after --warmup steps, each step timed with its own pair of events; a step is one
`nmf_algorithms_1D(...).update()` on one rank (both factors, the fused endings).  Sanity condition (checked here, exit status 1):
at 50 % observed the dense masked step is not slower than the CSR masked step on the same data, for both norms and both ranks.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pydnmfk_amd.engine import HIP_CSR_OPS, HIP_MASKED_OPS, HIP_OPS  # noqa: E402
from pydnmfk_amd.masked import MaskedDenseBlock  # noqa: E402
from pydnmfk_amd.sparse import SparseBlock  # noqa: E402
from tools.sparsebench import _args, timed  # noqa: E402


def bench(m, n, k, observed, steps, warmup, seed=0):
    from pydnmfk_amd.dist_nmf import nmf_algorithms_1D
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    A = torch.rand(m, n, device=dev, generator=g) + 0.05
    mask = torch.rand(m, n, device=dev, generator=g) < observed
    An = torch.where(mask, A, torch.full_like(A, float("nan")))
    blk = MaskedDenseBlock(An)
    idx = mask.nonzero()
    csr = SparseBlock.from_coo(idx[:, 0], idx[:, 1], A[mask], (m, n), keep_zeros=True, missing="unstored")
    Az = torch.where(mask, A, torch.zeros_like(A))
    del A, mask, idx
    W, H = torch.rand(m, k, device=dev), torch.rand(k, n, device=dev)
    out = {"m": m, "n": n, "k": k, "observed": observed, "n_observed": blk.n_observed}
    assert csr.nnz == blk.n_observed
    for norm in ("fro", "kl"):
        a = _args(m, n, k, norm)
        for name, data, ops in (("masked_dense", blk, HIP_MASKED_OPS), ("csr_masked", csr, HIP_CSR_OPS)):
            W.uniform_(); H.uniform_()
            out["%s_%s" % (name, norm)] = timed(lambda: nmf_algorithms_1D(data, W, H, params=a, ops=ops).update(), steps, warmup)
    a = _args(m, n, k, "kl")
    W.uniform_(); H.uniform_()
    out["dense_kl_zero_filled"] = timed(lambda: nmf_algorithms_1D(Az, W, H, params=a, ops=HIP_OPS).update(), steps, warmup)
    for norm in ("fro", "kl"):
        out["ratio_dense_over_csr_" + norm] = out["masked_dense_" + norm]["median_ms"] / out["csr_masked_" + norm]["median_ms"]
        out["ratio_dense_over_unmasked_kl_" + norm] = out["masked_dense_" + norm]["median_ms"] / out["dense_kl_zero_filled"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    opt = ap.parse_args()
    torch.cuda.set_device(0)
    m, n = 8192, 4096
    rows = [bench(m, n, k, obs, opt.steps, opt.warmup) for k in (32, 64) for obs in (0.1, 0.5, 0.9)]
    print("| m x n | k | observed | masked dense FRO ms (min-max) | masked dense KL ms (min-max) | CSR masked FRO ms | CSR masked KL ms | "
          "unmasked dense KL ms (zero-filled) | dense / CSR (fro, kl) | dense / unmasked KL (fro, kl) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        t = lambda key: "%.3f (%.3f-%.3f)" % (r[key]["median_ms"], r[key]["min_ms"], r[key]["max_ms"])      # noqa: E731
        print("| %d x %d | %d | %.0f %% | %s | %s | %.3f | %.3f | %.3f | %.3f, %.3f | %.2f, %.2f |" % (
            r["m"], r["n"], r["k"], 100 * r["observed"], t("masked_dense_fro"), t("masked_dense_kl"), r["csr_masked_fro"]["median_ms"],
            r["csr_masked_kl"]["median_ms"], r["dense_kl_zero_filled"]["median_ms"], r["ratio_dense_over_csr_fro"], r["ratio_dense_over_csr_kl"],
            r["ratio_dense_over_unmasked_kl_fro"], r["ratio_dense_over_unmasked_kl_kl"]))
    half = [r for r in rows if r["observed"] == 0.5]
    ok = all(r["ratio_dense_over_csr_" + norm] <= 1.0 for r in half for norm in ("fro", "kl"))
    print("sanity (50 %% observed, %d x %d): masked dense / CSR masked step = %s -> %s" % (
        m, n, ", ".join("k=%d %s %.3f" % (r["k"], norm, r["ratio_dense_over_csr_" + norm]) for r in half for norm in ("fro", "kl")),
        "OK" if ok else "THE DENSE MASKED STEP IS SLOWER"))
    if opt.json:
        with open(opt.json, "w") as f:
            json.dump({"rows": rows, "sanity_ok": ok}, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
