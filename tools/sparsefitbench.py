"""Sparse MU fits three ways on the same data and the SAME build: the Python step loop (`params.fit_loop = 'python'`: what every sparse
fit ran before the whole-fit entry point), whole-fit library calls one by one (dnmf_csr_mu_fit_batch with batch = 1), and ONE batched
call over the shared pattern (PyNMF.fit_batch; csrc/dnmf_csr_batch.h).

    python tools/sparsefitbench.py [--md out.md] [--json out.json] [--reps 5] [--sizes small,large] [--norm fro]

One MI355X.  Sizes: small = 2000 x 1500 at 2 % density, 100 steps; large = 2^20 x 2^16 with 5 10^7 uniformly placed entries (the shape of
tests/test_gpu_sparse.py::test_beyond_dense), 5 steps.  Problem counts 1 and 20 (copies of the block with values of their own:
SparseBlock.with_values, as an NMFk sweep makes them), k = 3, 16, 64.  The three paths alternate, `--reps` times after one untimed round
of each; a time is the host clock around the fits and a device synchronise, PyNMF objects are built outside it; the figures are medians
(min - max) in ms PER PROBLEM.  Before the timing the three paths' factors are compared once (they must be equal bit for bit).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pydnmfk_amd.pyDNMF import PyNMF  # noqa: E402
from pydnmfk_amd.sparse import SparseBlock, alloc_value_stacks  # noqa: E402

SIZES = {"small": (2000, 1500, 60_000, 100), "large": (2 ** 20, 2 ** 16, 50_000_000, 5)}      # m, n, entries drawn, steps
KS, BATCHES = (3, 16, 64), (1, 20)
PATHS = ("python", "whole", "batched")


def _block(m, n, nnz, dev, g):
    rows = torch.randint(0, m, (nnz,), device=dev, generator=g, dtype=torch.int32)
    cols = torch.randint(0, n, (nnz,), device=dev, generator=g, dtype=torch.int32)
    return SparseBlock.from_coo(rows, cols, torch.rand(nnz, device=dev, generator=g) + 0.05, (m, n))


def _copies(blk, B, g):
    """B blocks with blk's pattern and values of their own, held as rows of two value stacks"""
    val, t_val = alloc_value_stacks(B, blk.nnz, blk.device)
    perm = blk.transpose_perm()
    out = []
    for b in range(B):
        val[b].copy_(blk.val * (1.0 + 0.06 * torch.rand(blk.nnz, device=blk.device, generator=g)))
        torch.index_select(val[b], 0, perm, out=t_val[b])
        out.append(blk.with_values(val[b], t_val[b]))
    return out


def _params(k, itr, norm, loop):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.utils import parse
    comms = MPI_comm(None, 1, 1)
    args = parse()
    args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, 1, 1, k
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    args.itr, args.init, args.verbose, args.prune = itr, "rand", False, False
    args.norm, args.method, args.W_update = norm, "mu", True
    if loop:
        args.fit_loop = loop
    return args


def _stats(ts, per):
    ts = sorted(t / per for t in ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def bench(size, blocks, k, batch, itr, norm, reps, g):
    m, n = blocks[0].shape
    dev = blocks[0].device
    W0 = [torch.rand(m, k, device=dev, generator=g) + 0.01 for _ in range(batch)]
    H0 = [torch.rand(k, n, device=dev, generator=g) + 0.01 for _ in range(batch)]

    def run(path):
        args = _params(k, itr, norm, "python" if path == "python" else None)
        fits = [PyNMF(blocks[b], factors=[W0[b], H0[b]], params=args) for b in range(batch)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = PyNMF.fit_batch(fits) if path == "batched" else [f.fit() for f in fits]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res
    first = {p: run(p)[1] for p in PATHS}                                      # untimed round; the three paths' bits
    same = all(torch.equal(first[p][b][0], first["python"][b][0]) and torch.equal(first[p][b][1], first["python"][b][1])
               for p in PATHS for b in range(batch))
    ts = {p: [] for p in PATHS}
    for _ in range(reps):
        for p in PATHS:
            ts[p].append(run(p)[0])
    out = {"size": size, "m": m, "n": n, "nnz": blocks[0].nnz, "k": k, "batch": batch, "itr": itr, "bit_equal": same}
    out.update({p: _stats(v, batch) for p, v in ts.items()})
    out["python_over_batched"] = out["python"]["median_ms"] / out["batched"]["median_ms"]
    out["whole_over_batched"] = out["whole"]["median_ms"] / out["batched"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="small,large")
    ap.add_argument("--norm", default="fro")
    opt = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rows = []
    for size in opt.sizes.split(","):
        m, n, nnz, itr = SIZES[size]
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        blocks = _copies(_block(m, n, nnz, dev, g), max(BATCHES), g)
        for k in KS:
            for batch in BATCHES:
                rows.append(bench(size, blocks, k, batch, itr, opt.norm, opt.reps, g))
                print(json.dumps(rows[-1]), flush=True)
        del blocks
        torch.cuda.empty_cache()
    t = lambda s: "%.3f (%.3f - %.3f)" % (s["median_ms"], s["min_ms"], s["max_ms"])      # noqa: E731
    lines = ["norm='%s', method='mu'; ms per problem, median (min - max) of %d alternating runs" % (opt.norm, opt.reps), "",
             "| size | m x n | stored | steps | k | problems | step loop | whole fits one by one | one batched call | step loop / batched | "
             "one by one / batched | same bits |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    lines += ["| %s | %d x %d | %d | %d | %d | %d | %s | %s | %s | %.2f | %.2f | %s |" % (
        r["size"], r["m"], r["n"], r["nnz"], r["itr"], r["k"], r["batch"], t(r["python"]), t(r["whole"]), t(r["batched"]),
        r["python_over_batched"], r["whole_over_batched"], "yes" if r["bit_equal"] else "NO") for r in rows]
    text = "\n".join(lines)
    print(text)
    for path, body in ((opt.md, text + "\n"), (opt.json, json.dumps(rows, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(body)
    return 0


if __name__ == "__main__":
    sys.exit(main())
