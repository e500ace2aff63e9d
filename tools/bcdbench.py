"""ms per BCD iteration (method='bcd', the whole-fit call dnmf_bcd_fro_fit) next to the MU/FRO step on the same shape.

    python tools/bcdbench.py [--json out.json] [--quick]
    python tools/bcdbench.py --batch B --shape m,n,k [--json out.json]

Per iteration = (time of itr = 60 - time of itr = 10) / 50: the set-up of a fit (initial norms, scaling, the first A H^T) and its
end (normalisation, error) cancel.  Each figure is the median of --reps timed calls after one warm-up call.  Also reports whole-fit
times at the sizes of the reference's examples (t24x12, swim).  One GPU, float32 data, uniform [0, 1) A and factors.

--batch B: B same-shape device-resident problems through PyNMF.fit_batch (one batched library call) against the same B problems
fitted one after another (PyNMF.fit) in the same process; wall-clock time around each (both end with the host reading the errors),
differenced over the same two iteration counts, so what is reported is ms per iteration OF THE WHOLE BATCH.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pydnmfk_amd.engine import HIP_OPS  # noqa: E402


def time_fit(method, A, W0, H0, itr, reps):
    ops = HIP_OPS
    W, H = W0.clone(), H0.clone()
    ts = []
    for r in range(reps + 1):
        W.copy_(W0)
        H.copy_(H0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.fit(method, "fro", A, W, H, 1.1920929e-07, True, itr)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def per_iter(method, A, W0, H0, reps, lo=10, hi=60):
    return (time_fit(method, A, W0, H0, hi, reps) - time_fit(method, A, W0, H0, lo, reps)) / (hi - lo)


def _bcd_args(k, itr):
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.utils import parse
    comms = MPI_comm(None, 1, 1)
    args = parse()
    args.comm1, args.comm, args.p_r, args.p_c, args.k = comms.comm, comms, 1, 1, k
    args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
    args.itr, args.init, args.verbose, args.prune = itr, "rand", False, False
    args.norm, args.method, args.W_update = "fro", "bcd", True
    return args


def time_batch(probs, k, itr, reps, batched):
    """median wall-clock ms of fitting `probs` together (PyNMF.fit_batch) or one after another; the fits are set up outside the timer"""
    import time
    from pydnmfk_amd.pyDNMF import PyNMF
    ts = []
    for r in range(reps + 1):
        fits = [PyNMF(A, factors=[W0, H0], params=_bcd_args(k, itr)) for A, W0, H0 in probs]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if batched:
            PyNMF.fit_batch(fits)
        else:
            for f in fits:
                f.fit()
        torch.cuda.synchronize()
        if r:
            ts.append((time.perf_counter() - t0) * 1e3)
        del fits
    ts.sort()
    return ts[len(ts) // 2]


def batch_main(a):
    m, n, k = tuple(int(v) for v in a.shape.split(",")) if a.shape else (1024, 256, 4)
    B, lo, hi = a.batch, 10, 60
    probs = [(torch.rand(m, n, device="cuda"), torch.rand(m, k, device="cuda"), torch.rand(k, n, device="cuda")) for _ in range(B)]
    row = dict(shape=[m, n, k], batch=B)
    for name, batched in (("batched", True), ("single", False)):
        t_lo, t_hi = time_batch(probs, k, lo, a.reps, batched), time_batch(probs, k, hi, a.reps, batched)
        row["%s_ms_itr%d" % (name, lo)], row["%s_ms_itr%d" % (name, hi)] = round(t_lo, 3), round(t_hi, 3)
        row["%s_ms_per_iter" % name] = round((t_hi - t_lo) / (hi - lo), 4)
    row["speedup"] = round(row["single_ms_per_iter"] / row["batched_ms_per_iter"], 2)
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), batched=[row]), f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a smoke run)")
    ap.add_argument("--shape", default=None, help="m,n,k: this shape only, no fit sizes (for a profiler run)")
    ap.add_argument("--batch", type=int, default=0, help="B: time PyNMF.fit_batch of B problems of --shape against B single fits")
    a = ap.parse_args()
    if a.batch:
        return batch_main(a)
    torch.manual_seed(0)
    shapes = [(4096, 1024, 16)] if a.quick else [(262144, 8192, 64), (65536, 4096, 16), (65536, 4096, 32)]
    if a.shape:
        shapes = [tuple(int(v) for v in a.shape.split(","))]
    rows = []
    for m, n, k in shapes:
        A = torch.rand(m, n, device="cuda")
        W0, H0 = torch.rand(m, k, device="cuda"), torch.rand(k, n, device="cuda")
        bcd = per_iter("bcd", A, W0, H0, a.reps)
        mu = per_iter("mu", A, W0, H0, a.reps)
        gb = m * n * 4 / 1e9
        row = dict(shape=[m, n, k], bcd_ms_per_iter=round(bcd, 4), mu_fro_ms_per_step=round(mu, 4), ratio=round(bcd / mu, 3),
                   bcd_a_passes_tb_s=round(3 * gb / bcd, 3))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del A, W0, H0
        torch.cuda.empty_cache()
    fits = []
    for name, m, n, k, itr in () if a.shape else (("t24x12", 24, 12, 2, 2000), ("swim", 1024, 256, 4, 1000)):
        A = torch.rand(m, n, device="cuda")
        W0, H0 = torch.rand(m, k, device="cuda"), torch.rand(k, n, device="cuda")
        row = dict(fit=name, shape=[m, n, k], itr=itr, bcd_fit_ms=round(time_fit("bcd", A, W0, H0, itr, a.reps), 3),
                   mu_fro_fit_ms=round(time_fit("mu", A, W0, H0, itr, a.reps), 3))
        print(json.dumps(row), flush=True)
        fits.append(row)
    out = dict(device=torch.cuda.get_device_name(0), per_iteration=rows, fits=fits)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
