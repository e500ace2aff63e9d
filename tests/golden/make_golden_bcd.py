#!/opt/conda/bin/python3.9
"""Golden vectors of the BCD method (method='bcd', norm='fro'), captured from the UNMODIFIED reference.

Run in the build container only, like make_golden.py (whose partition helpers and reference imports it reuses):

    OMP_NUM_THREADS=1 /opt/conda/bin/python3.9 tests/golden/make_golden_bcd.py

Inputs are the existing tests/golden/data_<dataset>.npz (A, W0, H0), cast to float32.  For every case it captures, per rank:

  * `step<N>` : one bare `nmf_algorithms_{1D,2D}.update()` with params.itr = N (dist_nmf.py:66-83, :634-651 -> FRO_BCD_update
                runs N inner iterations, :474-579 / :967-1047), for N in (1, 2, 5, 10);
  * `fit<N>`  : `PyNMF.fit()` with itr = N (pyDNMF.py:151-152: ONE trip with i = itr - 1), W, H and the relative error, for
                N in (1, 11, 50) -- the clamp of pyDNMF.py:155/170 runs for 1 and 11, not for 50.
The low-rank cases (k = 64, 128) keep a subset of these (CASES below); meta lists what a file holds.

Files are named bcd_<dataset>_<grid>.npz, NOT case_*.npz: tests/_golden.case_names() globs case_* and the suites that
parametrize over it (and the oracle they compare with) know only MU / HALS.  Only data is written.
"""
import json
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402  (sets up the stand-in MPI and imports the reference)
from make_golden import MPI, MPI_comm, PyNMF, blk, factor_slices, nmf_algorithms_1D, nmf_algorithms_2D, parse  # noqa: E402

STEPS = (1, 2, 5, 10)
FITS = (1, 11, 50)


def run_case(dataset, grid, steps=STEPS, fits=FITS):
    d = np.load(os.path.join(HERE, "data_%s.npz" % dataset))
    A = np.ascontiguousarray(d["A"].astype(np.float32))
    W0, H0 = d["W0"].astype(np.float32), d["H0"].astype(np.float32)
    k = int(d["k"])
    m, n = A.shape
    p_r, p_c = grid

    def body(rank):
        comm = MPI.COMM_WORLD
        comms = MPI_comm(comm, p_r, p_c)
        out = {}

        def mkargs(itr):
            args = parse()
            args.size, args.rank, args.comm1, args.comm = comm.size, rank, comms.comm, comms
            args.p_r, args.p_c, args.k = p_r, p_c, k
            args.m, args.n = m, n
            args.itr, args.init = itr, "rand"
            args.row_comm, args.col_comm = comms.cart_1d_row(), comms.cart_1d_column()
            args.verbose, args.prune = False, False
            args.norm, args.method = "fro", "bcd"
            args.W_update = True
            return args

        (rs, cs), (re, ce) = blk(rank, (p_r, p_c), (m, n))
        A_ij = np.ascontiguousarray(A[rs:re + 1, cs:ce + 1])
        (w0, w1), (h0, h1) = factor_slices(rank, p_r, p_c, m, n)
        Wb, Hb = W0[w0:w1].copy(), H0[:, h0:h1].copy()
        out["A_range"] = np.array([rs, re + 1, cs, ce + 1])
        out["W_range"] = np.array([w0, w1])
        out["H_range"] = np.array([h0, h1])
        for N in steps:
            nmf = PyNMF(A_ij, factors=[Wb, Hb], params=mkargs(N))
            if nmf.topo == "2d":
                W1, H1 = nmf_algorithms_2D(nmf.A_ij, nmf.W_ij, nmf.H_ij, params=nmf.params).update()
            else:
                W1, H1 = nmf_algorithms_1D(nmf.A_ij, nmf.W_i, nmf.H_j, params=nmf.params).update()
            out["step%d_W" % N], out["step%d_H" % N] = np.array(W1), np.array(H1)
        out["eps"] = np.array(float(nmf.eps))
        for N in fits:
            Wf, Hf, err = PyNMF(A_ij, factors=[Wb, Hb], params=mkargs(N)).fit()
            out["fit%d_W" % N], out["fit%d_H" % N] = np.array(Wf), np.array(Hf)
            out["fit%d_err" % N] = np.array(float(err))
        return out

    res = MPI.run_ranks(p_r * p_c, body)
    flat = {}
    for r, o in enumerate(res):
        for key, v in o.items():
            flat["r%d_%s" % (r, key)] = v
    name = "%s_%dx%d" % (dataset, p_r, p_c)
    meta = dict(name=name, dataset=dataset, grid=[p_r, p_c], norm="fro", method="bcd", dtype="float32", steps=list(steps),
                itrs=list(fits), W_update=True, k=k, m=int(m), n=int(n), prune=False,
                out_dtypes={key: str(v.dtype) for key, v in res[0].items()},
                generator="reference lanl/pyDNMFk, python3.9, numpy %s (OpenBLAS, 1 thread), "
                          "mpi4py stand-in with rank-ordered sums" % np.__version__)
    flat["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "bcd_%s.npz" % name), **flat)
    print("%-24s err=%s  W %s H %s" % (name, {N: round(float(res[0]["fit%d_err" % N]), 7) for N in fits},
                                        res[0]["fit%d_W" % fits[0]].dtype, res[0]["fit%d_H" % fits[0]].dtype), flush=True)


# the low-rank MFMA-width cases keep fewer captures: their factors are incompressible floats (each file stays under 400 KB)
LR = dict(steps=(1, 10), fits=(11,))
CASES = [("t24x12", (1, 1), {}), ("t24x12", (1, 2), {}), ("t24x12", (2, 1), {}), ("t24x12", (2, 2), {}), ("r25x13", (3, 1), {}),
         ("swim", (1, 1), {}), ("lr200x136k64", (1, 1), LR), ("lr200x136k64", (1, 2), LR), ("lr150x140k128", (1, 1), dict(steps=(1,), fits=(11,)))]

if __name__ == "__main__":
    assert mg is not None
    only = sys.argv[1:]
    for ds, g, kw in CASES:
        if not only or "%s_%dx%d" % ((ds,) + g) in only:
            run_case(ds, g, **kw)
