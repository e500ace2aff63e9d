"""Helpers for the beta-divergence, `params.norm = 'beta'` with `params.beta` (TEST INFRASTRUCTURE, lives under tests/ only).

A float64 numpy statement of the rule on the WHOLE matrix.  With S' = W H + eps element-wise, eps the machine epsilon of the factors'
arithmetic (float32's in the fp32 path), P = S'^(beta - 2) and g = gamma(beta):

    W <- W * (((A P) H^T) / ((S' P) H^T + eps))^g      then, with the new W,      H <- H * ((W^T (A P)) / (W^T (S' P) + eps))^g
    g = 1 / (2 - beta) for beta < 1,   1 for 1 <= beta <= 2,   1 / (beta - 1) for beta > 2
    D_beta(A | S') = sum (a^beta + (beta - 1) s'^beta - beta a s'^(beta - 1)) / (beta (beta - 1))
    beta = 1: sum a log(a / s') - a + s' (s' where a = 0);     beta = 0: sum q - log q - 1, q = a / s'

`BetaOracleOps`: tests/_is.py::ISOracleOps plus the beta operations of engine.HipOps in numpy float64, so that the choreography
(dist_nmf.BETA_MU_update) runs on the CPU and under gloo, in float64 on float64 data (what lets a grid meet 1e-10: tests/_is.py).
`run_grid`: the ranks of a 1D grid as processes.  `exact`: the operands of tests/_is.py::exact with the answers at an integer beta.
"""
import traceback

import numpy as np
import torch

from tests import _exact as E
from tests import _is as I
from tests._ops_double import _n

EPS = I.EPS
BETA_RANGE = (-2.0, 4.0)
CPU_BETAS = (-1.0, 0.5, 1.0, 1.5, 3.0)                          # both gamma != 1 branches, gamma = 1 at its ends and inside
GPU_BETAS = (-2.0, -1.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0)          # the ends of the accepted range as well


# ---- the rule
def gamma(beta):
    return 1.0 / (2.0 - beta) if beta < 1 else (1.0 if beta <= 2 else 1.0 / (beta - 1.0))


def pair(A, W, H, side, beta, eps=EPS):
    """(num, den) in float64: m x k for side 'w', k x n for side 'h'"""
    A, W, H = (np.asarray(x, dtype=np.float64) for x in (A, W, H))
    S = W @ H + eps
    P = S ** (beta - 2.0)
    Un, Ud = A * P, S * P
    return (Un @ H.T, Ud @ H.T) if side == "w" else (W.T @ Un, W.T @ Ud)


def rule(X, num, den, beta, eps=EPS, clamp=False):
    x = np.asarray(X, dtype=np.float64) * (np.asarray(num, dtype=np.float64) / (np.asarray(den, dtype=np.float64) + eps)) ** gamma(beta)
    return np.maximum(x, eps) if clamp else x


def step(A, W, H, beta, eps=EPS, W_update=True, clamp=False):
    """one step in float64 (new arrays): W first, then H with the new W, then the clamp of pyDNMF.py:170-172"""
    W, H = np.array(W, dtype=np.float64), np.array(H, dtype=np.float64)
    if W_update:
        W = rule(W, *pair(A, W, H, "w", beta, eps), beta, eps)
    H = rule(H, *pair(A, W, H, "h", beta, eps), beta, eps)
    if clamp:
        H, W = np.maximum(H, eps), np.maximum(W, eps)
    return W, H


def iterate(A, W, H, beta, itr, eps=EPS, W_update=True):
    for i in range(itr):
        W, H = step(A, W, H, beta, eps, W_update, clamp=(i % 10 == 0))
    return W, H


def _terms(A, W, H, beta, eps):
    """the three terms of every element's divergence, already divided by beta (beta - 1): their sum is the divergence, the sum of
    their magnitudes is what its rounding error scales with"""
    return terms_of(A, np.asarray(W, dtype=np.float64) @ np.asarray(H, dtype=np.float64) + eps, beta)


def terms_of(A, S, beta):
    """the same three terms from the model values S = s' themselves (any shape)"""
    A, S = np.asarray(A, dtype=np.float64), np.asarray(S, dtype=np.float64)
    if beta == 1:
        pos = A > 0
        return np.where(pos, A * np.log(np.where(pos, A, 1.0) / S), 0.0), -A, S
    if beta == 0:
        q = A / S
        return q, -np.log(q), -np.ones_like(q)
    c = beta * (beta - 1.0)
    Ab = np.where(A > 0, np.where(A > 0, A, 1.0) ** beta, 0.0)                 # a^beta, 0 at a = 0 (beta > 0 there)
    return Ab / c, (beta - 1.0) * S ** beta / c, -beta * A * S ** (beta - 1.0) / c


def divergence(A, W, H, beta, eps=EPS):
    return float(sum(t.sum() for t in _terms(A, W, H, beta, eps)))


def divergence_scale(A, W, H, beta, eps=EPS):
    """sum (|a^beta| + |(beta - 1) s^beta| + |beta a s^(beta - 1)|) / |beta (beta - 1)| (the KL terms at beta = 1)"""
    return float(sum(np.abs(t).sum() for t in _terms(A, W, H, beta, eps)))


def fit(A, W0, H0, beta, itr, eps=EPS, W_update=True):
    """PyNMF.fit under norm='beta': the steps, normalize_features (pyDNMF.py:185-194), the Frobenius relative error (:205-218)"""
    A64 = np.asarray(A, dtype=np.float64)
    W, H = iterate(A64, W0, H0, beta, itr, eps, W_update)
    s = W.sum(axis=0)
    W = W / (s + eps)
    H = H * s[:, None]
    return W, H, float(np.linalg.norm(A64 - W @ H) / np.linalg.norm(A64))


# ---- the operator set
class BetaOracleOps(I.ISOracleOps):
    name = "oracle-beta"
    beta_dtypes = (torch.float32, torch.float64)

    def beta_aht_pair(self, A, W, H, eps, beta, buf):
        num, den = self._halves(buf, tuple(W.shape))
        a, b = pair(_n(A), _n(W), _n(H), "w", beta, eps)
        return self._store(num, a), self._store(den, b)

    def beta_wta_pair(self, A, W, H, eps, beta, buf):
        num, den = self._halves(buf, tuple(H.shape))
        a, b = pair(_n(A), _n(W), _n(H), "h", beta, eps)
        return self._store(num, a), self._store(den, b)

    def beta_ratio_update(self, X, num, den, eps, beta, clamp=False):
        return self._store(X, rule(_n(X), _n(num), _n(den), beta, eps, clamp))

    def beta_update_w(self, A, W, H, eps, beta):
        a, b = pair(_n(A), _n(W), _n(H), "w", beta, eps)
        return self.beta_ratio_update(W, torch.from_numpy(a), torch.from_numpy(b), eps, beta)

    def beta_update_h(self, A, W, H, eps, beta, clamp=False):
        a, b = pair(_n(A), _n(W), _n(H), "h", beta, eps)
        return self.beta_ratio_update(H, torch.from_numpy(a), torch.from_numpy(b), eps, beta, clamp)

    def beta_divergence(self, A, W, H, eps, beta):
        return torch.tensor([divergence(_n(A), _n(W), _n(H), beta, eps)], dtype=torch.float64)


# ---- problems
def problem(m=50, n=39, k=3, seed=5, zeros=0.0):
    """tests/_is.py::problem (strictly positive); `zeros`: that fraction of the entries of A set to 0 (legal data for beta > 0), no row
    or column wholly"""
    A, W0, H0, k = I.problem(m, n, k, seed)
    if zeros:
        rs = np.random.RandomState(seed + 101)
        A = np.where(rs.rand(m, n) < zeros, 0.0, A)
        assert (A > 0).any(axis=0).all() and (A > 0).any(axis=1).all() and (A == 0).sum() > 0.1 * A.size
    return A, W0, H0, k


def args_for(comms, p_r, p_c, k, itr, beta, W_update=True, **extra):
    return I.args_for(comms, p_r, p_c, k, itr, W_update, norm=extra.pop("norm", "beta"), beta=beta, **extra)


def one_rank_args(k, itr, beta, **kw):
    return I.one_rank_args(k, itr, norm=kw.pop("norm", "beta"), beta=beta, **kw)


GRID_ITR = 20
GRID_COMBOS = (True, False)                                  # W_update


def _grid_rank(rank, world, port, grid, q, use_hip, shape_k, betas):
    """this rank's slice of problem(): for every beta the GRID_ITR-step fits with W_update on and off, and each one's divergence"""
    try:
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        I._setup_rank(rank, world, port, use_hip)
        dt = np.float32 if use_hip else np.float64            # (the HIP kernels are float32; the checker set runs in float64)
        A, W0, H0, k = problem(*shape_k)
        comms = MPI_comm(None, grid[0], grid[1])
        sl, (w0, w1), (h0, h1) = I._slices(rank, grid, A.shape)
        out = {}
        for beta in betas:
            for wu in GRID_COMBOS:
                nmf = PyNMF(A[sl].astype(dt), factors=[W0[w0:w1].astype(dt), H0[:, h0:h1].astype(dt)],
                            params=args_for(comms, grid[0], grid[1], k, GRID_ITR, beta, wu), ops=None if use_hip else BetaOracleOps())
                assert nmf._ops().name == ("hip" if use_hip else "oracle-beta") and nmf.norm == "beta"
                W, H, err = nmf.fit()
                out[(beta, wu)] = ((w0, w1), (h0, h1), np.asarray(W), np.asarray(H), float(err), nmf.beta_divergence())
        q.put((rank, out, None))
        I._teardown_rank(world)
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def _bad_rank(rank, world, port, grid, q, use_hip, beta, value):
    """every rank's slice of problem() is fine but ONE entry of the last rank's, set to `value` (None: the data stay as they are, so
    the verdict is on `beta` alone): what each rank's PyNMF raises"""
    try:
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        I._setup_rank(rank, world, port, use_hip)
        A, W0, H0, k = problem()
        if value is not None:
            A[-1, -1] = value
        comms = MPI_comm(None, grid[0], grid[1])
        sl, (w0, w1), (h0, h1) = I._slices(rank, grid, A.shape)
        try:
            PyNMF(A[sl].astype(np.float32), factors=[W0[w0:w1].astype(np.float32), H0[:, h0:h1].astype(np.float32)],
                  params=args_for(comms, grid[0], grid[1], k, 3, beta), ops=None if use_hip else BetaOracleOps())
            got = (None, "")
        except Exception as ex:  # noqa: BLE001
            got = (type(ex).__name__, str(ex))
        q.put((rank, got, None))
        I._teardown_rank(world)
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_grid(grid, betas, use_hip=False, shape_k=(50, 39, 3), timeout=240):
    """{(beta, W_update): (W, H, err, divergence)} of the GRID_ITR-step fits of problem(*shape_k) on the grid, assembled from the ranks
    (a replicated factor, the error and the divergence must agree between the ranks bit for bit)"""
    res = I.spawn(_grid_rank, grid, (use_hip, shape_k, tuple(betas)), timeout)
    m, n, k = shape_k
    full = {}
    for key in res[0][1]:
        dt = res[0][1][key][2].dtype
        W, H = np.full((m, k), np.nan, dtype=dt), np.full((k, n), np.nan, dtype=dt)
        errs, divs = set(), set()
        for rank, out in res:
            (w0, w1), (h0, h1), Wr, Hr, err, div = out[key]
            for dst, src in ((W[w0:w1], Wr), (H[:, h0:h1], Hr)):
                assert np.isnan(dst).all() or np.array_equal(dst, src), (grid, key, rank)      # replicated: identical on every rank
                dst[...] = src
            errs.add(err)
            divs.add(div)
        assert len(errs) == 1 and len(divs) == 1 and np.isfinite(W).all() and np.isfinite(H).all(), (grid, key, errs, divs)
        full[key] = (W, H, errs.pop(), divs.pop())
    return full


def reference_fits(betas, shape_k=(50, 39, 3), eps=EPS, dtype=np.float64):
    """the whole-matrix float64 fits of problem(*shape_k), its arrays first rounded to `dtype` (float32: what the HIP ranks are
    handed): {(beta, W_update): (W, H, err, divergence, divergence_scale)}"""
    A, W0, H0, k = problem(*shape_k)
    A, W0, H0 = (x.astype(dtype).astype(np.float64) for x in (A, W0, H0))
    out = {}
    for beta in betas:
        for wu in GRID_COMBOS:
            W, H, err = fit(A, W0, H0, beta, GRID_ITR, eps, wu)
            out[(beta, wu)] = (W, H, err, divergence(A, W, H, beta, eps), divergence_scale(A, W, H, beta, eps))
    return out


# ---- exact operands: tests/_is.py::exact (every S = W H a power of two in [2, 32] that absorbs eps, A in 1..7, H = 2^(1..3), W one
# power of two 2^(0..2) per row) with the answers at an INTEGER beta: P = S^(beta - 2) is a power of two, A P and S P are exact, and all
# terms are non-negative -- every partial sum in every order is exact when the total stays below 2^24 of its unit (asserted).  At beta = 2
# P = 1, so the kernel's exp2(0 * log2 S) is exp2 of an exact zero, whatever log2 returns
def exact(m, n, k, beta):
    assert beta == int(beta)
    A, W, H, _ = I.exact_problem(m, n, k)
    A64, W64, H64 = (x.astype(np.float64) for x in (A, W, H))
    S = W64 @ H64
    P = S ** (beta - 2.0)
    Un, Ud = A64 * P, S * P
    ref = {"w": (Un @ H64.T, Ud @ H64.T), "h": (W64.T @ Un, W64.T @ Ud)}
    e = beta - 2.0
    un = 2.0 ** (5 * e if e < 0 else e)                                    # the smallest P: 32^e (e < 0) or 2^e
    ud = un * 2.0                                                          # S >= 2
    for side in ("w", "h"):
        E._bound(ref[side][0], un, np.float32, "beta %g num, side %s" % (beta, side))
        E._bound(ref[side][1], ud, np.float32, "beta %g den, side %s" % (beta, side))
        for x, unit in zip(ref[side], (un, ud)):
            assert np.array_equal(x / unit, np.round(x / unit)) and np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return A, W, H, ref


_EXACT = {}


def exact_problem(m, n, k, beta):
    """exact(m, n, k, beta), built once per process and shared: no test writes to it"""
    if (m, n, k, beta) not in _EXACT:
        _EXACT[(m, n, k, beta)] = exact(m, n, k, beta)
    return _EXACT[(m, n, k, beta)]
