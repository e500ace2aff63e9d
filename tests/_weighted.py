"""Per-entry weights, `params.weights` (TEST INFRASTRUCTURE): a float64 numpy statement on the WHOLE matrix.  With S = W H, S' = S + eps:
    (u_n, u_d) = (A, S) fro | (A / S', 1) kl | (A / S'^2, 1 / S') is | (A S'^(beta - 2), S'^(beta - 1)) beta,   both times V where V > 0, else 0
    X <- X * (num / (den + eps))^g, g = 1 (fro, kl), 1/2 (is), gamma(beta);   objective = sum v d(a | s'), half of v (a - s)^2 under fro
`WeightedOracleOps`: tests/_beta.py::BetaOracleOps plus the weighted operations of engine.HipOps, for the choreography on the CPU."""
import traceback

import numpy as np
import torch

from tests import _beta as B
from tests import _is as I
from tests._golden import rel_fro
from tests._ops_double import _n

EPS, EPS64 = I.EPS, float(np.finfo(np.float64).eps)
NORMS = (("fro", 0.0), ("kl", 0.0), ("is", 0.0), ("beta", 0.5), ("beta", 3.0))


def _power(norm, beta):
    return {"fro": 2.0, "kl": 1.0, "is": 0.0}.get(norm, beta)


def pair(A, V, W, H, side, norm, beta=0.0, eps=EPS):
    """(num, den) in float64: m x k for side 'w', k x n for side 'h'; A is not looked at where V is 0"""
    A, V, W, H = (np.asarray(x, dtype=np.float64) for x in (A, V, W, H))
    on = V > 0
    A = np.where(on, A, 1.0)
    S = W @ H
    Sp = S + eps
    Un, Ud = (A, S) if norm == "fro" else (A * Sp ** (_power(norm, beta) - 2.0), Sp ** (_power(norm, beta) - 1.0))
    Un, Ud = np.where(on, Un * V, 0.0), np.where(on, Ud * V, 0.0)
    return (Un @ H.T, Ud @ H.T) if side == "w" else (W.T @ Un, W.T @ Ud)


def rule(X, num, den, norm, beta=0.0, eps=EPS, clamp=False):
    g = 1.0 if norm == "fro" else B.gamma(_power(norm, beta))
    x = np.asarray(X, dtype=np.float64) * (np.asarray(num, dtype=np.float64) / (np.asarray(den, dtype=np.float64) + eps)) ** g
    return np.maximum(x, eps) if clamp else x


def step(A, V, W, H, norm, beta=0.0, eps=EPS, W_update=True, clamp=False):
    W, H = np.array(W, dtype=np.float64), np.array(H, dtype=np.float64)
    if W_update:
        W = rule(W, *pair(A, V, W, H, "w", norm, beta, eps), norm, beta, eps)
    H = rule(H, *pair(A, V, W, H, "h", norm, beta, eps), norm, beta, eps)
    if clamp:
        H, W = np.maximum(H, eps), np.maximum(W, eps)
    return W, H


def terms(A, V, W, H, norm, beta=0.0, eps=EPS):
    """the weighted terms of every element's objective (0 where V is 0): their sum is the objective"""
    A, V, W, H = (np.asarray(x, dtype=np.float64) for x in (A, V, W, H))
    on = V > 0
    A = np.where(on, A, 1.0)
    S = W @ H
    t = (0.5 * (A - S) ** 2,) if norm == "fro" else B.terms_of(A, S + eps, _power(norm, beta))
    return [np.where(on, V * x, 0.0) for x in t]


def objective(A, V, W, H, norm, beta=0.0, eps=EPS):
    return float(sum(t.sum() for t in terms(A, V, W, H, norm, beta, eps)))


def resid(A, V, W, H):
    """(sum v (a - s)^2, sum v a^2) over v > 0"""
    A, V, W, H = (np.asarray(x, dtype=np.float64) for x in (A, V, W, H))
    on = V > 0
    A = np.where(on, A, 0.0)
    return float(np.sum(np.where(on, V * (A - W @ H) ** 2, 0.0))), float(np.sum(V * A * A))


def fit(A, V, W0, H0, norm, beta, itr, eps=EPS, W_update=True):
    """PyNMF.fit under params.weights: the steps, normalize_features, the weighted relative error"""
    W, H = W0, H0
    for i in range(itr):
        W, H = step(A, V, W, H, norm, beta, eps, W_update, clamp=(i % 10 == 0))
    s = W.sum(axis=0)
    W, H = W / (s + eps), H * s[:, None]
    r = resid(A, V, W, H)
    return W, H, float(np.sqrt(r[0] / r[1]))


class WeightedOracleOps(B.BetaOracleOps):
    name = "oracle-weighted"
    weighted_dtypes = (torch.float32, torch.float64)

    def _pair(self, side, A, V, W, H, eps, norm, beta, buf):
        halves = self._halves(buf, tuple((W if side == "w" else H).shape))
        return [self._store(d, x) for d, x in zip(halves, pair(_n(A), _n(V), _n(W), _n(H), side, norm, beta, eps))]

    def weighted_aht_pair(self, *a):
        return self._pair("w", *a)

    def weighted_wta_pair(self, *a):
        return self._pair("h", *a)

    def weighted_ratio_update(self, X, num, den, eps, norm, beta, clamp=False):
        return self._store(X, rule(_n(X), _n(num), _n(den), norm, beta, eps, clamp))

    def weighted_update_w(self, A, V, W, H, eps, norm, beta):
        return self._store(W, rule(_n(W), *pair(_n(A), _n(V), _n(W), _n(H), "w", norm, beta, eps), norm, beta, eps))

    def weighted_update_h(self, A, V, W, H, eps, norm, beta, clamp=False):
        return self._store(H, rule(_n(H), *pair(_n(A), _n(V), _n(W), _n(H), "h", norm, beta, eps), norm, beta, eps, clamp))

    def weighted_resid_sqnorm(self, A, V, W, H):
        return torch.tensor(resid(_n(A), _n(V), _n(W), _n(H)), dtype=torch.float64)

    def weighted_divergence(self, A, V, W, H, eps, norm, beta):
        return torch.tensor([objective(_n(A), _n(V), _n(W), _n(H), norm, beta, eps)], dtype=torch.float64)


def weights(shape, seed, zero=0.3, pow2=False):
    """float32 weights in [0.25, 4) -- or powers of two 2^-3..2^3 --, a fraction `zero` of them 0"""
    rs = np.random.RandomState(seed)
    pos = 2.0 ** rs.randint(-3, 4, size=shape) if pow2 else 0.25 + 3.75 * rs.rand(*shape)
    return np.where(rs.rand(*shape) < zero, 0.0, pos).astype(np.float32)


def problem(m=50, n=39, k=3, seed=5, zero=0.3):
    """tests/_is.py::problem with weights(); NaN planted in A under the zero weights"""
    A, W0, H0, k = I.problem(m, n, k, seed)
    V = weights((m, n), seed + 7, zero).astype(np.float64)
    return np.where(V > 0, A, np.nan), V, W0, H0, k


def args(k, itr, norm, beta, **kw):
    return I.one_rank_args(k, itr, norm=norm, beta=beta, prune=kw.pop("prune", False), **kw)


def _grid_rank(rank, world, port, grid, q, use_hip, itr):
    """this rank's slice of problem(), every norm of NORMS: how far its factors, error and objective are from the whole-matrix float64
    statement (of the operands rounded to the rank's dtype), and the bytes of its replicated factor"""
    try:
        from pydnmfk_amd.dist_comm import MPI_comm
        from pydnmfk_amd.pyDNMF import PyNMF
        I._setup_rank(rank, world, port, use_hip)
        dt, eps = (np.float32, EPS) if use_hip else (np.float64, EPS64)
        A, V, W0, H0, k = problem()
        Ar, Wr0, Hr0 = (x.astype(dt).astype(np.float64) for x in (A, W0, H0))
        comms = MPI_comm(None, grid[0], grid[1])
        sl, (w0, w1), (h0, h1) = I._slices(rank, grid, A.shape)
        out = {}
        for norm, beta in NORMS:
            params = I.args_for(comms, grid[0], grid[1], k, itr, True, norm=norm, beta=beta, prune=False, weights=V[sl].astype(np.float32))
            nmf = PyNMF(A[sl].astype(dt), factors=[W0[w0:w1].astype(dt), H0[:, h0:h1].astype(dt)], params=params,
                        ops=None if use_hip else WeightedOracleOps())
            W, H, err = nmf.fit()
            Wr, Hr, err_r = fit(Ar, V, Wr0, Hr0, norm, beta, itr, eps)
            obj_r = objective(Ar, V, Wr, Hr, norm, beta, eps)
            assert W.dtype == dt
            out[(norm, beta)] = (rel_fro(W, Wr[w0:w1]), rel_fro(H, Hr[:, h0:h1]), abs(err - err_r) / err_r,
                                 abs(nmf.weighted_divergence() - obj_r) / obj_r, (W if grid[0] == 1 else H).tobytes())
        q.put((rank, out, None))
        I._teardown_rank(world)
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def run_grid(grid, use_hip=False, itr=20, timeout=240):
    """{(norm, beta): the largest (dW, dH, derr, dobjective) over the ranks}; the replicated factor is bit-identical on every rank"""
    res = I.spawn(_grid_rank, grid, (use_hip, itr), timeout)
    for key in res[0][1]:
        assert len({out[key][4] for _, out in res}) == 1, (grid, key)
    return {key: tuple(max(out[key][i] for _, out in res) for i in range(4)) for key in res[0][1]}
