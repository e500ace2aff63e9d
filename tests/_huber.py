"""`params.norm = 'huber'` (TEST INFRASTRUCTURE): a float64 numpy statement of the rule on the WHOLE matrix.  With S' = W H + eps (eps the
float32 machine epsilon) and P = 1 where |A - S'| <= delta, delta / |A - S'| elsewhere:
    W <- W * ((A P) H^T) / ((S' P) H^T + eps)      then, with the new W,      H <- H * (W^T (A P)) / (W^T (S' P) + eps)
    loss = sum rho(a - s'),   rho(r) = r^2 / 2 for |r| <= delta,   delta |r| - delta^2 / 2 otherwise"""
import traceback

import numpy as np

from tests import _is as I

EPS = I.EPS


def pair(A, W, H, side, delta, eps=EPS):
    """(num, den) in float64: m x k for side 'w', k x n for side 'h'"""
    A, W, H = (np.asarray(x, dtype=np.float64) for x in (A, W, H))
    S = W @ H + eps
    R = np.abs(A - S)
    P = np.where(R <= delta, 1.0, delta / np.where(R > 0, R, 1.0))
    return ((A * P) @ H.T, (S * P) @ H.T) if side == "w" else (W.T @ (A * P), W.T @ (S * P))


def step(A, W, H, delta, eps=EPS, W_update=True, clamp=False):
    """one step in float64 (new arrays): W first, then H with the new W, then the clamp of pyDNMF.py:170-172"""
    W, H = np.array(W, dtype=np.float64), np.array(H, dtype=np.float64)
    if W_update:
        num, den = pair(A, W, H, "w", delta, eps)
        W = W * num / (den + eps)
    num, den = pair(A, W, H, "h", delta, eps)
    H = H * num / (den + eps)
    return (np.maximum(W, eps), np.maximum(H, eps)) if clamp else (W, H)


def fit(A, W0, H0, delta, itr, eps=EPS, W_update=True):
    """PyNMF.fit under norm='huber': the steps, normalize_features (pyDNMF.py:185-194), the Frobenius relative error (:205-218)"""
    A, W, H = np.asarray(A, dtype=np.float64), W0, H0
    for i in range(itr):
        W, H = step(A, W, H, delta, eps, W_update, clamp=(i % 10 == 0))
    s = W.sum(axis=0)
    W, H = W / (s + eps), H * s[:, None]
    return W, H, float(np.linalg.norm(A - W @ H) / np.linalg.norm(A))


def loss(A, W, H, delta, eps=EPS):
    """(the loss, the sum of the magnitudes of its terms: r^2 / 2, or delta |r| and delta^2 / 2, the share of the entries with |r| > delta)"""
    R = np.abs(np.asarray(A, dtype=np.float64) - (np.asarray(W, dtype=np.float64) @ np.asarray(H, dtype=np.float64) + eps))
    d = np.where(R > delta, delta, 0.0)                             # (no inf * 0 at delta = inf)
    return tuple(float(x) for x in (np.where(R > delta, d * R - d * d / 2, R * R / 2).sum(), np.where(R > delta, d * R + d * d / 2, R * R / 2).sum(), np.mean(R > delta)))


def spiked(m, n, k, seed, share=0.02, height=50.0, noise=0.0):
    """(A, clean, W0, H0): a planted rank-k float32 block, `share` of its entries spikes of `height` to twice that times its mean"""
    rs = np.random.RandomState(seed)
    A = (rs.rand(m, k) + 0.1) @ (rs.rand(k, n) + 0.1) * (1.0 + noise * (rs.rand(m, n) - 0.5))
    hit = rs.rand(m, n) < share
    A = np.where(hit, A.mean() * height * (1.0 + rs.rand(m, n)), A).astype(np.float32)
    return A, ~hit, (rs.rand(m, k) + 0.05).astype(np.float32), (rs.rand(k, n) + 0.05).astype(np.float32)


GRID = dict(problem=dict(m=50, n=39, k=3, seed=5, share=0.05, height=20.0, noise=0.2), delta=0.5, itr=20)


def grid_rank(rank, world, port, grid, q):
    """this rank's slice of spiked(**GRID['problem']) on the GPU: the fits with W_update on and off, and each one's loss"""
    from pydnmfk_amd.dist_comm import MPI_comm
    from pydnmfk_amd.pyDNMF import PyNMF
    try:
        I._setup_rank(rank, world, port, True)
        A, _, W0, H0 = spiked(**GRID["problem"])
        sl, (w0, w1), (h0, h1) = I._slices(rank, grid, A.shape)
        out, comms = {}, MPI_comm(None, *grid)
        for wu in (True, False):
            args = I.args_for(comms, grid[0], grid[1], W0.shape[1], GRID["itr"], wu, norm="huber", delta=GRID["delta"])
            nmf = PyNMF(A[sl], factors=[W0[w0:w1], H0[:, h0:h1]], params=args)
            out[wu] = (slice(w0, w1), slice(h0, h1)) + tuple(np.asarray(x) for x in nmf.fit()) + (nmf.huber_loss(),)
        q.put((rank, out, None))
        I._teardown_rank(world)
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))
