"""NMFk: estimate the number of latent features k by NMF over perturbed copies of the data, custom clustering,
silhouettes and a Wilcoxon test on the regression errors -- drop-in for reference pyDNMFk/pyDNMFk.py
(`sample` :8-67, `PyNMFk` :70-299).  This is the main production CALLER of the MU hot path (20 x (k range) `PyNMF.fit`
calls); everything numeric inside `PyNMF` runs in libdnmf_hip.so, the logic here is host control.

    nopt = PyNMFk(A_ij, factors=None, params=args).fit()

Same `params` contract as the reference (`fpath`, `fname`, `start_k`/`end_k` or `k_range`, `step_k`, `perturbations`,
`noise_var`, `sampling`, `sill_thr`, `checkpoint`, `results_path`; defaults via var_init, pyDNMFk.py:143-164).
Differences: statistics are kept in memory for the p-value analysis (and written per k as the reference does; HDF5 when
h5py exists, else npz); no plots are drawn (plot_results is out of scope).  `params.hall_layout = 'aligned'` (not the
default) stacks the perturbations' H matrices as Hall[:, :, p] = H_p; the default 'reference' reproduces the reference's
vstack + C-order reshape (pyDNMFk.py:236-237), whose fibres mix perturbations -- it only seeds the regression fit.
Sparse input is swept as a SparseBlock (`SparseSweep`); dense float32 input with `params.missing = 'nan'` is swept as it is, NaN = not
observed: the raw array is kept, every perturbed copy keeps its NaNs, and the per-column error runs over the observed positions.
`params.norm = 'is'` (strictly positive dense float32 data, 'uniform' sampling -- multiplicative noise, the noise the Itakura-Saito
divergence is the likelihood of --, what PyNMF refuses under the norm is refused at construction): the per-column statistic `L_err` is
the mean divergence per entry of each column (PyNMF.is_column_divergence) instead of the scale-dependent Frobenius column error, and the
statistics gain 'is_div' (per perturbation) and 'avgDiv'; recon_err, avgErr and AIC keep their Frobenius definitions.
`params.norm = 'beta'` with `params.beta` in [-2, 4] is swept likewise (beta = 0 IS norm='is' and takes that path): data strictly positive
for beta <= 0 and non-negative for beta > 0, checked once; 'poisson' sampling for beta > 0 only; `L_err` is the divergence of each column
over the column's sum of a^beta (PyNMF.beta_column_divergence: scale-invariant for every beta; the Itakura-Saito statistic at beta = 0,
half the squared Frobenius column error at beta = 2); the statistics gain 'beta_div' (per perturbation), 'avgDiv' and 'beta'.
"""
import os

import numpy as np
import torch
from scipy.stats import wilcoxon

from .data_io import data_write
from .dist_clustering import custom_clustering
from .pyDNMF import PyNMF
from .utils import Checkpoint, var_init


class sample:
    """Perturbed copy of the data (pyDNMFk.py:8-67).  'uniform': X * (1 + nv + 2 nv U[0,1)) element-wise (:42-44);
    'poisson': Poisson(X) (:47-49).  numpy input uses the process-global numpy RNG seeded with `seed`, i.e. the
    reference's exact stream (and the `PyNMF` rand init that follows continues that stream, as in the reference);
    CUDA tensors are perturbed on the device with a torch generator seeded the same way (same distribution,
    different stream).

    A NaN-marked array (`missing='nan'`): a NaN entry stays NaN and an observed entry gets exactly the value the zero-filled array
    gets.  'uniform' needs nothing for that -- the multiplication keeps NaN, on the host and in dnmf_perturb_uniform (both of its
    kernels only multiply) --; 'poisson' draws from the zero-filled rates and puts NaN back, so no NaN rate reaches a generator, the
    generators are consumed as on the dense path, and a draw of 0 at an observed position is an observed zero."""

    def __init__(self, data, noise_var, method, seed=None, out=None, sparse=None, missing=None):
        self.X = data
        self.missing = missing
        self.out = out          # optional destination of the perturbed copy (a slice of the stack an NMFk batch is fitted from)
        # a SparseBlock: what the sweep keeps about it between the perturbations (SparseSweep; built here when the caller has none)
        self.sparse = sparse if sparse is not None or not getattr(data, "is_sparse_block", False) else SparseSweep(data)
        self.noise_var = noise_var
        self.seed = seed
        if self.seed is not None:
            np.random.seed(self.seed)
        self.method = method
        self.X_per = 0

    def randM(self):
        nv = self.noise_var
        if self.sparse is not None:
            self.X_per = self.sparse.uniform(nv, self.seed)
            return
        if isinstance(self.X, torch.Tensor):
            if self.X.is_cuda:      # one fused pass with a counter-based generator (dnmf_perturb_uniform): 1 GB of traffic per fit at
                from .engine import HIP_OPS        # 65536 x 4096 bf16 where the torch expression below moves about 9 GB
                out = HIP_OPS.perturb_uniform(self.X, nv, 0 if self.seed is None else int(self.seed), out=self.out)
                if out is not None:
                    self.X_per = out
                    return
            g = torch.Generator(device=self.X.device)
            g.manual_seed(0 if self.seed is None else int(self.seed))
            M = torch.rand(self.X.shape, dtype=torch.float32, device=self.X.device, generator=g)
            self.X_per = (self.X * (2 * nv * M + nv + 1)).to(self.X.dtype)   # bf16 storage: perturb in fp32, round once
        else:
            M = 2 * nv * np.random.random_sample(self.X.shape).astype(self.X.dtype) + nv
            self.X_per = np.multiply(self.X, M + 1)

    def poisson(self):
        if self.sparse is not None:
            self.X_per = self.sparse.poisson(self.seed)
            return
        nan = self.missing == "nan"
        if isinstance(self.X, torch.Tensor):
            g = torch.Generator(device=self.X.device)
            g.manual_seed(0 if self.seed is None else int(self.seed))
            gaps = torch.isnan(self.X) if nan else None
            rates = torch.where(gaps, torch.zeros_like(self.X), self.X) if nan else self.X
            self.X_per = torch.poisson(rates.float(), generator=g).to(self.X.dtype)
            if nan:
                self.X_per[gaps] = float("nan")
        elif nan:
            gaps = np.isnan(self.X)
            self.X_per = np.random.poisson(np.where(gaps, 0, self.X)).astype(self.X.dtype)
            self.X_per[gaps] = np.nan
        else:
            self.X_per = np.random.poisson(self.X).astype(self.X.dtype)

    def fit(self):
        if self.method == 'uniform':
            self.randM()
        elif self.method == 'poisson':
            self.poisson()
        return self.X_per


def host_uniform_values(crow, col, val, shape, nv, chunk_rows=None):
    """The reference's perturbation (pyDNMFk.py:42-44) of a CSR block from the process-global numpy stream: the values of
    np.multiply(dense, M + 1), M = 2 nv random_sample(dense.shape).astype(float32) + nv, at the stored positions.  The uniforms are
    drawn over the DENSE shape, `chunk_rows` rows at a time (random_sample fills row-major, so chunking by rows leaves the stream
    as it is), and only the draws at stored positions are kept: O(m n) time, O(chunk_rows n) memory, and the generator ends in
    the state the dense path leaves it in.  `crow`, `col`, `val`: numpy CSR arrays (columns in any order inside a row)."""
    m, n = int(shape[0]), int(shape[1])
    chunk_rows = int(chunk_rows) if chunk_rows else max(1, (1 << 22) // n)            # about 4 M draws (32 MB of float64) at a time
    out = np.empty_like(val)
    for r0 in range(0, m, chunk_rows):
        r1 = min(m, r0 + chunk_rows)
        M = 2 * nv * np.random.random_sample((r1 - r0, n)).astype(val.dtype) + nv
        p0, p1 = int(crow[r0]), int(crow[r1])
        rows = np.repeat(np.arange(r1 - r0), np.diff(crow[r0:r1 + 1]))
        out[p0:p1] = np.multiply(val[p0:p1], M[rows, col[p0:p1]] + 1)
    return out


class SparseSweep:
    """What an NMFk sweep over a SparseBlock keeps between its perturbations: the block, the permutation that carries the values
    from the block's image to the transpose's (computed once, not kept on every block) and, for numpy I/O, the host copy of the
    CSR arrays.  A perturbed copy is `block.with_values(...)`: it shares the pattern -- index arrays, long-row lists -- with the
    source, so `prune=True` sees the source's all-empty rows / columns in every copy.

    uniform: a block on the GPU that did not come from numpy I/O takes the keyed kernel (`ops.perturb_uniform`: the dense device
    path's values at the stored positions, bit for bit).  numpy I/O (scipy input) and CPU blocks reproduce the reference's numpy
    stream (host_uniform_values: O(m n) time on the host, O(chunk n) memory -- device input is the path that scales); PyNMF's rand
    init then continues that stream, as for dense numpy input.
    poisson: torch.poisson on the stored values with a generator seeded per perturbation; Poisson(0) = 0, so unstored zeros stay
    zero, and a draw of 0 stays stored and contributes zero."""

    def __init__(self, blk, numpy_io=False, ops=None):
        self.blk, self.numpy_io, self.ops = blk, numpy_io, ops
        self._perm = self._host = None

    @property
    def perm(self):
        if self._perm is None:
            self._perm = self.blk.transpose_perm()
        return self._perm

    def _with(self, val):
        return self.blk.with_values(val, val[self.perm])

    def uniform(self, nv, seed):
        blk = self.blk
        if blk.device.type == "cuda" and not self.numpy_io:
            ops = self.ops
            if ops is None:
                from .engine import HIP_CSR_OPS as ops
            return ops.perturb_uniform(blk, nv, 0 if seed is None else int(seed))
        if self._host is None:
            self._host = tuple(t.cpu().numpy() for t in (blk.crow, blk.col, blk.val))
        val = host_uniform_values(*self._host, blk.shape, nv)
        return self._with(torch.from_numpy(val).to(blk.device))

    def poisson(self, seed):
        g = torch.Generator(device=self.blk.device)
        g.manual_seed(0 if seed is None else int(seed))
        return self._with(torch.poisson(self.blk.val, generator=g))


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


class PyNMFk:
    """pyDNMFk.py:70-299."""

    def __init__(self, A_ij, factors=None, params=None, ops=None):
        from .sparse import is_sparse_input
        self._sparse = is_sparse_input(A_ij)
        self._is = str(getattr(params, "norm", None)).lower() in ("is", "itakura-saito")
        self._beta, self.beta = str(getattr(params, "norm", None)).lower() == "beta", None
        for norm in ("beta", "is"):         # ('beta' first: beta = 0 IS Itakura-Saito and is then held to that norm's check as well)
            if not (self._beta if norm == "beta" else self._is):
                continue
            # first of all: the sweep asks one operation beyond a fit, the per-column divergence (under norm='beta' with the column's sum
            # of a^beta).  (The 'uniform' perturbation is multiplicative noise, which is the noise the Itakura-Saito divergence is the
            # likelihood of, and keeps positive data positive)
            if ops is None:
                from .engine import HIP_OPS as opset
            else:
                opset = ops
            if not (getattr(opset, norm + "_nmfk", False) and hasattr(opset, norm + "_column_div")):
                raise NotImplementedError("PyNMFk with norm='%s' is not provided by operator set %r: rank estimation under %s needs a "
                                          "per-column divergence (PyNMF factorises at a given k)"
                                          % (norm, getattr(opset, "name", type(opset).__name__),
                                             "a beta-divergence" if norm == "beta" else "the Itakura-Saito objective"))
            if norm == "beta":
                self.beta = PyNMF._beta_value(params)
                # renamed, as PyNMF renames it, and swept on that path unchanged
                self._is, self._beta = self.beta == 0.0, self.beta != 0.0
            params.norm = 'is' if self._is else 'beta'
        self._masked = getattr(params, "missing", None) == "nan" and not self._sparse
        if self._masked and not (self._is or self._beta):           # (norm='is' and norm='beta' refuse missing= and sparse data by name in their setup)
            # as for a sparse block, the sweep touches A outside PyNMF.fit in the perturbed copy (NaN stays NaN through the
            # multiplication) and in the per-column error, which must run over the observed positions
            if ops is None:
                from .engine import HIP_MASKED_OPS as opset
            else:
                opset = ops
            if not (getattr(opset, "masked_nmfk", False) and hasattr(opset, "column_err_sums")):
                raise NotImplementedError("PyNMFk with missing='nan' is not provided by operator set %r: rank estimation over NaN-marked "
                                          "data needs a masked per-column error (PyNMF factorises such data at a given k)"
                                          % (getattr(opset, "name", type(opset).__name__),))
        if self._sparse and not (self._is or self._beta):
            # the sweep touches A outside PyNMF.fit in two operations: the perturbed copy and the per-column error
            if ops is None:
                from .engine import HIP_CSR_OPS as opset
            else:
                opset = ops
            if not (getattr(opset, "sparse_nmfk", False) and hasattr(opset, "column_err_sums")):
                raise NotImplementedError("PyNMFk on sparse data is not provided by operator set %r: it has no per-column error and no "
                                          "perturbed copy of a sparse block (PyNMF factorises sparse data at a given k)"
                                          % (getattr(opset, "name", type(opset).__name__),))
        self.A_ij = A_ij
        self.ops = ops
        self.local_m, self.local_n = self.A_ij.shape
        # `params.nmfk_split`: how a job of N ranks shares an NMFk sweep.  'data' (default) = the reference: X is cut into the
        # blocks of a p_r x p_c grid and every fit runs on all ranks (pyDNMFk.py:218-258).  'perturbations' = every rank
        # holds the WHOLE X (288 GB of HBM per MI355X) and fits the perturbations p = rank, rank + N, ... as one-rank problems
        # -- no exchange inside a fit; the factors then meet on every rank for the clustering (dist_clustering.py:84-160), the
        # regression fit and the statistics, which every rank evaluates on the full stacks: the numbers are those of the
        # 1 x 1 run, N times sooner through the fits.
        self.split = var_init(params, 'nmfk_split', default='data')
        if self.split not in ('data', 'perturbations'):
            raise ValueError("params.nmfk_split = %r: 'data' or 'perturbations'" % (self.split,))
        self.world = params.comm1
        if self.split == 'perturbations' and self.world.size > 1:
            import copy
            from .dist_comm import SoloGrid
            solo = SoloGrid(self.world.world_rank)
            params = copy.copy(params)          # the fits' own bag: one-rank communicators, a 1 x 1 grid
            params.comm1, params.comm, params.row_comm, params.col_comm = solo.comm, solo, solo.cart_1d_row(), solo.cart_1d_column()
            params.p_r = params.p_c = 1
            if "grid" in vars(params) and params.grid:
                params.grid = [1, 1]
            for stale in ("_native_comm", "exchange"):
                if hasattr(params, stale):
                    delattr(params, stale)
        self.params = params
        self.comm1 = self.params.comm1
        self.rank = self.world.rank
        if "grid" in vars(self.params) and self.params.grid:
            self.p_r, self.p_c = self.params.grid[0], self.params.grid[1]
        else:
            self.p_r, self.p_c = self.params.p_r, self.params.p_c
        self.fname = self.params.fname
        self.p = self.p_r * self.p_c
        self.topo = '2d' if (self.p_r != 1 and self.p_c != 1) else '1d'
        self.sampling = var_init(self.params, 'sampling', default='uniform')
        self.perturbations = var_init(self.params, 'perturbations', default=20)
        self.noise_var = var_init(self.params, 'noise_var', default=.03)
        self.step_k = var_init(self.params, 'step_k', default=1)
        if "k_range" in vars(self.params) and getattr(self.params, "grid", None):
            self.start_k, self.end_k = self.params.k_range[0], self.params.k_range[1]
        else:
            self.start_k, self.end_k = self.params.start_k, self.params.end_k
        self.first_k = self.start_k
        # how the P factor matrices H are stacked for the clustering / median (see pynmfk_per_k): 'reference' (default)
        # or 'aligned' (the layout the reference's comments describe)
        self.hall_layout = var_init(self.params, 'hall_layout', default='reference')
        self.sill_thr = var_init(params, 'sill_thr', default=0.9)
        self.verbose = var_init(params, 'verbose', default=False)
        self.params.checkpoint = var_init(params, 'checkpoint', default=True)
        self.params.rank = self.rank
        self.params.flag = 0   # 1: all perturbations factorised, 2: clustered, 3: results saved (pyDNMFk.py:165)
        self.cp = Checkpoint(checkpoint_save=self.params.checkpoint, params=self.params)
        self.stats = {}        # k -> cluster statistics (also written to disk per k)
        self.sweep = None
        if self._is or self._beta:
            self._div_setup(A_ij)           # (first: sparse data and missing= are refused in the norm's words)
        if self._sparse:
            self._sparse_setup(A_ij)
        if self._masked:
            self._masked_setup(A_ij)

    def _div_setup(self, A_ij):
        """norm='is' and norm='beta' (beta != 0): what PyNMF refuses under the norm is refused here, at construction, in its words (the
        sweep's largest rank stands for k), and the data's sign is checked ONCE, before the first fit -- strictly positive under 'is' and
        for beta <= 0, non-negative for beta > 0; the ranks agree on the verdict before any of them raises.  The 'uniform' perturbation
        keeps either property (1 + nv + 2 nv U > 0).  'poisson' sampling is refused where a draw of 0 makes the divergence infinite:
        under 'is' and for beta <= 0; for beta > 0 a zero is legal data and the sampling is allowed."""
        from .pyDNMF import storage_dtype
        params, beta = self.params, (self.beta if self._beta else None)
        a_dtype = torch.float32 if self._sparse else storage_dtype(A_ij, params)
        PyNMF._div_refusals('beta' if self._beta else 'is', params, self._sparse, getattr(params, "missing", None), a_dtype, self.ops,
                            var_init(params, 'method', default='mu'), self.p_r, self.p_c, int(self.end_k))
        if self.sampling == 'poisson' and beta is None:
            raise NotImplementedError("PyNMFk with norm='is' and sampling='poisson' is not provided: a Poisson draw of 0 makes the "
                                      "Itakura-Saito divergence infinite (sampling='uniform', multiplicative noise, keeps the data positive)")
        if self.sampling == 'poisson' and beta <= 0.0:
            raise NotImplementedError("PyNMFk with norm='beta', beta = %g and sampling='poisson' is not provided: a Poisson draw of 0 makes "
                                      "the divergence infinite for beta <= 0 (sampling='uniform', multiplicative noise, keeps the data "
                                      "positive; 'poisson' is accepted for beta > 0)" % beta)
        if self.ops is None:
            if isinstance(A_ij, torch.Tensor) and not A_ij.is_cuda:
                raise TypeError("PyNMFk: A_ij is a CPU tensor; pass a CUDA tensor or a numpy array (no CPU fallback)")
            if not torch.cuda.is_available():
                raise RuntimeError("PyNMFk: no GPU visible; the MI355X engine has no CPU fallback")
        PyNMF._sign_check(beta, float(A_ij.min()) if int(np.prod(A_ij.shape)) else 1.0, self.comm1, self.p)

    def _masked_setup(self, A_ij):
        """missing='nan': the raw array stays `self.A_ij` (every PyNMF wraps its perturbed copy in a MaskedDenseBlock itself); what PyNMF
        refuses under missing='nan' is refused here, at construction, in its words."""
        PyNMF._missing_checks(A_ij, self.params, False)          # method, storage and data type, gemm, 2D grid, nnsvd
        if var_init(self.params, 'prune', default=True):
            raise NotImplementedError("missing='nan' with prune=True is not provided (pruning drops all-ZERO rows and columns; under "
                                      "missing='nan' a row without an observation keeps its place and its factor row goes to zero): set "
                                      "params.prune = False")
        if int(self.end_k) > 128:
            raise NotImplementedError("missing='nan' with k = %d is not provided: the masked dense kernels serve 1 <= k <= 128" % int(self.end_k))
        if self.ops is None:
            if isinstance(A_ij, torch.Tensor) and not A_ij.is_cuda:
                raise TypeError("PyNMFk: A_ij is a CPU tensor; pass a CUDA tensor or a numpy array (no CPU fallback)")
            if not torch.cuda.is_available():
                raise RuntimeError("PyNMFk: no GPU visible; the MI355X engine has no CPU fallback")

    def _sparse_setup(self, A_ij):
        """The SparseBlock of the sweep, built ONCE (keep_zeros and the meaning of an unstored entry from params.missing) and handed
        to every PyNMF, which takes a block as it is; what PyNMF refuses for sparse data is refused here, in its words."""
        from .sparse import SparseBlock
        missing = PyNMF._missing_checks(A_ij, self.params, True)
        PyNMF._sparse_checks(A_ij, self.params)
        on_dev = isinstance(A_ij, torch.Tensor) or getattr(A_ij, "is_sparse_block", False)
        if self.ops is None:
            if isinstance(A_ij, torch.Tensor) and not A_ij.is_cuda:
                raise TypeError("PyNMFk: A_ij is a CPU tensor; pass a CUDA tensor or a scipy.sparse matrix (no CPU fallback)")
            if not torch.cuda.is_available():
                raise RuntimeError("PyNMFk: no GPU visible; the MI355X engine has no CPU fallback")
            device = A_ij.device if on_dev else torch.device("cuda", torch.cuda.current_device())
        else:
            device = A_ij.device if on_dev else torch.device("cpu")
        self.A_ij = SparseBlock.from_any(A_ij, device, keep_zeros=(missing == "unstored"), missing=missing)
        self.sweep = SparseSweep(self.A_ij, numpy_io=not on_dev, ops=self.ops)

    def fit(self):
        """pyDNMFk.py:169-215.  Returns the estimated number of latent features (same on every rank)."""
        self.params.results_path = self.params.results_path + self.params.fname + '/'
        if self.rank == 0:
            os.makedirs(self.params.results_path, exist_ok=True)
        if self.params.checkpoint:
            try:
                self.cp.load_from_checkpoint()
                self.start_k = self.cp.k + self.step_k if self.cp.flag > 3 else self.cp.k     # :191-194
            except (OSError, EOFError, AttributeError):
                pass
        for self.k in range(self.start_k, self.end_k + 1, self.step_k):
            self.params.k = self.k
            self.pynmfk_per_k()
        if self.rank == 0:
            nopt, _ = self.pvalueAnalysis()
            print('Rank estimated by NMFk = ', nopt)
        else:
            nopt = None
        nopt = self.world.bcast(nopt, root=0)
        self.world.barrier()
        from .dist_nmf import release_buffers
        release_buffers()                       # the sweep's scratch (sized for the largest k) is not kept alive
        return nopt

    def pynmfk_per_k(self):
        """pyDNMFk.py:218-258."""
        self.params.results_paths = self.params.results_path + str(self.k) + '/'
        if self.rank == 0:
            os.makedirs(self.params.results_paths, exist_ok=True)
        results = []
        divs = []                    # norm='is' / 'beta': the total divergence of every perturbation's fit
        if self.rank == 0:
            print('*************Computing for k=', self.k, '************')
        perturbation = 0
        # The perturbations are independent fits of one shape (:226-231 runs them one after another).  On one rank they are
        # set up in the reference's order -- perturbation p draws its data and then its initial factors from the stream
        # seeded p * 1000 -- and then fitted TOGETHER, `nb` at a time: one batched whole-fit call in which every kernel launch
        # covers all of them (PyNMF.fit_batch; bit-identical to the one-by-one fits, which nb = 1 still runs).
        from .engine import stack_alloc
        nb = self._batch_size()
        shared = self.split == 'perturbations' and self.world.size > 1
        mine = list(range(self.world.rank, self.perturbations, self.world.size)) if shared else list(range(self.perturbations))
        for p0 in range(0, len(mine), nb):
            fits, stack = [], None
            chunk = mine[p0:p0 + nb]
            for b, perturbation in enumerate(chunk):
                if self.rank == 0 and self.verbose:
                    print('Current perturbation =', perturbation)
                if nb > 1 and stack is None and isinstance(self.A_ij, torch.Tensor) and self.A_ij.is_cuda and self.A_ij.dim() == 2:
                    stack = stack_alloc(len(chunk), self.A_ij.shape[0], self.A_ij.shape[1], self.A_ij.dtype,
                                        self.A_ij.device)            # the perturbed copies are written straight into it
                data = sample(data=self.A_ij, noise_var=self.noise_var, method=self.sampling, seed=perturbation * 1000,
                              out=None if stack is None else stack[b], sparse=self.sweep,
                              missing="nan" if self._masked else None).fit()
                self.params.W_update = True
                if getattr(self.params, "rng", None) == "device":       # device-drawn init: one seed per (perturbation, k)
                    self.params.init_seed = perturbation * 1000 + self.k
                f = PyNMF(data, factors=None, params=self.params, ops=self.ops)                          # :230
                if nb > 1:
                    if stack is None or tuple(stack.shape[1:]) != tuple(f.A_ij.shape) or stack.dtype != f.A_ij.dtype:
                        if b == 0:           # (host data, bf16 storage of fp32 input, pruned shapes: the stack takes the fit's block)
                            stack = stack_alloc(len(chunk), f.A_ij.shape[0], f.A_ij.shape[1], f.A_ij.dtype, f.A_ij.device)
                    if stack is not None and tuple(stack.shape[1:]) == tuple(f.A_ij.shape) and stack.dtype == f.A_ij.dtype:
                        f.adopt_stack(stack, b)
                fits.append(f)
                del data
            results.extend(PyNMF.fit_batch(fits))
            if self._is:
                divs.extend(f.is_divergence() for f in fits)
            elif self._beta:
                divs.extend(f.beta_divergence() for f in fits)
            for perturbation in chunk:
                self.cp._save_checkpoint(self.params.flag, perturbation, self.k)
            del fits, stack
        if shared:
            results, divs = self._gather_fits(results, mine, divs if (self._is or self._beta) else None)
            perturbation = self.perturbations - 1
        self.params.flag = 1
        self.cp._save_checkpoint(self.params.flag, perturbation, self.k)
        # stack: W m_loc x k x P (column-major over (k, P) as the reference's order='F' reshape, :234-235), H k x n_loc x P
        # numpy in / numpy out fits: the stacks still go to the GPU for the clustering (its contractions over the row index
        # run on the update engine's kernels); with an injected checker back end they stay where they are
        dev = torch.device("cuda", torch.cuda.current_device()) if (self.ops is None and torch.cuda.is_available()) else None

        f64 = (self.A_ij.dtype == torch.float64) if isinstance(self.A_ij, torch.Tensor) else (self.A_ij.dtype == np.float64)

        def _t(x):
            t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
            # (float32 data with prune=True hand float64 factors back, as the reference does: the stacks stay float32 then;
            #  float64 data are clustered in float64)
            t = t.to(torch.float32) if (t.dtype == torch.float64 and not f64) else t
            return t.to(dev) if (dev is not None and not t.is_cuda) else t
        Ws = [_t(r[0]) for r in results]
        Hs = [_t(r[1]) for r in results]
        self.Wall = torch.stack(Ws, dim=-1)
        if self.hall_layout == 'reference':
            # exactly the reference's array: np.vstack(H_0 .. H_{P-1}) (P k x n) re-read in C order as (k, n, P), :236-237.
            # That is NOT "H of perturbation p in [:, :, p]" (entries of different perturbations, features and columns
            # share a fibre), but it is what its clustering permutes and what its median -- the initial H of the
            # regression fit below -- is taken over, so the default reproduces it.
            self.Hall = torch.cat(Hs, dim=0).reshape(self.k, Hs[0].shape[1], len(Hs)).contiguous()
        else:                                              # 'aligned': Hall[:, :, p] = H of perturbation p
            self.Hall = torch.stack(Hs, dim=-1)
        self.recon_err = [float(r[2]) for r in results]
        centroids, _, self.Hall, self.clusterSilhouetteCoefficients, self.avgSilhouetteCoefficients, _ = \
            custom_clustering(self.Wall, self.Hall, self.params, ops=self.ops).fit()                    # :239-240
        self.params.flag = 2
        self.cp._save_checkpoint(self.params.flag, perturbation, self.k)
        self.AvgH = _median_np_semantics(self.Hall)                                                     # :243
        self.AvgW = centroids
        self.params.W_update = False                                                                    # :245
        self.params.init_seed = None
        numpy_io = self.sweep.numpy_io if self._sparse else not isinstance(self.A_ij, torch.Tensor)
        f0 = [_np(self.AvgW), _np(self.AvgH)] if numpy_io else [self.AvgW, self.AvgH]
        regressH = PyNMF(self.A_ij, factors=f0, params=self.params, ops=self.ops)
        self.AvgW, self.AvgH, self.L_errDist = regressH.fit()                                           # :246-247
        # :248.  Under norm='is' the per-column statistic is the mean Itakura-Saito divergence per entry: the Frobenius column_err
        # weights the columns by their scale, which is what a user who chose this norm wanted to avoid
        # and under norm='beta' the divergence of each column over its sum of a^beta, scale-invariant for every beta
        self.col_err = (regressH.is_column_divergence() if self._is else regressH.beta_column_divergence() if self._beta
                        else regressH.column_err())
        self.avgErr = float(np.mean(self.recon_err))
        mn = self.params.m * self.params.n      # (sparse data too, under both meanings of an unstored entry, and NaN-marked data: DESIGN.md section 7)
        self.AIC = 2 * self.k + mn * np.log(self.avgErr / mn)                                           # :250
        cluster_stats = {'clusterSilhouetteCoefficients': self.clusterSilhouetteCoefficients,
                         'avgSilhouetteCoefficients': self.avgSilhouetteCoefficients, 'L_errDist': self.L_errDist,
                         'L_err': self.col_err, 'avgErr': self.avgErr, 'recon_err': self.recon_err, 'AIC': self.AIC}
        if self._is:                            # (recon_err, avgErr and AIC keep their Frobenius definitions)
            self.is_div = [float(d) for d in divs]
            cluster_stats['is_div'], cluster_stats['avgDiv'] = self.is_div, float(np.mean(self.is_div))
        if self._beta:
            self.beta_div = [float(d) for d in divs]
            cluster_stats['beta_div'], cluster_stats['avgDiv'], cluster_stats['beta'] = self.beta_div, float(np.mean(self.beta_div)), self.beta
        self.stats[self.k] = cluster_stats
        if getattr(self.params, "ftype", None) is None:
            self.params.ftype = None
        if not shared or self.rank == 0:        # (every rank of a perturbation-shared sweep holds the same results: rank 0 writes)
            writer = data_write(self.params)
            writer.save_factors([_np(self.AvgW), _np(self.AvgH)], reg=True)                             # :254-256
            writer.save_cluster_results(cluster_stats)
        self.params.flag = 3
        self.cp._save_checkpoint(self.params.flag, perturbation, self.k)

    def _gather_fits(self, results, mine, divs=None):
        """Perturbation-shared sweep: every rank has fitted its own perturbations; all ranks end with all (W, H, err) in
        perturbation order.  One allgather of the stacked factors per k (ranks with one perturbation fewer pad their stack).
        `divs` (norm='is', norm='beta'): this rank's divergences, carried as the errors are.  Returns (fits, divergences or None)."""
        world, P = self.world, self.perturbations
        numpy_io = bool(results) and not isinstance(results[0][0], torch.Tensor)
        dev = torch.device("cuda", torch.cuda.current_device()) if (self.ops is None and torch.cuda.is_available()) else torch.device("cpu")

        def _t(x):
            t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
            return t.to(dev)
        per = -(-P // world.size)                          # perturbations of the busiest rank
        if results:
            W0, H0 = _t(results[0][0]), _t(results[0][1])
            shp = (tuple(W0.shape), tuple(H0.shape), W0.dtype)
        else:
            shp = None
        shp = [s_ for s_ in world.allgather(shp) if s_ is not None][0]
        Ws = torch.zeros((per,) + shp[0], dtype=shp[2], device=dev)
        Hs = torch.zeros((per,) + shp[1], dtype=shp[2], device=dev)
        errs = torch.zeros(per, dtype=torch.float64, device=dev)
        for i, r in enumerate(results):
            Ws[i], Hs[i], errs[i] = _t(r[0]), _t(r[1]), float(r[2])
        allW = world.allgather_blocks(Ws, [tuple(Ws.shape)] * world.size)
        allH = world.allgather_blocks(Hs, [tuple(Hs.shape)] * world.size)
        allE = world.allgather_blocks(errs, [tuple(errs.shape)] * world.size)
        if divs is not None:
            dv = torch.zeros(per, dtype=torch.float64, device=dev)
            for i, d in enumerate(divs):
                dv[i] = float(d)
            allD = world.allgather_blocks(dv, [tuple(dv.shape)] * world.size)
        out = []
        for p in range(P):
            r, i = p % world.size, p // world.size
            W, H, e = allW[r][i], allH[r][i], float(allE[r][i])
            out.append((W.cpu().numpy(), H.cpu().numpy(), e) if numpy_io else (W, H, e))
        return out, (None if divs is None else [float(allD[p % world.size][p // world.size]) for p in range(P)])

    def _batch_size(self):
        """How many perturbation fits run together (PyNMF.fit_batch): all of them on one rank with the product's own
        operators -- as many as fit next to each other in the GPU's free memory (each holds its perturbed copy of the data) --
        else 1.  `params.nmfk_batch` = False / 0 / 1 keeps the one-by-one fits, an integer caps the batch."""
        want = getattr(self.params, "nmfk_batch", True)
        if self._sparse or self._masked or self._is or self._beta:          # no batched sparse, masked, Itakura-Saito or beta-divergence entry point: the fits run one by one, no stack is allocated
            return 1
        if want is False or self.p != 1 or self.ops is not None or not torch.cuda.is_available():
            return 1
        cap = self.perturbations if want is True else max(1, int(want))
        try:
            free = torch.cuda.mem_get_info()[0]
        except Exception:  # noqa: BLE001
            return 1
        m, n = self.A_ij.shape
        # per problem: its perturbed copy of the data in the data's own element size (float64 data are 8 bytes; fp32 data that the fit stores as
        # bf16 still pass through a full-size copy first), the float64 operator set's m x n quotient image (one per call, counted per problem to
        # stay on the safe side), the factors and their workspaces
        esz = self.A_ij.element_size() if isinstance(self.A_ij, torch.Tensor) else int(np.dtype(getattr(self.A_ij, "dtype", np.float32)).itemsize)
        per = m * n * esz * (2.25 if esz == 8 else 1.25) + (m + n) * max(int(self.end_k), 1) * esz * 8 + (64 << 20)
        if str(getattr(self.params, "method", "mu")).lower() == "bcd" and esz == 4:
            # a BCD problem's workspace slice holds four m x k and three k x n buffers next to the step workspace: ask the library
            # (the largest rank of the sweep) instead of trusting the estimate above
            from ._lib import lib
            kmax = max(int(self.end_k), 1)
            slice_bytes = lib.dnmf_bcd_ws_bytes_fit(int(m), int(n), kmax, 1)
            if slice_bytes:
                per = m * n * esz * 1.25 + (m + n) * kmax * esz * 2 + slice_bytes + (16 << 20)
        return int(max(1, min(cap, self.perturbations, (0.6 * free) // per)))

    def pvalueAnalysis(self):
        """pyDNMFk.py:261-299: walk k upwards; whenever the PREVIOUS k clustered well (min silhouette > sill_thr) and
        this k's column-error distribution differs from the current best (Wilcoxon p < 0.05), this k becomes the
        estimate."""
        from .data_io import read_cluster_results
        ks = list(range(self.first_k, self.end_k + 1, self.step_k))
        pvalue = np.ones(len(ks))
        sill_min, err = [], []
        for k in ks:
            st = self.stats.get(k)
            if st is None:                       # resumed run: statistics of finished k's come from disk
                st = read_cluster_results(self.params.results_path + str(k) + '/')
                st = {'L_err': st['L_err'], 'clusterSilhouetteCoefficients': st['clusterSilhouetteCoefficients']}
            err.append(np.asarray(st['L_err']))
            sill_min.append(round(float(np.min(np.asarray(st['clusterSilhouetteCoefficients']))), 2))
        one = err[0]
        nopt = 1
        i = 1
        while i < len(ks):
            if sill_min[i - 1] > self.sill_thr:
                pvalue[i] = wilcoxon(one, err[i])[1]
                if pvalue[i] < 0.05:
                    nopt = i
                    one = np.copy(err[i])
            i += 1
        return ks[nopt - 1], pvalue


def _median_np_semantics(t):
    """np.median over the last axis (pyDNMFk.py:243) for a torch tensor."""
    P = t.shape[-1]
    s = torch.sort(t, dim=-1).values
    if P % 2:
        return s[..., P // 2].contiguous()
    return (0.5 * (s[..., P // 2 - 1] + s[..., P // 2])).contiguous()
