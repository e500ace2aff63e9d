"""Single-k distributed NMF driver on MI355X -- drop-in for reference pyDNMFk/pyDNMF.py (`PyNMF`).

    W, H, recon_err = PyNMF(A_ij, factors=None, save_factors=False, params=args).fit()

Same `params` attribute bag, same loop semantics (pyDNMF.py:138-182): `itr` update steps, clamp to
eps when i % 10 == 0 (after that step's update), and on the last step column-normalise W
(:185-194) and evaluate the Frobenius relative error (:205-218).  A_ij / factors may be numpy arrays
(copied to the current GPU; numpy arrays come back) or torch CUDA tensors (torch tensors come back).
Everything numeric runs in libdnmf_hip.so; there is no CPU path.

Differences from the reference, all deliberate and documented in DESIGN.md:
  * compute dtype follows the data, as in the reference (pyDNMF.py:68): float32 (the tuned path) or float64 (the fp64 matrix
    cores, engine.HipOpsF64: correctness first, one plain tile shape); `params.precision = 'bfloat16'` (or a
    bfloat16 tensor) keeps the data block in HBM as bf16 -- storage only, Frobenius mu / hals -- with W, H and every
    product in float32: the fit equals the float32 fit of the bf16-rounded data (BASELINE config 5);
  * method is 'mu' (fro / kl), 'hals' (fro) or 'bcd' (fro; float32 data with the fp32 operator set -- float64, bf16-stored A and
    --gemm bf16x6 raise NotImplementedError); init is 'rand' or 'nnsvd' (1D grids);
  * sparse data (pydnmfk_amd.sparse) with `params.missing = 'unstored'`: an unstored entry is NOT OBSERVED instead of zero -- objective,
    MU rules (fro / kl) and the reported error run over the stored positions only (1D grids, method 'mu'; DESIGN.md "Sparse data");
  * dense float32 data with `params.missing = 'nan'`: an entry is observed iff it is not NaN (a zero is an observation) -- the same
    masked objective, rules and error on the matrix cores (pydnmfk_amd.masked, csrc/dnmf_masked.h; method 'mu', 1D grids, k <= 128;
    on one rank the whole fit is one library call, dnmf_masked_mu_fit; `column_err` runs over the observed positions).
    Without `params.missing` dense data are not scanned for NaN;
  * `params.norm = 'is'` (or 'itakura-saito'): the Itakura-Saito divergence by the majorisation-minimisation MU rule (csrc/dnmf_is.h;
    no counterpart in the reference) -- strictly positive dense float32 data, method 'mu', 1D grids, k <= 128; on one rank the whole fit
    is one library call, dnmf_is_mu_fit; `fit()` still returns the Frobenius relative error, `is_divergence()` reports the objective and
    `is_column_divergence()` its mean per entry column by column (the per-column statistic of PyNMFk under this norm);
  * `params.norm = 'beta'` with `params.beta` in [-2, 4]: the beta-divergence by the same kind of rule (csrc/dnmf_beta.h; scikit-learn's
    beta_loss=<float>) under the same restrictions; data strictly positive for beta <= 0, non-negative for beta > 0; beta = 0 IS norm='is'
    (the same bits), beta = 1 and 2 are the KL and Frobenius objectives under this family's rule, not the reference's; one library call
    per fit on one rank (dnmf_beta_mu_fit); `beta_divergence()` reports the objective and `beta_column_divergence()` each column's
    divergence over its sum of a^beta (scale-invariant for every beta: the per-column statistic of PyNMFk under this norm);
  * `prune=True` (the reference's default when the attribute is absent) drops all-zero rows / columns before the
    iterations and scatters the factors back afterwards.  numpy callers get float64 factors back in that case, exactly
    as from the reference (its unprune scatters into np.zeros, utils.py:195,198); tensor callers keep float32 on the GPU.
"""
import numpy as np
import torch

from .dist_nmf import nmf_algorithms_1D, nmf_algorithms_2D
from .utils import data_operations, var_init


def _to_device(x, device, dtype=torch.float32, what="A_ij"):
    if isinstance(x, torch.Tensor):
        t = x
    else:
        t = torch.from_numpy(np.ascontiguousarray(x))
    # factors take the data's compute dtype on entry, as in the reference (`factors[i].astype(self.A_ij.dtype)`,
    # pyDNMF.py:92-96): NMFk hands the float64 medians / centroids of its clustering to the regression fit
    return t.to(device=device, dtype=dtype).contiguous()


def storage_dtype(A_ij, params):
    """How the data block is held in HBM: float32, or bfloat16 when `params.precision` says so ('bfloat16' / 'bf16')
    or the caller hands over a bfloat16 tensor.  bf16 is storage only -- W, H and all arithmetic stay float32."""
    prec = getattr(params, "precision", None)
    if isinstance(prec, str) and prec.lower() in ("bfloat16", "bf16") or prec is torch.bfloat16:
        return torch.bfloat16
    if isinstance(A_ij, torch.Tensor) and A_ij.dtype == torch.bfloat16:
        return torch.bfloat16
    # float64 data are factorised in float64 (the reference computes in A_ij's dtype, pyDNMF.py:68; `precision` only casts
    # the file in data_read, main.py:29) on the fp64 matrix cores (engine.HipOpsF64)
    dt = A_ij.dtype if isinstance(A_ij, torch.Tensor) else getattr(A_ij, "dtype", None)
    if dt in (torch.float64, np.dtype("float64")):
        return torch.float64
    return torch.float32


_MASKS = ("row_zero_idx_x", "col_zero_idx_x", "row_zero_idx_w", "col_zero_idx_h")
_NATIVE_FITS = (("mu", "fro"), ("mu", "kl"), ("hals", "fro"), ("bcd", "fro"), ("mu", "is"), ("mu", "beta"))
BETA_RANGE = (-2.0, 4.0)             # where the value of (W H + eps)^(beta - 2) at a padded position is finite in float32 (csrc/dnmf_beta.h)


class PyNMF:
    """Reference pyDNMF.py:6-239 (the MU path of it)."""

    def __init__(self, A_ij, factors=None, save_factors=False, params=None, ops=None):
        from .sparse import is_sparse_input
        self._sparse = is_sparse_input(A_ij)
        # (sparse data: scipy input is numpy I/O, torch sparse tensors and SparseBlocks get CUDA tensors back)
        self._numpy_io = not (isinstance(A_ij, torch.Tensor) or getattr(A_ij, "is_sparse_block", False))
        self.ops = ops
        if ops is None:
            if isinstance(A_ij, torch.Tensor) and not A_ij.is_cuda and not self._sparse:
                raise TypeError("PyNMF: A_ij is a CPU tensor; pass a CUDA tensor or a numpy array (no CPU fallback)")
            if not torch.cuda.is_available():
                raise RuntimeError("PyNMF: no GPU visible; the MI355X engine has no CPU fallback")
            device = A_ij.device if isinstance(A_ij, torch.Tensor) and A_ij.is_cuda or getattr(A_ij, "is_sparse_block", False) \
                else torch.device("cuda", torch.cuda.current_device())
        else:
            device = A_ij.device if isinstance(A_ij, torch.Tensor) or getattr(A_ij, "is_sparse_block", False) else torch.device("cpu")
        self.device = device
        if ops is None and getattr(params, "shared_gpu", False):
            # (main.py --shared_gpu / params.shared_gpu = True) the launch-chain kernels from the start: no kernel of this process waits
            # for co-resident workgroups, so none can time out behind a co-tenant
            from ._lib import lib
            lib.dnmf_set_persistent(0)
        missing = self._missing_checks(A_ij, params, self._sparse)
        if self._sparse:
            self.a_dtype = self._sparse_checks(A_ij, params)
        else:
            self.a_dtype = storage_dtype(A_ij, params)
        self.c_dtype = torch.float64 if self.a_dtype == torch.float64 else torch.float32      # factors, products, eps
        self._masked_dense = (missing == "nan")
        if self._sparse:
            from .sparse import SparseBlock
            # (missing='unstored': a stored zero is an observation and stays stored; the block carries the meaning from here on)
            self.A_ij = SparseBlock.from_any(A_ij, device, keep_zeros=(missing == "unstored"), missing=missing)
        elif self._masked_dense:
            from .masked import MaskedDenseBlock
            # (the data stay as handed over, NaN at the missing positions: the block carries the meaning from here on)
            self.A_ij = MaskedDenseBlock(_to_device(A_ij, device, self.a_dtype))
        else:
            self.A_ij = _to_device(A_ij, device, self.a_dtype)
        self.params = params
        self.m_loc, self.n_loc = self.A_ij.shape
        self.init = self.params.init if getattr(self.params, "init", None) else 'rand'
        if "grid" in vars(self.params) and self.params.grid:
            self.p_r, self.p_c, self.k = self.params.grid[0], self.params.grid[1], self.params.k
            self.params.p_r, self.params.p_c = self.p_r, self.p_c
        else:
            self.p_r, self.p_c, self.k = self.params.p_r, self.params.p_c, self.params.k
        self.comm1 = self.params.comm1
        self.cart_1d_row, self.cart_1d_column, self.comm = self.params.row_comm, self.params.col_comm, self.params.comm
        self.verbose = self.params.verbose if getattr(self.params, "verbose", False) else False
        self.rank = self.comm1.rank
        self.eps = float(np.finfo(np.float64 if self.c_dtype == torch.float64 else np.float32).eps)   # pyDNMF.py:68
        self.params.eps = self.eps
        self.norm = var_init(self.params, 'norm', default='kl')     # :70
        self.method = var_init(self.params, 'method', default='mu')
        self.beta = None
        if str(self.norm).lower() == 'beta':
            self.beta = self._beta_value(self.params)
            # beta = 0 IS Itakura-Saito: handed to that path (its kernels, its bits), the way 'itakura-saito' is renamed
            self.norm = self.params.norm = 'is' if self.beta == 0.0 else 'beta'
        if str(self.norm).lower() in ('is', 'itakura-saito'):
            self.norm = self.params.norm = 'is'
        self._is = (self.norm == 'is')
        self._beta = (self.norm == 'beta')
        if self._is or self._beta:
            self._div_checks(missing)
        if self.a_dtype == torch.bfloat16 and str(self.norm).lower() == 'kl':
            raise TypeError("PyNMF: bfloat16 storage of A is provided for the Frobenius updates (mu / hals) only")
        self.prune = var_init(self.params, 'prune', default=True)
        if self._masked_dense and self.prune:
            raise NotImplementedError("missing='nan' with prune=True is not provided (pruning drops all-ZERO rows and columns; under "
                                      "missing='nan' a row without an observation keeps its place and its factor row goes to zero): set "
                                      "params.prune = False")
        if self._masked_dense and self.params.k > 128:
            raise NotImplementedError("missing='nan' with k = %d is not provided: the masked dense kernels serve 1 <= k <= 128" % self.params.k)
        self.save_factors = save_factors
        self.params.itr = var_init(self.params, 'itr', default=5000)
        self.itr = self.params.itr
        try:
            self.W_update = self.params.W_update
        except AttributeError:
            self.params.W_update = True
            self.W_update = True
        self.p = self.p_r * self.p_c
        self.topo = '2d' if (self.p_r != 1 and self.p_c != 1) else '1d'   # :83-87
        self.params.topo = self.topo
        self.data_op = data_operations(self.A_ij, self.params)      # :88 -> params.m, n, m_loc, n_loc, ...
        self.params = self.data_op.params
        if factors is not None:                                     # :90-96 (copied on entry)
            W0 = _to_device(factors[0], device, self.c_dtype, what="factors").clone()
            H0 = _to_device(factors[1], device, self.c_dtype, what="factors").clone()
        else:
            W0, H0 = self.init_factors()
        if self.topo == '1d':
            self.W_i, self.H_j = W0, H0
        else:
            self.W_ij, self.H_ij = W0, H0
        if self.prune:                                              # :99-101
            if self.topo == '1d':
                self.A_ij, self.W_i, self.H_j = self.data_op.prune_all(self.W_i, self.H_j)
            else:
                self.A_ij, self.W_ij, self.H_ij = self.data_op.prune_all(self.W_ij, self.H_ij)
            self.m_loc, self.n_loc = self.A_ij.shape
            # the keep-masks live on the (shared) params bag: this fit's own copy, for fits that are set up together and
            # finished later (fit_batch)
            self._masks = tuple(getattr(self.params, n_) for n_ in _MASKS)
            if self.topo == '2d':   # pruned slices are ragged: exchange the actual sizes once per fit
                self.params._slice_counts = (
                    [int(c) for c in self.cart_1d_column.allgather(int(self.W_ij.shape[0]))],
                    [int(c) for c in self.cart_1d_row.allgather(int(self.H_ij.shape[1]))])
        elif hasattr(self.params, "_slice_counts"):
            del self.params._slice_counts

    @staticmethod
    def _missing_checks(A_ij, params, sparse):
        """`params.missing`: None (an unstored entry of sparse data is a zero; dense data are not scanned for NaN), 'unstored' (sparse
        data: an unstored entry is not observed) or 'nan' (dense float32 data: a NaN entry is not observed).  Both meanings are provided
        with method 'mu' (fro / kl) on one rank and 1D grids."""
        missing = getattr(params, "missing", None)
        if missing not in (None, "unstored", "nan"):
            raise ValueError("params.missing = %r is not known: None (unstored entries are zeros), 'unstored' (sparse data: not observed) "
                             "or 'nan' (dense data: NaN entries are not observed)" % (missing,))
        if missing == "nan" and sparse:
            raise ValueError("params.missing = 'nan' marks the missing entries of DENSE data; for sparse data the unstored entries are the "
                             "missing ones: params.missing = 'unstored'")
        if getattr(A_ij, "is_sparse_block", False) and getattr(A_ij, "missing", None) != missing:
            raise ValueError("params.missing = %r, but the SparseBlock handed over was built with missing = %r: build the block with "
                             "the meaning (and keep_zeros) the fit is to use" % (missing, getattr(A_ij, "missing", None)))
        if missing is None:
            return None
        if missing == "unstored" and not sparse:
            raise NotImplementedError("missing='unstored' is not provided for dense data: mark the missing entries of a dense array with "
                                      "NaN and pass missing='nan', or hand the observed entries over as a sparse matrix")
        method = str(getattr(params, "method", None) or "mu").lower()
        if method != "mu":
            raise NotImplementedError("missing='%s' is provided for method 'mu' (fro / kl) only, not for '%s'" % (missing, method))
        if missing == "nan":
            PyNMF._masked_dense_checks(A_ij, params)
        return missing

    @staticmethod
    def _masked_dense_checks(A_ij, params):
        """What is refused under missing='nan', each by name (dense float32 data, fp32 arithmetic, 1D grids, init='rand' or factors)."""
        prec = getattr(params, "precision", None)
        dt = getattr(A_ij, "dtype", None)
        if isinstance(prec, str) and prec.lower() in ("bfloat16", "bf16") or prec is torch.bfloat16 or dt is torch.bfloat16:
            raise NotImplementedError("missing='nan' with bfloat16 storage of the data is not provided (float32 data only)")
        if dt in (torch.float64, np.dtype("float64")):
            raise NotImplementedError("missing='nan' with float64 data is not provided (float32 data only); cast the block to float32")
        if dt not in (torch.float32, np.dtype("float32")):
            raise NotImplementedError("missing='nan' is provided for dense float32 data (a numpy array or a torch tensor), not for %s"
                                      % (dt if dt is not None else type(A_ij).__name__,))
        if (getattr(params, "gemm", None) or "fp32") != "fp32":
            raise NotImplementedError("missing='nan' with --gemm %s is not provided (fp32 arithmetic only)" % params.gemm)
        grid = getattr(params, "grid", None) or (getattr(params, "p_r", 1), getattr(params, "p_c", 1))
        if grid[0] != 1 and grid[1] != 1:
            raise NotImplementedError("missing='nan' on a 2D grid (%d x %d) is not provided: use a 1D grid (p_r = 1 or p_c = 1)" % (grid[0], grid[1]))
        if getattr(params, "init", None) == "nnsvd":
            raise NotImplementedError("missing='nan' with init='nnsvd' is not provided (the SVD would read the NaNs): init='rand' or factors=...")

    # the phrases in which the refusals of the two divergence norms differ: (its kernels' name, the end of the sparse refusal)
    _DIV_WORDS = {"is": ("Itakura-Saito", ": the Itakura-Saito divergence is infinite at a zero entry (dense strictly positive float32 data only)"),
                  "beta": ("beta-divergence", " (dense float32 data only)")}

    def _div_checks(self, missing):
        """What is refused under norm='is' and norm='beta', each by name (dense float32 data without missing entries, fp32 arithmetic,
        method 'mu', 1D grids, k <= 128), and what the data must be: strictly positive under 'is' and for beta <= 0, non-negative for
        beta > 0.  The ranks agree on that verdict through comm1 BEFORE any of them raises, so none is left alone in a later collective."""
        self._div_refusals(self.norm, self.params, self._sparse, missing, self.a_dtype, self.ops, self.method, self.p_r, self.p_c, self.params.k)
        self._sign_check(self.beta if self._beta else None, float(self.A_ij.min()) if self.A_ij.numel() else 1.0, self.comm1,
                         self.p_r * self.p_c)

    @staticmethod
    def _div_refusals(norm, params, sparse, missing, a_dtype, ops, method, p_r, p_c, k):
        """the refusals of `norm` ('is' or 'beta') that need no look at the data (PyNMFk raises them at construction, with its largest
        rank as k)"""
        kernels, sparse_why = PyNMF._DIV_WORDS[norm]
        if missing is not None:
            raise NotImplementedError("norm='%s' with missing='%s' is not provided (dense data without missing entries only)" % (norm, missing))
        if sparse:
            raise NotImplementedError("norm='%s' is not provided for sparse data%s" % (norm, sparse_why))
        if a_dtype == torch.bfloat16:
            raise NotImplementedError("norm='%s' with bfloat16 storage of the data is not provided (float32 data only)" % norm)
        if (getattr(params, "gemm", None) or "fp32") != "fp32":
            raise NotImplementedError("norm='%s' with --gemm %s is not provided (fp32 arithmetic only)" % (norm, params.gemm))
        # (an operator set names the data types its operations under the norm take, `is_dtypes` / `beta_dtypes`: the HIP kernels are float32)
        if a_dtype not in (getattr(ops, norm + "_dtypes", ()) if ops is not None else (torch.float32,)):
            raise NotImplementedError("norm='%s' with %s data is not provided (float32 data only); cast the block to float32"
                                      % (norm, str(a_dtype).replace("torch.", "")))
        method = str(method).lower()
        if method != "mu":
            raise NotImplementedError("norm='%s' is provided for method 'mu' only, not for '%s': HALS and BCD are Frobenius methods"
                                      % (norm, method))
        if p_r != 1 and p_c != 1:
            raise NotImplementedError("norm='%s' on a 2D grid (%d x %d) is not provided: use a 1D grid (p_r = 1 or p_c = 1)"
                                      % (norm, p_r, p_c))
        if k > 128:
            raise NotImplementedError("norm='%s' with k = %d is not provided: the %s kernels serve 1 <= k <= 128" % (norm, k, kernels))

    @staticmethod
    def _beta_value(params):
        """`params.beta` as a float inside BETA_RANGE; a missing or an out-of-range value is a ValueError"""
        beta = getattr(params, "beta", None)
        if beta is None:
            raise ValueError("norm='beta' needs params.beta: a float in %g <= beta <= %g (main.py --beta)" % BETA_RANGE)
        beta = float(beta)
        if not BETA_RANGE[0] <= beta <= BETA_RANGE[1]:
            raise ValueError("norm='beta' with beta = %g is outside the accepted range %g <= beta <= %g" % ((beta,) + BETA_RANGE))
        return beta

    @staticmethod
    def _sign_check(beta, lo, comm1, nranks):
        """`lo`: the smallest entry of this rank's block; `beta`: None under norm='is'.  Every rank raises when any rank holds an entry
        that the norm does not take: <= 0 under 'is' and for beta <= 0, < 0 for beta > 0"""
        strict = beta is None or beta <= 0.0
        bad = not (lo > 0.0 if strict else lo >= 0.0)               # (a NaN minimum is refused as well)
        nbad = int(comm1.allreduce(1 if bad else 0))
        if nbad and beta is None:
            raise ValueError("norm='is' needs strictly positive data: the smallest entry of this rank's block is %g (%d of %d ranks hold "
                             "an entry <= 0); the Itakura-Saito divergence is infinite there" % (lo, nbad, nranks))
        if nbad:
            raise ValueError("norm='beta' with beta = %g needs %s data: the smallest entry of this rank's block is %g (%d of %d ranks hold "
                             "an entry %s 0)%s" % (beta, "strictly positive" if strict else "non-negative", lo, nbad, nranks,
                                                   "<=" if strict else "<",
                                                   "; the divergence is infinite at a zero for beta <= 0" if strict else ""))

    @staticmethod
    def _sparse_checks(A_ij, params):
        """What is refused for sparse data, each by name (float32 values, fp32 arithmetic, 1D grids, init='rand' or factors)."""
        prec = getattr(params, "precision", None)
        if isinstance(prec, str) and prec.lower() in ("bfloat16", "bf16") or prec is torch.bfloat16:
            raise NotImplementedError("precision='bfloat16' is not provided for sparse data (float32 values only)")
        dt = getattr(A_ij, "dtype", None)
        if dt in (torch.float64, np.dtype("float64")):
            raise NotImplementedError("float64 sparse data are not provided (float32 values only); cast the values to float32")
        if (getattr(params, "gemm", None) or "fp32") != "fp32":
            raise NotImplementedError("--gemm %s is not provided for sparse data (fp32 arithmetic only)" % params.gemm)
        grid = getattr(params, "grid", None) or (getattr(params, "p_r", 1), getattr(params, "p_c", 1))
        if grid[0] != 1 and grid[1] != 1:
            raise NotImplementedError("sparse data on a 2D grid (%d x %d) are not provided: use a 1D grid (p_r = 1 or p_c = 1)" % (grid[0], grid[1]))
        return torch.float32

    def init_factors(self):
        """pyDNMF.py:107-135, init='rand': uniform [0,1) from the process-global numpy RNG (so seeding numpy
        reproduces the reference's draw order), cast to float32; the replicated factor is broadcast from rank 0."""
        if self.init == 'nnsvd' and self._sparse:
            raise NotImplementedError("init='nnsvd' is not provided for sparse data: init='rand' or factors=...")
        if self.init == 'nnsvd':                                    # pyDNMF.py:130-135
            if self.topo != '1d':
                raise Exception('NNSVD init only available for 1D topology, please try with 1d topo.')
            from .dist_svd import DistSVD
            return DistSVD(self.params, self.A_ij, ops=self._ops()).nnsvd(flag=1, verbose=0)
        if self.init != 'rand':
            raise NotImplementedError("init='%s': 'rand', 'nnsvd' or factors=... are provided" % self.init)
        if getattr(self.params, "rng", None) == "device" and self.device.type == "cuda":
            return self._init_factors_device()
        f32 = np.float64 if self.c_dtype == torch.float64 else np.float32        # (`.astype(self.A_ij.dtype)`, pyDNMF.py:113)
        if self.topo == '2d':
            W = np.random.rand(self.params.m_loc, self.k).astype(f32)
            H = np.random.rand(self.k, self.params.n_loc).astype(f32)
        elif self.p_c == 1:
            W = np.random.rand(self.m_loc, self.k).astype(f32)
            H = np.random.rand(self.k, self.n_loc).astype(f32) if self.rank == 0 else None
            H = self.comm1.bcast(H, root=0)
        else:
            H = np.random.rand(self.k, self.n_loc).astype(f32)
            W = np.random.rand(self.m_loc, self.k).astype(f32) if self.rank == 0 else None
            W = self.comm1.bcast(W, root=0)
        return _to_device(W, self.device, self.c_dtype), _to_device(H, self.device, self.c_dtype)

    def _init_factors_device(self):
        """`params.rng = 'device'` (what main.py / pyDNMFk_Runner select): the same uniform [0,1) init (pyDNMF.py:110-129),
        drawn ON the GPU -- no m x k / k x n host arrays, no PCIe copy per fit (an NMFk sweep makes 20 x K fits).  Seeded by
        `params.init_seed` (NMFk sets one per perturbation; per-rank factors add the rank) or torch's global generator; the
        replicated factor of a 1D grid still comes from rank 0.  A different random stream than numpy's: the parity
        fixtures use the default `rng = 'numpy'`."""
        dev = self.device
        seed = getattr(self.params, "init_seed", None)

        def draw(shape, salt):
            if seed is None:
                return torch.rand(shape, dtype=self.c_dtype, device=dev)
            g = torch.Generator(device=dev)
            g.manual_seed(int(seed) * 1000003 + salt)
            return torch.rand(shape, dtype=self.c_dtype, device=dev, generator=g)
        if self.topo == '2d':
            return draw((self.params.m_loc, self.k), 2 * self.rank + 1), draw((self.k, self.params.n_loc), 2 * self.rank + 2)
        if self.p_c == 1:
            W = draw((self.m_loc, self.k), 2 * self.rank + 1)
            H = self.comm1.bcast(draw((self.k, self.n_loc), 0) if self.rank == 0 else torch.empty(self.k, self.n_loc, dtype=self.c_dtype, device=dev), root=0)
        else:
            H = draw((self.k, self.n_loc), 2 * self.rank + 2)
            W = self.comm1.bcast(draw((self.m_loc, self.k), 0) if self.rank == 0 else torch.empty(self.m_loc, self.k, dtype=self.c_dtype, device=dev), root=0)
        return W.contiguous(), H.contiguous()

    def _ops(self):
        if self.ops is None:
            from .engine import ops_for
            self.ops = ops_for(self.params, self.c_dtype, sparse=self._sparse, masked=self._masked_dense)
        return self.ops

    def _out(self, t):
        if not self._numpy_io:
            return t
        a = t.cpu().numpy()
        return a.astype(np.float64) if self.prune else a        # the reference's dtype after unprune (utils.py:195,198)

    def fit(self):
        """pyDNMF.py:138-182.  Returns (W, H, recon_err).

        Several kernels behind this loop need the GPU to themselves (their workgroups wait for each other: the whole fits of small
        problems, the persistent HALS W sweep, the one-pass MU/FRO step).  When one of them gives up -- another process or stream holds
        CUs -- the fit is NOT lost: the initial factors are kept until the end, the ranks agree on the time-out, every rank switches its
        process to the launch-chain kernels (engine.persistent_off: same update rules, no co-residency) and the fit runs again from them."""
        from ._lib import PersistentTimeout
        keep = self._initial_factors()
        nc = getattr(self.params, "_native_comm", None)
        if nc is not None and hasattr(nc, "fit_begin"):
            nc.fit_begin()
        try:
            return self._fit_once()
        except PersistentTimeout as ex:
            from .engine import persistent_off
            persistent_off(str(ex).split(" -- ")[0])
            self._restore_factors(keep)
            if nc is not None and hasattr(nc, "fit_begin"):
                nc.fit_begin()
            return self._fit_once()

    def _initial_factors(self):
        W, H = (self.W_ij, self.H_ij) if self.topo == '2d' else (self.W_i, self.H_j)
        return W.clone(), H.clone()

    def _restore_factors(self, keep):
        W, H = (self.W_ij, self.H_ij) if self.topo == '2d' else (self.W_i, self.H_j)
        W.copy_(keep[0])
        H.copy_(keep[1])
        for name in ("W_i", "H_j") if self.topo == '2d' else ():       # (the gathered copies relative_err made)
            if hasattr(self, name):
                delattr(self, name)

    def _fit_once(self):
        if self.method.lower() not in ('mu', 'hals', 'bcd'):
            raise NotImplementedError("method '%s' is not part of the MI355X engine (mu / hals / bcd)" % self.method)
        ops = self._ops()
        if self._whole_fit_ok(ops):
            # one rank: the whole loop below -- steps, clamps, normalisation, both squared norms -- is ONE library call
            # (dnmf_*_fit, csrc/dnmf_fit.hip): no Python, no ctypes call and no host synchronisation inside the fit
            if self._beta:                                          # dnmf_beta_mu_fit
                sq = ops.beta_fit(self.A_ij, self.W_i, self.H_j, self.eps, self.beta, self.W_update, self.itr)
            else:
                sq = ops.fit(self.method, self.norm, self.A_ij, self.W_i, self.H_j, self.eps, self.W_update, self.itr,
                             column_sweep=(getattr(self.params, "hals_sweep", None) == "columns"))
            return self._finish(sq[0])
        # bcd: ONE trip with i = itr - 1 (pyDNMF.py:152) -- its update() runs all itr iterations (dist_nmf.py:83, params.itr)
        trips = range(self.itr - 1, self.itr) if self.method.lower() == 'bcd' else range(self.itr)
        for i in trips:
            clamp = (i % 10 == 0)                                   # :155 / :170, fused into the step
            if self.topo == '2d':
                self.W_ij, self.H_ij = nmf_algorithms_2D(self.A_ij, self.W_ij, self.H_ij, params=self.params,
                                                         ops=ops).update(clamp=clamp, more=(i < self.itr - 1))
            else:
                self.W_i, self.H_j = nmf_algorithms_1D(self.A_ij, self.W_i, self.H_j, params=self.params,
                                                       ops=ops).update(clamp=clamp)
            if i == self.itr - 1:
                if self.topo == '2d':
                    self.W_ij, self.H_ij = self.normalize_features(self.W_ij, self.H_ij)
                else:
                    self.W_i, self.H_j = self.normalize_features(self.W_i, self.H_j)
                return self._finish(None)

    def _whole_fit_ok(self, ops):
        """One rank, the product's own fp32-MFMA operator set, a method / norm pair the library has a whole-fit entry point for
        (anything else keeps the step loop, which raises the reference's messages for invalid pairs).  `params.fit_loop =
        'python'` keeps the step loop (A/B runs, tests of the per-step API).  A NaN-marked block (missing='nan') has one with the
        'hip-masked' set: dnmf_masked_mu_fit, the launches of the step loop in its order (one problem per call: never batched)."""
        if (self._is or self._beta) and getattr(ops, "name", "") != "hip":
            return False                                            # (dnmf_is_mu_fit / dnmf_beta_mu_fit live in the fp32 operator set only)
        if self._masked_dense:
            return (self.p == 1 and self.topo == '1d' and self.itr >= 1 and getattr(ops, "name", "") == "hip-masked" and hasattr(ops, "fit")
                    and str(self.method).lower() == "mu" and str(self.norm).lower() in ("fro", "kl")
                    and getattr(self.params, "fit_loop", None) != "python" and not getattr(self.params, "native_always", False))
        return (not self._sparse and self.p == 1 and self.topo == '1d' and self.itr >= 1 and getattr(ops, "name", "") in ("hip", "hip-f64") and hasattr(ops, "fit")
                and not (getattr(ops, "name", "") == "hip-f64" and self.k > 128)
                and (str(self.method).lower(), str(self.norm).lower()) in _NATIVE_FITS
                and not (str(self.method).lower() == "bcd" and (getattr(ops, "name", "") != "hip" or self.a_dtype != torch.float32))
                and getattr(self.params, "fit_loop", None) != "python"
                and not getattr(self.params, "native_always", False))

    def _finish(self, sq):
        """The end of the last iteration (pyDNMF.py:158-166, :173-181): error, un-pruning, save.  `sq`: the device pair
        {sum (A - W H)^2, sum A^2} a whole-fit call left (None: evaluate them here)."""
        ops = self._ops()
        persistent = self.method.lower() == 'hals' or sq is not None or self.p == 1     # (paths that may have run a kernel of that kind)
        if persistent and hasattr(ops, "hals_check"):
            # a persistent kernel (the HALS W sweep; the whole-fit kernel of a small problem, csrc/dnmf_small.h; the one-pass MU/FRO step,
            # csrc/dnmf_team.h) that lost its co-residency raises here -- BEFORE the error's allreduce sees NaN factors, and on EVERY rank
            # (the word is per device: the ranks agree on it first, or the others would walk into the next collective alone); fit() then
            # runs the fit again on the launch-chain kernels
            from ._lib import PersistentTimeout
            bad = None
            try:
                ops.hals_check()
            except PersistentTimeout as ex:
                bad = ex
            nbad = int(self.params.comm1.allreduce(1 if bad is not None else 0))
            if nbad:
                raise bad if bad is not None else PersistentTimeout("a persistent kernel timed out on %d other rank(s)" % nbad)
        nc = getattr(self.params, "_native_comm", None)
        if nc is not None and getattr(nc, "direct_ready", False) and nc._get_direct_on():
            # a direct allreduce that gave up waiting for a peer has produced garbage since: fatal, on every rank together
            nbad = int(self.params.comm1.allreduce(1 if nc.direct_timed_out() else 0))
            if nbad:
                raise RuntimeError("direct allreduce: a wait timed out on %d rank(s) (a peer stalled longer than params.direct_timeout, "
                                   "default 30 s): the factors of this fit are invalid" % nbad)
        self.relative_err(sq)
        if self.verbose is True and self.rank == 0:
            print('relative error is:', self.recon_err)
        W, H = (self.W_ij, self.H_ij) if self.topo == '2d' else (self.W_i, self.H_j)
        if self.prune:                                      # :166,:180-181 (before the save here, so that the
            for n_, v in zip(_MASKS, getattr(self, "_masks", ())):
                setattr(self.params, n_, v)                 # (this fit's masks: the bag may have served another fit since)
            W, H = self.data_op.unprune_factors(W, H)       # saved blocks have the un-pruned shapes)
        if self.save_factors:
            from .data_io import data_write
            data_write(self.params).save_factors([W.cpu().numpy(), H.cpu().numpy()])
        return self._out(W), self._out(H), self.recon_err

    @staticmethod
    def fit_batch(fits):
        """Fit several independent problems TOGETHER: `fits` are PyNMF objects set up one after another (each has drawn
        its perturbation and its initial factors in the reference's order); the result is the list of their `fit()`
        results.  Same-shape problems on one rank run as ONE batched whole-fit call -- every kernel launch covers all of
        them (blockIdx.z = problem), each problem on the same kernels and operands as a fit of its own: the results are
        bit-identical to fitting them one by one (pyDNMFk.py:226-231 runs them one by one).  Anything the batched entry
        points do not cover falls back to exactly that."""
        from .engine import stack_alloc
        fits = list(fits)
        f0 = fits[0] if fits else None

        def same(f):
            return (not f._masked_dense and not f._is and not f._beta and f._whole_fit_ok(f._ops()) and f._ops() is f0._ops() and f.A_ij.shape == f0.A_ij.shape
                    and f.A_ij.dtype == f0.A_ij.dtype and f.A_ij.device == f0.A_ij.device and f.W_i.shape == f0.W_i.shape
                    and f.H_j.shape == f0.H_j.shape and (f.method, f.norm, f.itr, f.W_update, f.eps, f.k) ==
                    (f0.method, f0.norm, f0.itr, f0.W_update, f0.eps, f0.k))
        if len(fits) < 2 or not all(same(f) for f in fits):
            return [f.fit() for f in fits]
        if f0.method.lower() not in ('mu', 'hals', 'bcd'):
            raise NotImplementedError("method '%s' is not part of the MI355X engine (mu / hals / bcd)" % f0.method)
        A = getattr(f0, "_stack", None)
        if A is None or A.shape[0] != len(fits) or any(getattr(f, "_stack", None) is not A or f.A_ij.data_ptr() != A[b].data_ptr()
                                                       for b, f in enumerate(fits)):
            A = stack_alloc(len(fits), f0.A_ij.shape[0], f0.A_ij.shape[1], f0.A_ij.dtype, f0.A_ij.device)
            for b, f in enumerate(fits):                    # (callers that adopt_stack() as they go never get here)
                f.adopt_stack(A, b)
        W = stack_alloc(len(fits), f0.W_i.shape[0], f0.W_i.shape[1], f0.W_i.dtype, f0.W_i.device)
        H = stack_alloc(len(fits), f0.H_j.shape[0], f0.H_j.shape[1], f0.H_j.dtype, f0.H_j.device)
        for b, f in enumerate(fits):
            W[b].copy_(f.W_i)
            H[b].copy_(f.H_j)
        from ._lib import PersistentTimeout
        ops = f0._ops()
        for attempt in (0, 1):
            sq = ops.fit(f0.method, f0.norm, A, W, H, f0.eps, f0.W_update, f0.itr,
                         column_sweep=(getattr(f0.params, "hals_sweep", None) == "columns"))
            try:
                if hasattr(ops, "hals_check"):
                    ops.hals_check()
                break
            except PersistentTimeout as ex:                 # (one rank per problem here: nobody to agree with)
                if attempt:
                    raise
                from .engine import persistent_off
                persistent_off(str(ex).split(" -- ")[0])
                for b, f in enumerate(fits):                # the fits still hold their initial factors
                    W[b].copy_(f.W_i)
                    H[b].copy_(f.H_j)
        out = []
        sq_host = sq.cpu()                                  # ONE synchronisation for the whole batch
        for b, f in enumerate(fits):
            f.W_i, f.H_j = W[b], H[b]
            out.append(f._finish(sq_host[b]))
        return out

    def adopt_stack(self, stack, b):
        """Hold this fit's data block as slice `b` of `stack` ([B][m][n], the layout fit_batch hands to the library): copied
        there unless it already is that slice (NMFk perturbs straight into it), the block's own buffer is released."""
        if self.A_ij.data_ptr() != stack[b].data_ptr():
            stack[b].copy_(self.A_ij)
        self.A_ij = stack[b]
        self.data_op.ten = self.A_ij
        self._stack = stack

    def normalize_features(self, Wall, Hall):
        """pyDNMF.py:185-194: s = column sums of W (allreduced iff 2D or p_r != 1); W /= s + eps; H *= s^T."""
        ops = self._ops()
        s = ops.colsum(Wall, ops.zeros((self.k,), Wall))
        if self.topo == '2d' or self.p_r != 1:
            self.comm1.allreduce_(s)
        ops.scale_cols_div(Wall, s, self.eps)
        ops.scale_rows_mul(Hall, s)
        return Wall, Hall

    def cart_2d_collect_factors(self):
        """pyDNMF.py:197-202."""
        alg = nmf_algorithms_2D(self.A_ij, self.W_ij, self.H_ij, params=self.params, ops=self._ops())
        self.H_j = alg.gather_H()
        self.W_i = alg.gather_W()

    def relative_err(self, sq=None):
        """pyDNMF.py:205-218: ||A - W H||_F / ||A||_F; squared norms are summed over ranks, then sqrt.  `sq`: the pair of
        squared norms when a whole-fit call has already evaluated them (one rank: nothing to sum)."""
        ops = self._ops()
        if sq is None:
            if self.topo == '2d':
                self.cart_2d_collect_factors()
            sq = torch.cat([ops.resid_sqnorm(self.A_ij, self.W_i, self.H_j), ops.sqnorm(self.A_ij)])
            self.comm1.allreduce_(sq)
        num, den = (float(v) for v in sq.cpu())
        self.glob_norm_err, self.glob_norm_A = float(np.sqrt(num)), float(np.sqrt(den))
        self.recon_err = self.glob_norm_err / self.glob_norm_A
        return self.recon_err

    def _block_factors(self):
        """(W, H) of this rank's block as the kernels take them: where fit() has un-pruned the held factors, the rows and columns that
        the pruned block kept"""
        W, H = self.W_i, self.H_j
        if W.shape[0] != self.A_ij.shape[0]:
            W = W[self.params.row_zero_idx_x]
        if H.shape[1] != self.A_ij.shape[1]:
            H = H[:, self.params.col_zero_idx_x]
        return W.contiguous(), H.contiguous()

    def _global_columns(self, *sums):
        """[len(sums)][params.n] float64 zeros with this rank's column range filled from `sums`, each one value per column of this
        block; the sums of a pruned block go to the columns it kept (`col_zero_idx_x`), the pruned ones stay 0"""
        from .utils import determine_block_params
        blk = determine_block_params(self.comm1, (self.p_r, self.p_c), (self.params.m, self.params.n))
        c0 = blk.determine_block_index_range_asymm()[0][1]
        ncol = blk.determine_block_shape_asymm()[1]
        col = torch.zeros(len(sums), self.params.n, dtype=torch.float64, device=sums[0].device)
        keep = getattr(self.params, "col_zero_idx_x", None) if self.prune else None
        for row, x in zip(col, sums):
            if keep is not None and int(keep.numel()) == ncol and x.numel() != ncol:
                row[c0:c0 + ncol][keep] = x
            else:
                row[c0:c0 + ncol] = x
        return col

    def _norm_op(self, norm, op, caller):
        """ops.<norm>_<op>(A, W, H, eps[, beta]) on this block and its current factors, for the norm this fit runs ('is' or 'beta'); a
        fit under another norm is refused in `caller`'s name"""
        if not (self._is if norm == 'is' else self._beta):
            raise ValueError("%s: this fit runs norm='%s'; the divergence is reported under norm='%s'%s"
                             % (caller, self.norm, norm,
                                " (beta = 0 is norm='is': %s())" % caller.replace("beta_", "is_") if norm == 'beta' and self._is else ""))
        W, H = self._block_factors()
        return getattr(self._ops(), "%s_%s" % (norm, op))(self.A_ij, W, H, self.eps, *((self.beta,) if norm == 'beta' else ()))

    def _divergence(self, norm):
        d = self._norm_op(norm, "divergence", norm + "_divergence")
        self.comm1.allreduce_(d)
        return float(d.cpu())

    def is_divergence(self):
        """D_IS(A | W H + eps) = sum (q - log q - 1), q = A / (W H + eps), of the CURRENT factors, summed over the grid (norm='is':
        1D grids, where every rank's block meets its own W rows and H columns).  The objective the Itakura-Saito rule does not
        increase; `fit()` keeps returning the Frobenius relative error, as it does for norm='kl'."""
        return self._divergence('is')

    def beta_divergence(self):
        """D_beta(A | W H + eps) of the CURRENT factors, summed over the grid (norm='beta': 1D grids, where every rank's block meets its own
        W rows and H columns).  The objective the rule does not increase; `fit()` keeps returning the Frobenius relative error."""
        return self._divergence('beta')

    def is_column_divergence(self):
        """The Itakura-Saito divergence of the CURRENT factors column by column, over the GLOBAL n columns, each divided by the global row
        count `params.m`: a mean per entry, scale-invariant (a column's scale cancels in q = A / (W H + eps)) and comparable across k.
        What an NMFk sweep under norm='is' takes where the Frobenius `column_err()` stands (which weights the columns by their scale);
        `column_err()` itself is unchanged under every norm.  Its scheme: each rank fills its own column range with its sums over its own
        rows, one float64 allreduce (row shards add partial sums, column shards fill disjoint ranges), then the division."""
        col = self._global_columns(self._norm_op('is', "column_div", "is_column_divergence"))[0]
        self.comm1.allreduce_(col)
        return (col / float(self.params.m)).cpu().numpy()

    def beta_column_divergence(self):
        """The beta-divergence of the CURRENT factors column by column, over the GLOBAL n columns, each divided by the column's sum of
        a^beta:  stat[c] = sum_i d_beta(a_ic | s'_ic) / sum_i a_ic^beta,  s' = W H + eps,  a^beta := 0 at a = 0 (beta > 0).  Both sums
        scale as lambda^beta when a column is scaled by lambda, so the ratio is scale-invariant for every beta and comparable across k:
        what an NMFk sweep under norm='beta' takes where the Frobenius `column_err()` stands.  At beta = 0 the denominator is the global
        row count and this is `is_column_divergence()`; at beta = 2 it is column_err()^2 / 2.  A column without a positive entry has
        no scale to divide by: nan, as from `column_err()`.  The scheme of `is_column_divergence()`: each rank fills its own column
        range of both arrays with its sums over its own rows, one float64 allreduce (row shards add partial sums, column shards fill
        disjoint ranges), then the ratio."""
        col = self._global_columns(*self._norm_op('beta', "column_div", "beta_column_divergence"))   # [div | pw]: ONE allreduce carries both
        self.comm1.allreduce_(col)
        col = col.cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(col[1] > 0.0, col[0] / col[1], np.nan)

    def column_err(self):
        """pyDNMF.py:221-239: per-column relative error sqrt(sum_i (A - W H)^2 / sum_i A^2) over the GLOBAL n columns
        (each rank fills its own column range, float64 allreduce).  Used once per k by NMFk; the per-column sums come
        from one kernel pass over A (dnmf_column_err: the residual tile stays in accumulators)."""
        if self.topo == '2d' and not hasattr(self, "W_i"):
            self.cart_2d_collect_factors()
        W, H = self._block_factors()
        col_num, col_den = self._global_columns(*self._ops().column_err_sums(self.A_ij, W, H))   # one pass over A, no temporaries
        self.comm1.allreduce_(col_num)                  # (pruned all-zero columns stay 0 / 0 -> nan, as in numpy)
        self.comm1.allreduce_(col_den)
        return torch.sqrt(col_num / col_den).cpu().numpy()
