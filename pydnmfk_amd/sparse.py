"""A sparse data block: what stands where the dense `A_ij` stands when the data are given as a sparse matrix.

    blk = SparseBlock.from_any(scipy_or_torch_sparse_matrix, device)
    W, H, err = PyNMF(scipy_or_torch_sparse_matrix, params=args).fit()        # PyNMF builds the block itself

The block lives on the device as CSR (int32 row pointers and column indices, float32 values, columns sorted inside a row,
duplicates summed, explicit zeros dropped unless `keep_zeros`) AND as the CSR of its transpose, built once here: A H^T gathers
rows of H^T along the block's rows, W^T A gathers rows of W along the transpose's rows (csrc/dnmf_csr.h).  Rows with more than
`dnmf_csr_seg()` stored entries are listed per image (`long_rows`, `long_segptr`): the kernels cut those into segments.
Building uses torch ops (sort / bincount / cumsum): set-up, not the hot path.  There is no dense image anywhere except in
`to_dense()`, which tests use.

What an UNSTORED entry means is an attribute of the block, `missing`: None (the default) -- a zero that W H must reproduce; 'unstored'
-- not observed: the objective, the update rules and the reported error run over the stored positions only (PyNMF sets it
from `params.missing`).  A stored zero is an observation under that meaning, so such a block is built with `keep_zeros=True`.

Limits: nnz < 2^31, m, n < 2^31 (ValueError); float32 values only (float64 sparse data: NotImplementedError).
"""
import numpy as np
import torch

_I32_MAX = 2 ** 31
SEG_DEFAULT = 1024                     # dnmf_csr_seg() (the library is asked when it is loaded; CPU-only tests use this)


def _seg():
    try:
        from ._lib import lib
        return int(lib.dnmf_csr_seg())
    except Exception:  # noqa: BLE001  (no library on this machine: the checker back ends do not read the long-row lists)
        return SEG_DEFAULT


def _is_scipy_sparse(x):
    mod = type(x).__module__ or ""
    if not mod.startswith("scipy.sparse"):
        return False
    import scipy.sparse as sp                      # lazily: the package imports without scipy
    return sp.issparse(x)


class _StoredPattern:
    """`block != 0`: what utils.data_operations sums along an axis to find all-zero rows / columns (counts of stored entries)"""

    def __init__(self, blk):
        self.blk = blk

    def sum(self, axis):
        return self.blk.nnz_per_row() if axis == 1 else self.blk.nnz_per_col()


def is_sparse_input(x):
    """True for everything PyNMF treats as sparse data: a SparseBlock, a scipy.sparse matrix / array, a torch sparse tensor."""
    if getattr(x, "is_sparse_block", False):
        return True
    if isinstance(x, torch.Tensor):
        return x.layout in (torch.sparse_csr, torch.sparse_coo, torch.sparse_csc)
    return _is_scipy_sparse(x)


def _check_dims(m, n, nnz):
    if m >= _I32_MAX or n >= _I32_MAX:
        raise ValueError("sparse data block: shape %d x %d exceeds the int32 index limit (m, n < 2^31)" % (m, n))
    if nnz >= _I32_MAX:
        raise ValueError("sparse data block: %d stored entries exceed the int32 limit (nnz < 2^31)" % nnz)
    if m < 1 or n < 1:
        raise ValueError("sparse data block: empty shape %d x %d" % (m, n))


def _check_dtype(dt):
    if dt in (torch.float64, np.dtype("float64")):
        raise NotImplementedError("sparse data block: float64 sparse data are not provided (float32 values only); cast the values to float32")
    if dt in (torch.bfloat16, torch.float16, np.dtype("float16")):
        raise NotImplementedError("sparse data block: %s sparse data are not provided (float32 values only)" % (dt,))


MISSING = (None, "unstored")


def _check_missing(missing):
    if missing not in MISSING:
        raise ValueError("sparse data block: missing=%r is not known (None: unstored entries are zeros; 'unstored': they are "
                         "not observed)" % (missing,))
    return missing


class SparseBlock:
    is_sparse_block = True
    dtype = torch.float32
    missing = None

    def __init__(self, crow, col, val, shape, _trusted=False, keep_zeros=False, missing=None):
        """Raw device arrays of a CSR block: `crow` [m + 1], `col` [nnz], `val` [nnz], `shape` = (m, n).  Unless they come from
        this module's own builders the arrays are re-normalised (columns sorted, duplicates summed, zeros dropped unless
        `keep_zeros`).  `missing`: what an unstored entry means (module docstring)."""
        m, n = int(shape[0]), int(shape[1])
        self.missing = _check_missing(missing)
        _check_dims(m, n, int(col.numel()))
        _check_dtype(val.dtype)
        if crow.numel() != m + 1 or col.numel() != val.numel():
            raise ValueError("sparse data block: crow has %d entries for %d rows, col %d, val %d" % (crow.numel(), m, col.numel(), val.numel()))
        if not _trusted:
            counts = (crow[1:] - crow[:-1]).long()
            rows = torch.repeat_interleave(torch.arange(m, device=col.device), counts)
            blk = SparseBlock.from_coo(rows, col, val, (m, n), keep_zeros=keep_zeros, missing=missing)
            self.__dict__.update(blk.__dict__)
            return
        self.shape = (m, n)
        self.crow, self.col, self.val = crow.to(torch.int32).contiguous(), col.to(torch.int32).contiguous(), val.to(torch.float32).contiguous()
        self.nnz = int(self.col.numel())
        self._build_transpose()
        self.long_rows, self.long_segptr, self.n_long, self.nseg = self._bins(self.crow)
        self.t_long_rows, self.t_long_segptr, self.t_n_long, self.t_nseg = self._bins(self.t_crow)

    # ---- builders
    @classmethod
    def from_coo(cls, rows, cols, vals, shape, keep_zeros=False, missing=None):
        """Entries (rows[i], cols[i]) = vals[i] in any order on one device; duplicates are summed (in float64, rounded once),
        entries that are or sum to zero are dropped -- or, with `keep_zeros`, stay stored (observed zeros of a block whose
        unstored entries are missing)."""
        m, n = int(shape[0]), int(shape[1])
        _check_dims(m, n, int(vals.numel()))
        _check_dtype(vals.dtype)
        dev = vals.device
        if vals.numel():
            lo_r, hi_r, lo_c, hi_c = int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())
            if lo_r < 0 or hi_r >= m or lo_c < 0 or hi_c >= n:
                raise ValueError("sparse data block: an index lies outside the %d x %d shape" % (m, n))
        key = rows.long() * n + cols.long()
        key, perm = torch.sort(key, stable=True)
        vals = vals.to(torch.float32)[perm]
        del perm
        if key.numel() > 1:
            first = torch.ones(key.numel(), dtype=torch.bool, device=dev)
            torch.ne(key[1:], key[:-1], out=first[1:])
            if not bool(first.all()):
                seg = torch.cumsum(first, 0) - 1
                key = key[first]
                acc = torch.zeros(key.numel(), dtype=torch.float64, device=dev)
                acc.index_add_(0, seg, vals.double())
                del seg
                vals = acc.float()
                del acc
            del first
        if not keep_zeros:
            keep = vals != 0
            if not bool(keep.all()):
                key, vals = key[keep], vals[keep]
            del keep
        r = torch.div(key, n, rounding_mode="floor")
        col = (key - r * n).to(torch.int32)
        del key
        crow = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(r, minlength=m), 0, out=crow[1:])
        del r
        return cls(crow.to(torch.int32), col, vals, (m, n), _trusted=True, missing=missing)

    @classmethod
    def from_any(cls, x, device, keep_zeros=False, missing=None):
        """A SparseBlock on `device` from a SparseBlock, a scipy.sparse matrix of any format, or a torch sparse tensor.  A
        SparseBlock is taken as it was built: its stored entries and its `missing` attribute are its builder's."""
        device = torch.device(device)
        _check_missing(missing)
        if getattr(x, "is_sparse_block", False):
            return x if x.device == device else x.to(device)
        if isinstance(x, torch.Tensor):
            _check_dtype(x.dtype)
            if x.dim() != 2:
                raise ValueError("sparse data block: a 2-D sparse tensor is expected, got %d-D" % x.dim())
            _check_dims(int(x.shape[0]), int(x.shape[1]), int(x._nnz()))
            if x.layout == torch.sparse_csr:
                crow, col, val = x.crow_indices().to(device), x.col_indices().to(device), x.values().to(device)
                counts = crow[1:] - crow[:-1]
                rows = torch.repeat_interleave(torch.arange(x.shape[0], device=device), counts)
                return cls.from_coo(rows, col, val, x.shape, keep_zeros=keep_zeros, missing=missing)
            if x.layout == torch.sparse_csc:
                x = x.to_sparse_coo()
            idx = x._indices().to(device)
            return cls.from_coo(idx[0], idx[1], x._values().to(device), x.shape, keep_zeros=keep_zeros, missing=missing)
        if _is_scipy_sparse(x):
            _check_dtype(np.dtype(x.dtype))
            _check_dims(int(x.shape[0]), int(x.shape[1]), int(x.nnz))
            c = x.tocoo()
            return cls.from_coo(torch.from_numpy(np.ascontiguousarray(c.row).astype(np.int64)).to(device),
                                torch.from_numpy(np.ascontiguousarray(c.col).astype(np.int64)).to(device),
                                torch.from_numpy(np.ascontiguousarray(c.data).astype(np.float32)).to(device), x.shape,
                                keep_zeros=keep_zeros, missing=missing)
        raise TypeError("sparse data block: cannot be built from %s" % type(x))

    def _build_transpose(self):
        m, n = self.shape
        dev = self.col.device
        counts = (self.crow[1:] - self.crow[:-1]).long()
        rows = torch.repeat_interleave(torch.arange(m, device=dev, dtype=torch.int32), counts)
        # a STABLE sort by column keeps the rows ascending inside a column: the transpose's CSR has sorted indices too
        _, perm = torch.sort(self.col, stable=True)
        self.t_col = rows[perm].contiguous()
        del rows
        self.t_val = self.val[perm].contiguous()
        del perm
        t_crow = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(self.col.long(), minlength=n) if self.nnz else torch.zeros(n, dtype=torch.int64, device=dev), 0,
                     out=t_crow[1:])
        self.t_crow = t_crow.to(torch.int32)

    @staticmethod
    def _bins(crow):
        """Rows by length: (long_rows int32, long_segptr int32, n_long, nseg) for the rows with more than SEG entries."""
        seg = _seg()
        counts = (crow[1:] - crow[:-1]).long()
        long_rows = torch.nonzero(counts > seg).flatten()
        n_long = int(long_rows.numel())
        segptr = torch.zeros(n_long + 1, dtype=torch.int64, device=crow.device)
        if n_long:
            torch.cumsum((counts[long_rows] + seg - 1) // seg, 0, out=segptr[1:])
        nseg = int(segptr[-1])
        return long_rows.to(torch.int32).contiguous(), segptr.to(torch.int32).contiguous(), n_long, nseg

    # ---- what the host classes ask of a data block
    @property
    def device(self):
        return self.val.device

    def to(self, device):
        out = object.__new__(SparseBlock)
        out.__dict__.update({k_: (v.to(device) if isinstance(v, torch.Tensor) else v) for k_, v in self.__dict__.items()})
        return out

    def with_values(self, val, t_val):
        """A block with this block's pattern and new values (NMFk's perturbed copies): `crow` / `col` / `t_crow` / `t_col` and the
        long-row lists are SHARED with this block, `val` (row-image order) and `t_val` (the same entries in the transpose's order)
        are the new block's own.  `missing` carries over; nothing cached from the old values does."""
        if val.shape != self.val.shape or t_val.shape != self.t_val.shape or val.dtype != torch.float32 or t_val.dtype != torch.float32:
            raise ValueError("sparse data block: with_values() takes two float32 arrays of %d values" % self.nnz)
        out = object.__new__(SparseBlock)
        out.__dict__.update({k_: v for k_, v in self.__dict__.items() if k_ != "_sqnorm"})
        out.val, out.t_val = val.contiguous(), t_val.contiguous()
        return out

    def transpose_perm(self):
        """perm with t_val == val[perm]: the stable sort by column that _build_transpose applies (int64, on the block's device)"""
        return torch.sort(self.col, stable=True)[1]

    def nnz_per_row(self):
        return (self.crow[1:] - self.crow[:-1]).long()

    def nnz_per_col(self):
        return (self.t_crow[1:] - self.t_crow[:-1]).long()

    def compact(self, row_keep, col_keep):
        """The block without the rows / columns whose keep-mask is False (pruning, utils.py:156-172): an index remap.  Rows and
        columns that go hold no stored entry here (the masks are counts of STORED entries over the whole grid: all of them
        non-zero by default; under missing='unstored' a stored zero is an observation and counts, so what is pruned is a row or
        column without any observation)."""
        m, n = self.shape
        row_keep, col_keep = row_keep.to(self.device), col_keep.to(self.device)
        counts = self.nnz_per_row()
        if int(counts[~row_keep].sum()) or int(self.nnz_per_col()[~col_keep].sum()):
            raise ValueError("sparse data block: compact() would drop stored entries")
        colmap = (torch.cumsum(col_keep.long(), 0) - 1).to(torch.int32)
        crow = torch.zeros(int(row_keep.sum()) + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(counts[row_keep], 0, out=crow[1:])
        return SparseBlock(crow.to(torch.int32), colmap[self.col.long()], self.val, (int(row_keep.sum()), int(col_keep.sum())), _trusted=True,
                           missing=self.missing)

    # ---- the three expressions utils.data_operations applies to a data block when it prunes (utils.py:117-172), so that its
    # dense lines serve a sparse block unchanged: `ten != 0` -> .sum(1) / .sum(0); `ten[rows][:, cols].contiguous()`
    def __ne__(self, other):
        if isinstance(other, (int, float)) and other == 0:
            # (the stored pattern: non-zero by construction unless the block was built with keep_zeros -- then a stored zero is an
            # observation, and a row / column counts as empty only when nothing of it was observed)
            return _StoredPattern(self)
        return NotImplemented

    __hash__ = object.__hash__

    def __getitem__(self, key):
        m, n = self.shape
        if isinstance(key, torch.Tensor) and key.dtype == torch.bool and key.dim() == 1 and key.numel() == m:
            return self.compact(key, torch.ones(n, dtype=torch.bool, device=self.device))
        if isinstance(key, tuple) and len(key) == 2 and key[0] == slice(None) and isinstance(key[1], torch.Tensor) \
                and key[1].dtype == torch.bool and key[1].numel() == n:
            return self.compact(torch.ones(m, dtype=torch.bool, device=self.device), key[1])
        raise NotImplementedError("a sparse data block is indexed by a boolean row mask or [:, boolean column mask] only "
                                  "(pruning); it is not sliced")

    def contiguous(self):
        return self

    def to_dense(self):
        """The dense image (tests only)."""
        m, n = self.shape
        out = torch.zeros(m, n, dtype=torch.float32, device=self.device)
        rows = torch.repeat_interleave(torch.arange(m, device=self.device), self.nnz_per_row())
        out[rows, self.col.long()] = self.val
        return out

    def __repr__(self):
        return "SparseBlock(%d x %d, nnz=%d, %s%s)" % (self.shape[0], self.shape[1], self.nnz, self.device,
                                                       ", missing=%r" % self.missing if self.missing else "")
