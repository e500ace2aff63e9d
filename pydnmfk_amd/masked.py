"""Dense data with missing entries: `params.missing = 'nan'`.

A measurement with gaps -- a sensor grid, spectra with dead channels, an assay plate -- arrives as a dense float32 array with NaN in the
gaps.  `MaskedDenseBlock` holds the rank's block exactly as handed over: an entry is OBSERVED iff it is not NaN (a zero is an
observation), and there is no separate mask array -- the kernels (csrc/dnmf_masked.h) test `a == a`, so the mask costs no bytes.  The
update choreography (dist_nmf.py) dispatches on the block: `dist_nmf._is_masked` is true for it, `_is_sparse` is not, and
`engine.ops_for` hands out the `hip-masked` operator set, whose operations that touch A are the masked ones.

Objective, MU rules (fro / kl) and the reported error run over the observed positions only ("Dense data with
missing entries"): method 'mu', one rank and the two 1D grids, 1 <= k <= 128.  `PyNMFk` sweeps such data too: it keeps the raw array,
perturbs it (NaN stays NaN) and lets every `PyNMF` wrap its copy in a block ("NMFk over a NaN-marked block").
"""
import torch

MISSING = "nan"
MAX_K = 128


class MaskedDenseBlock:
    """The rank's float32 block with NaN at the missing positions.  `.tensor` is the 2-D tensor itself (never copied, never written);
    `.n_observed` the count of observed entries; `._sqnorm` the cached ||P_Omega(A)||^2 (a device double, filled by the operator set's
    `sqnorm` on first use: it never changes during a fit)."""

    is_masked_dense = True
    missing = MISSING

    def __init__(self, tensor):
        if not isinstance(tensor, torch.Tensor) or tensor.dim() != 2:
            raise TypeError("MaskedDenseBlock: a 2-D torch tensor is expected, got %s" % (type(tensor),))
        if tensor.dtype != torch.float32:
            raise NotImplementedError("missing='nan' is provided for float32 data only, not for %s" % str(tensor.dtype).replace("torch.", ""))
        if tensor.numel() and tensor.stride(1) != 1:
            raise ValueError("MaskedDenseBlock: the block must be row-major with unit inner stride")
        self.tensor = tensor
        self._sqnorm = None
        self._count = None

    shape = property(lambda self: self.tensor.shape)
    dtype = property(lambda self: self.tensor.dtype)
    device = property(lambda self: self.tensor.device)

    @property
    def n_observed(self):
        if self._count is None:
            self._count = int(torch.count_nonzero(self.tensor == self.tensor))
        return self._count

    def __repr__(self):
        return "MaskedDenseBlock(%d x %d, missing='nan', %s)" % (self.shape[0], self.shape[1], self.device)


def is_masked_dense(x):
    return bool(getattr(x, "is_masked_dense", False))
