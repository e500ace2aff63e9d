"""Typed wrappers over the C ABI operating on torch CUDA(HIP) tensors.

PyTorch is plumbing here: it owns device memory and the stream; every arithmetic operation
of the hot path runs in libdnmf_hip.so.  All tensors must be float32, on a CUDA device and
row-major with unit inner stride; anything else raises (no silent host fallback).  The one
exception is the data matrix A of the Frobenius paths, which may be STORED as bfloat16 (the
`*_bf16a` entry points: half the HBM bytes, fp32 arithmetic).
"""
import contextlib
import ctypes
import os
import weakref

import torch

from ._lib import DnmfError, PersistentTimeout, check, lib

_ws_cache = {}


def _req(t, name, ndim=2):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch.Tensor on a CUDA device, got %s (no CPU fallback)" % (name, type(t)))
    if not t.is_cuda:
        raise TypeError("%s: tensor is on %s; the MU engine only runs on the GPU (no CPU fallback)" % (name, t.device))
    _same_device(t, name)
    if t.dtype != torch.float32:
        raise TypeError("%s: dtype %s unsupported; the engine computes in float32" % (name, t.dtype))
    if t.dim() != ndim or (t.numel() and t.stride(-1) != 1):
        raise ValueError("%s: must be %d-D row-major with unit inner stride" % (name, ndim))
    return t


def _same_device(t, name):
    """Kernels are launched on the CURRENT device's current stream; a tensor of another GPU would be reached through peer
    access without any ordering against its own stream (or fault).  One process drives one GPU: fail loudly instead."""
    if t.device.index is not None and t.device.index != torch.cuda.current_device():
        raise ValueError("%s lives on %s but the current device is cuda:%d; call torch.cuda.set_device(%d) "
                         "(one process per GPU)" % (name, t.device, torch.cuda.current_device(), t.device.index))


def _req_a(t, name="A"):
    """The data matrix: float32, or bfloat16 STORAGE (Frobenius paths only; arithmetic stays float32)."""
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bfloat16:
        _same_device(t, name)
        if t.dim() != 2 or (t.numel() and t.stride(-1) != 1):
            raise ValueError("%s: must be 2-D row-major with unit inner stride" % name)
        return "_bf16a"
    _req(t, name)
    return ""


def _fn(base, sfx):
    return getattr(lib, "dnmf_" + base + sfx)


def _ld(t):
    # stride(0) == 0 (a row broadcast with .expand) is passed through: every row aliases the same memory
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _req_g(G, k, name="G"):
    """a Gram buffer the library WRITES: the zero-padded KP x KP block with ld = KP (include/dnmf.h) -- its size is part of the
    contract (KP = 256 for 128 < k <= 256), so a smaller tensor is refused here rather than overrun there"""
    _req(G, name)
    n = kp(k)
    if G.shape[0] < n or G.shape[1] != n or G.stride(0) != n:
        raise ValueError("%s: rank %d needs the contiguous %d x %d Gram buffer (dnmf_kp), got %s with pitch %d" % (name, k, n, n, tuple(G.shape), G.stride(0)))
    return G


_downgraded = False


def persistent_off(reason=""):
    """For the rest of this process every path takes its launch-chain kernels (dnmf_set_persistent(0)): called by PyNMF when a kernel
    that needs the GPU to itself has timed out.  Warns once."""
    global _downgraded
    lib.dnmf_set_persistent(0)
    if not _downgraded:
        _downgraded = True
        import warnings
        warnings.warn("pydnmfk_amd: a persistent kernel lost its residency (%s); this process continues on the launch-chain kernels "
                      "-- same results, no co-residency needed (dnmf_set_persistent(1) switches back)" % (reason or "shared GPU"), RuntimeWarning, stacklevel=3)


def kp(k):
    v = lib.dnmf_kp(int(k))
    if v < 0:
        raise ValueError("rank k=%d unsupported (1 <= k <= 256)" % k)
    return v


def _scratch(nbytes, device):
    """ONE scratch buffer per (device, stream), grown on demand and shared by every operator set (fp32 and bf16x6 entry points
    alike: calls are stream-ordered and none keeps state in the scratch between calls)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = None
        _ws_cache.pop(key, None)                # release the smaller buffer before asking for the larger one
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def workspace(m, n, k, device):
    """Scratch buffer large enough for any entry point on an m x n block: one buffer per device, grown on demand (an
    NMFk sweep over k would otherwise keep one buffer per rank alive).  Stream-ordered reuse: every entry point is
    enqueued on the current stream, so consecutive calls never overlap on the scratch."""
    nbytes = lib.dnmf_ws_bytes(int(m), int(n), int(k))
    if nbytes == 0:
        raise ValueError("bad problem shape m=%d n=%d k=%d" % (m, n, k))
    return _scratch(nbytes, device)


def stack_alloc(B, rows, cols, dtype, device):
    """[B][rows][cols] with contiguous members whose distance is a multiple of 16 bytes -- the layout the batched whole-fit
    entry points take (include/dnmf.h: every problem then has problem 0's alignment)."""
    per = 16 // torch.empty(0, dtype=dtype).element_size()
    stride = -(-(rows * cols) // per) * per
    return torch.empty(B * stride, dtype=dtype, device=device).as_strided((B, rows, cols), (stride, cols, 1))


_HALS_MAX_WG = 1024                      # slots per column of the persistent HALS W sweep (csrc/dnmf_common.h)


def new_gram(k, device):
    return torch.zeros(kp(k), kp(k), dtype=torch.float32, device=device)


# ---- the transposed image of A (csrc/dnmf_timg.hip): the W phase of MU/Frobenius at 32 < k <= 64 streams
# At = A^T instead of A.  Results are bit-equal with and without it, so everything here only decides WHEN an image exists.
# One slot per device.  A slot belongs to ONE tensor object (weak reference; its death frees the image) in ONE state: the key
# is (A._version, data_ptr, shape, strides), and any mismatch throws the slot away -- an image never outlives a change of A
# that torch can see.  Writes torch cannot see (library calls that write through data_ptr()) call _wimage_forget.
WIMAGE_RESERVE = 2 << 30        # device memory that must stay free after an image is allocated (else the step stays on A)
_wimage_slots = {}


def wimage_mode_from_env(environ):
    """DNMF_WIMAGE=0|1|2 -> the mode to set at import (None: leave the library's default, 1 = auto)"""
    v = environ.get("DNMF_WIMAGE", "").strip()
    return int(v) if v in ("0", "1", "2") else None


def set_wimage(mode):
    """0 off, 1 auto (blocks whose shape the library's sweep found to gain, from their second consecutive call), 2 forced (built on first sight).
    Returns the previous mode; switching off frees every image."""
    was = lib.dnmf_set_wimage(int(mode))
    if int(mode) == 0:
        _wimage_slots.clear()
    return was


def _wimage_mode():
    return lib.dnmf_set_wimage(-1)                    # (values outside 0..2 only query)


class _WimageSlot:
    __slots__ = ("ref", "key", "buf", "ldat", "event", "refused")


def _wimage_key(A):
    return (A._version, A.data_ptr(), tuple(A.shape), tuple(A.stride()))


def _wimage_forget(t):
    """`t` is about to be written behind torch's back: drop the image of whatever tensor shares its storage"""
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    slot = _wimage_slots.get(dev)
    if slot is None:
        return
    A = slot.ref()
    if A is None or A.untyped_storage().data_ptr() == t.untyped_storage().data_ptr():
        _wimage_slots.pop(dev, None)


def _wimage_reaper(dev):
    def dead(r):                                      # the imaged tensor has been collected: free its image
        slot = _wimage_slots.get(dev)
        if slot is not None and slot.ref is r:
            _wimage_slots.pop(dev, None)
    return dead


def _wimage_lookup(A, H, W, G=None):
    """The slot whose image the next library call on (A, H, W) may use, or None.  Builds the image when it is due."""
    mode = _wimage_mode()
    if mode == 0 or A.dtype != torch.float32 or A.dim() != 2 or A._base is not None or not A.is_cuda:
        return None
    m, n = A.shape
    k = H.shape[0]
    lda = _ld(A)
    plan = (ctypes.c_int * 6)()
    a_ok = A.data_ptr() % 16 == 0 and H.data_ptr() % 16 == 0 and _ld(H) % 4 == 0
    w_ok = W.data_ptr() % 16 == 0 and _ld(W) % 4 == 0 and (G is None or G.data_ptr() % 16 == 0) and (128 * _ld(W) + 64) * 4 < 2**31 - 1
    lib.dnmf_wimage_plan(m, n, k, lda, int(a_ok), int(w_ok), plan)
    if not plan[0]:
        return None                                   # (the slot of another tensor, if any, stays: this call never binds)
    dev = A.device.index if A.device.index is not None else torch.cuda.current_device()
    key = _wimage_key(A)
    slot = _wimage_slots.get(dev)
    if slot is None or slot.ref() is not A or slot.key != key:
        _wimage_slots.pop(dev, None)                  # frees the old image before a new one is asked for
        slot = _WimageSlot()
        slot.ref = weakref.ref(A, _wimage_reaper(dev))
        slot.key, slot.buf, slot.ldat, slot.event, slot.refused = key, None, 0, None, False
        _wimage_slots[dev] = slot
        if mode != 2:
            return None                               # auto: first sight -- the image is built on the second consecutive call
    if slot.buf is None:
        if slot.refused:
            return None
        nbytes = lib.dnmf_wimage_bytes(m, n)
        free, _ = torch.cuda.mem_get_info(A.device)
        if free - nbytes < WIMAGE_RESERVE:
            slot.refused = True
            return None
        try:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=A.device)
        except torch.cuda.OutOfMemoryError:
            slot.refused = True
            return None
        ldat = -(-m // 4) * 4
        check(lib.dnmf_wimage_build(A.data_ptr(), m, n, lda, buf.data_ptr(), ldat, _stream()))
        slot.buf, slot.ldat = buf, ldat
        slot.event = torch.cuda.current_stream().record_event()
    else:
        torch.cuda.current_stream().wait_event(slot.event)      # (a no-op on the stream that built it)
    return slot


class _wimage_bound:
    """with _wimage_bound(A, H, W): the library call inside sees A's image, if there is one; unbound on every exit path"""

    def __init__(self, A, H, W, G=None):
        self.slot = _wimage_lookup(A, H, W, G)
        self.A = A

    def __enter__(self):
        if self.slot is not None:
            A = self.A
            check(lib.dnmf_wimage_bind(A.data_ptr(), A.shape[0], A.shape[1], _ld(A), self.slot.buf.data_ptr(), self.slot.ldat))
        return self

    def __exit__(self, *exc):
        if self.slot is not None:
            lib.dnmf_wimage_unbind()
        return False


class ClockProbe:
    """The shader clock the GPU holds while other work runs (dnmf_clock_probe; a measurement aid, bench.py / tools).

        probe = ClockProbe(duration_ms)      # starts one sampling wave on a stream of its own, returns at once
        ... enqueue the work on the current stream, synchronise ...
        ghz = probe.held_ghz(t0_ms, t1_ms)   # median clock between t0 and t1 after the probe started (None: no samples)
    """

    def __init__(self, duration_ms, device=None, period_us=20.0):
        naps = max(1, int(round(period_us / 4.0)))
        self.n = max(8, int(duration_ms * 1000.0 / (naps * 4.0) * 1.5) + 64)   # naps are ~4 us at 2 GHz, longer when the clock drops
        self.buf = torch.zeros(2 * self.n, dtype=torch.int64, device=device or torch.device("cuda", torch.cuda.current_device()))
        self.stream = torch.cuda.Stream(device=self.buf.device)
        self.stream.wait_stream(torch.cuda.current_stream())          # (the zero fill above ran on the current stream)
        check(lib.dnmf_clock_probe(self.buf.data_ptr(), self.n, naps, self.stream.cuda_stream))

    def samples(self):
        """(t_ms since the probe's first sample, GHz over the interval that ends there), after a device synchronisation"""
        self.stream.synchronize()
        b = self.buf.cpu().view(-1, 2).double()
        b = b[b[:, 1] > 0]
        if b.shape[0] < 2:
            return torch.empty(0), torch.empty(0)
        ghz = (b[1:, 0] - b[:-1, 0]) / (b[1:, 1] - b[:-1, 1]) * 0.1
        return (b[1:, 1] - b[0, 1]) * 1e-5, ghz

    def held_ghz(self, t0_ms=0.0, t1_ms=float("inf")):
        t, ghz = self.samples()
        x = ghz[(t >= t0_ms) & (t <= t1_ms)]
        return float(x.median()) if x.numel() else None


class HipOps:
    """The operator set the update choreography (dist_nmf.py) is written against."""

    name = "hip"

    # ---- grams
    def gram_hht(self, H, out):
        _req(H, "H"); _req_g(out, H.shape[0])
        k, n = H.shape
        ws = workspace(k, n, k, H.device)
        check(lib.dnmf_gram_hht(H.data_ptr(), k, n, _ld(H), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def gram_wtw(self, W, out):
        _req(W, "W"); _req_g(out, W.shape[1])
        m, k = W.shape
        ws = workspace(m, k, k, W.device)
        check(lib.dnmf_gram_wtw(W.data_ptr(), m, k, _ld(W), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out

    # ---- big contractions
    def aht(self, A, H, out):
        sfx = _req_a(A); _req(H, "H"); _req(out, "AH")
        m, n = A.shape
        k = H.shape[0]
        check(_fn("aht", sfx)(A.data_ptr(), m, n, _ld(A), H.data_ptr(), k, _ld(H), out.data_ptr(), _ld(out), _stream()))
        return out

    def aht_hblocks(self, A, Hs, out):
        """aht with H as column blocks: `Hs` is the contiguous stack [n / n_h][k][n_h] an allgather of the slices leaves
        (float32 A; n_h a multiple of 32)."""
        _req(A, "A"); _req(Hs, "Hs", 3); _req(out, "AH")
        m, n = A.shape
        nb, k, nh = Hs.shape
        if not Hs.is_contiguous() or nb * nh != n:
            raise ValueError("aht_hblocks: Hs must be a contiguous [n / n_h][k][n_h] stack matching A")
        check(lib.dnmf_aht_hblocks(A.data_ptr(), m, n, _ld(A), Hs.data_ptr(), nh, k, out.data_ptr(), _ld(out), _stream()))
        return out

    def wta(self, A, W, out):
        sfx = _req_a(A); _req(W, "W"); _req(out, "AtW")
        m, n = A.shape
        k = W.shape[1]
        ws = workspace(m, n, k, A.device)
        check(_fn("wta", sfx)(A.data_ptr(), m, n, _ld(A), W.data_ptr(), k, _ld(W), out.data_ptr(), _ld(out),
                           ws.data_ptr(), ws.numel(), _stream()))
        return out

    def wta_gram(self, A, W, out, G):
        """out = W^T A and G = W^T W (KP x KP, zero padded): the H phase's two reductions (dist_nmf.py:705, :747-748); for k <= 16
        the Gram rides in the W^T A launches (dnmf_wta_gram).  Operator sets that override `wta` keep their own product."""
        if type(self).wta is not HipOps.wta:
            self.gram_wtw(W, G)
            return self.wta(A, W, out)
        sfx = _req_a(A); _req(W, "W"); _req(out, "AtW"); _req_g(G, W.shape[1])
        m, n = A.shape
        k = W.shape[1]
        ws = workspace(m, n, k, A.device)
        check(_fn("wta_gram", sfx)(A.data_ptr(), m, n, _ld(A), W.data_ptr(), k, _ld(W), out.data_ptr(), _ld(out), G.data_ptr(),
                                ws.data_ptr(), ws.numel(), _stream()))
        return out

    # ---- updates
    def mu_update_w(self, W, AH, G, eps):
        _req(W, "W"); _req(AH, "AH"); _req(G, "G")
        m, k = W.shape
        check(lib.dnmf_mu_update_w(W.data_ptr(), m, k, _ld(W), AH.data_ptr(), _ld(AH), G.data_ptr(), float(eps),
                                   _stream()))

    def mu_update_h(self, H, AtW, G, eps, clamp=False):
        _req(H, "H"); _req(AtW, "AtW"); _req(G, "G")
        k, n = H.shape
        check(lib.dnmf_mu_update_h(H.data_ptr(), k, n, _ld(H), AtW.data_ptr(), _ld(AtW), G.data_ptr(), float(eps),
                                   int(bool(clamp)), _stream()))

    def aht_update_w(self, A, H, G, W, eps):
        sfx = _req_a(A); _req(H, "H"); _req(G, "G"); _req(W, "W")
        m, n = A.shape
        k = H.shape[0]
        if k > 128:      # beyond the fused kernel's rank: the product (two passes over A), then the update
            AH = torch.empty(m, k, dtype=torch.float32, device=W.device)
            self.aht(A, H, AH)
            return self.mu_update_w(W, AH, G, eps)
        with _wimage_bound(A, H, W, G):
            check(_fn("aht_update_w", sfx)(A.data_ptr(), m, n, _ld(A), H.data_ptr(), k, _ld(H), G.data_ptr(), W.data_ptr(),
                                        _ld(W), float(eps), _stream()))

    def mu_fro_step(self, A, W, H, eps, w_update=True, clamp=False):
        sfx = _req_a(A); _req(W, "W"); _req(H, "H")
        m, n = A.shape
        k = W.shape[1]
        ws = workspace(m, n, k, A.device)
        with _wimage_bound(A, H, W):
            check(_fn("mu_fro_step", sfx)(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), k,
                                       float(eps), int(bool(w_update)), int(bool(clamp)), ws.data_ptr(), ws.numel(),
                                       _stream()))

    # ---- HALS sweeps
    def hals_ss2(self, k, like):
        """k device doubles: per-column sums of squares of the W sweep."""
        return torch.zeros(k, dtype=torch.float64, device=like.device)

    def hals_w_col(self, W, AH, G, kk, ss2, eps):
        _req(W, "W"); _req(AH, "AH"); _req(G, "G")
        m, k = W.shape
        prev = ss2[kk - 1:].data_ptr() if kk > 0 else None
        check(lib.dnmf_hals_w_col(W.data_ptr(), m, k, _ld(W), AH.data_ptr(), _ld(AH), G.data_ptr(), int(kk), prev,
                                  float(eps), ss2[kk:].data_ptr(), _stream()))

    def hals_w_scale(self, W, col, ss2):
        _req(W, "W")
        check(lib.dnmf_hals_w_scale(W.data_ptr(), W.shape[0], _ld(W), int(col), ss2[col:].data_ptr(), _stream()))

    def hals_update_w(self, W, AH, G, eps):
        """The whole W sweep of a rank with local column norms: one persistent launch when the rows fit on the device at
        once, else one launch per column (decided inside the library).  Returns the k column sums of squares (device doubles)."""
        _req(W, "W"); _req(AH, "AH"); _req(G, "G")
        m, k = W.shape
        ws = workspace(m, k, k, W.device)
        check(lib.dnmf_hals_sweep_w(W.data_ptr(), m, k, _ld(W), AH.data_ptr(), _ld(AH), G.data_ptr(), float(eps),
                                    ws.data_ptr(), ws.numel(), _stream()))
        # the k column sums of squares: the library keeps them behind the slot slab of its workspace (dnmf_hals_sweep_w, csrc/dnmf_hals.hip:
        # KP x HALS_MAX_WG slots of 8 bytes)
        off = kp(k) * _HALS_MAX_WG * 8
        return ws[off:off + 8 * k].view(torch.float64).clone()

    def hals_sweep_plan(self, W, AH):
        """What `hals_update_w` runs for these views on this device (dnmf_hals_sweep_plan): (route, KP, grid, transform, vec, cap) --
        route 1 = the persistent sweep, 0 = column launches; see include/dnmf.h."""
        import ctypes
        out = (ctypes.c_int * 6)()
        check(lib.dnmf_hals_sweep_plan(W.shape[0], W.shape[1], _ld(W), _ld(AH), int(W.data_ptr() % 16 == 0), int(AH.data_ptr() % 16 == 0), out))
        return tuple(out)

    def hals_check(self):
        """Raise if a persistent W sweep on this device gave up waiting for its other workgroups (they were not co-resident:
        another process or stream shared the GPU).  W is NaN after such a sweep; `params.hals_sweep = 'columns'` selects the
        one-launch-per-column sweep, which needs no co-residency.  Synchronises the current stream."""
        import ctypes
        flag = ctypes.c_int(0)
        check(lib.dnmf_hals_sweep_status(ctypes.byref(flag), _stream()))
        if flag.value:
            raise PersistentTimeout("a persistent kernel (the HALS W sweep, the whole-fit kernel of a small problem, the one-pass MU/FRO step) "
                                    "timed out -- its workgroups were not all resident (is the GPU shared with another process or stream?); the "
                                    "factors are invalid.  PyNMF fits again on the launch-chain kernels (dnmf_set_persistent(0)); through the C ABI: "
                                    "dnmf_set_persistent(0), or hals_sweep = 'columns' / fit_loop = 'python' per fit.")

    def hals_update_w_columns(self, W, AH, G, eps):
        """The same sweep as k column launches (what the persistent kernel falls back to; kept callable for A/B tests).  Returns the k
        column sums of squares (device doubles)."""
        _req(W, "W"); _req(AH, "AH"); _req(G, "G")
        m, k = W.shape
        ss2 = self.hals_ss2(k, W)
        check(lib.dnmf_hals_update_w(W.data_ptr(), m, k, _ld(W), AH.data_ptr(), _ld(AH), G.data_ptr(), float(eps),
                                     ss2.data_ptr(), _stream()))
        return ss2

    def hals_update_h(self, H, AtW, G, eps):
        _req(H, "H"); _req(AtW, "AtW"); _req(G, "G")
        k, n = H.shape
        check(lib.dnmf_hals_update_h(H.data_ptr(), k, n, _ld(H), AtW.data_ptr(), _ld(AtW), G.data_ptr(), float(eps),
                                     _stream()))

    # ---- KL
    def kl_uht(self, A, W, H, eps, out):
        _req(A, "A"); _req(W, "W"); _req(H, "H"); _req(out, "UHT")
        m, n = A.shape
        k = W.shape[1]
        ws = workspace(m, n, k, A.device)
        check(lib.dnmf_kl_uht(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), k, float(eps),
                              out.data_ptr(), _ld(out), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def kl_uht_hblocks(self, A, W, Hs, eps, out):
        """kl_uht with H as column blocks: `Hs` is the contiguous stack [n / n_h][k][n_h] an allgather of the slices leaves."""
        _req(A, "A"); _req(W, "W"); _req(Hs, "Hs", 3); _req(out, "UHT")
        m, n = A.shape
        nb, k, nh = Hs.shape
        if not Hs.is_contiguous() or nb * nh != n or k != W.shape[1]:
            raise ValueError("kl_uht_hblocks: Hs must be a contiguous [n / n_h][k][n_h] stack matching A and W")
        nbytes = lib.dnmf_ws_bytes_hblocks(int(m), int(n), int(k), int(nh))
        if nbytes == 0:
            raise ValueError("kl_uht_hblocks: bad shape m=%d n=%d k=%d n_h=%d" % (m, n, k, nh))
        ws = _scratch(nbytes, A.device)
        check(lib.dnmf_kl_uht_hblocks(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), Hs.data_ptr(), nh, k, float(eps),
                                      out.data_ptr(), _ld(out), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def kl_wtu(self, A, W, H, eps, out):
        _req(A, "A"); _req(W, "W"); _req(H, "H"); _req(out, "WTU")
        m, n = A.shape
        k = W.shape[1]
        ws = workspace(m, n, k, A.device)
        check(lib.dnmf_kl_wtu(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), k, float(eps),
                              out.data_ptr(), _ld(out), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def rowsum(self, H, out):
        _req(H, "H"); _req(out, "x", 1)
        k, n = H.shape
        check(lib.dnmf_rowsum(H.data_ptr(), k, n, _ld(H), out.data_ptr(), _stream()))
        return out

    def colsum(self, W, out):
        _req(W, "W"); _req(out, "x", 1)
        m, k = W.shape
        ws = workspace(m, k, k, W.device)
        check(lib.dnmf_colsum(W.data_ptr(), m, k, _ld(W), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def kl_update_w(self, W, S, x, eps):
        _req(W, "W"); _req(S, "S"); _req(x, "x", 1)
        m, k = W.shape
        check(lib.dnmf_kl_update_w(W.data_ptr(), m, k, _ld(W), S.data_ptr(), _ld(S), x.data_ptr(), float(eps),
                                   _stream()))

    def kl_update_h(self, H, S, x, eps, clamp=False):
        _req(H, "H"); _req(S, "S"); _req(x, "x", 1)
        k, n = H.shape
        check(lib.dnmf_kl_update_h(H.data_ptr(), k, n, _ld(H), S.data_ptr(), _ld(S), x.data_ptr(), float(eps),
                                   int(bool(clamp)), _stream()))

    def mu_kl_step(self, A, W, H, eps, w_update=True, clamp=False):
        _req(A, "A"); _req(W, "W"); _req(H, "H")
        m, n = A.shape
        k = W.shape[1]
        ws = workspace(m, n, k, A.device)
        check(lib.dnmf_mu_kl_step(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), k,
                                  float(eps), int(bool(w_update)), int(bool(clamp)), ws.data_ptr(), ws.numel(),
                                  _stream()))

    # ---- fit helpers
    def clamp_min(self, X, eps):
        _req(X, "X")
        check(lib.dnmf_clamp_min(X.data_ptr(), X.shape[0], X.shape[1], _ld(X), float(eps), _stream()))

    def scale_cols_div(self, W, s, eps):
        _req(W, "W"); _req(s, "s", 1)
        check(lib.dnmf_scale_cols_div(W.data_ptr(), W.shape[0], W.shape[1], _ld(W), s.data_ptr(), float(eps),
                                      _stream()))

    def scale_rows_mul(self, H, s):
        _req(H, "H"); _req(s, "s", 1)
        check(lib.dnmf_scale_rows_mul(H.data_ptr(), H.shape[0], H.shape[1], _ld(H), s.data_ptr(), _stream()))

    def perturb_uniform(self, X, noise_var, seed, out=None):
        """X * (1 + nv + 2 nv U[0,1)) element-wise in ONE pass (NMFk's `sample.randM`, pyDNMFk.py:42-44), in X's storage type
        (float32 or bfloat16), any shape: the value of an element depends on (seed, position) only.  None for tensors the
        kernel does not take (not 2-D / strided columns: the caller keeps its torch expression).  `out`:
        a contiguous destination of X's shape and type (else a new tensor)."""
        if not (X.is_cuda and X.dim() == 2 and X.dtype in (torch.float32, torch.bfloat16) and X.stride(1) == 1):
            return None
        rows, cols = X.shape
        ld = _ld(X)
        if out is None or out.shape != X.shape or out.dtype != X.dtype or not out.is_contiguous():
            out = torch.empty(rows, cols, dtype=X.dtype, device=X.device)
        _wimage_forget(out)          # written through its raw pointer: torch's version counter does not see it
        check(lib.dnmf_perturb_uniform(X.data_ptr(), out.data_ptr(), rows, cols, ld, cols, float(noise_var), int(seed) & (2**64 - 1),
                                       int(X.dtype == torch.bfloat16), _stream()))
        return out

    def sqnorm(self, A):
        sfx = _req_a(A)
        out = torch.empty(1, dtype=torch.float64, device=A.device)
        check(_fn("sqnorm", sfx)(A.data_ptr(), A.shape[0], A.shape[1], _ld(A), out.data_ptr(), _stream()))
        return out

    def resid_sqnorm(self, A, W, H):
        sfx = _req_a(A); _req(W, "W"); _req(H, "H")
        out = torch.empty(1, dtype=torch.float64, device=A.device)
        ws = workspace(A.shape[0], A.shape[1], W.shape[1], A.device)      # room for the zero-padded factor images (ragged ranks)
        check(_fn("resid_sqnorm_ws", sfx)(A.data_ptr(), A.shape[0], A.shape[1], _ld(A), W.data_ptr(), _ld(W), H.data_ptr(),
                                       _ld(H), W.shape[1], out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def column_err_sums(self, A, W, H):
        """(num, den): per-column sums over this rank's rows of (A - W H)^2 and A^2, fp64 device vectors of length n."""
        sfx = _req_a(A); _req(W, "W"); _req(H, "H")
        n = A.shape[1]
        out = torch.zeros(2, n, dtype=torch.float64, device=A.device)
        check(_fn("column_err", sfx)(A.data_ptr(), A.shape[0], n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H),
                                  W.shape[1], out[0].data_ptr(), out[1].data_ptr(), _stream()))
        return out[0], out[1]

    # ---- BCD primitives (csrc/dnmf_bcd.hip; the choreography is dist_nmf._Base._bcd).  `st` is the method's float64 state block
    # (16 device doubles): every scalar of an iteration stays in it, nothing here returns a value to the host.
    def bcd_state(self, like):
        return torch.zeros(16, dtype=torch.float64, device=like.device)

    @staticmethod
    def _req_d(t, name, numel):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() >= numel):
            raise TypeError("%s: expected a contiguous float64 CUDA tensor of at least %d elements" % (name, numel))
        _same_device(t, name)

    def bcd_state_init(self, st, sq):
        self._req_d(st, "st", 16); self._req_d(sq, "sq", 3)
        check(lib.dnmf_bcd_state_init(st.data_ptr(), sq.data_ptr(), _stream()))

    def bcd_init_factor(self, X0, Xold, Xm, st, which):
        _req(X0, "X0"); _req(Xold, "X_old"); _req(Xm, "X_m"); self._req_d(st, "st", 16)
        r, c = X0.shape
        if Xold.shape != X0.shape or Xm.shape != X0.shape:
            raise ValueError("bcd_init_factor: shapes differ")
        check(lib.dnmf_bcd_init_factor(X0.data_ptr(), r, c, _ld(X0), Xold.data_ptr(), _ld(Xold), Xm.data_ptr(), _ld(Xm), st.data_ptr(),
                                       int(which), _stream()))

    def bcd_lipschitz(self, G, k, st, which):
        _req_g(G, k); self._req_d(st, "st", 16)
        check(lib.dnmf_bcd_lipschitz(G.data_ptr(), int(k), st.data_ptr(), int(which), _stream()))

    def bcd_update_w(self, Wm, AH, G, st, W, s):
        _req(Wm, "Wm"); _req(AH, "AH"); _req(W, "W"); _req(s, "s", 1); self._req_d(st, "st", 16)
        m, k = W.shape
        _req_g(G, k)
        if Wm.shape != W.shape or AH.shape != W.shape or s.numel() < k:
            raise ValueError("bcd_update_w: shapes W %s, Wm %s, AH %s, s %s" % (tuple(W.shape), tuple(Wm.shape), tuple(AH.shape), tuple(s.shape)))
        ws = _scratch(lib.dnmf_bcd_ws_bytes_w(int(m), int(k)), W.device)
        check(lib.dnmf_bcd_update_w(Wm.data_ptr(), _ld(Wm), AH.data_ptr(), _ld(AH), G.data_ptr(), m, k, st.data_ptr(), W.data_ptr(), _ld(W),
                                    s.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))

    def bcd_scale_cols(self, W, s):
        _req(W, "W"); _req(s, "s", 1)
        check(lib.dnmf_bcd_scale_cols(W.data_ptr(), W.shape[0], W.shape[1], _ld(W), s.data_ptr(), _stream()))

    def bcd_update_h(self, Hm, AtW, G, st, H):
        _req(Hm, "Hm"); _req(AtW, "AtW"); _req(H, "H"); self._req_d(st, "st", 16)
        k, n = H.shape
        _req_g(G, k)
        if Hm.shape != H.shape or AtW.shape != H.shape:
            raise ValueError("bcd_update_h: shapes H %s, Hm %s, AtW %s" % (tuple(H.shape), tuple(Hm.shape), tuple(AtW.shape)))
        check(lib.dnmf_bcd_update_h(Hm.data_ptr(), _ld(Hm), AtW.data_ptr(), _ld(AtW), G.data_ptr(), k, n, st.data_ptr(), H.data_ptr(), _ld(H),
                                    _stream()))

    def bcd_decide(self, st, sq):
        self._req_d(st, "st", 16); self._req_d(sq, "sq", 1)
        check(lib.dnmf_bcd_decide(st.data_ptr(), sq.data_ptr(), _stream()))

    def bcd_extrapolate(self, W, Wold, Wm, H, Hold, Hm, AH, AHk, G, Gk, st):
        for t, nm in ((W, "W"), (Wold, "W_old"), (Wm, "Wm"), (H, "H"), (Hold, "H_old"), (Hm, "Hm"), (AH, "AH"), (AHk, "AH kept")):
            _req(t, nm)
        m, k = W.shape
        n = H.shape[1]
        _req_g(G, k); _req_g(Gk, k); self._req_d(st, "st", 16)
        if not (Wold.shape == Wm.shape == AH.shape == AHk.shape == W.shape and Hold.shape == Hm.shape == H.shape and H.shape[0] == k):
            raise ValueError("bcd_extrapolate: shapes do not match")
        check(lib.dnmf_bcd_extrapolate(W.data_ptr(), _ld(W), Wold.data_ptr(), _ld(Wold), Wm.data_ptr(), _ld(Wm), m, H.data_ptr(), _ld(H),
                                       Hold.data_ptr(), _ld(Hold), Hm.data_ptr(), _ld(Hm), n, k, AH.data_ptr(), _ld(AH), AHk.data_ptr(),
                                       _ld(AHk), G.data_ptr(), Gk.data_ptr(), st.data_ptr(), _stream()))

    # ---- whole fits (csrc/dnmf_fit.hip, csrc/dnmf_bcd.hip)
    def fit(self, method, norm, A, W, H, eps, w_update, itr, column_sweep=False):
        """`itr` update steps (clamp after the steps i % 10 == 0), normalize_features and the squared norms of relative_err in
        ONE library call (dnmf_{mu_fro,mu_kl,hals_fro}_fit; pyDNMF.py:138-182 on one rank).  A, W, H are matrices -- one
        problem -- or stacks [B][m][n], [B][m][k], [B][k][n] of B same-shape problems that every launch then covers together
        (blockIdx.z = problem; bit-identical to B single fits).  W, H are updated in place; returns the device tensor
        [B][2] of {sum (A - W H)^2, sum A^2}.  norm 'is' (method 'mu', one problem): `is_fit`, dnmf_is_mu_fit."""
        method, norm = method.lower(), norm.lower()
        batched = A.dim() == 3
        if W.dim() != A.dim() or H.dim() != A.dim():
            raise ValueError("fit: A, W, H must all be matrices or all be stacks")
        if norm == "is":                                   # dnmf_is_mu_fit: one problem per call
            if method != "mu" or batched:
                raise NotImplementedError("norm='is' is provided for method 'mu' on one problem per call, not for '%s'%s"
                                          % (method, " on a stack" if batched else ""))
            return self.is_fit(A, W, H, eps, w_update, itr)
        A3, W3, H3 = (A, W, H) if batched else (A[None], W[None], H[None])
        sfx = _req_a(A3[0]); _req(W3[0], "W"); _req(H3[0], "H")
        B, m, n = A3.shape
        k = W3.shape[2]
        if W3.shape != (B, m, k) or H3.shape != (B, k, n):
            raise ValueError("fit: shapes A %s, W %s, H %s do not match" % (tuple(A3.shape), tuple(W3.shape), tuple(H3.shape)))
        if (norm, method) == ("fro", "bcd"):
            return self._bcd_fit(A3, W3, H3, eps, w_update, itr, sfx, batched)
        if (norm, method) == ("kl", "mu"):
            if sfx:
                raise TypeError("fit: KL needs float32 data")
            fn, extra = lib.dnmf_mu_kl_fit, ()
        elif (norm, method) == ("fro", "mu"):
            fn, extra = _fn("mu_fro_fit", sfx), ()
        elif (norm, method) == ("fro", "hals"):
            fn, extra = _fn("hals_fro_fit", sfx), (int(bool(column_sweep)),)
        else:
            raise ValueError("fit: no whole-fit entry point for method %r / norm %r" % (method, norm))
        nbytes = lib.dnmf_ws_bytes_fit(int(m), int(n), int(k), int(B))
        if nbytes == 0:
            raise ValueError("fit: bad problem shape m=%d n=%d k=%d batch=%d" % (m, n, k, B))
        ws = _scratch(nbytes, A.device)
        sq = torch.empty(B, 2, dtype=torch.float64, device=A.device)
        for t, name in ((A3, "A"), (W3, "W"), (H3, "H")):
            if t.stride(2) != 1 and t.numel():
                raise ValueError("fit: %s must have unit inner stride" % name)
        # one MU/Frobenius problem: every step of the fit may stream A's image
        with _wimage_bound(A, H, W) if not batched and (norm, method) == ("fro", "mu") else contextlib.nullcontext():
            check(fn(A3.data_ptr(), m, n, _ld(A3[0]), W3.data_ptr(), _ld(W3[0]), H3.data_ptr(), _ld(H3[0]), k, float(eps),
                     int(bool(w_update)), int(itr), *extra, int(B), A3.stride(0), W3.stride(0), H3.stride(0), sq.data_ptr(),
                     ws.data_ptr(), ws.numel(), _stream()))
        return sq

    # ---- the Itakura-Saito objective (csrc/dnmf_is.h, dnmf_is_*): dense strictly positive float32 data, 1 <= k <= 128.  With S = W H
    # and R = 1 / (S + eps): num = (A . R . R) F, den = R F (F = H^T / W), X <- X * sqrt(num / (den + eps))
    is_dtypes = (torch.float32,)       # the data types these operations take (PyNMF and the choreography refuse any other by name)

    _is_ranks = "norm='is' with k = %d: the Itakura-Saito kernels serve 1 <= k <= 128"

    # ---- what the dense pair rules share (dnmf_is_* here, dnmf_masked_* in HipMaskedOps; the sparse set uses the last two)
    @staticmethod
    def _pair_args(what, T, W, H, eps, nbytes_fn, ranks, mode=(), pair=None):
        """(A, W, H) checked against each other, the scratch `nbytes_fn` sizes (0: the rank is refused with `ranks`), and the
        arguments every entry point of a dense pair rule starts with (`mode`: the masked rules' kl) and ends with.  pair = (side,
        num, den): two views of the side's shape with one leading dimension, appended to the head."""
        _req(T, "A"); _req(W, "W"); _req(H, "H")
        m, n = T.shape
        k = W.shape[1]
        if tuple(W.shape) != (m, k) or tuple(H.shape) != (k, n):
            raise ValueError("%s: shapes A %s, W %s, H %s do not match" % (what, tuple(T.shape), tuple(W.shape), tuple(H.shape)))
        nbytes = nbytes_fn(int(m), int(n), int(k))
        if nbytes == 0:
            raise NotImplementedError(ranks % k)
        ws = _scratch(nbytes, T.device)
        head = (T.data_ptr(), m, n, _ld(T), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), int(k), float(eps)) + tuple(mode)
        if pair is not None:
            side, num, den = pair
            _req(num, "num"); _req(den, "den")
            want = (m, k) if side == "w" else (k, n)
            if tuple(num.shape) != want or tuple(den.shape) != want or _ld(num) != _ld(den):
                raise ValueError("%s: num %s and den %s must both be %s with one leading dimension" % (what, tuple(num.shape), tuple(den.shape), want))
            head += (num.data_ptr(), den.data_ptr(), _ld(num))
        return head, (ws.data_ptr(), ws.numel(), _stream())

    def _pair_fit(self, what, fit_fn, T, W, H, eps, nbytes_fn, ranks, mode, w_update, itr):
        """a whole fit under a dense pair rule as one library call: returns the device tensor [1][2] of its two squared norms"""
        head, tail = self._pair_args(what, T, W, H, eps, nbytes_fn, ranks, mode)
        sq = torch.empty(1, 2, dtype=torch.float64, device=T.device)
        check(fit_fn(*head, int(bool(w_update)), int(itr), sq.data_ptr(), *tail))
        return sq

    @staticmethod
    def _halves(buf, shape):
        """[num | den]: the halves of one contiguous buffer (what ONE allreduce carries) as two views of `shape`"""
        r, c = shape
        if buf.numel() < 2 * r * c or not buf.is_contiguous() or buf.dtype != torch.float32:
            raise ValueError("pair buffer: a contiguous float32 buffer of 2 x %d x %d elements is expected" % (r, c))
        return buf[: r * c].view(r, c), buf[r * c: 2 * r * c].view(r, c)

    @staticmethod
    def _ratio_args(what, X, num, den, eps, clamp):
        """the arguments of a rule on a stored pair (dnmf_csr_ratio_update, dnmf_is_ratio_update)"""
        _req(X, "X"); _req(num, "num"); _req(den, "den")
        if tuple(num.shape) != tuple(X.shape) or tuple(den.shape) != tuple(X.shape) or _ld(num) != _ld(den):
            raise ValueError("%s: X %s, num %s, den %s" % (what, tuple(X.shape), tuple(num.shape), tuple(den.shape)))
        r, c = X.shape
        return X.data_ptr(), r, c, _ld(X), num.data_ptr(), den.data_ptr(), _ld(num), float(eps), int(bool(clamp)), _stream()

    # ---- ONE implementation of both families.  `p` is the library prefix ('is' or 'beta'), `mode` what follows `eps` in every call
    # (() or (beta,)); the rank message is _is_ranks / _beta_ranks.  The public is_* and beta_* methods below are its callers.
    def _fam(self, p, what, A, W, H, eps, mode, pair=None, ws="ws_bytes"):
        return self._pair_args(what, A, W, H, eps, _fn(p + "_" + ws, ""), getattr(self, "_%s_ranks" % p), mode=mode, pair=pair)

    def _fam_pair(self, p, mode, side, A, W, H, eps, num, den):
        head, tail = self._fam(p, p + " pair", A, W, H, eps, mode, pair=(side, num, den))
        check(_fn(p + ("_aht_pair" if side == "w" else "_wta_pair"), "")(*head, *tail))
        return num, den

    def _fam_update(self, p, mode, side, A, W, H, eps, *clamp):
        what = "%s_update_%s" % (p, side)
        head, tail = self._fam(p, what, A, W, H, eps, mode)
        check(_fn(what, "")(*head, *clamp, *tail))
        return W if side == "w" else H

    def _fam_ratio_update(self, p, mode_of, X, num, den, eps, clamp):
        a = self._ratio_args(p + "_ratio_update", X, num, den, eps, clamp)
        check(_fn(p + "_ratio_update", "")(*a[:8], *mode_of(), *a[8:]))
        return X

    def _fam_divergence(self, p, mode, A, W, H, eps):
        head, tail = self._fam(p, p + "_divergence", A, W, H, eps, mode)
        out = torch.empty(1, dtype=torch.float64, device=A.device)
        check(_fn(p + "_divergence", "")(*head, out.data_ptr(), *tail))
        return out

    def _fam_column_div(self, p, mode, nout, A, W, H, eps):
        head, tail = self._fam(p, p + "_column_div", A, W, H, eps, mode, ws="column_div_ws_bytes")
        out = torch.empty(nout, A.shape[1], dtype=torch.float64, device=A.device)
        check(_fn(p + "_column_div", "")(*head, *(o.data_ptr() for o in out), *tail))
        return out

    def _fam_fit(self, p, mode, A, W, H, eps, w_update, itr):
        return self._pair_fit(p + "_fit", _fn(p + "_mu_fit", ""), A, W, H, eps, _fn(p + "_ws_bytes_fit", ""),
                              getattr(self, "_%s_ranks" % p), mode, w_update, itr)

    def is_aht_pair(self, A, W, H, eps, buf):
        """buf = [num | den], each m x k: (A . R . R) H^T and R H^T"""
        return self._fam_pair("is", (), "w", A, W, H, eps, *self._halves(buf, tuple(W.shape)))

    def is_wta_pair(self, A, W, H, eps, buf):
        """buf = [num | den], each k x n: W^T (A . R . R) and W^T R"""
        return self._fam_pair("is", (), "h", A, W, H, eps, *self._halves(buf, tuple(H.shape)))

    def is_pair_into(self, side, A, W, H, eps, num, den):
        """the same pair into two views of the caller's (one leading dimension, any pitch): side 'w' (m x k) or 'h' (k x n)"""
        return self._fam_pair("is", (), side, A, W, H, eps, num, den)

    def is_update_w(self, A, W, H, eps):
        """W <- W * sqrt(num / (den + eps)): the pass, then the rule on its partial sums (this rank's W rows see all their columns)"""
        return self._fam_update("is", (), "w", A, W, H, eps)

    def is_update_h(self, A, W, H, eps, clamp=False):
        """H <- H * sqrt(num / (den + eps)), max(., eps) with `clamp` (this rank's H columns see all their rows)"""
        return self._fam_update("is", (), "h", A, W, H, eps, int(bool(clamp)))

    def is_ratio_update(self, X, num, den, eps, clamp=False):
        """X <- X * sqrt(num / (den + eps)), max(., eps) with `clamp`: the rule on a pair that was summed over the ranks"""
        return self._fam_ratio_update("is", tuple, X, num, den, eps, clamp)

    def is_divergence(self, A, W, H, eps):
        """D_IS(A | W H + eps) = sum (q - log q - 1), q = A / (W H + eps), over this block: one device double (stored, not
        accumulated: two calls are bit-identical)"""
        return self._fam_divergence("is", (), A, W, H, eps)

    is_nmfk = True                     # PyNMFk looks for this and `is_column_div`: the per-column statistic of a sweep under norm='is'

    def is_column_div(self, A, W, H, eps):
        """div[c] = sum_i (q - log q - 1), q = A / (W H + eps), over this block's rows: n device doubles, column SUMS (dnmf_is_column_div:
        stored, not accumulated -- two calls are bit-identical)"""
        return self._fam_column_div("is", (), 1, A, W, H, eps)[0]

    def is_fit(self, A, W, H, eps, w_update, itr):
        """`itr` Itakura-Saito MU steps (clamps after the steps i % 10 == 0), normalize_features and the squared norms of relative_err in
        ONE library call (dnmf_is_mu_fit: the launches of the step loop in its order).  One problem; W, H are updated in place; returns
        the device tensor [1][2] of {sum (A - W H)^2, sum A^2}."""
        return self._fam_fit("is", (), A, W, H, eps, w_update, itr)

    # ---- the beta-divergence, -2 <= beta <= 4 (csrc/dnmf_beta.h, dnmf_beta_*): dense float32 data, 1 <= k <= 128.  With S' = W H + eps and
    # P = S'^(beta - 2): num = (A . P) F, den = (S' . P) F (F = H^T / W), X <- X * (num / (den + eps))^gamma(beta).  `beta` follows `eps`
    beta_dtypes = (torch.float32,)     # the data types these operations take (PyNMF and the choreography refuse any other by name)
    BETA_RANGE = (-2.0, 4.0)

    _beta_ranks = "norm='beta' with k = %d: the beta-divergence kernels serve 1 <= k <= 128"

    @classmethod
    def _beta_mode(cls, beta):
        beta = float(beta)
        if not cls.BETA_RANGE[0] <= beta <= cls.BETA_RANGE[1]:
            raise ValueError("beta = %r is outside the accepted range %g <= beta <= %g" % ((beta,) + cls.BETA_RANGE))
        return (beta,)

    def beta_aht_pair(self, A, W, H, eps, beta, buf):
        """buf = [num | den], each m x k: (A . P) H^T and (S' . P) H^T"""
        return self._fam_pair("beta", self._beta_mode(beta), "w", A, W, H, eps, *self._halves(buf, tuple(W.shape)))

    def beta_wta_pair(self, A, W, H, eps, beta, buf):
        """buf = [num | den], each k x n: W^T (A . P) and W^T (S' . P)"""
        return self._fam_pair("beta", self._beta_mode(beta), "h", A, W, H, eps, *self._halves(buf, tuple(H.shape)))

    def beta_pair_into(self, side, A, W, H, eps, beta, num, den):
        """the same pair into two views of the caller's (one leading dimension, any pitch): side 'w' (m x k) or 'h' (k x n)"""
        return self._fam_pair("beta", self._beta_mode(beta), side, A, W, H, eps, num, den)

    def beta_update_w(self, A, W, H, eps, beta):
        """W <- W * (num / (den + eps))^gamma: the pass, then the rule on its partial sums (this rank's W rows see all their columns)"""
        return self._fam_update("beta", self._beta_mode(beta), "w", A, W, H, eps)

    def beta_update_h(self, A, W, H, eps, beta, clamp=False):
        """H <- H * (num / (den + eps))^gamma, max(., eps) with `clamp` (this rank's H columns see all their rows)"""
        return self._fam_update("beta", self._beta_mode(beta), "h", A, W, H, eps, int(bool(clamp)))

    def beta_ratio_update(self, X, num, den, eps, beta, clamp=False):
        """X <- X * (num / (den + eps))^gamma, max(., eps) with `clamp`: the rule on a pair that was summed over the ranks"""
        return self._fam_ratio_update("beta", lambda: self._beta_mode(beta), X, num, den, eps, clamp)

    def beta_divergence(self, A, W, H, eps, beta):
        """D_beta(A | W H + eps) over this block: one device double (stored, not accumulated: two calls are bit-identical)"""
        return self._fam_divergence("beta", self._beta_mode(beta), A, W, H, eps)

    beta_nmfk = True                   # PyNMFk looks for this and `beta_column_div`: the per-column statistic of a sweep under norm='beta'

    def beta_column_div(self, A, W, H, eps, beta):
        """(div, pw): div[c] = sum_i d_beta(A | W H + eps) and pw[c] = sum_i A^beta over this block's rows, n device doubles each, column
        SUMS (dnmf_beta_column_div: stored, not accumulated -- two calls are bit-identical).  div / pw, after the sums have crossed the
        ranks, is the scale-invariant per-column statistic (PyNMF.beta_column_divergence)."""
        out = self._fam_column_div("beta", self._beta_mode(beta), 2, A, W, H, eps)
        return out[0], out[1]

    def beta_fit(self, A, W, H, eps, beta, w_update, itr):
        """`itr` beta-divergence MU steps (clamps after the steps i % 10 == 0), normalize_features and the squared norms of relative_err in
        ONE library call (dnmf_beta_mu_fit: the launches of the step loop in its order).  One problem; W, H are updated in place; returns
        the device tensor [1][2] of {sum (A - W H)^2, sum A^2}."""
        return self._fam_fit("beta", self._beta_mode(beta), A, W, H, eps, w_update, itr)

    def _bcd_fit(self, A3, W3, H3, eps, w_update, itr, sfx, batched):
        """method 'bcd' (dnmf_bcd_fro_fit): float32 data; a stack of B problems is ONE library call in which every launch
        covers all of them.  Each problem keeps its own state block in its workspace slice, so the problems accept or restart
        independently; bit-identical to B single fits."""
        if sfx:
            raise NotImplementedError("method 'bcd' with bfloat16-stored A is not provided (float32 data only)")
        B, m, n = A3.shape
        k = W3.shape[2]
        nbytes = lib.dnmf_bcd_ws_bytes_fit(int(m), int(n), int(k), int(B))
        if nbytes == 0:
            raise ValueError("fit: bad problem shape m=%d n=%d k=%d batch=%d for method 'bcd'" % (m, n, k, B))
        ws = _scratch(nbytes, A3.device)
        sq = torch.empty(B, 2, dtype=torch.float64, device=A3.device)
        for t, name in ((A3, "A"), (W3, "W"), (H3, "H")):
            if t.stride(2) != 1 and t.numel():
                raise ValueError("fit: %s must have unit inner stride" % name)
        check(lib.dnmf_bcd_fro_fit(A3.data_ptr(), m, n, _ld(A3[0]), W3.data_ptr(), _ld(W3[0]), H3.data_ptr(), _ld(H3[0]), k, float(eps),
                                   int(bool(w_update)), int(itr), int(B), A3.stride(0), W3.stride(0), H3.stride(0), sq.data_ptr(),
                                   ws.data_ptr(), ws.numel(), _stream()))
        return sq

    # ---- allocation helpers used by the choreography
    def empty(self, shape, like):
        return torch.empty(shape, dtype=torch.float32, device=like.device)

    def zeros(self, shape, like):
        return torch.zeros(shape, dtype=torch.float32, device=like.device)


HIP_OPS = HipOps()
if wimage_mode_from_env(os.environ) is not None:
    lib.dnmf_set_wimage(wimage_mode_from_env(os.environ))


class HipOpsBf16x6(HipOps):
    """The same operator set with the two big contractions A H^T and W^T A of an fp32 data matrix taken on the bf16 matrix
    cores as sums of six bf16 piece products (`dnmf_*_bf16x6`, csrc/dnmf_split.h): fp32-grade products at a rate the HBM,
    not the fp32 MFMA, bounds; with bf16-STORED A (`*_bf16a_bf16x6`) A is its own single piece and a product is three MFMAs.
    Opt-in (`params.gemm = 'bf16x6'`); shapes without a split kernel run the fp32 kernels, everything else of a step is the
    fp32 code either way."""

    name = "hip-bf16x6"
    is_dtypes = ()                 # (no split form of the Itakura-Saito pairs)
    is_nmfk = False                # (nor an NMFk sweep under norm='is')
    beta_dtypes = ()               # (nor of the beta-divergence pairs)
    beta_nmfk = False              # (nor an NMFk sweep under norm='beta')
    kl_uht_hblocks = None          # (no block-column variant of the split kernels: the 2D step concatenates H for them)
    aht_hblocks = None

    @staticmethod
    def _ws6(m, n, k, device):
        nbytes = lib.dnmf_ws_bytes_bf16x6(int(m), int(n), int(k))
        if nbytes == 0:
            raise ValueError("bad problem shape m=%d n=%d k=%d" % (m, n, k))
        return _scratch(nbytes, device)         # the same buffer the inherited fp32 operators use

    def aht(self, A, H, out):
        sfx = _req_a(A); _req(H, "H"); _req(out, "AH")
        m, n = A.shape
        k = H.shape[0]
        ws = self._ws6(m, n, k, A.device)
        check(_fn("aht", sfx + "_bf16x6")(A.data_ptr(), m, n, _ld(A), H.data_ptr(), k, _ld(H), out.data_ptr(), _ld(out),
                                  ws.data_ptr(), ws.numel(), _stream()))
        return out

    def wta(self, A, W, out):
        sfx = _req_a(A); _req(W, "W"); _req(out, "AtW")
        m, n = A.shape
        k = W.shape[1]
        ws = self._ws6(m, n, k, A.device)
        check(_fn("wta", sfx + "_bf16x6")(A.data_ptr(), m, n, _ld(A), W.data_ptr(), k, _ld(W), out.data_ptr(), _ld(out),
                                  ws.data_ptr(), ws.numel(), _stream()))
        return out

    def aht_update_w(self, A, H, G, W, eps):
        sfx = _req_a(A); _req(H, "H"); _req(G, "G"); _req(W, "W")
        m, n = A.shape
        k = H.shape[0]
        if k > 128:
            return HipOps.aht_update_w(self, A, H, G, W, eps)
        ws = self._ws6(m, n, k, A.device)
        check(_fn("aht_update_w", sfx + "_bf16x6")(A.data_ptr(), m, n, _ld(A), H.data_ptr(), k, _ld(H), G.data_ptr(), W.data_ptr(),
                                           _ld(W), float(eps), ws.data_ptr(), ws.numel(), _stream()))

    def mu_fro_step(self, A, W, H, eps, w_update=True, clamp=False):
        sfx = _req_a(A); _req(W, "W"); _req(H, "H")
        m, n = A.shape
        k = W.shape[1]
        ws = self._ws6(m, n, k, A.device)
        check(_fn("mu_fro_step", sfx + "_bf16x6")(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), k,
                                          float(eps), int(bool(w_update)), int(bool(clamp)), ws.data_ptr(), ws.numel(),
                                          _stream()))


    def kl_uht(self, A, W, H, eps, out):
        _req(A, "A"); _req(W, "W"); _req(H, "H"); _req(out, "UHT")
        m, n = A.shape
        k = W.shape[1]
        ws = self._ws6(m, n, k, A.device)
        check(lib.dnmf_kl_uht_bf16x6(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), k, float(eps),
                                     out.data_ptr(), _ld(out), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def kl_wtu(self, A, W, H, eps, out):
        _req(A, "A"); _req(W, "W"); _req(H, "H"); _req(out, "WTU")
        m, n = A.shape
        k = W.shape[1]
        ws = self._ws6(m, n, k, A.device)
        check(lib.dnmf_kl_wtu_bf16x6(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), k, float(eps),
                                     out.data_ptr(), _ld(out), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def mu_kl_step(self, A, W, H, eps, w_update=True, clamp=False):
        _req(A, "A"); _req(W, "W"); _req(H, "H")
        m, n = A.shape
        k = W.shape[1]
        ws = self._ws6(m, n, k, A.device)
        check(lib.dnmf_mu_kl_step_bf16x6(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), k,
                                         float(eps), int(bool(w_update)), int(bool(clamp)), ws.data_ptr(), ws.numel(),
                                         _stream()))


HIP_OPS_BF16X6 = HipOpsBf16x6()



class HipCsrOps(HipOps):
    """The operator set for a SPARSE data block (pydnmfk_amd.sparse.SparseBlock): the eight operations that touch A run on its
    CSR images (csrc/dnmf_csr.h, `dnmf_csr_*`); everything else of a step -- update kernels, Gram matrices, clamps,
    normalisation -- is the fp32 code of HipOps, which never sees A.  There is no fused local step and no whole fit for sparse
    data (`mu_fro_step`, `mu_kl_step`, `fit` refuse it): the host's choreography sequences the primitives.  A dense tensor
    in A's place (BCD asks for the squared norms of W and H) takes the dense kernels.
    A block whose unstored entries are MISSING (`A.missing == 'unstored'`) takes the masked operations: `masked_aht_pair` /
    `masked_wta_pair` (numerator and denominator of the rule over the stored positions, as one contiguous [num | den] buffer for
    ONE allreduce), `ratio_update` after it, and `masked_update_w` / `masked_update_h` where nothing crosses ranks (the pass writes
    the factor itself); `resid_sqnorm` then sums over the stored positions only.
    An NMFk sweep adds `perturb_uniform` (a new block with the source's pattern) and `column_err_sums` on a block (`sparse_nmfk`)."""

    name = "hip-csr"
    kl_uht_hblocks = None
    aht_hblocks = None

    def __init__(self):
        super().__init__()
        self._bufs = {}

    def _buf(self, role, numel, device, dtype=torch.float32):
        """one persistent buffer per role and device, grown on demand: a step allocates nothing once it has run"""
        key = (device, role, dtype)
        t = self._bufs.get(key)
        if t is None or t.numel() < numel:
            t = torch.empty(max(int(numel), 1), dtype=dtype, device=device)
            self._bufs[key] = t
        return t

    @staticmethod
    def _sp(A):
        return getattr(A, "is_sparse_block", False)

    def _ws(self, A, k):
        m, n = A.shape
        nbytes = lib.dnmf_csr_ws_bytes(int(m), int(n), int(k), int(max(A.nseg, A.t_nseg)))
        if nbytes == 0:
            raise ValueError("sparse block: bad problem shape m=%d n=%d k=%d" % (m, n, k))
        return _scratch(nbytes, A.device)

    def _pack(self, X, transpose, role):
        """the packed image [rows x KPAD] of W (transpose=False) or of H^T (transpose=True) in this operator set's buffer `role`"""
        _req(X, role)
        r, c = X.shape
        k = r if transpose else c
        kpad = lib.dnmf_csr_kpad(int(k))
        if kpad < 0:
            raise ValueError("rank k=%d unsupported (1 <= k <= 256)" % k)
        P = self._buf(role, (c if transpose else r) * kpad, X.device)
        check(lib.dnmf_csr_pack(X.data_ptr(), r, c, _ld(X), int(bool(transpose)), P.data_ptr(), _stream()))
        return P

    @staticmethod
    def _req_sp(A):
        if not A.val.is_cuda:
            raise TypeError("sparse block is on %s; the engine only runs on the GPU (no CPU fallback)" % A.device)
        _same_device(A.val, "A")

    def _mm(self, A, transposed, Fp, k, out, L=None, eps=0.0):
        self._req_sp(A)
        if transposed:
            crow, col, val, rows = A.t_crow, A.t_col, A.t_val, A.shape[1]
            lr, ls, nl, ns = A.t_long_rows, A.t_long_segptr, A.t_n_long, A.t_nseg
        else:
            crow, col, val, rows = A.crow, A.col, A.val, A.shape[0]
            lr, ls, nl, ns = A.long_rows, A.long_segptr, A.n_long, A.nseg
        ws = self._ws(A, k)
        tail = (lr.data_ptr() if nl else None, ls.data_ptr() if nl else None, nl, ns, ws.data_ptr(), ws.numel(), _stream())
        if L is None:
            check(lib.dnmf_csr_mm(crow.data_ptr(), col.data_ptr(), val.data_ptr(), rows, Fp.data_ptr(), int(k), out.data_ptr(), _ld(out),
                                  int(transposed), *tail))
        else:
            check(lib.dnmf_csr_kl_mm(crow.data_ptr(), col.data_ptr(), val.data_ptr(), rows, L.data_ptr(), Fp.data_ptr(), int(k), float(eps),
                                     out.data_ptr(), _ld(out), int(transposed), *tail))
        return out

    # ---- a block whose unstored entries are missing (dnmf_csr_masked_*): `norm` = 'fro' or 'kl'
    def _masked_ws(self, A, k):
        m, n = A.shape
        nbytes = lib.dnmf_csr_masked_ws_bytes(int(m), int(n), int(k), int(max(A.nseg, A.t_nseg)))
        if nbytes == 0:
            raise ValueError("sparse block: bad problem shape m=%d n=%d k=%d" % (m, n, k))
        return _scratch(nbytes, A.device)

    def _masked(self, A, transposed, W, H, eps, norm, pair=None, X=None, clamp=False):
        """one masked pass over the block's image (the W side) or the transpose's (the H side): the pair stored, or applied to X"""
        self._req_sp(A)
        if str(norm).lower() not in ("fro", "kl"):
            raise ValueError("masked update: norm %r (fro / kl)" % (norm,))
        kl = int(str(norm).lower() == "kl")
        _req(W, "W")
        _req(H, "H")
        k = W.shape[1]
        Wp, HTp = self._pack(W, False, "W"), self._pack(H, True, "HT")
        if transposed:
            crow, col, val, rows = A.t_crow, A.t_col, A.t_val, A.shape[1]
            lr, ls, nl, ns = A.t_long_rows, A.t_long_segptr, A.t_n_long, A.t_nseg
            Lp, Fp = HTp, Wp
        else:
            crow, col, val, rows = A.crow, A.col, A.val, A.shape[0]
            lr, ls, nl, ns = A.long_rows, A.long_segptr, A.n_long, A.nseg
            Lp, Fp = Wp, HTp
        ws = self._masked_ws(A, k)
        tail = (lr.data_ptr() if nl else None, ls.data_ptr() if nl else None, nl, ns, ws.data_ptr(), ws.numel(), _stream())
        head = (crow.data_ptr(), col.data_ptr(), val.data_ptr(), rows, Lp.data_ptr(), Fp.data_ptr(), int(k), float(eps), kl)
        if X is None:
            num, den = pair
            check(lib.dnmf_csr_masked_mm(*head, num.data_ptr(), den.data_ptr(), _ld(num), int(transposed), *tail))
            return num, den
        check(lib.dnmf_csr_masked_update(*head, int(bool(clamp)), X.data_ptr(), _ld(X), int(transposed), *tail))
        return X

    def masked_aht_pair(self, A, W, H, eps, norm, buf):
        """buf = [num | den], each m x k: A H^T and P(W H) H^T ('fro'), or U H^T and the stored-position row sums of H ('kl')"""
        return self._masked(A, False, W, H, eps, norm, pair=self._halves(buf, tuple(W.shape)))

    def masked_wta_pair(self, A, W, H, eps, norm, buf):
        """buf = [num | den], each k x n: W^T A and W^T P(W H) ('fro'), or W^T U and the stored-position column sums of W ('kl')"""
        return self._masked(A, True, W, H, eps, norm, pair=self._halves(buf, tuple(H.shape)))

    def masked_update_w(self, A, W, H, eps, norm):
        """W <- W * num / (den + eps) in the pass itself (the W rows of this rank see all their columns)"""
        return self._masked(A, False, W, H, eps, norm, X=W)

    def masked_update_h(self, A, W, H, eps, norm, clamp=False):
        """H <- H * num / (den + eps), max(., eps) with `clamp`, in the pass itself (the H columns of this rank see all their rows)"""
        return self._masked(A, True, W, H, eps, norm, X=H, clamp=clamp)

    def ratio_update(self, X, num, den, eps, clamp=False):
        """X <- X * num / (den + eps), max(., eps) with `clamp`: the rule on a pair that was summed over the ranks"""
        check(lib.dnmf_csr_ratio_update(*self._ratio_args("ratio_update", X, num, den, eps, clamp)))
        return X

    def aht(self, A, H, out):
        if not self._sp(A):
            return super().aht(A, H, out)
        _req(out, "AH")
        return self._mm(A, False, self._pack(H, True, "HT"), H.shape[0], out)

    def wta(self, A, W, out):
        if not self._sp(A):
            return super().wta(A, W, out)
        _req(out, "AtW")
        return self._mm(A, True, self._pack(W, False, "W"), W.shape[1], out)

    def wta_gram(self, A, W, out, G):
        if not self._sp(A):
            self.gram_wtw(W, G)
            return super().wta(A, W, out)
        self.gram_wtw(W, G)
        return self.wta(A, W, out)

    def aht_update_w(self, A, H, G, W, eps):
        if not self._sp(A):
            return super().aht_update_w(A, H, G, W, eps)
        m, k = W.shape
        AH = self._buf("AH", m * k, W.device)[: m * k].view(m, k)
        self.aht(A, H, AH)
        return self.mu_update_w(W, AH, G, eps)

    def kl_uht(self, A, W, H, eps, out):
        if not self._sp(A):
            return super().kl_uht(A, W, H, eps, out)
        _req(out, "UHT")
        Wp, HTp = self._pack(W, False, "W"), self._pack(H, True, "HT")
        return self._mm(A, False, HTp, W.shape[1], out, L=Wp, eps=eps)

    def kl_wtu(self, A, W, H, eps, out):
        if not self._sp(A):
            return super().kl_wtu(A, W, H, eps, out)
        _req(out, "WTU")
        Wp, HTp = self._pack(W, False, "W"), self._pack(H, True, "HT")
        return self._mm(A, True, Wp, W.shape[1], out, L=HTp, eps=eps)

    def sqnorm(self, A):
        if not self._sp(A):
            return super().sqnorm(A)
        self._req_sp(A)
        if A.nnz == 0:
            return torch.zeros(1, dtype=torch.float64, device=A.device)
        # the value array as a 1 x nnz matrix.  dnmf_sqnorm ends in a float64 atomic sum whose order varies between runs, and
        # ||A||^2 never changes during a fit (BCD asks for it per fit, relative_err per fit): evaluated once per block and kept
        if getattr(A, "_sqnorm", None) is None:
            A._sqnorm = super().sqnorm(A.val.view(1, -1))
        return A._sqnorm.clone()

    def resid_sqnorm(self, A, W, H):
        if not self._sp(A):
            return super().resid_sqnorm(A, W, H)
        self._req_sp(A)
        m, n = A.shape
        k = W.shape[1]
        Wp, HTp = self._pack(W, False, "W"), self._pack(H, True, "HT")
        out = torch.empty(1, dtype=torch.float64, device=A.device)
        masked = getattr(A, "missing", None) == "unstored"       # ||P(A - W H)||^2 over the stored positions
        ws = self._masked_ws(A, k) if masked else self._ws(A, k)
        fn = lib.dnmf_csr_masked_resid_sqnorm if masked else lib.dnmf_csr_resid_sqnorm
        check(fn(A.crow.data_ptr(), A.col.data_ptr(), A.val.data_ptr(), m, n, Wp.data_ptr(), HTp.data_ptr(), int(k),
                 A.long_rows.data_ptr() if A.n_long else None, A.long_segptr.data_ptr() if A.n_long else None,
                 A.n_long, A.nseg, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def _dense_only(self, what, A):
        if self._sp(A):
            raise NotImplementedError("%s is not provided for sparse data (the choreography sequences the sparse primitives)" % what)

    def mu_fro_step(self, A, W, H, eps, w_update=True, clamp=False):
        self._dense_only("the fused local MU/FRO step", A)
        return super().mu_fro_step(A, W, H, eps, w_update, clamp)

    def mu_kl_step(self, A, W, H, eps, w_update=True, clamp=False):
        self._dense_only("the fused local MU/KL step", A)
        return super().mu_kl_step(A, W, H, eps, w_update, clamp)

    def fit(self, method, norm, A, W, H, eps, w_update, itr, column_sweep=False):
        self._dense_only("a whole-fit entry point", A)
        return super().fit(method, norm, A, W, H, eps, w_update, itr, column_sweep=column_sweep)

    # ---- NMFk on a sparse block: the two operations of the sweep that touch A outside a fit
    sparse_nmfk = True

    def perturb_uniform(self, X, noise_var, seed, out=None):
        """A SparseBlock: a NEW block with X's pattern (index arrays and long-row lists shared, `SparseBlock.with_values`) whose
        values are X's times (1 + nv + 2 nv U) -- U keyed by (seed, position in the dense block), so both images hold what
        HipOps.perturb_uniform gives the densified block at the stored positions, bit for bit.  Dense tensors: the inherited path."""
        if not self._sp(X):
            return super().perturb_uniform(X, noise_var, seed, out=out)
        self._req_sp(X)
        m, n = X.shape
        val, t_val = torch.empty_like(X.val), torch.empty_like(X.t_val)
        if X.nnz:
            sd = int(seed) & (2**64 - 1)
            check(lib.dnmf_csr_perturb_uniform(X.crow.data_ptr(), X.col.data_ptr(), X.val.data_ptr(), m, n, 0, float(noise_var), sd,
                                               val.data_ptr(), _stream()))
            check(lib.dnmf_csr_perturb_uniform(X.t_crow.data_ptr(), X.t_col.data_ptr(), X.t_val.data_ptr(), n, n, 1, float(noise_var), sd,
                                               t_val.data_ptr(), _stream()))
        return X.with_values(val, t_val)

    def column_err_sums(self, A, W, H):
        """(num, den) per column over this rank's rows, float64 [n]: sum (A - W H)^2 and sum A^2 -- or, under missing='unstored', both
        over the stored positions only -- from the transpose's image (dnmf_csr_column_err); a dense tensor takes the dense kernel."""
        if not self._sp(A):
            return super().column_err_sums(A, W, H)
        self._req_sp(A)
        m, n = A.shape
        k = W.shape[1]
        Wp, HTp = self._pack(W, False, "W"), self._pack(H, True, "HT")
        masked = int(getattr(A, "missing", None) == "unstored")
        nbytes = lib.dnmf_csr_column_err_ws_bytes(int(n), int(m), int(k), masked, int(A.t_nseg))
        if nbytes == 0:
            raise ValueError("sparse block: bad problem shape m=%d n=%d k=%d" % (m, n, k))
        ws = _scratch(nbytes, A.device)
        out = torch.empty(2, n, dtype=torch.float64, device=A.device)
        nl = A.t_n_long
        check(lib.dnmf_csr_column_err(A.t_crow.data_ptr(), A.t_col.data_ptr(), A.t_val.data_ptr(), n, m, HTp.data_ptr(), Wp.data_ptr(), int(k),
                                      masked, A.t_long_rows.data_ptr() if nl else None, A.t_long_segptr.data_ptr() if nl else None, nl,
                                      A.t_nseg, out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out[0], out[1]


HIP_CSR_OPS = HipCsrOps()


class HipMaskedOps(HipOps):
    """The operator set for a DENSE data block whose missing entries are NaN (pydnmfk_amd.masked.MaskedDenseBlock, `params.missing =
    'nan'`): the operations that touch A are the masked ones of csrc/dnmf_masked.h (`dnmf_masked_*`: S = W H tiles in MFMA accumulators,
    one compare and two selects per element, two second products) -- `masked_aht_pair` / `masked_wta_pair` (numerator and denominator
    over the observed positions as one contiguous [num | den] buffer for ONE allreduce), `ratio_update` after it, `masked_update_w` /
    `masked_update_h` where nothing crosses ranks, `resid_sqnorm` and `sqnorm` over the observed positions, `column_err_sums` (the per-column
    error of an NMFk sweep, `masked_nmfk`) and `fit` (a whole fit on one rank as one library call).  Everything that never sees A --
    clamps, normalisation, scaling -- is the fp32 code of HipOps.  Every dense operation that would read A as numbers (the fused local
    steps, the plain products) refuses the block: those kernels would consume the NaNs."""

    name = "hip-masked"
    kl_uht_hblocks = None
    aht_hblocks = None
    ratio_update = HipCsrOps.ratio_update
    _masked_ranks = "missing='nan' with k = %d: the masked dense kernels serve 1 <= k <= 128"

    @staticmethod
    def _blk(A):
        return getattr(A, "is_masked_dense", False)

    def _masked(self, side, A, W, H, eps, norm, pair=None, X=None, clamp=False):
        if not self._blk(A):
            raise TypeError("masked update: the data must be a MaskedDenseBlock, got %s" % (type(A),))
        if str(norm).lower() not in ("fro", "kl"):
            raise ValueError("masked update: norm %r (fro / kl)" % (norm,))
        kl = int(str(norm).lower() == "kl")
        head, tail = self._pair_args("masked update" if pair is None else "masked pair", A.tensor, W, H, eps, lib.dnmf_masked_ws_bytes,
                                     self._masked_ranks, (kl,), pair=None if pair is None else (side,) + tuple(pair))
        if pair is not None:
            check((lib.dnmf_masked_aht_pair if side == "w" else lib.dnmf_masked_wta_pair)(*head, *tail))
            return pair
        if side == "w":
            check(lib.dnmf_masked_update_w(*head, *tail))
        else:
            check(lib.dnmf_masked_update_h(*head, int(bool(clamp)), *tail))
        return X

    def masked_aht_pair(self, A, W, H, eps, norm, buf):
        """buf = [num | den], each m x k: P(A) H^T and P(W H) H^T ('fro'), or P(A / (W H + eps)) H^T and P(1) H^T ('kl')"""
        return self._masked("w", A, W, H, eps, norm, pair=self._halves(buf, tuple(W.shape)))

    def masked_wta_pair(self, A, W, H, eps, norm, buf):
        """buf = [num | den], each k x n: W^T P(A) and W^T P(W H) ('fro'), or W^T P(A / (W H + eps)) and W^T P(1) ('kl')"""
        return self._masked("h", A, W, H, eps, norm, pair=self._halves(buf, tuple(H.shape)))

    def masked_pair_into(self, side, A, W, H, eps, norm, num, den):
        """the same pair into two views of the caller's (one leading dimension, any pitch): side 'w' (m x k) or 'h' (k x n)"""
        return self._masked(side, A, W, H, eps, norm, pair=(num, den))

    def masked_update_w(self, A, W, H, eps, norm):
        """W <- W * num / (den + eps): the pass, then the rule on its partial sums (this rank's W rows see all their columns)"""
        return self._masked("w", A, W, H, eps, norm, X=W)

    def masked_update_h(self, A, W, H, eps, norm, clamp=False):
        """H <- H * num / (den + eps), max(., eps) with `clamp` (this rank's H columns see all their rows)"""
        return self._masked("h", A, W, H, eps, norm, X=H, clamp=clamp)

    def _observed_sums(self, A):
        """(||P(A)||^2, |Omega|) as two device doubles, evaluated once per block: the sum ends in float64 atomics whose order varies
        between runs, and neither value changes during a fit"""
        if A._sqnorm is None:
            T = _req(A.tensor, "A")
            out = torch.empty(2, dtype=torch.float64, device=T.device)
            check(lib.dnmf_masked_sqnorm(T.data_ptr(), T.shape[0], T.shape[1], _ld(T), out.data_ptr(), _stream()))
            A._sqnorm = out
        return A._sqnorm

    def sqnorm(self, A):
        if not self._blk(A):
            return super().sqnorm(A)
        return self._observed_sums(A)[:1].clone()

    def resid_sqnorm(self, A, W, H):
        if not self._blk(A):
            return super().resid_sqnorm(A, W, H)
        T = _req(A.tensor, "A"); _req(W, "W"); _req(H, "H")
        out = torch.empty(1, dtype=torch.float64, device=T.device)
        check(lib.dnmf_masked_resid_sqnorm(T.data_ptr(), T.shape[0], T.shape[1], _ld(T), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H),
                                           int(W.shape[1]), out.data_ptr(), _stream()))
        return out

    # ---- NMFk on a NaN-marked block: the per-column error (the perturbed copy is HipOps.perturb_uniform on the raw tensor: NaN stays NaN)
    masked_nmfk = True

    def column_err_sums(self, A, W, H):
        """(num, den) per column over this rank's rows, float64 [n]: sum (A - W H)^2 and sum A^2 over the OBSERVED positions of a
        MaskedDenseBlock (dnmf_masked_column_err: stored, not accumulated -- two calls are bit-identical; a column without an observation
        gives (0, 0)).  A plain tensor takes the dense kernel."""
        if not self._blk(A):
            return super().column_err_sums(A, W, H)
        head, tail = self._pair_args("masked column_err_sums", A.tensor, W, H, 0.0, lib.dnmf_masked_column_err_ws_bytes, self._masked_ranks)
        out = torch.empty(2, A.tensor.shape[1], dtype=torch.float64, device=A.tensor.device)
        check(lib.dnmf_masked_column_err(*head[:-1], out[0].data_ptr(), out[1].data_ptr(), *tail))      # (this entry point takes no eps)
        return out[0], out[1]

    def fit(self, method, norm, A, W, H, eps, w_update, itr, column_sweep=False):
        """A MaskedDenseBlock: `itr` masked MU steps (clamps after the steps i % 10 == 0), normalize_features and the squared norms of
        relative_err over the observed positions in ONE library call (dnmf_masked_mu_fit: the launches of the step loop in its order).
        One problem; W, H are updated in place; returns the device tensor [1][2].  A plain tensor takes the inherited whole fits."""
        if not self._blk(A):
            return super().fit(method, norm, A, W, H, eps, w_update, itr, column_sweep=column_sweep)
        method, norm = str(method).lower(), str(norm).lower()
        if method != "mu" or norm not in ("fro", "kl"):
            raise NotImplementedError("missing='nan' is provided for method 'mu' (fro / kl) only, not for '%s' / '%s'" % (method, norm))
        return self._pair_fit("masked fit", lib.dnmf_masked_mu_fit, A.tensor, W, H, eps, lib.dnmf_masked_ws_bytes_fit, self._masked_ranks,
                              (int(norm == "kl"),), w_update, itr)

    def _refuse(self, what, A):
        if self._blk(A):
            raise NotImplementedError("%s is not provided under missing='nan': it would read the NaNs of the block as data (the "
                                      "choreography sequences the masked operations)" % what)


def _masked_refusal(name, what):
    def method(self, A, *args, **kwargs):
        self._refuse(what, A)
        return getattr(HipOps, name)(self, A, *args, **kwargs)
    method.__name__ = name
    return method


for _name, _what in (("aht", "the product A H^T"), ("wta", "the product W^T A"), ("wta_gram", "the product W^T A"),
                     ("aht_update_w", "the fused A H^T update"), ("mu_fro_step", "the fused local MU/FRO step"),
                     ("mu_kl_step", "the fused local MU/KL step"), ("kl_uht", "the dense KL product U H^T"),
                     ("kl_wtu", "the dense KL product W^T U")):
    setattr(HipMaskedOps, _name, _masked_refusal(_name, _what))


HIP_MASKED_OPS = HipMaskedOps()


class HipOpsF64:
    """The operator set in float64 (csrc/dnmf_f64.hip: the fp64 matrix cores, one plain tile shape per kernel family).  The
    reference computes in the dtype of A_ij (pyDNMF.py:68): float64 data are factorised in float64, eps = 2.22e-16.  The same
    method surface as HipOps for the primitives the choreography (dist_nmf.py) sequences, plus the whole one-rank fit (`fit`); no
    whole-step entry points (the choreography's generic path runs), no bf16 storage, no block-column products."""

    name = "hip-f64"
    aht_hblocks = None
    kl_uht_hblocks = None
    dtype = torch.float64

    @staticmethod
    def _r(t, name, ndim=2):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise TypeError("%s: expected a CUDA tensor (no CPU fallback)" % name)
        _same_device(t, name)
        if t.dtype != torch.float64:
            raise TypeError("%s: dtype %s in the float64 operator set" % (name, t.dtype))
        if t.dim() != ndim or (t.numel() and t.stride(-1) != 1):
            raise ValueError("%s: must be %d-D row-major with unit inner stride" % (name, ndim))
        return t

    @staticmethod
    def _ws(m, n, k, device):
        nbytes = lib.dnmf_f64_ws_bytes(int(m), int(n), int(k))
        if nbytes == 0:
            raise ValueError("bad problem shape m=%d n=%d k=%d" % (m, n, k))
        return _scratch(nbytes, device)

    _img = {}

    @classmethod
    def _image(cls, m, n, device):
        """the m x n float64 image the KL quotient / the squared residual are materialised in (one per device, grown on demand)"""
        key = device.index if device.index is not None else torch.cuda.current_device()
        t = cls._img.get(key)
        if t is None or t.numel() < m * n:
            cls._img.pop(key, None)
            t = torch.empty(m * n, dtype=torch.float64, device=device)
            cls._img[key] = t
        return t[: m * n].view(m, n)

    def fit(self, method, norm, A, W, H, eps, w_update, itr, column_sweep=False):
        """`itr` steps, normalize_features and the squared norms of relative_err in ONE library call (dnmf_f64_fit: the primitives
        of this class in the choreography's order -- the same bits as the step loop, without its Python frames).  Matrices, or
        stacks [B][m][n] / [B][m][k] / [B][k][n] fitted one after the other.  W, H are updated in place; returns the device tensor
        [B][2] of {sum (A - W H)^2, sum A^2}."""
        code = {("mu", "fro"): 0, ("mu", "kl"): 1, ("hals", "fro"): 2}.get((method.lower(), norm.lower()))
        if code is None:
            raise ValueError("fit: no whole-fit entry point for method %r / norm %r" % (method, norm))
        A3, W3, H3 = (A, W, H) if A.dim() == 3 else (A[None], W[None], H[None])
        B, m, n = A3.shape
        k = W3.shape[2]
        if W3.shape != (B, m, k) or H3.shape != (B, k, n):
            raise ValueError("fit: shapes A %s, W %s, H %s do not match" % (tuple(A3.shape), tuple(W3.shape), tuple(H3.shape)))
        nbytes = lib.dnmf_f64_ws_bytes_fit(int(m), int(n), int(k))
        if nbytes == 0:
            raise ValueError("fit: bad problem shape m=%d n=%d k=%d" % (m, n, k))
        ws = _scratch(nbytes, A.device)
        sq = torch.empty(B, 2, dtype=torch.float64, device=A.device)
        for b in range(B):
            self._r(A3[b], "A"); self._r(W3[b], "W"); self._r(H3[b], "H")
            check(lib.dnmf_f64_fit(code, A3[b].data_ptr(), m, n, _ld(A3[b]), W3[b].data_ptr(), _ld(W3[b]), H3[b].data_ptr(), _ld(H3[b]), k,
                                   float(eps), int(bool(w_update)), int(itr), sq[b].data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return sq

    # ---- grams and the two big contractions
    def gram_hht(self, H, out):
        r = self._r; r(H, "H"); r(out, "G")
        k, n = H.shape
        ws = self._ws(k, n, k, H.device)
        check(lib.dnmf_f64_aht(H.data_ptr(), k, n, _ld(H), H.data_ptr(), k, _ld(H), out.data_ptr(), _ld(out), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def gram_wtw(self, W, out):
        r = self._r; r(W, "W"); r(out, "G")
        m, k = W.shape
        ws = self._ws(m, k, k, W.device)
        check(lib.dnmf_f64_wta(W.data_ptr(), m, k, _ld(W), W.data_ptr(), k, _ld(W), out.data_ptr(), _ld(out), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def aht(self, A, H, out):
        r = self._r; r(A, "A"); r(H, "H"); r(out, "AH")
        m, n = A.shape
        k = H.shape[0]
        ws = self._ws(m, n, k, A.device)
        check(lib.dnmf_f64_aht(A.data_ptr(), m, n, _ld(A), H.data_ptr(), k, _ld(H), out.data_ptr(), _ld(out), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def wta(self, A, W, out):
        r = self._r; r(A, "A"); r(W, "W"); r(out, "AtW")
        m, n = A.shape
        k = W.shape[1]
        ws = self._ws(m, n, k, A.device)
        check(lib.dnmf_f64_wta(A.data_ptr(), m, n, _ld(A), W.data_ptr(), k, _ld(W), out.data_ptr(), _ld(out), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def wta_gram(self, A, W, out, G):
        self.gram_wtw(W, G)
        return self.wta(A, W, out)

    # ---- updates
    def mu_update_w(self, W, AH, G, eps):
        r = self._r; r(W, "W"); r(AH, "AH"); r(G, "G")
        m, k = W.shape
        check(lib.dnmf_f64_mu_update_w(W.data_ptr(), m, k, _ld(W), AH.data_ptr(), _ld(AH), G.data_ptr(), _ld(G), float(eps), _stream()))

    def mu_update_h(self, H, AtW, G, eps, clamp=False):
        r = self._r; r(H, "H"); r(AtW, "AtW"); r(G, "G")
        k, n = H.shape
        check(lib.dnmf_f64_mu_update_h(H.data_ptr(), k, n, _ld(H), AtW.data_ptr(), _ld(AtW), G.data_ptr(), _ld(G), float(eps),
                                       int(bool(clamp)), _stream()))

    def aht_update_w(self, A, H, G, W, eps):
        """W *= (A H^T) / (W G + eps) (dist_nmf.py:716-732): the product, then the update"""
        m, k = W.shape
        AH = torch.empty(m, k, dtype=torch.float64, device=W.device)
        self.aht(A, H, AH)
        self.mu_update_w(W, AH, G, eps)

    # ---- HALS
    def hals_ss2(self, k, like):
        return torch.zeros(k, dtype=torch.float64, device=like.device)

    def hals_w_col(self, W, AH, G, kk, ss2, eps):
        r = self._r; r(W, "W"); r(AH, "AH"); r(G, "G")
        m, k = W.shape
        ws = self._ws(m, k, k, W.device)
        prev = ss2[kk - 1:].data_ptr() if kk > 0 else None
        check(lib.dnmf_f64_hals_w_col(W.data_ptr(), m, k, _ld(W), AH.data_ptr(), _ld(AH), G.data_ptr(), _ld(G), int(kk), prev, float(eps),
                                      ss2[kk:].data_ptr(), ws.data_ptr(), ws.numel(), _stream()))

    def hals_w_scale(self, W, col, ss2):
        self._r(W, "W")
        check(lib.dnmf_f64_hals_w_scale(W.data_ptr(), W.shape[0], _ld(W), int(col), ss2[col:].data_ptr(), _stream()))

    def hals_update_w(self, W, AH, G, eps):
        k = W.shape[1]
        ss2 = self.hals_ss2(k, W)
        for kk in range(k):
            self.hals_w_col(W, AH, G, kk, ss2, eps)
        self.hals_w_scale(W, k - 1, ss2)
        return ss2

    hals_update_w_columns = hals_update_w

    def hals_check(self):
        pass                                           # (no persistent sweep in this operator set)

    def hals_update_h(self, H, AtW, G, eps):
        r = self._r; r(H, "H"); r(AtW, "AtW"); r(G, "G")
        k, n = H.shape
        check(lib.dnmf_f64_hals_update_h(H.data_ptr(), k, n, _ld(H), AtW.data_ptr(), _ld(AtW), G.data_ptr(), _ld(G), float(eps), _stream()))

    # ---- KL
    def _quot(self, A, W, H, eps):
        r = self._r; r(A, "A"); r(W, "W"); r(H, "H")
        m, n = A.shape
        U = self._image(m, n, A.device)
        check(lib.dnmf_f64_kl_quot(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), W.shape[1], float(eps),
                                   U.data_ptr(), n, _stream()))
        return U

    def _kl_product(self, fn, A, W, H, eps, out):
        """one of the two KL products: fused up to k = 64 (the quotient stays in registers, csrc/dnmf_f64_kl.h), through the m x n
        image beyond"""
        r = self._r; r(A, "A"); r(W, "W"); r(H, "H"); r(out, "S")
        m, n = A.shape
        k = W.shape[1]
        U = self._image(m, n, A.device) if k > 64 else None
        ws = self._ws(m, n, k, A.device)
        check(fn(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), k, float(eps), out.data_ptr(), _ld(out),
                 U.data_ptr() if U is not None else None, ws.data_ptr(), ws.numel(), _stream()))
        return out

    def kl_uht(self, A, W, H, eps, out):
        return self._kl_product(lib.dnmf_f64_kl_uht, A, W, H, eps, out)      # (A / (W H + eps)) H^T, dist_nmf.py:806,810

    def kl_wtu(self, A, W, H, eps, out):
        return self._kl_product(lib.dnmf_f64_kl_wtu, A, W, H, eps, out)      # W^T (A / (W H + eps)), dist_nmf.py:806,808

    def rowsum(self, H, out):
        self._r(H, "H"); self._r(out, "x", 1)
        check(lib.dnmf_f64_rowsum(H.data_ptr(), H.shape[0], H.shape[1], _ld(H), out.data_ptr(), _stream()))
        return out

    def colsum(self, W, out):
        self._r(W, "W"); self._r(out, "x", 1)
        m, k = W.shape
        ws = self._ws(m, k, k, W.device)
        check(lib.dnmf_f64_colsum(W.data_ptr(), m, k, _ld(W), 0, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def _ew(self, op, X, S, x, eps, clamp=False):
        self._r(X, "X")
        check(lib.dnmf_f64_ew(op, X.data_ptr(), X.shape[0], X.shape[1], _ld(X), S.data_ptr() if S is not None else None,
                              _ld(S) if S is not None else 0, x.data_ptr() if x is not None else None, float(eps), int(bool(clamp)), _stream()))

    def kl_update_w(self, W, S, x, eps):
        self._r(S, "S"); self._r(x, "x", 1)
        self._ew(4, W, S, x, eps)

    def kl_update_h(self, H, S, x, eps, clamp=False):
        self._r(S, "S"); self._r(x, "x", 1)
        self._ew(3, H, S, x, eps, clamp)

    # ---- fit helpers
    def clamp_min(self, X, eps):
        self._ew(0, X, None, None, eps)

    def scale_cols_div(self, W, s, eps):
        self._r(s, "s", 1)
        self._ew(1, W, None, s, eps)

    def scale_rows_mul(self, H, s):
        self._r(s, "s", 1)
        self._ew(2, H, None, s, 0.0)

    def perturb_uniform(self, X, noise_var, seed, out=None):
        return None                                    # (the caller's torch expression, in float64)

    def sqnorm(self, A):
        self._r(A, "A")
        out = torch.empty(1, dtype=torch.float64, device=A.device)
        ws = self._ws(A.shape[0], A.shape[1], 1, A.device)
        check(lib.dnmf_f64_sum(A.data_ptr(), A.shape[0], A.shape[1], _ld(A), 1, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def _sqdiff(self, A, W, H):
        r = self._r; r(A, "A"); r(W, "W"); r(H, "H")
        m, n = A.shape
        R = self._image(m, n, A.device)
        check(lib.dnmf_f64_sqdiff(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), W.shape[1], R.data_ptr(), n, _stream()))
        return R

    def resid_sqnorm(self, A, W, H):
        R = self._sqdiff(A, W, H)
        out = torch.empty(1, dtype=torch.float64, device=A.device)
        ws = self._ws(A.shape[0], A.shape[1], W.shape[1], A.device)
        check(lib.dnmf_f64_sum(R.data_ptr(), R.shape[0], R.shape[1], R.shape[1], 0, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out

    def column_err_sums(self, A, W, H):
        m, n = A.shape
        out = torch.zeros(2, n, dtype=torch.float64, device=A.device)
        ws = self._ws(m, n, W.shape[1], A.device)
        R = self._sqdiff(A, W, H)
        check(lib.dnmf_f64_colsum(R.data_ptr(), m, n, n, 0, out[0].data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        check(lib.dnmf_f64_colsum(A.data_ptr(), m, n, _ld(A), 1, out[1].data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return out[0], out[1]

    def empty(self, shape, like):
        return torch.empty(shape, dtype=torch.float64, device=like.device)

    def zeros(self, shape, like):
        return torch.zeros(shape, dtype=torch.float64, device=like.device)


HIP_OPS_F64 = HipOpsF64()


class NativeComm:
    """The grid's RCCL communicators INSIDE libdnmf_hip.so (csrc/dnmf_comm.hip) and the whole-step entry points on top of
    them (csrc/dnmf_grid.hip): one library call enqueues kernels -> allreduce -> kernels, no Python between the launches.  Built
    from the host's existing communicator (`comm`: a dist_comm.TorchComm over all ranks), which only carries the 128-byte RCCL id
    from rank 0 to the others.  `params.exchange = 'native'` makes nmf_algorithms_1D / _2D use it for MU (Frobenius, KL) and HALS steps, fp32
    and bf16-stored data (created on first use; `NativeComm.hosted` builds one whose collectives the host performs)."""

    def __init__(self, comm, p_r, p_c):
        import ctypes
        if not torch.cuda.is_available():
            raise RuntimeError("NativeComm: needs a GPU (RCCL communicators live on the current HIP device)")
        # Bring-up is COLLECTIVE-SAFE: rank 0 always takes part in the broadcast -- it sends the id or an error
        # marker -- and after dnmf_comm_create every rank learns whether ALL ranks hold a communicator; any failure raises
        # on every rank together, so callers that fall back to the torch.distributed choreography do so on every rank.
        idbuf = ctypes.create_string_buffer(128)
        payload = None
        if comm.rank == 0:
            try:
                check(lib.dnmf_comm_unique_id(idbuf))
                payload = ("id", bytes(idbuf.raw))
            except Exception as ex:  # noqa: BLE001
                payload = ("error", repr(ex))
        kind, raw = comm.bcast(payload, root=0)
        if kind != "id":
            raise RuntimeError("NativeComm: rank 0 could not create the RCCL id (%s)" % raw)
        h = ctypes.c_void_p()
        mine = None
        try:
            check(lib.dnmf_comm_create(raw, int(comm.size), int(comm.rank), int(p_r), int(p_c), ctypes.byref(h)))
        except Exception as ex:  # noqa: BLE001
            mine = ex
        nbad = int(comm.allreduce(1 if mine is not None else 0)) if comm.size > 1 else (1 if mine is not None else 0)
        if nbad:
            if mine is None:
                lib.dnmf_comm_destroy(h)
            raise RuntimeError("NativeComm: dnmf_comm_create failed on %d of %d ranks%s" % (
                nbad, comm.size, " (here: %s)" % mine if mine is not None else ""))
        self.handle, self.size, self.rank, self.p_r, self.p_c = h, int(comm.size), int(comm.rank), int(p_r), int(p_c)
        self.device = torch.cuda.current_device()
        self._ws = None
        self.overlap_chunks = 1
        self.steps = 0                 # whole steps the choreography handed to the library (tests read it)

    @classmethod
    def hosted(cls, size, rank, p_r, p_c, collective):
        """A communicator whose collectives the HOST performs (dnmf_comm_create_hosted): `collective(op, group, send_ptr,
        recv_ptr, count, stream_ptr) -> 0` is called on the calling thread for every exchange of the step entry points (op
        0 / 1 / 2 = allreduce / allgather / reduce-scatter, group 0 / 1 / 2 = world / cart_1d_row / cart_1d_column, device
        pointers; include/dnmf.h).  No RCCL involved: the multi-rank tests run the C steps over gloo this way."""
        import ctypes
        from ._lib import COLLECTIVE_FN
        if not torch.cuda.is_available():
            raise RuntimeError("NativeComm: needs a GPU")
        self = cls.__new__(cls)

        def _cb(user, op, group, send, recv, count, stream):
            try:
                return int(collective(int(op), int(group), int(send or 0), int(recv or 0), int(count), int(stream or 0)))
            except Exception:                                         # never let an exception cross the C frame
                import traceback
                traceback.print_exc()
                return 1
        self._cb = COLLECTIVE_FN(_cb)                                  # keep the trampoline alive as long as the communicator
        h = ctypes.c_void_p()
        check(lib.dnmf_comm_create_hosted(int(size), int(rank), int(p_r), int(p_c), self._cb, None, ctypes.byref(h)))
        self.handle, self.size, self.rank, self.p_r, self.p_c = h, int(size), int(rank), int(p_r), int(p_c)
        self.device = torch.cuda.current_device()
        self._ws = None
        self.overlap_chunks = 1
        self.steps = 0                 # whole steps the choreography handed to the library (tests read it)
        return self

    @classmethod
    def emulated(cls, p_r, p_c, rank=0):
        """MEASUREMENT ONLY (bench.py --emulate-ranks): member `rank` of a p_r x p_c grid on a one-GPU box; every collective of
        the step entry points is issued for real on a one-rank RCCL communicator (dnmf_comm_create_emulated)."""
        import ctypes
        self = cls.__new__(cls)
        h = ctypes.c_void_p()
        check(lib.dnmf_comm_create_emulated(int(p_r), int(p_c), int(rank), ctypes.byref(h)))
        self.handle, self.size, self.rank, self.p_r, self.p_c = h, int(p_r) * int(p_c), int(rank), int(p_r), int(p_c)
        self.device = torch.cuda.current_device()
        self._ws = None
        self.overlap_chunks = 1
        self.steps = 0
        self.is_emulated = True
        return self

    def close(self):
        if getattr(self, "handle", None):
            host = getattr(self, "_direct_host", None)
            if host is not None and host.size > 1:
                # peers may still be reading this rank's exported region (their last gather): drain the device and meet
                # the others before the region is freed.  Best effort -- a rank that is already gone cannot be waited for.
                try:
                    torch.cuda.synchronize()
                    host.barrier()
                except Exception:  # noqa: BLE001
                    pass
            lib.dnmf_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        # not while the interpreter shuts down: the HIP / RCCL runtimes may already be gone, and the process is ending anyway
        import sys
        if not sys.is_finalizing():
            self.close()

    def enable_direct(self, host_comm, max_floats):
        """Set up the direct two-shot allreduce over IPC peer buffers (dnmf_comm_direct_*; include/dnmf.h): every rank exports a
        region for messages of up to `max_floats` floats, `host_comm` (a dist_comm.TorchComm over the same ranks) carries the
        64-byte handles.  Collective; returns True when EVERY rank is connected (the ranks agree before anybody uses it), else
        False on every rank.  `set_direct(True)` then routes the world allreduces that fit through it."""
        import ctypes
        from ._lib import DIRECT_HANDLE_BYTES
        hbuf = ctypes.create_string_buffer(DIRECT_HANDLE_BYTES)
        ok = 1
        self.direct_error = None
        try:
            check(lib.dnmf_comm_direct_init(self.handle, int(max_floats), hbuf))
        except Exception as ex:  # noqa: BLE001
            ok, self.direct_error = 0, ex
        handles = host_comm.allgather(bytes(hbuf.raw))
        if ok:
            try:   # (a rank that sized its region differently, or failed its init, fails the connect on EVERY rank)
                check(lib.dnmf_comm_direct_connect(self.handle, b"".join(handles)))
            except Exception as ex:  # noqa: BLE001
                ok, self.direct_error = 0, ex
        nbad = int(host_comm.allreduce(0 if ok else 1)) if host_comm.size > 1 else (0 if ok else 1)
        self.direct_ready = nbad == 0
        self.direct_max_floats = int(max_floats)
        if not self.direct_ready:
            # nobody uses the regions: unmap and free them now (a later enable_direct starts from scratch); the barrier keeps a
            # region alive until every peer has unmapped it
            if host_comm.size > 1:
                host_comm.barrier()
            lib.dnmf_comm_direct_teardown(self.handle)
        else:
            self._direct_host = host_comm
        return self.direct_ready

    def hals_xsweeps(self):
        """cross-rank persistent HALS W sweeps issued through the peer regions so far (dnmf_comm_hals_xsweeps)"""
        import ctypes
        n = ctypes.c_ulonglong(0)
        check(lib.dnmf_comm_hals_xsweeps(self.handle, ctypes.byref(n)))
        return int(n.value)

    def set_direct_timeout(self, seconds):
        check(lib.dnmf_comm_set_direct_timeout(self.handle, float(seconds)))

    def fit_begin(self):
        """every rank, before the first step of a fit: the cross-rank HALS sweep agrees anew on the first sweep (dnmf_comm_fit_begin)"""
        check(lib.dnmf_comm_fit_begin(self.handle))

    def direct_self_check(self, host_comm, count=4096):
        """First contact: the same random vector summed by the direct allreduce and by the communicator's own allreduce (RCCL or
        the hosted function) -- both sum in a fixed order per element, but not the SAME order, so the comparison allows fp32
        rounding of the sum -- and the status word; the ranks agree on the outcome.  The stacked-rank tests of this
        repository run all ranks on one GPU (one L2): what can go wrong across xGMI -- a peer's freshly copied send buffer not
        yet visible to a system-scope load -- shows here, on the machine at hand, before any factor depends on it."""
        g = torch.Generator(device="cuda")
        g.manual_seed(977 + self.rank)
        count = max(2, min(int(count), int(getattr(self, "direct_max_floats", count))) // 2 * 2)      # (an even count within the regions)
        x = torch.rand(count, device="cuda", generator=g)
        ok = 1
        try:
            for _ in range(3):                                  # both parities of the buffers, twice
                a, b = x.clone(), x.clone()
                check(lib.dnmf_comm_allreduce_direct(self.handle, a.data_ptr(), a.numel(), _stream()))
                was = self._get_direct_on()
                self.set_direct(False)
                try:
                    self.allreduce_(b)
                finally:
                    self.set_direct(was)
                if not bool(((a - b).abs() <= 1e-5 * self.size).all()) or self.direct_timed_out():
                    ok = 0
                x = x * 0.5 + 0.25
        except Exception as ex:  # noqa: BLE001
            ok, self.direct_error = 0, ex
        nbad = int(host_comm.allreduce(0 if ok else 1)) if host_comm.size > 1 else (0 if ok else 1)
        return nbad == 0

    def _get_direct_on(self):
        return bool(getattr(self, "_direct_on", False))

    def set_direct(self, on=True):
        check(lib.dnmf_comm_set_direct(self.handle, int(bool(on))))
        self._direct_on = bool(on)

    def allreduce_direct_(self, t):
        _req(t, "t", t.dim())
        if not t.is_contiguous():
            raise ValueError("allreduce_direct_: contiguous tensors only")
        check(lib.dnmf_comm_allreduce_direct(self.handle, t.data_ptr(), t.numel(), _stream()))
        return t

    def allreduce_direct_f64_(self, t):
        if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or not 1 <= t.numel() <= 8:
            raise ValueError("allreduce_direct_f64_: 1..8 contiguous float64 values on the GPU")
        check(lib.dnmf_comm_allreduce_direct_f64(self.handle, t.data_ptr(), t.numel(), _stream()))
        return t

    def direct_timed_out(self):
        import ctypes
        w = ctypes.c_int(0)
        check(lib.dnmf_comm_direct_status(self.handle, ctypes.byref(w)))
        return bool(w.value)

    def set_overlap_chunks(self, n):
        check(lib.dnmf_comm_set_overlap_chunks(self.handle, int(n)))
        self.overlap_chunks = int(n)

    def set_always_exchange(self, on=True):
        """Testing aid: a one-rank communicator still issues its RCCL calls."""
        check(lib.dnmf_comm_set_always_exchange(self.handle, int(bool(on))))

    def set_null_exchange(self, on=True):
        """Measurement aid: the step entry points skip their RCCL calls (a rank's compute without the exchange; wrong results
        on more than one rank)."""
        check(lib.dnmf_comm_set_null_exchange(self.handle, int(bool(on))))

    def allreduce_(self, t, group=0):
        _req(t, "t", t.dim())
        if not t.is_contiguous():
            raise ValueError("allreduce_: contiguous tensors only")
        check(lib.dnmf_comm_allreduce(self.handle, t.data_ptr(), t.numel(), int(group), _stream()))
        return t

    def _workspace(self, nbytes, device):
        """the communicator's one workspace, grown to `nbytes` (what dnmf_ws_bytes_1d / _2d asked for; 0: the shape is refused)"""
        if nbytes == 0:
            raise ValueError("bad problem shape for the steps of a %d x %d grid" % (self.p_r, self.p_c))
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self._ws

    def step_1d(self, norm, A, W, H, eps, w_update=True, clamp=False):
        """One MU step (norm 'fro' / 'kl') of this rank of a 1D grid, exchanges included (dnmf_mu_{fro,kl}_step_1d)."""
        _req(W, "W"); _req(H, "H")
        m, n = A.shape
        k = W.shape[1]
        ws = self._workspace(lib.dnmf_ws_bytes_1d(int(m), int(n), int(k)), A.device)
        if norm.lower() == "fro":
            fn = _fn("mu_fro_step_1d", _req_a(A))                      # fp32 or bf16-stored A
        else:
            _req(A, "A")
            fn = lib.dnmf_mu_kl_step_1d
        check(fn(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), k, float(eps),
                 int(bool(w_update)), int(bool(clamp)), ws.data_ptr(), ws.numel(), self.handle, _stream()))

    def hals_step_1d(self, A, W, H, eps, w_update=True, clamp=False, column_sweep=False):
        """One HALS / Frobenius step of this rank of a 1D grid, exchanges and column norms included (dnmf_hals_fro_step_1d)."""
        sfx = _req_a(A); _req(W, "W"); _req(H, "H")
        m, n = A.shape
        k = W.shape[1]
        ws = self._workspace(lib.dnmf_ws_bytes_1d(int(m), int(n), int(k)), A.device)
        check(_fn("hals_fro_step_1d", sfx)(A.data_ptr(), m, n, _ld(A), W.data_ptr(), _ld(W), H.data_ptr(), _ld(H), k, float(eps),
                                        int(bool(w_update)), int(bool(clamp)), int(bool(column_sweep)), ws.data_ptr(), ws.numel(),
                                        self.handle, _stream()))

    def step_2d(self, norm, A, W, H, eps, w_update=True, clamp=False):
        """One step of this rank of a 2D grid, exchanges included -- MU (norm 'fro' / 'kl': dnmf_mu_{fro,kl}_step_2d) or HALS /
        Frobenius (norm 'hals': dnmf_hals_fro_step_2d): W, H are the
        rank's SLICES (m_w x k, k x n_h), even or ragged per the partition rule.  Raises DnmfError (DNMF_EINVAL) on slices off that
        rule or strided -- `step_2d_ok` tells beforehand."""
        _req(W, "W"); _req(H, "H")
        m, n = A.shape
        k = W.shape[1]
        ws = self._workspace(lib.dnmf_ws_bytes_2d(int(m), int(n), int(k), self.p_r, self.p_c), A.device)
        sfx = _req_a(A)
        if norm.lower() == "kl" and sfx:
            raise ValueError("step_2d: KL needs float32 data")
        fn = {"fro": _fn("mu_fro_step_2d", sfx), "kl": lib.dnmf_mu_kl_step_2d, "hals": _fn("hals_fro_step_2d", sfx)}[norm.lower()]
        check(fn(A.data_ptr(), m, n, _ld(A), W.data_ptr(), W.shape[0], _ld(W), H.data_ptr(), H.shape[1], _ld(H), k, float(eps),
                 int(bool(w_update)), int(bool(clamp)), ws.data_ptr(), ws.numel(), self.handle, _stream()))

    def step_2d_ok(self, A, W, H):
        """What the 2D entry points take (include/dnmf.h): contiguous factor slices whose sizes follow the partition rule of
        the grid (utils.py:36-41: the first total % p members hold one item more) -- even or ragged."""
        m, n = A.shape
        i, j = self.rank // self.p_c, self.rank % self.p_c
        mw = m // self.p_c + (1 if j < m % self.p_c else 0)
        nh = n // self.p_r + (1 if i < n % self.p_r else 0)
        return (m >= self.p_c and n >= self.p_r and W.shape[0] == mw and H.shape[1] == nh
                and W.is_contiguous() and H.is_contiguous())


def _torch_hosted_collective(groups):
    """The three collectives of dnmf_comm_create_hosted on top of dist_comm.TorchComm objects (`groups`: {0: world, 1:
    cart_1d_row, 2: cart_1d_column}) -- any torch.distributed backend, gloo included: the device buffers are copied into
    tensors of our own, exchanged, and copied back, with the stream drained on both sides.  A correctness transport (the
    multi-rank tests run the C step entry points with it); RCCL is the product's."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    D2D = 3

    def collective(op, group, send, recv, count, stream):
        comm = groups[group]
        n = comm.size
        torch.cuda.synchronize()                                    # everything that produces `send` has run
        dev = torch.device("cuda", torch.cuda.current_device())
        t = torch.empty(count * (n if op == 2 else 1), dtype=torch.float64 if op == 3 else torch.float32, device=dev)
        if hip.hipMemcpy(t.data_ptr(), send, t.numel() * t.element_size(), D2D):
            return 1
        if op in (0, 3):
            out = comm.allreduce_(t)
        elif op == 1:
            out = torch.cat([b.reshape(-1) for b in comm.allgather_blocks(t, [(count,)] * n)])
        else:
            out = comm.reduce_scatter_rows(t.view(n, count), [1] * n).reshape(-1)
        out = out.contiguous()
        torch.cuda.synchronize()
        if hip.hipMemcpy(recv, out.data_ptr(), out.numel() * out.element_size(), D2D):
            return 1
        return 0
    return collective


def native_comm_for(params):
    """The NativeComm of `params` when it asks for the in-library exchange (`params.exchange = 'native'`); created on first use
    and kept on the params bag (`params._native_comm`).  None otherwise."""
    mode = getattr(params, "exchange", None)
    if mode not in ("native", "native-hosted"):
        return None
    nc = getattr(params, "_native_comm", None)
    stale = nc is not None and not getattr(nc, "is_emulated", False) and (nc.size != int(params.comm1.size) or (
        int(params.p_r) * int(params.p_c) == nc.size and (nc.p_r, nc.p_c) != (int(params.p_r), int(params.p_c))))
    if stale:      # (a grid that does not multiply to the communicator's size is an emulated share -- bench.py, tests -- and is left alone)
        # the bag was reused with another grid (pyDNMFk_Runner.run(grid=...) twice): every rank sees the same mismatch, so
        # the rebuild below is collective
        nc.close()
        nc = params._native_comm = None
    if nc is None:
        if mode == "native":
            try:
                nc = NativeComm(params.comm1, params.p_r, params.p_c)
            except Exception as ex:      # no RCCL in reach, or the communicator did not come up -- on EVERY rank (the
                # constructor agrees on that before it raises): the host choreography still works
                import warnings
                warnings.warn("params.exchange = 'native': %s -- falling back to the torch.distributed choreography" % ex)
                params.exchange = "torch"
                return None
        else:       # 'native-hosted': the C step entry points over the host's torch.distributed groups (any backend)
            groups = {0: params.comm1, 1: getattr(params, "row_comm", None) or params.comm1,
                      2: getattr(params, "col_comm", None) or params.comm1}
            nc = NativeComm.hosted(params.comm1.size, params.comm1.rank, params.p_r, params.p_c, _torch_hosted_collective(groups))
        if getattr(params, "direct_allreduce", False) and params.comm1.size > 1:
            # params.direct_allreduce: the world allreduces of the library-sequenced 1D steps (the packed [W^T A | W^T W] message)
            # go through the two-shot form over IPC peer buffers instead of RCCL / the hosted function (one node; collective set-up;
            # every rank falls back together when any rank cannot connect)
            kk = int(getattr(params, "end_k", None) or getattr(params, "k", None) or 128)
            kp = 32 if kk <= 32 else (64 if kk <= 64 else 128)
            nmax = kk * max(int(params.m), int(params.n)) + 8 * 64 + kp * kp + 2048      # (global sizes: the same on every rank)
            import warnings
            if not nc.enable_direct(params.comm1, nmax):
                warnings.warn("params.direct_allreduce: the peer regions could not be connected on every rank (%s) -- staying on the "
                              "communicator's own allreduce" % (nc.direct_error,))
            else:
                if getattr(params, "direct_timeout", None):
                    nc.set_direct_timeout(params.direct_timeout)
                if nc.direct_self_check(params.comm1):           # first contact on THIS machine, agreed over the ranks
                    nc.set_direct(True)
                else:
                    warnings.warn("params.direct_allreduce: the direct allreduce did not reproduce the communicator's own sum on this "
                                  "machine (%s) -- staying on the communicator's own allreduce" % (nc.direct_error,))
        params._native_comm = nc
    return nc


def ops_for(params=None, dtype=None, sparse=False, masked=False):
    """The operator set `params` asks for: `params.gemm` = 'fp32' (default: the fp32-MFMA contractions, the parity
    reference) or 'bf16x6' (HipOpsBf16x6); float64 data (`dtype`) take the float64 set whatever `gemm` says.  `sparse`: the
    data block is a SparseBlock -- HipCsrOps (float32 values, fp32 arithmetic only).  `masked`: it is a MaskedDenseBlock (dense
    float32 data, NaN = not observed) -- HipMaskedOps."""
    if masked:
        if (getattr(params, "gemm", None) or "fp32") != "fp32":
            raise NotImplementedError("missing='nan' with params.gemm = %r is not provided (fp32 arithmetic only)" % (params.gemm,))
        return HIP_MASKED_OPS
    if sparse:
        if (getattr(params, "gemm", None) or "fp32") != "fp32":
            raise NotImplementedError("params.gemm = %r is not provided for sparse data (fp32 arithmetic only)" % (params.gemm,))
        return HIP_CSR_OPS
    if dtype is torch.float64:
        return HIP_OPS_F64
    mode = getattr(params, "gemm", None) or "fp32"
    if mode == "fp32":
        return HIP_OPS
    if mode == "bf16x6":
        return HIP_OPS_BF16X6
    raise ValueError("params.gemm = %r: expected 'fp32' or 'bf16x6'" % (mode,))
