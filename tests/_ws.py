"""The guarded workspace (tests/test_gpu_workspace.py): every entry point's `ws` as a view between two sentinel bands, of EXACTLY the
size its query names (or a stated excess), holding a stated content before each call.

include/dnmf.h promises three things about `ws`: scratch of at least the family's size query, nothing retained between calls, the
result a function of the operands only.  `engine._scratch` hands one cached buffer, with `ws.numel()` as `ws_bytes`, to every
operator family in turn, and `NativeComm._workspace` does the same for the grid steps -- so in production the buffer is as large as
the biggest problem the process has seen and holds what the last call of any family left.  GuardedScratch stands in for both for the
duration of one case:

    with guarded(engine, state, extra) as g:          # restores engine._scratch / NativeComm._workspace / HipOpsF64._image on exit
        ... calls ...
        g.check()                                     # both bands untouched (compared on the device)
    g.sizes                                           # the sequence of sizes the engine asked for

state   0xFF  NaN as fp32 and fp64, all-ones tags, the value the HALS slab treats as "empty"
        0x00
        0x7F  3.39e38 as fp32, finite, and a tag larger than any real one
        "leftover"  nothing is filled: the view holds what the previous call -- of another family, the driver runs one -- left there
extra   bytes the view is larger than the query: an int, or a function of the query (a buffer "left by a bigger problem")
lead    bytes before the view (512: torch's alignment; 512 + 16: the header's "16-byte aligned", which torch never exercises)
"""
import contextlib

import torch

SENTINEL = 0xA5                       # distinct from every fill (0xFF, 0x00, 0x7F)
GUARD = 4096
STATES = (0xFF, 0x00, 0x7F, "leftover")


def bigger(nbytes):
    """the view a four times larger problem would have left in the engine's cache"""
    return 3 * nbytes + 4096 + 16


class GuardedScratch:
    """Callable as `engine._scratch(nbytes, device)`; `workspace_method()` gives the stand-in of `NativeComm._workspace`."""

    def __init__(self, state, extra=0, lead=512, guard=GUARD):
        assert state in STATES and guard >= 4096 and lead >= 0
        self.state, self.extra, self.lead, self.guard = state, extra, int(lead), int(guard)
        self.sizes = []               # every size asked for, in order
        self.buf = None               # the backing buffer: [lead | view | guard | rest]
        self.span = 0                 # bytes of the current view
        self.checked = 0              # how many seatings were checked

    def _extra(self, nbytes):
        return int(self.extra(nbytes)) if callable(self.extra) else int(self.extra)

    def __call__(self, nbytes, device):
        nbytes = int(nbytes)
        self.sizes.append(nbytes)
        if self.buf is not None:
            self.check()              # the previous seating, before its bands are moved (stream-ordered after the call that used it)
        span = nbytes + self._extra(nbytes)
        total = self.lead + span + self.guard
        if self.buf is None or self.buf.numel() < total or self.buf.device != torch.device(device):
            new = torch.empty(total, dtype=torch.uint8, device=device)
            if self.state == "leftover":
                # a grown buffer keeps what the smaller one held (repeated over the new length): never fresh, possibly zero, memory
                if self.buf is not None and self.buf.device == new.device:
                    new.copy_(self.buf.repeat(-(-total // self.buf.numel()))[:total])
                else:
                    new.fill_(0x7F)
            self.buf = new
        self.span = span
        view = self.buf[self.lead:self.lead + span]
        if self.state != "leftover":
            view.fill_(self.state)
        self.buf[:self.lead].fill_(SENTINEL)
        self.buf[self.lead + span:self.lead + span + self.guard].fill_(SENTINEL)
        return view

    def fill(self, byte):
        """overwrite the current view (what a foreign call would have left, when the driver wants a particular content)"""
        if self.buf is not None:
            self.buf[self.lead:self.lead + self.span].fill_(byte)

    def check(self, what=""):
        """both bands of the current seating hold the sentinel: compared on the device, one flag read back"""
        assert self.buf is not None, "%s: the engine asked for no workspace" % what
        lo = self.buf[:self.lead]
        hi = self.buf[self.lead + self.span:self.lead + self.span + self.guard]
        bad_lo, bad_hi = (lo != SENTINEL), (hi != SENTINEL)
        if bool(bad_lo.any()) or bool(bad_hi.any()):
            first_lo = int(bad_lo.nonzero()[0]) - self.lead if bool(bad_lo.any()) else None
            first_hi = int(bad_hi.nonzero()[0]) if bool(bad_hi.any()) else None
            raise AssertionError("%s: a kernel wrote outside its workspace of %d bytes (query %d): %s bytes before it (first at offset %s), "
                                 "%s bytes behind it (first %s bytes past the end)"
                                 % (what, self.span, self.sizes[-1], int(bad_lo.sum()), first_lo, int(bad_hi.sum()), first_hi))
        self.checked += 1

    def workspace_method(self):
        g = self

        def _workspace(comm, nbytes, device):
            if nbytes == 0:
                raise ValueError("bad problem shape for the steps of a %d x %d grid" % (comm.p_r, comm.p_c))
            return g(nbytes, device)
        return _workspace


@contextlib.contextmanager
def guarded(engine, state, extra=0, lead=512):
    """engine._scratch, NativeComm._workspace and the float64 image under guard for the block; everything is restored on exit.  The
    float64 image (HipOpsF64._img: operand-sized, not part of `ws`) is dirtied the way tests/test_gpu_exact.py::_scratch_runs does."""
    g = GuardedScratch(state, extra, lead)
    was_scratch, was_ws, was_image = engine._scratch, engine.NativeComm._workspace, engine.HipOpsF64.__dict__["_image"]
    image = was_image.__func__

    def _image(cls, m, n, device):
        t = image(cls, m, n, device)
        if state != "leftover":
            t.view(torch.uint8).fill_(state)          # (a contiguous m x n head of the cached image)
        return t

    engine._scratch = g
    engine.NativeComm._workspace = g.workspace_method()
    engine.HipOpsF64._image = classmethod(_image)
    try:
        yield g
    finally:
        engine._scratch = was_scratch
        engine.NativeComm._workspace = was_ws
        engine.HipOpsF64._image = was_image


class Recorder:
    """Wraps `lib.<name>` for a list of names for the duration of a block and reports which were called:

        with Recorder(lib, names) as rec: ...
        rec.missing()          # the names never called
    ctypes' CDLL keeps its functions as instance attributes, so the wrapper replaces the attribute and puts the function back."""

    def __init__(self, lib, names):
        self.lib, self.names, self.calls, self._orig = lib, tuple(names), {}, {}

    def __enter__(self):
        for name in self.names:
            fn = getattr(self.lib, name)
            self._orig[name] = fn
            self.calls[name] = 0
            setattr(self.lib, name, self._wrap(name, fn))
        return self

    def _wrap(self, name, fn):
        def call(*args):
            self.calls[name] += 1
            return fn(*args)
        return call

    def __exit__(self, *exc):
        for name, fn in self._orig.items():
            setattr(self.lib, name, fn)
        return False

    def missing(self):
        return [n for n in self.names if not self.calls[n]]
