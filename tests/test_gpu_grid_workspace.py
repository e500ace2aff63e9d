"""Where the library-sequenced grid steps (dnmf_*_step_{1d,2d}, csrc/dnmf_grid.hip) keep what they exchange: every buffer a
step hands to a collective lies inside the workspace the library asked for (dnmf_ws_bytes_1d / _2d) or inside W or H, the
two buffers of one call are the same or apart, and the k doubles of the HALS column norms are a region of their own, clear of
every float message of the step.  One process: a hosted communicator (dnmf_comm_create_hosted) per rank position of a grid, whose
host collective RECORDS each call and fills the receive buffer the way the emulated communicator does (this member's block in
every member's place for an allgather, the member's block of the send buffer for a reduce-scatter, nothing for an in-place
allreduce) -- the step runs on finite numbers, its results are not a factorisation of anything."""
import ctypes

import numpy as np
import pytest

from tests import _exact as ex

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ALLREDUCE, ALLGATHER, REDUCE_SCATTER, ALLREDUCE_F64 = 0, 1, 2, 3           # include/dnmf.h DNMF_ALLREDUCE ...
FAMILIES = ("fro", "kl", "hals")


def part(total, p, q):
    """the partition rule (utils.py:36-41): the count of member q"""
    return total // p + (1 if q < total % p else 0)


class Position:
    """One rank position of a p_r x p_c grid on an (m, n, k) problem: its block of A, a recording communicator, one step per call."""

    def __init__(self, grid, rank, shape, chunks=1):
        from pydnmfk_amd.engine import NativeComm
        (self.p_r, self.p_c), (m, n, self.k) = grid, shape
        self.rank, self.i, self.j = rank, rank // self.p_c, rank % self.p_c
        self.m_l, self.n_l = part(m, self.p_r, self.i), part(n, self.p_c, self.j)
        self.two_d = self.p_r > 1 and self.p_c > 1
        self.m_w = part(self.m_l, self.p_c, self.j) if self.two_d else self.m_l
        self.n_h = part(self.n_l, self.p_r, self.i) if self.two_d else self.n_l
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.trace, self.W, self.H = [], None, None
        self.comm = NativeComm.hosted(self.p_r * self.p_c, rank, self.p_r, self.p_c, self._collective)
        if chunks > 1:
            self.comm.set_overlap_chunks(chunks)

    def close(self):
        self.comm.close()

    def ws_bytes(self):
        from pydnmfk_amd._lib import lib
        if self.two_d:
            return int(lib.dnmf_ws_bytes_2d(self.m_l, self.n_l, self.k, self.p_r, self.p_c))
        return int(lib.dnmf_ws_bytes_1d(self.m_l, self.n_l, self.k))

    def _where(self, ptr):
        """(buffer name, byte offset) of a device pointer: the workspace, W or H -- '?' for anything else"""
        for name, t in (("ws", self.comm._ws), ("W", self.W), ("H", self.H)):
            if t is not None and t.data_ptr() <= ptr < t.data_ptr() + t.numel() * t.element_size():
                return name, ptr - t.data_ptr()
        return "?", ptr

    def _collective(self, op, group, send, recv, count, stream):
        members = (self.p_r * self.p_c, self.p_r, self.p_c)[group]
        es = 8 if op == ALLREDUCE_F64 else 4
        self.trace.append((op, group, self._where(send), self._where(recv), count, es))
        torch.cuda.synchronize()                                        # everything that produces `send` has run
        if op == ALLGATHER:
            for q in range(members):
                if self.hip.hipMemcpy(recv + q * count * es, send, count * es, 3):
                    return 1
        elif op == REDUCE_SCATTER:
            member = self.i if group == 1 else self.j
            if self.hip.hipMemcpy(recv, send + member * count * es, count * es, 3):
                return 1
        return 0

    def step(self, family, w_update=True, clamp=False, bf16=False, seed=0):
        """one step of `family` from fresh factors; returns the trace of its collectives"""
        dev = torch.device("cuda", torch.cuda.current_device())
        rs = np.random.RandomState(1000 * self.rank + seed + self.k)
        A = torch.from_numpy((rs.rand(self.m_l, self.n_l) + 0.05).astype(np.float32)).to(dev)
        if bf16:
            A = A.to(torch.bfloat16)
        self.W = torch.from_numpy((rs.rand(self.m_w, self.k) + 0.05).astype(np.float32)).to(dev)
        self.H = torch.from_numpy((rs.rand(self.k, self.n_h) + 0.05).astype(np.float32)).to(dev)
        eps = float(np.finfo(np.float32).eps)
        self.trace = []
        if self.two_d:
            self.comm.step_2d(family, A, self.W, self.H, eps, w_update, clamp)
        elif family == "hals":
            self.comm.hals_step_1d(A, self.W, self.H, eps, w_update, clamp)
        else:
            self.comm.step_1d(family, A, self.W, self.H, eps, w_update, clamp)
        torch.cuda.synchronize()
        return self.trace


def ranges(entry, pos):
    """((buffer, start, end) of send, the same of recv) of one recorded call"""
    op, group, (sname, soff), (rname, roff), count, es = entry
    members = (pos.p_r * pos.p_c, pos.p_r, pos.p_c)[group]
    ns = count * es * (members if op == REDUCE_SCATTER else 1)
    nr = count * es * (members if op == ALLGATHER else 1)
    return (sname, soff, soff + ns), (rname, roff, roff + nr)


def apart(a, b):
    return a[0] != b[0] or a[2] <= b[1] or b[2] <= a[1]


def check_trace(trace, pos, family):
    limit = {"ws": pos.ws_bytes(), "W": pos.W.numel() * 4, "H": pos.H.numel() * 4}
    assert limit["ws"] > 0
    floats, doubles = [], []
    for entry in trace:
        send, recv = ranges(entry, pos)
        for r in (send, recv):
            assert r[0] in limit and 0 <= r[1] and r[2] <= limit[r[0]], (family, entry, r, limit)
        assert send == recv or apart(send, recv), (family, entry)
        if entry[0] == ALLREDUCE:
            assert send == recv, (family, entry)                         # (in place)
        (doubles if entry[0] == ALLREDUCE_F64 else floats).extend((send, recv))
    if family == "hals":
        # W's rows are spread over ranks on a row grid and on every 2D grid: the sum of squares of each column is exchanged
        assert bool(doubles) == (pos.p_r > 1), (pos.p_r, pos.p_c, len(doubles))
    else:
        assert not doubles
    if doubles:
        starts = sorted({d[1] for d in doubles})
        assert {d[0] for d in doubles} == {"ws"} and all(d[2] - d[1] == 8 for d in doubles)
        assert starts[0] % 8 == 0 and starts == [starts[0] + 8 * q for q in range(pos.k)], (starts, pos.k)
        norms = ("ws", starts[0], starts[0] + 8 * pos.k)
        for f in floats:
            assert apart(norms, f), (family, norms, f)
    assert trace, "a step of more than one rank exchanges something"


# the smallest grids of tests/_exact.py GRID_EXACT that reach each exchange branch, each at its first shape; the row grid also with
# the H phase of the MU/Frobenius step cut into overlapped chunks
_GRIDS = {e[0]: (e[1], e[2][0]) for e in ex.GRID_EXACT}
CASES = [(name, *_GRIDS[name], 1) for name in ("3x1", "1x3", "2x2-blockable", "2x2-sliceable", "2x2-ragged", "2x3")]
CASES.insert(1, ("3x1-overlap4", *_GRIDS["3x1"], 4))


@pytest.mark.parametrize("grid,shape,chunks", [pytest.param(*c[1:], id=c[0]) for c in CASES])
def test_exchanged_ranges_stay_inside_their_regions(grid, shape, chunks):
    torch.cuda.set_device(0)
    for rank in range(grid[0] * grid[1]):
        pos = Position(grid, rank, shape, chunks)
        try:
            for family in FAMILIES:
                trace = pos.step(family, w_update=True)
                check_trace(trace, pos, family)
                assert bool(torch.isfinite(pos.W).all()) and bool(torch.isfinite(pos.H).all()), (rank, family)
        finally:
            pos.close()

