"""The workspace contract of include/dnmf.h, what can be held without a GPU (tests/test_gpu_workspace.py runs the kernels):

  * completeness: every entry point of _lib.SIGNATURES that takes `(ws, ws_bytes)` is reached by a case of the GPU file's table, or is a
    host-only function named in EXEMPT -- no entry point that launches a kernel is left out;
  * the plan of every ws-taking dense entry point is the same at ws_bytes = query, query + 256, 4 query + 4096 and 2^33: the engine
    passes the size of a cached buffer, which depends on what the process ran before, so "run-to-run bit-reproducible" (DESIGN.md
    section 5) needs the choice to follow the query, not the gift;
  * dnmf_ws_bytes(m, k, k) always covers the T image of the persistent HALS sweep (csrc/dnmf_hals.hip decides between the sweep and
    the column launches by `ws_bytes`);
  * every size a case of the GPU table lets the engine ask is a nonzero answer of the query include/dnmf.h names for it (the engine
    methods themselves refuse host tensors: that they ask exactly these sizes is asserted on the GPU, from the recorded sequence)."""
import ctypes

import pytest

pytest.importorskip("torch")

from pydnmfk_amd import _lib  # noqa: E402
from tests import test_gpu_workspace as G  # noqa: E402

lib = _lib.lib

# host-only functions with a (void*, size_t) pair in their argument list: nothing here launches a kernel
EXEMPT = {
    "dnmf_dense_plan": "host only: reports the plan of a dense entry point for a given ws_bytes (held to size invariance below)",
}


def ws_taking():
    """the names of SIGNATURES whose argument list holds c_void_p followed by c_size_t, outside dnmf_comm_*"""
    out = []
    for name, args in _lib.SIGNATURES.items():
        if name.startswith("dnmf_comm_"):
            continue
        if any(args[i] is ctypes.c_void_p and args[i + 1] is ctypes.c_size_t for i in range(len(args) - 1)):
            out.append(name)
    return out


def test_every_ws_taking_entry_point_is_in_the_case_table():
    names = ws_taking()
    assert len(names) == 73, "the ABI changed: %d entry points take (ws, ws_bytes) -- extend the case table of tests/test_gpu_workspace.py" % len(names)
    covered = {n for c in G.CASES for n in c.names}
    assert covered <= set(names), "the case table names entry points without a workspace: %s" % sorted(covered - set(names))
    missing = [n for n in names if n not in covered and n not in EXEMPT]
    assert not missing, "no case of tests/test_gpu_workspace.py reaches %s" % missing
    assert not set(EXEMPT) & covered and set(EXEMPT) <= set(names)
    assert len(names) - len(EXEMPT) == 72                           # the launching entry points: none exempt
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))


def test_exempt_functions_launch_nothing():
    """an EXEMPT function answers without a device: dnmf_dense_plan fills its plan on this host"""
    p = _lib.dense_plan("wta", 300, 130, 5)
    assert p["family"] != "none"


M = (1, 33, 129, 300, 513, 1000, 2049, 4100, 8200, 20000)
N = (4, 31, 97, 128, 260, 515, 1024, 2052, 4100)
K = (1, 5, 16, 17, 32, 33, 64, 65, 128)
WS_OPS = ("wta", "wta_gram", "gram_hht", "gram_wtw", "kl_uht", "kl_wtu", "resid_sqnorm")      # the dense entry points that take (ws, ws_bytes)


@pytest.mark.parametrize("op", WS_OPS)
def test_dense_plan_does_not_depend_on_the_size_of_the_gift(op):
    """10 x 9 x 9 shapes x 3 larger workspaces per op (17 010 comparisons over the seven ops), fp32 A; bf16-stored A where the op has it"""
    for bf16a in (False, True) if op in ("wta", "wta_gram", "resid_sqnorm") else (False,):
        for m in M:
            for n in N:
                for k in K:
                    q = int(lib.dnmf_ws_bytes(m, n, k))
                    assert q > 0
                    at_query = _lib.dense_plan(op, m, n, k, bf16a=bf16a, ws_bytes=q)
                    for more in (q + 256, 4 * q + 4096, 1 << 33):
                        p = _lib.dense_plan(op, m, n, k, bf16a=bf16a, ws_bytes=more)
                        assert p == at_query, "%s %dx%d k=%d bf16a=%s: the plan at ws_bytes = %d differs from the plan at the query %d: %s" % (
                            op, m, n, k, bf16a, more, q, {f: (at_query[f], p[f]) for f in p if p[f] != at_query[f]})


def test_hblocks_plan_does_not_depend_on_the_size_of_the_gift():
    """kl_uht_hblocks on its own query (dnmf_ws_bytes_hblocks), 32-column blocks"""
    nh = 32
    for m in M:
        for n in (32, 128, 1024, 65 * 32):
            for k in K:
                q = int(lib.dnmf_ws_bytes_hblocks(m, n, k, nh))
                assert q > 0
                at_query = _lib.dense_plan("kl_uht_hblocks", m, n, k, ld=[n, k, nh, k], ws_bytes=q)
                for more in (q + 256, 4 * q + 4096, 1 << 33):
                    assert _lib.dense_plan("kl_uht_hblocks", m, n, k, ld=[n, k, nh, k], ws_bytes=more) == at_query, (m, n, k, more)


HALS_MAX_WG = 1024                                                  # slots per column of the slab (csrc/dnmf_common.h; engine._HALS_MAX_WG)


def test_the_dense_query_covers_the_persistent_hals_sweep():
    """dnmf_hals_sweep_w takes the persistent sweep when ws_bytes >= t_off + m KP 4 (t_off: the slot slab and the KP sums of squares,
    rounded up to 256) and column launches otherwise: the query of its workspace, dnmf_ws_bytes(m, k, k), must never decide that"""
    from pydnmfk_amd import engine
    assert engine._HALS_MAX_WG == HALS_MAX_WG
    ms = sorted({1, 2, 255, 256, 257, 511, 512, 513, 1000, 4095, 4096, 65536, 100000, 262143, 262144} | {512 * w + d for w in (1, 64, 256, 511) for d in (-1, 0, 1)})
    for kp, ks in ((32, (1, 5, 32)), (64, (33, 64)), (128, (65, 100, 128))):
        for k in ks:
            assert lib.dnmf_kp(k) == kp
            slab = kp * HALS_MAX_WG * 8
            t_off = (slab + kp * 8 + 255) // 256 * 256
            for m in ms:
                assert int(lib.dnmf_ws_bytes(m, k, k)) >= t_off + m * kp * 4, (m, k, int(lib.dnmf_ws_bytes(m, k, k)), t_off + m * kp * 4)


@pytest.mark.parametrize("case", [c for c in G.CASES if c.query is not None], ids=lambda c: c.id)
def test_the_queries_of_the_case_table_answer(case):
    """the sizes the GPU file holds the engine to are nonzero answers of the library's queries"""
    sizes = {int(q) for q in case.query(lib)}
    assert sizes and all(q > 0 for q in sizes), (case.id, sizes)


def test_every_case_names_its_queries():
    assert [c.id for c in G.CASES if c.query is None] == []
