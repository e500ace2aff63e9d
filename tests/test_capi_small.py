"""The small whole-fit kernels (csrc/dnmf_small.h) without a GPU: which instantiation every test shape of the suite runs, as
dnmf_small_fit_plan reports it from the functions the launches call.  The tables below were recorded once and are asserted, so an
edit of the plans cannot silently move a shape to another kernel; tests/_exact.py::SMALL_REACH holds one shape for every instantiation
there is (tests/test_gpu_small_exact.py runs them all), and a scan of the query shows that the plans choose no geometry the table
lacks.  Also: the refusals of the two new entry points, and the workspace query against the bytes the plan's own numbers ask for.
Plans are {route, KP, NW, ALDS, P, ns, cw, bf16_resident}; route 0: the launch chain, 1: the barrier kernel, 2: the W-fixed MU/KL
kernel, 3: the HALS kernel (include/dnmf.h)."""
import ctypes

import pytest

from tests import _exact as ex
from tests.test_capi import _align256, _refused

METHOD = {("mu", "fro"): 0, ("mu", "kl"): 1, ("hals", "fro"): 2}
NONE = (0,) * 8


def _plan(method, bf16, w_update, m, n, k):
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_int * 8)(*([-7] * 8))
    assert lib.dnmf_small_fit_plan(method, bf16, w_update, m, n, k, out) == 0, lib.dnmf_last_error()
    return tuple(out)


# ---- 1. the shapes the suite had: tests/test_gpu_fit.py CASES (k <= 32; both settings of W_update, as its tests run them) ...
FIT_CASES = {
    ('mu', 'kl', 'float32', 1, 1000, 250, 9): (1, 16, 8, 1, 8, 256, 0, 0),
    ('mu', 'kl', 'float32', 0, 1000, 250, 9): (2, 16, 8, 0, 16, 256, 0, 0),
    ('mu', 'kl', 'float32', 1, 4100, 400, 20): (1, 32, 8, 0, 33, 400, 0, 0),
    ('mu', 'kl', 'float32', 0, 4100, 400, 20): (1, 32, 8, 0, 33, 400, 0, 0),
    ('mu', 'kl', 'float32', 1, 70, 33, 3): (1, 16, 4, 1, 2, 48, 0, 0),
    ('mu', 'kl', 'float32', 0, 70, 33, 3): (2, 16, 8, 0, 3, 48, 0, 0),
    ('mu', 'fro', 'float32', 1, 1000, 250, 9): (1, 16, 8, 1, 8, 256, 0, 0),
    ('mu', 'fro', 'float32', 0, 1000, 250, 9): (0, 0, 0, 0, 0, 0, 0, 0),
    ('mu', 'fro', 'float32', 1, 4100, 400, 20): (1, 32, 8, 0, 33, 400, 0, 0),
    ('mu', 'fro', 'float32', 0, 4100, 400, 20): (0, 0, 0, 0, 0, 0, 0, 0),
    ('mu', 'fro', 'float32', 1, 96, 21, 4): (1, 16, 4, 1, 2, 32, 0, 0),
    ('mu', 'fro', 'float32', 0, 96, 21, 4): (0, 0, 0, 0, 0, 0, 0, 0),
    ('hals', 'fro', 'bfloat16', 1, 1024, 256, 9): (3, 16, 8, 1, 8, 256, 32, 1),
    ('hals', 'fro', 'bfloat16', 0, 1024, 256, 9): (0, 0, 0, 0, 0, 0, 0, 0),
    ('hals', 'fro', 'float32', 1, 1000, 250, 20): (3, 32, 8, 0, 8, 256, 32, 0),
    ('hals', 'fro', 'float32', 0, 1000, 250, 20): (0, 0, 0, 0, 0, 0, 0, 0),
    ('hals', 'fro', 'float32', 1, 96, 21, 4): (3, 16, 4, 0, 2, 32, 16, 0),
    ('hals', 'fro', 'float32', 0, 96, 21, 4): (0, 0, 0, 0, 0, 0, 0, 0),
    ('mu', 'fro', 'bfloat16', 1, 1024, 256, 5): (1, 16, 8, 1, 8, 256, 0, 0),
    ('mu', 'fro', 'bfloat16', 0, 1024, 256, 5): (0, 0, 0, 0, 0, 0, 0, 0),
    ('mu', 'fro', 'bfloat16', 1, 1000, 250, 20): (1, 32, 8, 1, 8, 256, 0, 0),
    ('mu', 'fro', 'bfloat16', 0, 1000, 250, 20): (0, 0, 0, 0, 0, 0, 0, 0),
    ('mu', 'kl', 'float32', 1, 1024, 256, 16): (1, 16, 8, 1, 8, 256, 0, 0),
    ('mu', 'kl', 'float32', 0, 1024, 256, 16): (2, 16, 8, 0, 16, 256, 0, 0),
    ('mu', 'kl', 'float32', 1, 1024, 256, 17): (1, 32, 6, 1, 11, 256, 0, 0),
    ('mu', 'kl', 'float32', 0, 1024, 256, 17): (2, 32, 8, 0, 16, 256, 0, 0),
    ('mu', 'fro', 'float32', 1, 1024, 256, 4): (1, 16, 8, 1, 8, 256, 0, 0),
    ('mu', 'fro', 'float32', 0, 1024, 256, 4): (0, 0, 0, 0, 0, 0, 0, 0),
    ('mu', 'fro', 'float32', 1, 300, 200, 7): (1, 16, 8, 1, 3, 208, 0, 0),
    ('mu', 'fro', 'float32', 0, 300, 200, 7): (0, 0, 0, 0, 0, 0, 0, 0),
    ('mu', 'kl', 'float32', 1, 300, 200, 7): (1, 16, 8, 1, 3, 208, 0, 0),
    ('mu', 'kl', 'float32', 0, 300, 200, 7): (2, 16, 8, 0, 13, 208, 0, 0),
    ('hals', 'fro', 'bfloat16', 1, 2048, 512, 6): (3, 16, 8, 0, 16, 512, 32, 0),
    ('hals', 'fro', 'bfloat16', 0, 2048, 512, 6): (0, 0, 0, 0, 0, 0, 0, 0),
    ('hals', 'fro', 'float32', 1, 333, 129, 3): (3, 16, 8, 0, 3, 144, 48, 0),
    ('hals', 'fro', 'float32', 0, 333, 129, 3): (0, 0, 0, 0, 0, 0, 0, 0),
}
# ... test_persistent_fits_on_padded_operands_through_the_c_abi: (norm, w_update, m, n, k) ...
ABI_CASES = {
    ('kl', 1, 17, 5, 1): (1, 16, 4, 1, 1, 16, 0, 0),
    ('kl', 0, 17, 5, 1): (2, 16, 8, 0, 1, 16, 0, 0),
    ('fro', 1, 17, 5, 1): (1, 16, 4, 1, 1, 16, 0, 0),
    ('fro', 0, 17, 5, 1): (0, 0, 0, 0, 0, 0, 0, 0),
    ('kl', 1, 33, 300, 2): (1, 16, 4, 1, 1, 304, 0, 0),
    ('kl', 0, 33, 300, 2): (2, 16, 8, 0, 19, 304, 0, 0),
    ('fro', 1, 33, 300, 2): (1, 16, 4, 1, 1, 304, 0, 0),
    ('fro', 0, 33, 300, 2): (0, 0, 0, 0, 0, 0, 0, 0),
    ('kl', 1, 130, 47, 16): (1, 16, 8, 1, 2, 48, 0, 0),
    ('kl', 0, 130, 47, 16): (2, 16, 8, 0, 3, 48, 0, 0),
    ('fro', 1, 130, 47, 16): (1, 16, 8, 1, 2, 48, 0, 0),
    ('fro', 0, 130, 47, 16): (0, 0, 0, 0, 0, 0, 0, 0),
    ('kl', 1, 2050, 130, 17): (1, 32, 8, 1, 17, 144, 0, 0),
    ('kl', 0, 2050, 130, 17): (1, 32, 8, 1, 17, 144, 0, 0),
    ('fro', 1, 2050, 130, 17): (1, 32, 8, 1, 17, 144, 0, 0),
    ('fro', 0, 2050, 130, 17): (0, 0, 0, 0, 0, 0, 0, 0),
    ('kl', 1, 8192, 64, 32): (1, 32, 8, 1, 64, 64, 0, 0),
    ('kl', 0, 8192, 64, 32): (1, 32, 8, 1, 64, 64, 0, 0),
    ('fro', 1, 8192, 64, 32): (1, 32, 8, 1, 64, 64, 0, 0),
    ('fro', 0, 8192, 64, 32): (0, 0, 0, 0, 0, 0, 0, 0),
    ('kl', 1, 100, 500, 9): (1, 16, 4, 0, 2, 512, 0, 0),
    ('kl', 0, 100, 500, 9): (2, 16, 8, 0, 32, 512, 0, 0),
    ('fro', 1, 100, 500, 9): (1, 16, 4, 0, 2, 512, 0, 0),
    ('fro', 0, 100, 500, 9): (0, 0, 0, 0, 0, 0, 0, 0),
    ('kl', 1, 1500, 16, 5): (1, 16, 8, 1, 12, 16, 0, 0),
    ('kl', 0, 1500, 16, 5): (2, 16, 8, 0, 1, 16, 0, 0),
    ('fro', 1, 1500, 16, 5): (1, 16, 8, 1, 12, 16, 0, 0),
    ('fro', 0, 1500, 16, 5): (0, 0, 0, 0, 0, 0, 0, 0),
    ('kl', 1, 60, 2000, 12): (1, 16, 4, 0, 1, 2000, 0, 0),
    ('kl', 0, 60, 2000, 12): (2, 16, 8, 0, 125, 2000, 0, 0),
    ('fro', 1, 60, 2000, 12): (1, 16, 4, 0, 1, 2000, 0, 0),
    ('fro', 0, 60, 2000, 12): (0, 0, 0, 0, 0, 0, 0, 0),
    ('kl', 1, 40, 1100, 30): (1, 32, 4, 0, 1, 1104, 0, 0),
    ('kl', 0, 40, 1100, 30): (2, 32, 8, 0, 69, 1104, 0, 0),
    ('fro', 1, 40, 1100, 30): (1, 32, 4, 0, 1, 1104, 0, 0),
    ('fro', 0, 40, 1100, 30): (0, 0, 0, 0, 0, 0, 0, 0),
}
# ... and FIT of tests/test_gpu_exact.py (test_fit_itr1: mu-fro with W updated, mu-kl with W fixed)
EXACT_FIT = {
    ('fro', 1, 300, 130, 5): (1, 16, 8, 1, 3, 144, 0, 0),
    ('kl', 0, 300, 130, 5): (2, 16, 8, 0, 9, 144, 0, 0),
    ('fro', 1, 1000, 260, 16): (1, 16, 6, 1, 11, 272, 0, 0),
    ('kl', 0, 1000, 260, 16): (2, 16, 8, 0, 17, 272, 0, 0),
    ('fro', 1, 257, 600, 32): (1, 32, 8, 0, 3, 608, 0, 0),
    ('kl', 0, 257, 600, 32): (2, 32, 8, 0, 38, 608, 0, 0),
    ('fro', 1, 1030, 515, 17): (1, 32, 8, 0, 9, 528, 0, 0),
    ('kl', 0, 1030, 515, 17): (2, 32, 8, 0, 33, 528, 0, 0),
}


def test_earlier_fit_cases_run_what_the_table_says():
    from tests.test_gpu_fit import CASES
    want = {(method, norm, prec, wu, m, n, k) for m, n, k, method, norm, prec, itr in CASES if k <= 32 for wu in (1, 0)}
    assert want == set(FIT_CASES), "tests/test_gpu_fit.py CASES changed: record the plans of %s" % sorted(want ^ set(FIT_CASES))
    for (method, norm, prec, wu, m, n, k), plan in FIT_CASES.items():
        assert _plan(METHOD[(method, norm)], int(prec == "bfloat16"), wu, m, n, k) == plan, (method, norm, prec, wu, m, n, k)
    for m, n, k, method, norm, prec, itr in CASES:                         # beyond k = 32 there is no small kernel: refused, not planned
        if k > 32:
            from pydnmfk_amd._lib import lib
            assert lib.dnmf_small_fit_plan(METHOD[(method, norm)], int(prec == "bfloat16"), 1, m, n, k, (ctypes.c_int * 8)()) != 0


def test_padded_abi_cases_run_what_the_table_says():
    import inspect
    from tests import test_gpu_fit
    shapes = dict(inspect.signature(test_gpu_fit.test_persistent_fits_on_padded_operands_through_the_c_abi).parameters)   # (the test exists)
    assert {"m", "n", "k", "norm"} <= set(shapes)
    marks = [mk for mk in test_gpu_fit.test_persistent_fits_on_padded_operands_through_the_c_abi.pytestmark if mk.name == "parametrize" and mk.args[0] == "m,n,k"]
    want = {(norm, wu, m, n, k) for m, n, k in marks[0].args[1] for norm in ("kl", "fro") for wu in (1, 0)}
    assert want == set(ABI_CASES), "the shapes of the padded-operand test changed: record the plans of %s" % sorted(want ^ set(ABI_CASES))
    for (norm, wu, m, n, k), plan in ABI_CASES.items():
        assert _plan(METHOD[("mu", norm)], 0, wu, m, n, k) == plan, (norm, wu, m, n, k)
        # the test skips a shape dnmf_mu_fit_persistent refuses: none is (its Frobenius fits with W fixed take the launch chain on purpose)
        assert (plan != NONE) == (norm == "kl" or wu == 1), (norm, wu, m, n, k)


def test_exact_fit_cases_run_what_the_table_says():
    from tests.test_gpu_exact import FIT
    want = {(norm, wu) + tuple(p.values[:3]) for p in FIT for norm, wu in (("fro", 1), ("kl", 0))}
    assert want == set(EXACT_FIT), sorted(want ^ set(EXACT_FIT))
    for (norm, wu, m, n, k), plan in EXACT_FIT.items():
        assert _plan(METHOD[("mu", norm)], 0, wu, m, n, k) == plan, (norm, wu, m, n, k)


def _geometries(table):
    """{family: set of (route, KP, NW, ALDS, bf16_resident)} of a {.. m, n, k: plan} table keyed like the three above"""
    out = {}
    for key, plan in table:
        out.setdefault(key, set()).add((plan[0], plan[1], plan[2], plan[3], plan[7]))
    return out


def test_what_the_earlier_shapes_never_reached():
    """the gap SMALL_REACH closes, pinned: before it no test ran the MU/KL kernel with 96-row slabs at KP = 16 or with a streamed 128-row
    slab at KP = 16, nor either Frobenius kernel with 64-row slabs at KP = 32 and A in LDS, nor six of the eight geometries on bf16-stored
    data, nor the barrier kernel with W fixed at KP = 16, nor seven of the twelve HALS variants"""
    fam = lambda method, norm, prec, wu: ("hals" if method == "hals" else norm) + ("_bf16" if prec == "bfloat16" else "") + ("" if wu or method == "hals" else "_wfixed")
    old = [(fam(me, no, pr, wu), p) for (me, no, pr, wu, m, n, k), p in FIT_CASES.items()]
    old += [(fam("mu", no, "float32", wu), p) for table in (ABI_CASES, EXACT_FIT) for (no, wu, m, n, k), p in table.items()]
    had = _geometries((f, p) for f, p in old if p != NONE)
    now = _geometries((f, p) for f, m, n, k, p in ex.SMALL_REACH)
    missing = {f: sorted(now[f] - had.get(f, set())) for f in now if now[f] - had.get(f, set())}
    assert missing == NEVER_REACHED, missing


NEVER_REACHED = {
    "kl": [(1, 16, 6, 1, 0), (1, 16, 8, 0, 0), (1, 32, 4, 1, 0)],
    "fro": [(1, 16, 8, 0, 0), (1, 32, 4, 1, 0), (1, 32, 6, 1, 0)],
    "fro_bf16": [(1, 16, 4, 0, 0), (1, 16, 4, 1, 0), (1, 16, 8, 0, 0), (1, 32, 4, 0, 0), (1, 32, 4, 1, 0), (1, 32, 8, 0, 0)],
    "kl_wfixed": [(1, 16, 8, 1, 0)],
    "hals": [(3, 32, 4, 0, 0)],
    "hals_bf16": [(3, 16, 4, 0, 0), (3, 16, 4, 1, 1), (3, 32, 4, 0, 0), (3, 32, 4, 1, 1), (3, 32, 8, 0, 0), (3, 32, 8, 1, 1)],
}


# ---- 2. the reach table
@pytest.mark.parametrize("family,m,n,k,plan", ex.SMALL_REACH, ids=lambda v: str(v) if not isinstance(v, tuple) else "")
def test_reach_shapes_run_what_their_table_entry_says(family, m, n, k, plan):
    assert _plan(*ex.SMALL_FAMILIES[family], m, n, k) == plan
    route, kp, nw, alds, P, ns, cw, res = plan
    assert kp == (16 if k <= 16 else 32) and ns == -(-n // 16) * 16 and 1 <= m <= 8192 and n <= 4096
    if family.startswith("fro"):
        assert m % 3 and n % 3, "a Frobenius fixed point needs m and n not divisible by 3 (tests/_exact.py: fro_fixed)"
    if route == 2:
        assert family == "kl_wfixed" and P == ns // 16 and nw == 8
    else:
        assert route == (3 if family.startswith("hals") else 1) and P == -(-m // (16 * nw)) and 1 <= P <= 64 and (nw == 4 or P >= 2)
    if route == 3:
        assert cw == -(-ns // P) and alds == res and (res == 0 or family == "hals_bf16")


GEOM_MU = {(kp, nw, alds) for kp in (16, 32) for nw, alds in ((8, 1), (6, 1), (8, 0), (4, 1), (4, 0))}
GEOM_BF = {(kp, nw, alds) for kp in (16, 32) for nw, alds in ((8, 1), (8, 0), (4, 1), (4, 0))}
GEOM_HALS = {(kp, nw) for kp in (16, 32) for nw in (8, 4)}


def _of(family):
    return [e for e in ex.SMALL_REACH if e[0] == family]


def test_reach_table_holds_every_instantiation():
    """every kernel csrc/dnmf_fit.hip can launch: ten MU/KL and ten fp32 MU/FRO geometries, eight on bf16-stored data, both W-fixed
    kernels and the barrier kernel with W fixed, and the four HALS geometries reading A as streamed fp32, resident bf16 and streamed bf16"""
    for family, geoms in (("kl", GEOM_MU), ("fro", GEOM_MU), ("fro_bf16", GEOM_BF)):
        assert {p[1:4] for f, m, n, k, p in _of(family)} == geoms, family
        assert all(p[0] == 1 for f, m, n, k, p in _of(family))
    assert {(p[0], p[1]) for f, m, n, k, p in _of("kl_wfixed")} == {(2, 16), (2, 32), (1, 16), (1, 32)}
    assert {p[1:3] for f, m, n, k, p in _of("hals")} == GEOM_HALS and all(p[7] == 0 and p[3] == 0 for f, m, n, k, p in _of("hals"))
    for res in (0, 1):
        assert {p[1:3] for f, m, n, k, p in _of("hals_bf16") if p[7] == res} == GEOM_HALS, res


@pytest.mark.parametrize("family", ["kl", "fro", "fro_bf16", "hals", "hals_bf16"])
def test_reach_table_holds_the_edges_of_every_family(family):
    rows = _of(family)
    assert any(p[4] == 1 and p[2] == 4 for f, m, n, k, p in rows), "a single slab"
    assert any(p[4] == 64 for f, m, n, k, p in rows), "the maximum of 64 slabs"
    assert any(m % (16 * p[2]) for f, m, n, k, p in rows), "a ragged last slab"
    assert any(n % 16 for f, m, n, k, p in rows), "n % 16 != 0"
    assert {1, 16, 17, 32} <= {k for f, m, n, k, p in rows}, "k = 1, 16, 17, 32"
    if not family.startswith("hals"):                                       # the W phase: whole groups of four column tiles, a tail, both
        ncts = [p[5] // 16 for f, m, n, k, p in rows]
        assert any(c % 4 == 0 for c in ncts) and any(c < 4 for c in ncts) and any(c > 4 and c % 4 for c in ncts)
        assert any(p[5] > 256 for f, m, n, k, p in rows), "a second pass of the copy of H (256 columns per pass)"


def test_no_plan_leaves_the_table():
    """a scan of the query over m <= 8192, n <= 4096 (strided, with the slab boundaries) at k = 1, 16, 17, 32 -- the plans depend on k only
    through KP = 16 or 32 --: every plan is one of the instantiations above (a geometry the dispatch
    macros of csrc/dnmf_fit.hip do not list would fall through to the launch chain without a word), none of them is unreachable,
    and the limits of the table hold (P <= 64, a single slab only with NW = 4)"""
    ms = sorted(set(list(range(1, 140, 7)) + list(range(140, 8193, 379)) + [96, 97, 128, 129, 8192]))
    ns = sorted(set(list(range(1, 64, 9)) + list(range(64, 4097, 131)) + [4096]))
    seen = {f: set() for f in ex.SMALL_FAMILIES}
    for family, (method, bf16, wu) in ex.SMALL_FAMILIES.items():
        for k in (1, 16, 17, 32):
            for m in ms:
                for n in ns:
                    p = _plan(method, bf16, wu, m, n, k)
                    if p == NONE:
                        continue
                    assert 1 <= p[4] <= (64 if p[0] != 2 else 256) and (p[0] == 2 or p[2] == 4 or p[4] >= 2), (family, m, n, k, p)
                    seen[family].add((p[0], p[1], p[2], p[3], p[7]))
    table = _geometries((f, p) for f, m, n, k, p in ex.SMALL_REACH)
    # (W fixed is a run-time argument of the barrier kernel: its instantiations are the MU/KL family's, of which the table runs two)
    wf_seen, wf_table = seen.pop("kl_wfixed"), table.pop("kl_wfixed")
    assert {g for g in wf_seen if g[0] == 2} == {g for g in wf_table if g[0] == 2} and {g for g in wf_table if g[0] == 1} <= {g for g in wf_seen if g[0] == 1} <= table["kl"]
    assert seen == table, {f: (sorted(seen[f] - table[f]), sorted(table[f] - seen[f])) for f in seen if seen[f] != table[f]}


# ---- 3. refusals, the counters, the workspace
def test_small_fit_plan_refusals():
    from pydnmfk_amd._lib import lib
    out = (ctypes.c_int * 8)()
    good = dict(method=1, bf16=0, w_update=1, m=130, n=37, k=5, out=ctypes.addressof(out))
    for bad in (dict(method=3), dict(method=-1), dict(k=0), dict(k=33), dict(k=-1), dict(m=0), dict(n=0), dict(m=-3), dict(out=None),
                dict(bf16=1)):                                              # (bfloat16 storage is for the Frobenius updates)
        _refused(lib, "dnmf_small_fit_plan", "small_fit_plan", good, **bad)
    _refused(lib, "dnmf_small_fit_launches", "small_fit_launches", dict(out=ctypes.addressof(out)), out=None)
    # past the limits of the plans the answer is "none", not a refusal
    assert _plan(1, 0, 1, 8193, 37, 5) == NONE and _plan(1, 0, 1, 130, 4097, 5) == NONE and _plan(2, 0, 0, 130, 37, 5) == NONE


def test_launch_counters_are_readable_and_only_grow():
    from pydnmfk_amd._lib import lib
    a, b = (ctypes.c_ulonglong * 4)(*([7] * 4)), (ctypes.c_ulonglong * 4)()
    assert lib.dnmf_small_fit_launches(a) == 0 and lib.dnmf_small_fit_launches(b) == 0
    assert all(y >= x for x, y in zip(a, b)) and max(b) < 1 << 40                # (written: the 7s are gone unless real counts)


def _plan_bytes(plan):
    """the bytes the persistent kernels use behind the step workspace of one problem (csrc/dnmf_fit.hip): the slabs' partials [P][KP][ns]
    and [P][KP][KP], HALS: the column-norm slots [2][KP][P], the granules of H [KP][ns] x 8 bytes, all in 4-byte words with the areas 16-byte
    aligned, rounded up to 256 bytes, and 256 bytes for the arrival counter"""
    route, kp, nw, alds, P, ns, cw, res = plan
    if route == 2:
        return 0
    words = -(-(P * kp * ns + P * kp * kp) // 4) * 4
    if route == 3:
        words += -(-(2 * kp * P) // 4) * 4
    return _align256((words + 2 * kp * ns) * 4) + 256


def test_fit_workspace_covers_the_plan():
    from pydnmfk_amd._lib import lib
    for family, m, n, k, plan in ex.SMALL_REACH:
        one = lib.dnmf_ws_bytes_fit(m, n, k, 1)
        assert one >= lib.dnmf_ws_bytes(m, n, k) + _plan_bytes(plan) > 0, (family, m, n, k)
        assert lib.dnmf_ws_bytes_fit(m, n, k, 3) == 3 * one and one % 256 == 0
