"""Which kernel a shape takes on the float64 entry points (csrc/dnmf_f64.hip), without a GPU: dnmf_f64_plan is answered by the plan
functions the entry points launch from.  Every shape of the table in tests/_exact.py (the cases of tests/test_gpu_exact_f64.py) must
report the variant it is listed with, the union of the variants must be EVERY instantiation the dispatch can launch, and both sides of
every host branch must be taken.

The launchable set, from the template-argument ranges of the *_CASE macros of csrc/dnmf_f64.hip:
  f64_nt_kernel<RT, NT, VEC>          NT_ROWS: RT in {1, 2, 4} x NT in {1, 2, 4}; NT = 8 with RT in {1, 2}; VEC both          22
  f64_tn_kernel<NT, VEC>              TN_CASE: NT in {1, 2, 4, 8}; VEC both                                                    8
  f64_kl_uht_kernel<NT, RT, VEC, FULL>  UHT_CASE: RT = 4 with NT in {1, 2}, RT in {1, 2} with NT in {1, 2, 4};
                                      (VEC, FULL) in {(1, 1), (1, 0), (0, 0)}                                                 24
  f64_kl_wtu_kernel<NT, CT, VEC>      WTU_CASE: NT in {1, 2, 4}, CT = kl_ct(NT); VEC both                                      6
  f64_nn_cols_kernel<KS, MODE, VEC>   NNC_CASE: KS in {4, 8, 16, 32} x {QUOT, SQDIFF}; VEC both                                16
  f64_nn_rows_kernel<KS, NN_UPD_W>, f64_upd_h_kernel<KS>      KS in {4, 8, 16, 32}                                            4 + 4
  f64_reduce_kernel<V>                V in {1, 2}, after each of NT, TN, KL_UHT, KL_WTU, COLSUM
84 instantiations of the matrix-core kernels in all."""
import ctypes
import itertools

import pytest

from pydnmfk_amd._lib import f64_plan, lib
from tests import _exact as ex


def _ld(aligned, *cols):
    return [ex.f64_pitch(c, aligned) for c in cols]


def _both(op, m, n, k, *cols):
    """the plan at the pitches of an aligned and of an unaligned Poisoned view: the same (pitches only enter the window checks)"""
    a, u = (f64_plan(op, m, n, k, _ld(al, *cols)) for al in (True, False))
    assert a == u == f64_plan(op, m, n, k), (op, m, n, k)
    return a


def _is(p, **want):
    got = {f: p[f] for f in want}
    assert got == {f: (int(v) if not isinstance(v, str) else v) for f, v in want.items()}, (p, want)


def aht_plan(m, n, k):
    return _both("aht", m, n, k, n, n)


def wta_plan(m, n, k):
    return _both("wta", m, n, k, n, k)


@pytest.mark.parametrize("case", ex.F64_AHT, ids=str)
def test_aht_shapes(case):
    m, n, k, rt, nt, vec, splits, v = case
    p = aht_plan(m, n, k)
    _is(p, family="nt", rt=rt, nt=nt, vec=vec, d=3 if nt == 1 else 2, count=splits, v=v, grid_y=splits, grid_x=-(-(-(-m // (16 * rt))) // 4))
    assert (splits - 1) * p["per"] < n <= splits * p["per"] and p["per"] % 16 == 0
    _is(aht_plan(k, n, k), family="nt", rt=1, nt=nt, vec=vec, count=splits)         # gram_hht: the k x n factor against itself


@pytest.mark.parametrize("case", ex.F64_WTA, ids=str)
def test_wta_shapes(case):
    m, n, k, nt, ct, vec, chunks, rpc, v = case
    p = wta_plan(m, n, k)
    _is(p, family="tn", nt=nt, rt=ct, vec=vec, count=chunks, per=rpc, v=v, waves=chunks * -(-n // (16 * ct)))
    assert (chunks - 1) * rpc < m <= chunks * rpc
    g = wta_plan(m, k, k)                                                            # gram_wtw: n = k
    _is(g, family="tn", nt=nt, rt=ct, vec=k % ct == 0 and k % min(nt, 4) == 0)


@pytest.mark.parametrize("case", ex.F64_KL_UHT + [(m, n, k, nt, rt, True, True, s, v) for m, n, k, nt, rt, s, v in ex.F64_KL_UHT_BIG], ids=str)
def test_kl_uht_shapes(case):
    m, n, k, nt, rt, vec, full, splits, v = case
    p = _both("kl_uht", m, n, k, n, k, n)
    _is(p, family="kl_uht", nt=nt, rt=rt, vec=vec, full=full, count=splits, v=v, grid_y=splits)
    assert (splits - 1) * p["per"] < n <= splits * p["per"] and p["per"] % 64 == 0
    assert full == (n % p["per"] == 0)


@pytest.mark.parametrize("case", ex.F64_KL_WTU, ids=str)
def test_kl_wtu_shapes(case):
    m, n, k, nt, ct, vec, chunks, v = case
    p = _both("kl_wtu", m, n, k, n, k, n)
    _is(p, family="kl_wtu", nt=nt, rt=ct, vec=vec, count=chunks, v=v)
    assert (chunks - 1) * p["per"] < m <= chunks * p["per"] and p["per"] % 16 == 0


@pytest.mark.parametrize("case", ex.F64_IMAGE, ids=str)
def test_image_shapes(case):
    m, n, k, ks, ct, vec, chunks = case
    for op in ("kl_quot", "sqdiff"):
        p = _both(op, m, n, k, n, k, n, n)
        _is(p, family="nn_cols", nt=ks, rt=ct, vec=vec, count=chunks)
        assert (chunks - 1) * p["per"] < m <= chunks * p["per"]
    for op in ("kl_uht", "kl_wtu"):
        assert (f64_plan(op, m, n, k)["family"] == "image") == (k > 64)


@pytest.mark.parametrize("case", ex.F64_MU, ids=str)
def test_mu_update_shapes(case):
    m, n, k, ks = case
    _is(f64_plan("mu_update_w", m, n, k), family="nn_rows", nt=ks, grid_x=-(-(-(-m // 16)) // 4))
    _is(f64_plan("mu_update_h", m, n, k), family="upd_h", nt=ks, grid_x=-(-(-(-n // 16)) // 4))
    assert k % 4 and m % 16 and n % 16


@pytest.mark.parametrize("method,cases", [(0, ex.F64_FIT_FRO), (1, ex.F64_FIT_KL)])
def test_fit_shapes(method, cases):
    for m, n, k, fam in cases:
        assert f64_plan("fit", m, n, k, method=method)["family"] == fam, (m, n, k)
        assert lib.dnmf_f64_fit_tiny(m, n, k, method) == int(fam == "fit_tiny")
    tiny = [c for c in cases if c[3] == "fit_tiny"]
    assert any(m * k > 256 and k * n > 256 and n > 256 for m, n, k, _ in tiny) and any(k == 1 for _, _, k, _ in tiny)
    m, n, k, _ = tiny[-1]                                                            # the largest: one more row or column leaves
    assert k == 16 and not lib.dnmf_f64_fit_tiny(m + 1, n, k, method) and not lib.dnmf_f64_fit_tiny(m, n + 1, k, method)
    chain = [c for c in cases if c[3] == "fit_chain"]
    assert any(k > 16 for _, _, k, _ in chain)
    m, n, k, _ = chain[0]                                                            # just past the LDS limit
    assert k <= 16 and (lib.dnmf_f64_fit_tiny(m - 1, n, k, method) or lib.dnmf_f64_fit_tiny(m, n - 1, k, method))
    assert f64_plan("fit", *ex.F64_FIT_STACK, method=0)["family"] == "fit_tiny"


def test_every_launchable_instantiation_is_reached():
    vec = (0, 1)
    want = set()
    want |= {("nt", rt, nt, v) for rt in (1, 2, 4) for nt in (1, 2, 4) for v in vec} | {("nt", rt, 8, v) for rt in (1, 2) for v in vec}
    want |= {("tn", nt, v) for nt in (1, 2, 4, 8) for v in vec}
    want |= {("kl_uht", nt, rt, v, f) for nt, rt in ((1, 4), (2, 4), (1, 2), (2, 2), (4, 2), (1, 1), (2, 1), (4, 1)) for v, f in ((1, 1), (1, 0), (0, 0))}
    want |= {("kl_wtu", nt, 4 if nt <= 2 else 2, v) for nt in (1, 2, 4) for v in vec}
    want |= {("nn_cols", ks, mode, v) for ks in (4, 8, 16, 32) for mode in ("kl_quot", "sqdiff") for v in vec}
    want |= {(fam, ks) for fam in ("nn_rows", "upd_h") for ks in (4, 8, 16, 32)}
    want |= {("reduce", after, v) for after in ("nt", "tn", "kl_uht", "kl_wtu", "colsum") for v in (1, 2)}
    assert len(want - {w for w in want if w[0] == "reduce"}) == 22 + 8 + 24 + 6 + 16 + 4 + 4

    got = set()

    def red(p):
        if p["v"]:
            got.add(("reduce", p["family"], p["v"]))

    for m, n, k, *_ in ex.F64_AHT:
        for p in (aht_plan(m, n, k), aht_plan(k, n, k)):
            got.add(("nt", p["rt"], p["nt"], p["vec"])); red(p)
    for m, n, k, *_ in ex.F64_WTA:
        for p in (wta_plan(m, n, k), wta_plan(m, k, k)):
            got.add(("tn", p["nt"], p["vec"])); red(p)
    for m, n, k, *_ in ex.F64_KL_UHT + ex.F64_KL_UHT_BIG:
        p = f64_plan("kl_uht", m, n, k)
        got.add(("kl_uht", p["nt"], p["rt"], p["vec"], p["full"])); red(p)
    for m, n, k, *_ in ex.F64_KL_WTU:
        p = f64_plan("kl_wtu", m, n, k)
        got.add(("kl_wtu", p["nt"], p["rt"], p["vec"])); red(p)
    for m, n, k, *_ in ex.F64_IMAGE:
        for op in ("kl_quot", "sqdiff"):
            p = f64_plan(op, m, n, k)
            got.add(("nn_cols", p["nt"], op, p["vec"]))
        red(f64_plan("colsum", m, n, k))                                            # column_err_sums: the column sums of the image
        if k > 64:                                                                   # the KL products on the image: the NT and TN forms again
            for p in (aht_plan(m, n, k), wta_plan(m, n, k)):
                got.add((p["family"],) + ((p["rt"], p["nt"], p["vec"]) if p["family"] == "nt" else (p["nt"], p["vec"]))); red(p)
    for m, n, k, _ in ex.F64_MU:
        got.add(("nn_rows", f64_plan("mu_update_w", m, n, k)["nt"]))
        got.add(("upd_h", f64_plan("mu_update_h", m, n, k)["nt"]))
        red(f64_plan("colsum", m, k, k))                                            # colsum of W (k = 9: V = 1)
    assert got == want, "never launched: %s; not in the stated set: %s" % (sorted(want - got, key=str), sorted(got - want, key=str))


def test_both_sides_of_every_host_branch():
    """splits or none, one chunk or several, idle waves in the last workgroup or none, a reduction or none, grid-stride loops of one
    trip and of several, the fused KL kernels and the image path, the tiny fit and the chain"""
    aht = [aht_plan(m, n, k) for m, n, k, *_ in ex.F64_AHT]
    assert {p["count"] > 1 for p in aht} == {False, True} and {p["v"] for p in aht} == {0, 1, 2}
    assert any(n % p["per"] for (m, n, *_), p in zip(ex.F64_AHT, aht) if p["count"] > 1)                    # a ragged last split
    # NT = 1, RT = 1: steps of 32 columns through a ring of three register sets -- trip counts of every residue
    assert {-(-n // 32) % 3 for m, n, k, rt, nt, vec, splits, v in ex.F64_AHT if (rt, nt, splits) == (1, 1, 1)} == {0, 1, 2}
    for plans, table in (([wta_plan(m, n, k) for m, n, k, *_ in ex.F64_WTA], ex.F64_WTA),
                         ([f64_plan("kl_wtu", m, n, k) for m, n, k, *_ in ex.F64_KL_WTU], ex.F64_KL_WTU)):
        assert {p["count"] > 1 for p in plans} == {False, True} and {p["v"] for p in plans} == {1, 2}
        assert any(m % p["per"] for (m, *_), p in zip(table, plans) if p["count"] > 1)                      # a ragged last chunk
        assert {p["waves"] % 4 != 0 for p in plans} == {False, True}                                       # idle waves in the last workgroup
        assert any(p["per"] % 32 for p in plans if p["count"] > 1)                                          # a chunk of an odd number of 16-row tiles
    uht = [f64_plan("kl_uht", m, n, k) for m, n, k, *_ in ex.F64_KL_UHT + ex.F64_KL_UHT_BIG]
    assert {(p["rt"], p["count"] > 1) for p in uht} == set(itertools.product((1, 2, 4), (False, True)))
    assert {p["v"] for p in uht} == {0, 1, 2}
    assert {f64_plan("kl_uht", m, n, k)["family"] for m, n, k, *_ in ex.F64_IMAGE} == {"kl_uht", "image"}
    img = [f64_plan("sqdiff", m, n, k) for m, n, k, *_ in ex.F64_IMAGE]
    assert {p["count"] > 1 for p in img} == {False, True}
    trips = lambda op, m, n: -(-m * n // (256 * f64_plan(op, m, n, 1)["grid_x"]))
    assert max(trips("sum", m, n) for m, n, *_ in ex.F64_IMAGE) > 8 >= min(trips("sum", m, n) for m, n, *_ in ex.F64_IMAGE)
    assert {trips("ew", m, n) > 1 for m, n, *_ in ex.F64_IMAGE} == {False, True}
    assert {f64_plan("colsum", m, n, 1)["count"] > 1 for m, n, *_ in ex.F64_IMAGE} == {False, True}
    for method, cases in ((0, ex.F64_FIT_FRO), (1, ex.F64_FIT_KL)):
        assert {f64_plan("fit", m, n, k, method=method)["family"] for m, n, k, _ in cases} == {"fit_tiny", "fit_chain"}


def test_the_window_and_the_refusals():
    """a pitch beyond the 2 GiB window: the entry point refuses (family none) or halves its row tiles; bad arguments are refused"""
    assert f64_plan("aht", 16400, 72, 9, [1 << 24, 72])["family"] == "none"
    assert f64_plan("aht", 16400, 72, 9, [1 << 22, 72])["rt"] == 2 and f64_plan("aht", 16400, 72, 9, [1 << 21, 72])["rt"] == 4
    assert f64_plan("kl_uht", 65500, 68, 20, [1 << 22, 20, 68])["rt"] == 2
    assert f64_plan("kl_uht", 40, 64, 9, [1 << 24, 9, 64])["family"] == "image"
    assert f64_plan("sqdiff", 40, 64, 9, [64, 9, 64, 1 << 24])["family"] == "none"
    out = (ctypes.c_long * 12)()
    for op, m, n, k, method in ((-1, 4, 4, 1, 0), (12, 4, 4, 1, 0), (0, 0, 4, 1, 0), (0, 4, 0, 1, 0), (0, 4, 4, 0, 0), (0, 4, 4, 129, 0), (11, 4, 4, 1, 3)):
        assert lib.dnmf_f64_plan(op, m, n, k, None, method, out) != 0
    assert lib.dnmf_f64_plan(0, 4, 4, 1, None, 0, None) != 0
