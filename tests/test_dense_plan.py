"""Which kernel a shape takes on the fp32 dense entry points (csrc/dnmf.hip, csrc/dnmf_kl.hip), without a GPU: dnmf_dense_plan is
answered by the selectors the entry points launch from, and dnmf_dense_plan_variants lists what those selectors can return by calling
them over their whole input domain.  Every case of DENSE_REACH / DENSE_EW (tests/_exact.py: the cases of tests/test_gpu_exact_dense.py)
must report the plan it is listed with; the union of the cases must be EVERY variant of that list, both sides of every host branch and
every loop-trip class named below; and the reach of the older exact shapes (PRIM / FRO of tests/test_gpu_exact.py) is computed the same
way and held against the table in DESIGN.md, so the gap this tier closes is on paper.

Left out, by name (ex.DENSE_EXEMPT): only what needs an operand above 1 GiB -- the 2 GiB descriptor-window fallbacks, which stay with
tests/test_gpu_kernels.py -- and what the selectors cannot return at all (asserted here).  """
import os

import pytest

from pydnmfk_amd import _lib as L
from tests import _exact as ex

VF = L.DENSE_VARIANT_FIELDS


def plan(case, quantum8=True):
    cid, op, m, n, k, aligned, bf16, _ = case
    ld, off = ex.dense_plan_args(op, m, n, k, aligned, bf16, quantum8)
    ws = L.lib.dnmf_ws_bytes_hblocks(m, n, k, ex.DENSE_HBLK) if op == "kl_uht_hblocks" else None
    return L.dense_plan(op, max(m, 1), max(n, 1), k, ld, off, bf16a=bf16, ws_bytes=ws)


def ew_plan(case):
    cid, op, rows, cols, aligned, _ = case
    pitch, lead = ex.dense_pitch(cols, aligned is not False)
    offx = 12 if aligned == "x" else 0                             # the vector x: a 1-D tensor, 16-byte aligned unless the case says so
    return L.dense_plan("ew", rows, cols, 1, [pitch, pitch, 0], [lead * 4 % 16, lead * 4 % 16, offx], ew_op=op)


def variant(p, bf16):
    return tuple([p["family"]] + [p[f] for f in VF[1:-1]] + [int(bool(bf16))])


PLANS = [(c, plan(c)) for c in ex.DENSE_REACH]
EW_PLANS = [(c, ew_plan(c)) for c in ex.DENSE_EW]


def _is(p, want, cid):
    got = {f: p[f] for f in want}
    assert got == {f: (v if isinstance(v, str) else int(v)) for f, v in want.items()}, (cid, p)


@pytest.mark.parametrize("case", ex.DENSE_REACH, ids=lambda c: c[0])
def test_case_plan(case):
    _is(plan(case), case[-1], case[0])


@pytest.mark.parametrize("case", ex.DENSE_EW, ids=lambda c: c[0])
def test_ew_case_plan(case):
    _is(ew_plan(case), case[-1], case[0])


def test_recorded_partitions():
    """ex.DENSE_CHUNKS, which the CPU proofs of the operands walk, is what the library plans"""
    want = {c[0]: (p["count"], p["per"]) for c, p in PLANS if c[1] in ("wta", "wta_gram", "gram_wtw", "gram_hht", "kl_wtu")}
    assert ex.DENSE_CHUNKS == want


def test_ids_are_unique():
    ids = [c[0] for c in ex.DENSE_REACH + ex.DENSE_EW]
    assert len(ids) == len(set(ids))


def _reached():
    return {variant(p, c[6]) for c, p in PLANS} | {variant(p, False) for c, p in EW_PLANS}


def test_every_variant_is_reached():
    """the selectors' own list against the table: nothing is missing, and the table reaches nothing the list does not know (the list
    would be incomplete)"""
    every = L.dense_plan_variants()
    got = _reached()
    assert got <= every, sorted(got - every)
    assert every == got, sorted(every - got)
    fams = {v[0] for v in every}
    assert fams == set(L.DENSE_FAMILIES) - {"none", "wide"}


def test_unreachable():
    """what the template set holds and the selectors never return: update_w_seq_kernel<KT, 4, OCC, false> (an aligned W with whole
    ranks and whole 32-row tiles is update_w16_kernel's -- its window test cannot fail below the pitch mu_update_w refuses)"""
    every = L.dense_plan_variants()
    assert not [v for v in every if v[0] == "update_w_seq" and v[VF.index("v")] == 4 and v[VF.index("edge")] == 0]
    big = 1 << 23
    assert L.dense_plan("mu_update_w", 64, 1, 64, [big, 68])["family"] == "none"
    assert L.dense_plan("mu_update_w", 64, 1, 64, [big - 4, big - 4])["family"] == "update_w16"
    assert L.dense_plan("mu_update_h", 1, 64, 64, [1 << 24, 68])["family"] == "none"


def _both(values, what):
    assert set(values) == {0, 1}, "%s: only %s" % (what, sorted(set(values)))


def test_host_branches_both_ways():
    nt = [(c, p) for c, p in PLANS if p["family"] == "nt"]
    tn = [(c, p) for c, p in PLANS if p["family"] == "tn"]
    for kt in (1, 2, 4):
        _both([p["fast"] for c, p in nt if p["kt"] == kt], "nt fast, KT %d" % kt)
        _both([p["fast"] for c, p in tn if p["kt"] == kt], "tn fast, KT %d" % kt)
        _both([int(p["interior"] > 0) for c, p in nt if p["kt"] == kt and p["fast"]], "nt interior, KT %d" % kt)
        _both([int(p["pf"] == 13) for c, p in nt if p["kt"] == kt and p["pf"] in (10, 13)], "PF 13 / 10, KT %d" % kt)
        _both([int(p["eligible"] > 0) for c, p in nt if p["kt"] == kt and p["pf"] in (10, 13)], "descriptor loop, KT %d" % kt)
        _both([int(p["pf"] == 1) for c, p in nt if p["kt"] == kt and p["fast"] and not c[6]], "store_all keeps PF 1, KT %d" % kt)
    _both([p["wfast"] for c, p in nt if p["mode"] == 1 and p["fast"]], "wfast")
    _both([int(p["interior"] > 0) for c, p in nt if c[6] and p["fast"]], "bf16 interior")
    _both([int(p["family"] == "nt16") for c, p in PLANS if c[1].startswith("aht") and c[4] <= 16], "nt16 at k <= 16")
    _both([int(p["family"].startswith("tn16")) for c, p in PLANS if c[1].startswith("wta") and c[4] <= 16], "tn16 at k <= 16")
    _both([int(p["family"] == "tn16_gram") for c, p in PLANS if c[1] == "wta_gram" and p["family"].startswith("tn16")], "riding Gram")
    assert {p["reduce"] for c, p in PLANS if c[1].startswith("wta")} == {"single", "wide", "two_stage"}
    assert {p["reduce"] for c, p in PLANS if c[1] == "gram_wtw"} == {"single", "two_stage"}
    assert {p["reduce"] for c, p in PLANS if c[1] == "gram_hht"} == {"single", "two_stage"}
    assert {p["count"] > 1 for c, p in PLANS if c[1] == "gram_hht"} == {False, True}
    upw = [(c, p) for c, p in PLANS if c[1] == "mu_update_w"]
    uph = [(c, p) for c, p in PLANS if c[1] == "mu_update_h"]
    for kt in (1, 2, 4):
        _both([int(p["family"] == "update_w16") for c, p in upw if p["kt"] == kt], "update_w16, KT %d" % kt)
        _both([p["fast"] for c, p in upw if p["kt"] == kt and p["family"] == "update_w_seq"], "update_w_seq V, KT %d" % kt)
        _both([p["edge"] for c, p in upw if p["kt"] == kt and p["v"] == 1], "update_w_seq<V = 1> EDGE, KT %d" % kt)
        _both([p["nt"] - 1 for c, p in uph if p["kt"] == kt], "update_h_seq NT, KT %d" % kt)
        _both([p["edge"] for c, p in uph if p["kt"] == kt and p["nt"] == 1], "update_h_seq EDGE, KT %d" % kt)
        _both([p["ntemp"] for c, p in uph if p["kt"] == kt and p["nt"] == 2], "update_h_seq nontemporal, KT %d" % kt)
    for f in ("mode", "ntemp"):
        _both([p[f] for c, p in EW_PLANS], "ew " + f)
    _both([int(p["v"] == 4) for c, p in EW_PLANS if p["mode"] == 1], "ew long rows: vector")
    _both([int(p["v"] == 4) for c, p in EW_PLANS if p["mode"] == 0], "ew patch: vector")
    # the workspace branches of W^T A at k <= 16: slabs that do not fit send the shape on to tn_kernel, whose slabs are larger still, so
    # the entry point refuses; a Gram that does not fit behind the slabs does not ride (the engine's workspace always fits: the query alone
    # can take these sides)
    assert L.dense_plan("wta", 300, 128, 16, ws_bytes=2 * 16 * 128 * 4 - 1)["family"] == "none"
    assert L.dense_plan("wta", 300, 128, 16, ws_bytes=2 * 16 * 128 * 4)["family"] == "tn16"
    assert L.dense_plan("wta_gram", 300, 128, 16, ws_bytes=2 * 16 * 128 * 4)["family"] == "tn16"
    assert L.dense_plan("gram_wtw", 300, 1, 64, ws_bytes=1 << 10)["family"] == "none"
    assert L.dense_plan("ew", 65536, 2000, 1)["family"] == "none"                       # neither a long-row nor a patch shape
    assert L.dense_plan("aht", 300, 96, 200)["family"] == "wide" and L.dense_plan("gram_wtw", 300, 1, 129)["count"] == 4


def _nks(pf, kt, bf16=False, modes=(0, 1)):
    return [p["nk"] for c, p in PLANS if p["family"] == "nt" and p["pf"] == pf and p["kt"] == kt and p["eligible" if pf != 5 else "interior"] > 0
            and bool(c[6]) == bf16 and p["mode"] in modes]


def test_nt_loop_trip_classes():
    for kt in (1, 2, 4):
        nk = set(_nks(10, kt))                                      # nt_mainloop_p2: kt + 2 <= nk body, if (kt < nk) tail
        assert {1, 2, 3} <= nk and [x for x in nk if x >= 4 and x % 2 == 0] and [x for x in nk if x >= 5 and x % 2], (kt, nk)
        assert _nks(10, kt, modes=(0,)) and _nks(10, kt, modes=(1,))
        nk = set(_nks(13, kt))                                      # nt_mainloop_p3t: six tiles per trip, rem = 0..5
        assert {1, 2} <= nk and {x % 6 for x in nk if x >= 6} == set(range(6)), (kt, nk)
        assert _nks(13, kt, modes=(1,))
        nk = set(_nks(5, kt, bf16=True))                            # the bf16 interior loop, 64-wide tiles
        assert {1, 2} <= nk and [x for x in nk if x >= 3 and x % 2], (kt, nk)
    for c, p in PLANS:                                              # a rotated tile order somewhere in every case that has two tiles
        if p["family"] == "nt" and p["pf"] in (5, 10, 13) and p["nk"] > 1:
            assert any(b * 37 % p["nk"] for b in range(p["grid_x"])), c[0]
        if p["family"] == "nt" and p["pf"] == 10:
            assert p["grid_x"] * p["grid_y"] > 256 and p["interior"] < p["grid_x"], c[0]      # one ragged tile beside the interior ones
            assert c[2] * c[3] * 4 < 30e6, c[0]                                                # A stays below 30 MB
    assert {p["mode"] for c, p in PLANS if c[1] == "aht_hblocks"} == {0} and {p["pf"] for c, p in PLANS if c[1] == "aht_hblocks"} == {10, 13}
    assert {p["nk"] % 2 for c, p in PLANS if p["family"] == "nt16"} == {0, 1}              # nt16_kernel: pairs of tiles, an odd one


def test_tn_loop_trip_classes():
    """tn_mainloop: two batches of 8 rows per trip, `if (b < nb)` for an odd count, the predicated loop for the last 1..7 rows -- on
    the last chunk (chunks are multiples of 16 rows, so every other chunk has an even count and no tail)"""
    for fam_ops in (("wta", "wta_gram"), ("gram_wtw",)):
        tn = [p for c, p in PLANS if p["family"] == "tn" and p["fast"] and c[1] in fam_ops]
        full = {p["bl_full"] for p in tn}
        assert {0, 1} <= full and [x for x in full if x >= 3 and x % 2] and [x for x in full if x >= 2 and x % 2 == 0], (fam_ops, full)
        assert [p for p in tn if p["count"] > 1 and p["b0_full"] != p["bl_full"]]
    assert {p["bl_tail"] for c, p in PLANS if p["family"] == "tn" and p["fast"]} >= set(range(8))
    t16 = [p for c, p in PLANS if p["family"].startswith("tn16")]
    assert {0, 1} <= {p["bl_full"] for p in t16} and [p for p in t16 if p["bl_full"] >= 2 and p["bl_full"] % 2 == 0]
    # tn16_body's predicated loop takes 4 rows per step: no tail, whole steps only (12), a last step of 1 and of 3 rows (13, 3)
    assert {p["bl_tail"] for p in t16} >= {0, 1, 3, 12, 13}
    # clamped lanes: n short of the wave's column tile (32 NT) and k short of KP
    assert [c for c, p in PLANS if p["family"] == "tn" and p["fast"] and c[3] % (32 * p["nt"]) and c[1] != "gram_wtw"]
    assert [c for c, p in PLANS if p["family"] == "tn" and p["fast"] and c[4] % 32]
    # two-stage reductions: more than 64 partials in slices of 32, the last slice ragged
    for op in ("wta", "gram_wtw", "gram_hht", "wta_gram"):
        two = [p for c, p in PLANS if c[1] == op and p["reduce"] == "two_stage"]
        assert two and all(p["count"] > 64 and p["slices"] == -(-p["count"] // 32) for p in two), op
        assert [p for p in two if p["count"] % 32], op


def test_update_loop_trip_classes():
    w16 = {p["kt"]: p for c, p in PLANS if p["family"] == "update_w16" and p["aux"] == 2}
    assert set(w16) == {2, 4}                                       # KT = 1 is not capped: one tile per wave
    for kt, p in w16.items():
        per_trip = p["grid_x"] * p["block"] // 64
        assert p["grid_x"] == 1024 and per_trip < p["count"] < 2 * per_trip, (kt, p)          # a second, ragged trip
        assert p["count"] * 16 - per_trip * 16 <= 64                                           # m just above the cap
    assert [p for c, p in PLANS if p["family"] == "update_w16" and p["kt"] == 1 and p["aux"] == 1 and p["grid_x"] > 1024]
    for fam in ("update_w_seq", "update_h_seq"):                    # capped at 1024 workgroups at KT = 4
        assert [p for c, p in PLANS if p["family"] == fam and p["kt"] == 4 and p["aux"] == 2 and p["grid_x"] == 1024], fam
    h2 = [c for c, p in PLANS if p["family"] == "update_h_seq" and p["nt"] == 2]
    assert min(c[3] for c in h2) == 65536 and ("mu_update_h", 131072, 128) in {(c[1], c[3], c[4]) for c in h2}


def test_kl_and_residual_classes():
    """csrc/dnmf_kl.hip: the pipelined U H^T of every KT with a ragged last row tile (both kernels write into one output) and without;
    W^T U with a ragged last chunk; two-stage reductions of both products; resid_lds_kernel of every KT and storage type at m = 4096 plus
    a ragged remainder; colerr_kernel with one and with several row blocks per wave; sqnorm_kernel with a second grid-stride trip"""
    by = lambda fam: [(c, p) for c, p in PLANS if p["family"] == fam]
    for kt in (1, 2, 4):
        _both([p["edge"] for c, p in by("kl_uht_pipe") if p["kt"] == kt and not p["mode"]], "kl_uht_pipe ragged tile, KT %d" % kt)
        _both([p["mode"] for c, p in by("kl_uht_pipe") if p["kt"] == kt], "kl_uht_pipe on padded images, KT %d" % kt)
        _both([p["fast"] for c, p in by("kl_uht") if p["kt"] == kt], "kl_uht_kernel FAST, KT %d" % kt)
        _both([p["fast"] for c, p in by("kl_wtu") if p["kt"] == kt], "kl_wtu_kernel FAST, KT %d" % kt)
        assert [p for c, p in by("kl_wtu") if p["kt"] == kt and p["count"] > 1 and p["bl_tail"] and p["bl_full"] != p["b0_full"]]
        assert {c[6] for c, p in by("resid_lds") if p["kt"] == kt and not p["mode"] and c[2] == 4096 + 36} == {False, True}
        _both([p["fast"] for c, p in by("resid") if p["kt"] == kt], "resid_kernel FAST, KT %d" % kt)
        _both([p["fast"] for c, p in by("colerr") if p["kt"] == kt], "colerr_kernel FAST, KT %d" % kt)
    for op in ("kl_uht_hblocks", "kl_wtu"):
        two = [p for c, p in PLANS if c[1] == op and p["reduce"] == "two_stage"]
        assert two and all(p["count"] > 64 and p["count"] % 32 for p in two), op
    assert {p["reduce"] for c, p in PLANS if c[1] == "kl_uht"} == {"none", "single"}
    assert {p["reduce"] for c, p in PLANS if c[1] == "kl_wtu"} == {"single", "wide", "two_stage"}
    assert {p["per"] for c, p in by("colerr")} == {32, 64}
    assert {(p["fast"], p["aux"]) for c, p in by("sqnorm")} >= {(1, 2), (0, 2), (1, 1)}
    # the 16-wide KL kernels: friendly and padded factors, the direct store and the slabs, whole and ragged row tiles, odd and even tile
    # and block counts, and both sides of "the 16-wide kernel applies" at k <= 16
    u16, w16 = by("kl16_uht"), by("kl16_wtu")
    assert {(p["mode"], p["edge"]) for c, p in u16} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {p["mode"] for c, p in w16} == {0, 1}
    assert {p["aux"] > 0 for c, p in u16} == {False, True} and {p["nk"] % 2 for c, p in u16} == {0, 1} and {p["count"] > 1 for c, p in u16} == {False, True}
    assert {p["bl_full"] % 2 for c, p in w16} == {0, 1} and {p["bl_tail"] > 0 for c, p in w16} == {False, True}
    for op, fam in (("kl_uht", "kl16_uht"), ("kl_wtu", "kl16_wtu")):
        _both([int(p["family"] == fam) for c, p in PLANS if c[1] == op and c[4] <= 16], "%s at k <= 16" % fam)
    assert {p["reduce"] for c, p in u16} == {"none", "single", "two_stage"} and {p["reduce"] for c, p in w16} == {"single", "wide", "two_stage"}
    assert L.dense_plan("kl_uht", 300, 96, 9, ws_bytes=0)["family"] == "kl_uht"          # no room for slabs or images: the 32-wide kernel


# ------------------------------------------------------------------------------------------ what the older exact shapes reach
def _old_cases():
    """the calls tests/test_gpu_exact.py makes on PRIM (test_products, test_mu_updates) and FRO (the two-pass step), as cases"""
    from tests import test_gpu_exact as old
    out = []
    for prm in old.PRIM:
        m, n, k, aligned = prm.values
        if k > 128:
            continue
        for bf16 in (False, True):
            out += [(prm.id, op, m, n, k, aligned, bf16, None) for op in ("aht", "wta", "wta_gram")]
        out += [(prm.id, op, m, n, k, aligned, False, None) for op in ("gram_hht", "gram_wtw", "mu_update_w", "mu_update_h", "aht_update_w")]
        out += [(prm.id, op, m, n, k, aligned, False, None) for op in ("kl_uht", "kl_wtu")]      # test_kl
        if prm in old.SUB:                                           # test_elementwise_and_norms
            out += [(prm.id, op, m, n, k, aligned, b, None) for op in ("resid_sqnorm", "column_err", "sqnorm") for b in (False, True)]
    for prm in old.FRO + old.HB:
        m, n, k, aligned = prm.values
        if k > 128:
            continue
        if prm in old.HB:
            out.append((prm.id, "aht_hblocks", m, n, k, aligned, False, None))
            out.append((prm.id, "kl_uht_hblocks", m, n, k, aligned, False, None))
            continue
        for bf16 in (False, True):
            out += [(prm.id, op, m, n, k, aligned, bf16, None) for op in ("aht_update_w", "wta_gram")]
        out += [(prm.id, op, m, n, k, aligned, False, None) for op in ("gram_hht", "mu_update_h")]
    return out


def _classes(plans):
    """the loop-trip classes of the reach table, as a dict name -> sorted values reached"""
    d = {}

    def add(name, v):
        d.setdefault(name, set()).add(v)
    for c, p in plans:
        f = p["family"]
        if f == "nt" and p["pf"] in (10, 13) and p["eligible"]:
            add("nt PF %d KT %d %s: nk" % (p["pf"], p["kt"], ("store", "fused W")[p["mode"]]), p["nk"])
        if f == "nt" and p["pf"] == 5 and p["interior"]:
            add("nt PF 5 (bf16) KT %d: nk" % p["kt"], p["nk"])
        if f == "tn" and p["fast"]:
            add("tn KT %d: full batches of the last chunk" % p["kt"], p["bl_full"])
            add("tn: tail rows of the last chunk", p["bl_tail"])
        if p["reduce"] != "none":
            add("reduction after %s" % c[1], p["reduce"])
        if f == "kl_uht_pipe":
            add("kl_uht_pipe KT %d: (padded, ragged last tile)" % p["kt"], (p["mode"], p["edge"]))
        if f == "kl16_uht":
            add("kl16_uht: (padded, direct store, splits > 1, ragged last tile)", (p["mode"], p["edge"], int(p["count"] > 1), int(p["aux"] > 0)))
        if f == "kl16_wtu":
            add("kl16_wtu: (padded, 16-row blocks of the last chunk, tail rows)", (p["mode"], p["bl_full"], p["bl_tail"]))
        if f in ("resid_lds", "resid", "colerr"):
            add("%s: (KT, FAST, bf16)" % f, (p["kt"], p["fast"], int(bool(c[6]))))
        if f == "sqnorm":
            add("sqnorm: (FAST, trips)", (p["fast"], p["aux"]))
        if f == "update_w16":
            add("update_w16 KT %d: trips" % p["kt"], p["aux"])
        if f == "update_w_seq":
            add("update_w_seq: (V, EDGE)", (p["v"], p["edge"]))
        if f == "update_h_seq":
            add("update_h_seq KT %d: (NT, EDGE, nontemporal)" % p["kt"], (p["nt"], p["edge"], p["ntemp"]))
    return {k: sorted(v) for k, v in d.items()}


def reach_table():
    """the table of DESIGN.md: loop-trip class | what PRIM / FRO / HB reach | what DENSE_REACH reaches"""
    old = _classes([(c, plan(c, quantum8=False)) for c in _old_cases()])
    new = _classes(PLANS)
    fmt = lambda v: ", ".join(str(x).replace("'", "") for x in v) if v else "--"
    return ["| %s | %s | %s |" % (name, fmt(old.get(name, [])), fmt(new[name])) for name in sorted(new)]


def test_old_shapes_reach_and_design_table():
    old = [(c, plan(c, quantum8=False)) for c in _old_cases()]
    reached = {variant(p, c[6]) for c, p in old}
    every = L.dense_plan_variants()
    pf = VF.index("pf")
    assert not [v for v in reached if v[0] == "nt" and v[pf] == 10], "the older shapes launch nt_mainloop_p2 after all"
    p3 = [(c, p) for c, p in old if p["family"] == "nt" and p["pf"] == 13 and p["eligible"]]
    assert {(c[2], c[3], c[4], p["nk"]) for c, p in p3} == {(2048, 1024, 32, 32)}            # one shape: five whole trips and a tail of 2
    assert not [p for c, p in old if p["family"] == "nt" and p["pf"] == 5 and p["interior"]]
    assert {p["family"] for c, p in old if p["reduce"] == "two_stage"} == {"kl16_wtu"}      # 4100 x 1024, k = 16: 65 chunks of 64 rows
    assert not [p for c, p in old if p["family"] == "update_w16" and p["aux"] > 1]
    assert not [p for c, p in old if p["family"] == "update_h_seq" and p["nt"] == 2]
    assert not [p for c, p in old if p["family"] == "update_w_seq" and p["edge"] == 0]
    assert len(every - reached) > len(every) // 3
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")) as f:
        design = f.read()
    for line in reach_table():
        assert line in design, "DESIGN.md lacks the reach-table line (python -m tests.test_dense_plan prints the table):\n" + line


# ------------------------------------------------------------------------------------------ ranks 128 < k <= 256
# WIDE_REACH (tests/_exact.py: the cases of tests/test_gpu_exact_wide.py).  At a wide rank dnmf_dense_plan answers family = wide and, for
# the ops that launch a plain kernel of csrc/dnmf_wide.hip, that launch; the tuned calls are queried as the entry point issues them
# (ex.wide_panel_plans).
WIDE_PLANS = [(c, ex.wide_case_plans(c)) for c in ex.WIDE_REACH]


@pytest.mark.parametrize("case", ex.WIDE_REACH, ids=lambda c: c[0])
def test_wide_case_plan(case):
    ex.wide_assert_plans(case, *ex.wide_case_plans(case))


def test_wide_ids_are_unique_and_operands_stay_small():
    ids = [c[0] for c in ex.WIDE_REACH]
    assert len(ids) == len(set(ids))
    for cid, op, m, n, k, aligned, bf16, _ in ex.WIDE_REACH:
        assert 128 < k <= 256 and max(m, 1) * max(n, 1) * 4 < 64 << 20 and max(n, 1) * k * 4 < 64 << 20, cid
        # W: below 64 MiB except at the one-range shape, which needs m > 131072 rows of more than 128 columns
        assert max(m, 1) * k * 4 < 64 << 20 or (m, n) == ex.WIDE_TALL, cid


def _second_panels():
    return [(c, pl[-1]) for c, (w, pl) in WIDE_PLANS if pl]


def test_wide_second_panels_cover_the_tuned_kernels():
    """the union of the second-panel plans: nt16, nt at KT 1 / 2 / 4, tn16 and tn at KT 1 / 2 / 4, FAST and not at every KT, for every
    op that issues panels -- and the classes the cases are named after, per op"""
    sp = _second_panels()
    got = {(p["family"], p["kt"]) for c, p in sp}
    assert got == {("nt16", 1), ("nt", 1), ("nt", 2), ("nt", 4), ("tn16", 1), ("tn", 1), ("tn", 2), ("tn", 4)}, sorted(got)
    for fam in ("nt", "tn"):
        for kt in (1, 2, 4):
            _both([p["fast"] for c, p in sp if (p["family"], p["kt"]) == (fam, kt)], "second panel %s FAST, KT %d" % (fam, kt))
    for op in ("aht", "wta", "wta_gram", "gram_hht", "gram_wtw", "kl_uht", "kl_wtu"):
        mine = [(c, p) for c, p in sp if c[1] == op]
        r = {c[4] - 128 for c, p in mine}
        assert {2, 3, 4, 16, 17, 32, 33, 65, 127} <= r, (op, sorted(r))
        assert {c[4] % 4 for c, p in mine} == {0, 1, 2, 3}, op
        assert {c[5] for c, p in mine} == {True, False}, op         # aligned views, and views at an odd base with pitch = width + 3
        small = [(c, p) for c, p in mine if c[4] - 128 <= 16]
        if op != "gram_wtw":                                        # (block (1, 1) of W^T W has n = r columns: never whole 64-column blocks)
            _both([int(p["family"] in ("nt16", "tn16")) for c, p in small], "%s: a 16-wide second panel at r <= 16" % op)
            assert {c[4] for c, p in small if p["family"] in ("nt16", "tn16")} == {132, 144}, op
        assert all(p["kt"] == 1 for c, p in small), op
        # r <= 16 off the 16-wide kernels through an unaligned view, through n % 32 != 0, and at k = 130, 131
        off16 = {(c[4], c[5], c[3] % 32 == 0) for c, p in small if p["family"] in ("nt", "tn")}
        assert {k for k, al, whole in off16} >= {130, 131}, op
        if op not in ("gram_wtw", "kl_wtu"):                         # (kl_wtu: U is aligned whatever the views are)
            assert [1 for k, al, whole in off16 if not al and whole and k % 4 == 0], op
        if op != "gram_wtw":
            assert [1 for k, al, whole in off16 if al and not whole and k % 4 == 0], op
    for op in ("aht", "wta", "wta_gram"):
        b = {p["family"] for c, p in sp if c[1] == op and c[6]}
        assert b == ({"nt16", "nt"} if op == "aht" else {"tn16", "tn"}), (op, b)
    # the r x 128 block of W^T W on the 16-wide kernel, and off it
    g10 = {(c[1], pl[2]["family"]) for c, (w, pl) in WIDE_PLANS if c[1] in ("gram_wtw", "wta_gram")}
    assert g10 == {(op, f) for op in ("gram_wtw", "wta_gram") for f in ("tn16", "tn")}


def test_wide_plain_kernel_classes():
    """wide_nn_rows_kernel: both sides of "more than 4 tiles per range" and of "one range", ragged last ranges and tiles, n < 16, n = 1,
    m % 16 != 0, a last workgroup with one live wave; W_UPD_W at k % 16 != 0 and at k = 256; wide_upd_h_kernel with ragged last row and
    column tiles and a partly filled last workgroup"""
    rows = [(c, w) for c, (w, pl) in WIDE_PLANS if c[1] in ex.WIDE_ROWS_OPS]
    for op in ("kl_uht", "resid_sqnorm", "column_err"):             # (kl_wtu launches the same W_QUOT kernel)
        mine = [(c, w) for c, w in rows if c[1] == op]
        _both([int(w["aux"] > 4) for c, w in mine], "%s: more than 4 tiles per range" % op)
        _both([int(w["grid_y"] == 1) for c, w in mine], "%s: one range" % op)
        big = [(c, w) for c, w in mine if w["aux"] > 4]
        # several ranges of more than 4 tiles, the last range shorter, its last tile ragged
        assert [1 for c, w in big if w["grid_y"] > 1 and 0 < c[3] - (w["grid_y"] - 1) * 16 * w["aux"] < 16 * w["aux"] and c[3] % 16], op
        # the one range of want = 1: more than 8192 strips, n above the 64-column minimum, a ragged last tile, one live wave at the end
        assert [1 for c, w in big if w["grid_y"] == 1 and -(-c[2] // 16) > 8192 and c[3] > 64 and c[3] % 16 and -(-c[2] // 16) % 4 == 1], op
        assert {1, 9} <= {c[3] for c, w in mine}, op
        assert [1 for c, w in mine if c[2] % 16] and [1 for c, w in mine if -(-c[2] // 16) % 4 == 1], op
        assert {c[4] % 4 for c, w in mine} >= {2, 3} or op == "kl_uht", op
    assert {c[4] % 4 for c, w in rows if c[1].startswith("kl")} == {0, 1, 2, 3}
    for c, w in rows:
        m, n = c[2], c[3]
        assert w["grid_x"] == -(-(-(-m // 16)) // 4) and (w["grid_y"] - 1) * 16 * w["aux"] < n <= w["grid_y"] * 16 * w["aux"], c[0]
    upw = [(c, w) for c, (w, pl) in WIDE_PLANS if c[1] == "mu_update_w"]
    assert {c[4] for c, w in upw} >= {130, 131, 255, 256} and all(w["grid_y"] == 1 and w["aux"] == -(-c[4] // 16) for c, w in upw)
    assert {c[5] for c, w in upw} == {True, False} and [1 for c, w in upw if c[2] % 16] and [1 for c, w in upw if -(-c[2] // 16) % 4 == 1]
    uph = [(c, w) for c, (w, pl) in WIDE_PLANS if c[1] == "mu_update_h"]
    assert [1 for c, w in uph if c[4] % 16 and c[3] % 16 and -(-c[3] // 16) % 4] and [1 for c, w in uph if c[4] == 256 and c[3] % 64 == 0]
    assert {1, 9} <= {c[3] for c, w in uph} and {c[5] for c, w in uph} == {True, False} and {c[4] % 4 for c, w in uph} >= {1, 2, 3, 0}
    assert all(w["grid_x"] == -(-(-(-c[3] // 16)) // 4) and w["aux"] == -(-c[4] // 16) for c, w in uph)


def _old_wide_cases():
    """the calls tests/test_gpu_exact.py makes at a wide rank: PRIM (test_products, test_mu_updates, test_kl, SUB: the residual sums) and
    FRO (the two-pass step: gram_hht, aht, mu_update_w, wta_gram, mu_update_h)"""
    from tests import test_gpu_exact as old
    out = []
    for prm in old.PRIM + old.FRO:
        m, n, k, aligned = prm.values
        if k <= 128:
            continue
        ops = ["aht", "wta_gram", "gram_hht", "mu_update_w", "mu_update_h"]
        if prm in old.PRIM:
            ops += ["wta", "gram_wtw", "kl_uht", "kl_wtu"] + (["resid_sqnorm", "column_err"] if prm in old.SUB else [])
        out += [("%s-%s" % (op, prm.id), op, m if op != "gram_hht" else 0, n if op != "gram_wtw" else 0, k, aligned, False, None) for op in ops]
    return out


def _wide_classes(plans):
    d = {}

    def add(name, v):
        d.setdefault(name, set()).add(v)
    for c, (w, pl) in plans:
        op, m, n, k = c[1:5]
        if pl:
            p = pl[-1]
            add("second panel of %s: (family, KT)" % op, (p["family"], p["kt"]))
            add("second panel: r = k - 128", k - 128)
        if op in ("gram_wtw", "wta_gram"):
            add("r x 128 block of W^T W: family", pl[2]["family"])
        add("k % 4", k % 4)
        if op in ex.WIDE_ROWS_OPS:
            add("wide_nn_rows_kernel: (ranges, tiles of a full range)", (w["grid_y"], w["aux"]))
            add("wide_nn_rows_kernel: n", n)
        if op == "mu_update_w":
            add("wide_nn_rows_kernel<W_UPD_W>: (k % 16, m % 16)", (k % 16, m % 16))
        if op == "mu_update_h":
            add("wide_upd_h_kernel: (k % 16, n % 16, waves of the last workgroup)", (k % 16, n % 16, (-(-n // 16) - 1) % 4 + 1))
    return {k: sorted(v) for k, v in d.items()}


def wide_reach_table():
    """the table of DESIGN.md: class | what PRIM / FRO reach at a wide rank | what WIDE_REACH reaches"""
    old = _wide_classes([(c, ex.wide_case_plans(c)) for c in _old_wide_cases()])
    new = _wide_classes(WIDE_PLANS)
    fmt = lambda v: ", ".join(str(x).replace("'", "") for x in v) if v else "--"
    return ["| %s | %s | %s |" % (name, fmt(old.get(name, [])), fmt(new[name])) for name in sorted(new)]


def test_old_wide_shapes_do_not_reach_the_new_classes():
    old = [(c, ex.wide_case_plans(c)) for c in _old_wide_cases()]
    assert {c[4] for c, _ in old} == {129, 192, 256}
    sp = [(c, pl[-1]) for c, (w, pl) in old if pl]
    assert not [c for c, p in sp if p["family"] in ("nt16", "tn16")], "an older shape has a 16-wide second panel after all"
    assert {c[4] - 128 for c, p in sp} == {1, 64, 128} and {c[4] % 4 for c, _ in old} == {0, 1}
    assert {(p["family"], p["kt"]) for c, p in sp if c[4] - 128 <= 16} == {("nt", 1), ("tn", 1)}
    rows = [(c, w) for c, (w, pl) in old if c[1] in ex.WIDE_ROWS_OPS]
    assert rows and all(w["aux"] == 4 and w["grid_y"] > 1 and c[3] >= 16 for c, w in rows), "an older shape has a long or a single range"
    assert all(c[4] % 16 in (0, 1) for c, _ in old if c[1] == "mu_update_w")
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")) as f:
        design = f.read()
    for line in wide_reach_table():
        assert line in design, "DESIGN.md lacks the wide reach-table line (python -m tests.test_dense_plan prints the table):\n" + line


if __name__ == "__main__":
    print("\n".join(reach_table()))
    print()
    print("\n".join(wide_reach_table()))
