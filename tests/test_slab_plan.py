"""The slab fits' C ABI (include/dnmf_slab_api.h, _lib.SLAB_SIGNATURES) without a GPU: header against table and exports, the plan of the
shapes of tests/test_gpu_slab.py, and what the two fit entry points refuse before any HIP call."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# m, n, k of the GPU fits -> KP: element-wise loads below one slab; several slabs and a partial last H panel; KP = 32 and several W panels;
# KP = 64 ragged; KP = 64 full and aligned; the shape the resident plan refuses
GPU_SHAPES = {(50, 39, 3): 16, (130, 290, 16): 16, (290, 70, 17): 32, (150, 140, 33): 64, (200, 136, 64): 64, (1024, 256, 32): 32}


def test_header_table_and_exports_agree():
    from pydnmfk_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dnmf_slab_api.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dnmf_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.SLAB_SIGNATURES) == ["dnmf_pair_slab_fit_batch", "dnmf_pair_slab_plan", "dnmf_pair_slab_weighted_fit_batch"]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, sig in _lib.SLAB_SIGNATURES.items():
        assert hasattr(raw, name) and getattr(_lib.lib, name).argtypes == sig, name
    assert not set(_lib.SLAB_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.RESIDENT_SIGNATURES))


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=str)
def test_plan_of_the_gpu_shapes(shape):
    from pydnmfk_amd._lib import slab_plan
    m, n, k = shape
    p, kp = slab_plan(m, n, k), GPU_SHAPES[shape]
    assert (p["eligible"], p["kp"], p["waves"]) == (1, kp, 4)
    assert p["row_slabs"] == p["h_phase_panels"] == -(-m // 64) and p["col_slabs"] == p["w_phase_panels"] == -(-n // 64)
    # two panels of the wider phase, pitches 4 (mod 8): about 35 KiB at KP = 64, so several workgroups share a CU
    assert p["lds_bytes"] == 8 * max(kp * 68, 64 * (kp + 4)) <= 35 * 1024


def test_shapes_reach_every_path_and_limits_are_named():
    from pydnmfk_amd._lib import resident_plan, slab_plan
    from pydnmfk_amd.engine import HipOps
    plans = [slab_plan(*s) for s in GPU_SHAPES]
    assert {p["kp"] for p in plans} == {16, 32, 64}
    assert any(p["w_phase_panels"] > 2 and n % 64 for p, (m, n, k) in zip(plans, GPU_SHAPES))      # an odd, partial count of H panels
    assert any(p["row_slabs"] == p["col_slabs"] == 1 for p in plans) and any(p["h_phase_panels"] > 2 for p in plans)
    assert not resident_plan(1024, 256, 32)["eligible"] and HipOps.slab_refusal(1024, 256, 32) is None
    for k in (0, 65):
        assert slab_plan(50, 39, k)["eligible"] == 0 and slab_plan(50, 39, k)["kp"] == 0
        assert "1 <= k <= 64" in HipOps.slab_refusal(50, 39, k)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_bad_arguments_are_refused_before_any_hip_call(weighted):
    from pydnmfk_amd._lib import lib
    assert lib.dnmf_pair_slab_plan(0, 8, 3, None) == -1 and b"pair_slab_plan" in lib.dnmf_last_error()
    p = 4096                                                                   # never dereferenced
    fn, who = (lib.dnmf_pair_slab_weighted_fit_batch, b"pair_slab_weighted_fit_batch") if weighted else (lib.dnmf_pair_slab_fit_batch, b"pair_slab_fit_batch")

    def call(mode=0, beta=0.0, A=p, V=p, W=p, k=3, batch=1, w_stride=24):
        v = (V, 64, 8) if weighted else ()
        return fn(mode, beta, A, 64, 8, *v, W, w_stride, 3, p, 24, 8, 8, 8, k, 1e-7, 1, 5, batch, p, None)
    cases = [(dict(W=None), b"null pointer"), (dict(mode=7), b"norm=7" if weighted else b"mode 7"), (dict(mode=3 if weighted else 1, beta=5.0), b"beta=5"),
             (dict(k=0), b"rank k=0"), (dict(k=65), b"1 <= k <= 64"), (dict(batch=0), b"batch=0"), (dict(batch=2, w_stride=8), b"overlap")]
    for change, text in cases + ([(dict(V=None), b"null pointer")] if weighted else []):
        assert call(**change) == -1, change
        assert who in lib.dnmf_last_error() and text in lib.dnmf_last_error(), (change, lib.dnmf_last_error())
