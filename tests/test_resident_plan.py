"""dnmf_pair_resident_plan (include/dnmf_resident_api.h) without a GPU: which shapes one workgroup holds, at which KP, and that the
shapes of tests/test_gpu_resident.py enter the tile loops they are there for."""
import pytest

LDS_MAX = 160 * 1024
# the shapes of the GPU fits: ragged everywhere; more column tiles, then more row tiles, than waves on either side of KP; full tiles at k = 32
GPU_SHAPES = ((50, 39, 3), (33, 290, 16), (290, 33, 17), (64, 64, 32))


def _plan(m, n, k):
    from pydnmfk_amd._lib import resident_plan
    return resident_plan(m, n, k)


@pytest.mark.parametrize("shape, kp", [((50, 39, 3), 16), ((120, 90, 16), 16), ((120, 90, 17), 32), ((1024, 256, 16), 16)] +
                         [(s, 16 if s[2] <= 16 else 32) for s in GPU_SHAPES[1:]], ids=str)
def test_eligible_shapes(shape, kp):
    m, n, k = shape
    p = _plan(m, n, k)
    assert p["eligible"] == 1 and p["kp"] == kp and 0 < p["lds_bytes"] <= LDS_MAX
    assert p["row_tiles"] == -(-m // 16) and p["col_tiles"] == -(-n // 16)
    assert p["row_tiles_per_wave"] == -(-p["row_tiles"] // p["waves"]) and p["col_tiles_per_wave"] == -(-p["col_tiles"] // p["waves"])
    assert p["lds_bytes"] >= 4 * (m * k + k * n)


@pytest.mark.parametrize("shape", [(50, 39, 33), (50, 39, 0), (4096, 4096, 32), (1024, 256, 32), (1 << 40, 8, 1)], ids=str)
def test_ineligible_shapes(shape):
    p = _plan(*shape)
    assert p["eligible"] == 0
    from pydnmfk_amd.engine import HipOps
    why = HipOps.resident_refusal(*shape)
    assert ("k = %d" % shape[2]) in why and ("1 <= k <= 32" in why or str(LDS_MAX) in why)


def test_gpu_shapes_enter_both_tile_loops():
    plans = [_plan(*s) for s in GPU_SHAPES]
    assert any(p["row_tiles_per_wave"] > 1 for p in plans) and any(p["col_tiles_per_wave"] > 1 for p in plans)
    assert {p["kp"] for p in plans} == {16, 32}
    assert any(p["row_tiles"] < p["waves"] for p in plans)          # and idle waves in a phase


def test_bad_arguments_are_refused():
    from pydnmfk_amd._lib import lib
    assert lib.dnmf_pair_resident_plan(0, 8, 3, None) == -1 and b"pair_resident_plan" in lib.dnmf_last_error()
    args = (None, 0, 8, None, 0, 3, None, 0, 8, 8, 8, 3, 1e-7, 1, 5, 1, None, None)
    assert lib.dnmf_pair_resident_fit_batch(0, 0.0, *args) == -1 and b"null pointer" in lib.dnmf_last_error()
    assert lib.dnmf_pair_resident_fit_batch(7, 0.0, *args) == -1 and b"mode" in lib.dnmf_last_error()
    assert lib.dnmf_pair_resident_fit_batch(1, 5.0, *args) == -1 and b"beta" in lib.dnmf_last_error()
