"""The transposed image of A (csrc/dnmf_timg.hip) without a GPU: the plan's conditions and descriptor windows, the mode switch
and the environment variable.  The plan query is answered by the function the launch decides with."""
import ctypes

import pytest

from pydnmfk_amd._lib import lib

TAKEN, OFF, SHAPE, A_ALIGN, W_ALIGN, RANK, SMALL, WINDOW = range(8)


def plan(m, n, k, lda=None, a=1, w=1):
    out = (ctypes.c_int * 6)()
    assert lib.dnmf_wimage_plan(m, n, k, n if lda is None else lda, a, w, out) == 0
    return list(out)


@pytest.fixture
def forced():
    was = lib.dnmf_set_wimage(2)
    yield
    lib.dnmf_set_wimage(was)


def window_rows(m):
    """largest power of two 8 <= R <= 2^20 with (R + 8) * ldat * 4 < 2^31"""
    ldat = -(-m // 4) * 4
    r = 8
    while r < 2**20 and (2 * r + 8) * ldat * 4 < 2**31 - 1:
        r *= 2
    return r


@pytest.mark.parametrize("m,n", [(128, 32), (132, 64), (516, 96), (1024, 224), (260, 8192), (262144, 8192), (8388736, 64)])
def test_taken_shapes_grid_and_window(forced, m, n):
    taken, reason, R, grid, kt, _ = plan(m, n, 64)
    assert (taken, reason, kt) == (1, TAKEN, 2)
    waves = -(-m // 128)                                    # one wave per 128-row block; four to a workgroup beyond 1024 waves
    assert grid == (-(-waves // 4) if waves > 1024 else waves)
    assert R == window_rows(m) and R >= 8 and R & (R - 1) == 0
    assert (R + 8) * (-(-m // 4) * 4) * 4 < 2**31


def test_window_at_the_headline_and_at_long_rows(forced):
    assert plan(262144, 8192, 64)[2] == 1024                # a row of the image is 1 MiB: 2047 rows per 2 GiB window
    assert plan(8388736, 64, 64)[2] == 32                   # 32 MiB rows: the window holds 63 of them
    assert plan(8388736, 64, 64)[2] < 64
    assert plan(2**25, 32, 64)[:2] == [0, WINDOW]           # 128 MiB rows: not even 16 fit


@pytest.mark.parametrize("k,reason", [(64, TAKEN), (60, TAKEN), (40, TAKEN), (36, TAKEN), (33, W_ALIGN), (62, W_ALIGN), (32, RANK), (16, RANK),
                                      (65, RANK), (128, RANK)])
def test_ranks(forced, k, reason):
    p = plan(516, 96, k)
    assert p[1] == reason and p[0] == (reason == TAKEN)


def test_refusals(forced):
    assert plan(516, 100, 64)[:2] == [0, SHAPE]             # n % 32
    assert plan(130, 96, 64)[:2] == [0, SHAPE]              # m % 4
    assert plan(516, 96, 64, lda=98)[:2] == [0, A_ALIGN]
    assert plan(516, 96, 64, lda=100)[:2] == [1, TAKEN]     # a padded A is fine
    assert plan(516, 96, 64, a=0)[:2] == [0, A_ALIGN]
    assert plan(516, 96, 64, w=0)[:2] == [0, W_ALIGN]


def test_mode_switch_and_threshold():
    was = lib.dnmf_set_wimage(1)
    try:
        assert lib.dnmf_set_wimage(-1) == 1                 # out-of-range values only query
        assert lib.dnmf_set_wimage(7) == 1 and lib.dnmf_set_wimage(-1) == 1
        # auto = where the sweep of profiles/r07_wimage_sweep.md measured a gain: whole half-rounds of 1024 blocks of 128 rows
        # (m a multiple of 131072) and at least 2^27 elements
        for m, n in ((262144, 8192), (131072, 1024), (131072, 16384), (393216, 4096), (2097152, 512)):
            assert plan(m, n, 64)[:2] == [1, TAKEN], (m, n)
        for m, n in ((131072, 992), (196608, 8192), (262272, 8192), (98304, 8192), (65536, 32768), (32768, 8192), (516, 96)):
            assert plan(m, n, 64)[:2] == [0, SMALL], (m, n)
        assert plan(516, 100, 64)[:2] == [0, SHAPE]         # a shape refusal is reported before the size
        assert lib.dnmf_set_wimage(0) == 1
        assert plan(262144, 8192, 64)[:2] == [0, OFF]
        assert lib.dnmf_set_wimage(2) == 0
        assert plan(516, 96, 64)[:2] == [1, TAKEN]
    finally:
        lib.dnmf_set_wimage(was)


def test_image_bytes():
    # the image (n rows of m rounded up to 4 floats, 256-byte aligned) + H^T as n x 64 floats
    assert lib.dnmf_wimage_bytes(516, 96) == (96 * 516 * 4 + 255) // 256 * 256 + 96 * 64 * 4
    assert lib.dnmf_wimage_bytes(130, 32) == (32 * 132 * 4 + 255) // 256 * 256 + 32 * 64 * 4
    assert lib.dnmf_wimage_bytes(262144, 8192) == 262144 * 8192 * 4 + 8192 * 64 * 4
    assert lib.dnmf_wimage_bytes(0, 8) == 0


def test_build_and_bind_validate_without_touching_memory():
    assert lib.dnmf_wimage_build(None, 8, 8, 8, None, 8, None) == -1
    assert lib.dnmf_wimage_build(16, 130, 32, 32, 32, 132, None) == -1 and b"multiples of 4" in lib.dnmf_last_error()
    assert lib.dnmf_wimage_bind(16, 132, 32, 32, 32, 136) == -1           # ldat must be m rounded up to 4
    lib.dnmf_wimage_unbind()


def test_environment_variable():
    from pydnmfk_amd.engine import wimage_mode_from_env
    assert wimage_mode_from_env({}) is None
    assert [wimage_mode_from_env({"DNMF_WIMAGE": v}) for v in ("0", "1", "2", " 2 ")] == [0, 1, 2, 2]
    assert wimage_mode_from_env({"DNMF_WIMAGE": "3"}) is None and wimage_mode_from_env({"DNMF_WIMAGE": "on"}) is None
