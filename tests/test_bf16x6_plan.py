"""Which kernels a shape takes on the bf16x6 entry points (csrc/dnmf_split.hip), without a GPU: dnmf_bf16x6_plan is answered by the
functions the entry points decide with.  Every shape of tests/test_gpu_exact_split.py must report the kernel and the loop trip counts it
is named after -- and no shape of the older exact tests is a split shape: `test_bf16x6_products` and `test_mu_fro_step_two_pass` of
tests/test_gpu_exact.py run on n = 130, 2052, ..., 333, none a multiple of 128, i.e. on the forwarding to the fp32 kernels."""
import ctypes

import pytest

from pydnmfk_amd._lib import lib
from tests import _exact as ex

FRO, KL, KT, NSET, TNX_CHUNKS, TNX_ROWS, WTUX_CHUNKS, WTUX_BLOCKS, UHTX_SPLITS, UHTX_COLS, NTX_STREAMED, TNX_STREAMED = range(12)


def plan(m, n, k, lda=0, bf16=False, aligned=True):
    out = (ctypes.c_long * 12)()
    assert lib.dnmf_bf16x6_plan(m, n, k, lda or n, int(bf16), int(aligned), out) == 0
    return list(out)


def default_lda(n, bf16):
    return n + (8 if bf16 else 4)                             # the pitch of an aligned ex.Poisoned view


@pytest.mark.parametrize("case", ex.X6_F32 + ex.X6_BF16, ids=lambda c: c[0])
def test_frobenius_shapes_report_the_plan_they_are_named_after(case):
    name, m, n, k, lda, _, (kt, nset, chunks, rows) = case
    bf16 = case in ex.X6_BF16
    p = plan(m, n, k, lda or default_lda(n, bf16), bf16)
    assert p[FRO] == 1 and p[KL] == (0 if bf16 else 1)
    assert (p[KT], p[NSET], p[TNX_CHUNKS], p[TNX_ROWS]) == (kt, nset, chunks, rows)
    assert (p[NTX_STREAMED], p[TNX_STREAMED]) == (0, 0)
    # what the names say, from the sizes alone
    assert rows % 64 == 0 and (chunks - 1) * rows < m <= chunks * rows
    assert kt == (1 if k <= 32 else 2 if k <= 64 else 4) and nset == (4 if kt == 2 and not bf16 else 2)
    assert (n // (64 if bf16 else 32)) % nset == 0            # whole trips of the pipelined loop
    if "edge-only" in name:
        assert m < 128
    if "interior-only" in name:
        assert m % 128 == 0
    if "both" in name:
        assert m > 128 and m % 128
    if "ragged-chunk" in name:
        assert m % rows
    if "rotation" in name:
        nk = n // (64 if bf16 else 32)
        assert len({(b * 37) % nk for b in range(-(-m // 128))}) == -(-m // 128) > 1


@pytest.mark.parametrize("case", ex.X6_KL, ids=lambda c: c[0])
def test_kl_shapes_report_the_plan_they_are_named_after(case):
    name, m, n, k, lda, _, (kt, chunks, blocks, splits, cols) = case
    p = plan(m, n, k, lda or default_lda(n, False))
    assert p[KL] == 1 and p[FRO] == (1 if k >= 33 else 0)
    assert (p[KT], p[WTUX_CHUNKS], p[WTUX_BLOCKS], p[UHTX_SPLITS], p[UHTX_COLS]) == (kt, chunks, blocks, splits, cols)
    assert (chunks - 1) * blocks < -(-m // 32) <= chunks * blocks
    assert cols % 64 == 0 and (splits - 1) * cols < n <= splits * cols
    if "one-live-wave" in name:
        assert chunks % 4 == 1                                # the last workgroup of four waves has one chunk
    if "three-splits" in name:
        assert [min(cols, n - s * cols) for s in range(splits)] == [320, 320, 256]


@pytest.mark.parametrize("case", ex.X6_STREAMED, ids=lambda c: c[0])
def test_streamed_shapes_are_the_smallest_past_the_threshold(case):
    _, m, n, k, bf16, (kt, nset, chunks, rows) = case
    p = plan(m, n, k, n, bf16)
    assert p[FRO] == 1 and (p[KT], p[NSET], p[TNX_CHUNKS], p[TNX_ROWS], p[NTX_STREAMED], p[TNX_STREAMED]) == (kt, nset, chunks, rows, 1, 1)
    assert m * n * (2 if bf16 else 4) == 256 << 20
    q = plan(m - 128, n, k, n, bf16)
    assert q[FRO] == 1 and (q[NTX_STREAMED], q[TNX_STREAMED]) == (0, 0)


@pytest.mark.parametrize("case", ex.X6_FALLBACK, ids=lambda c: c[0])
def test_ranks_below_the_kernels_take_the_fp32_route(case):
    _, m, n, k, bf16 = case
    assert plan(m, n, k, default_lda(n, bf16), bf16)[FRO] == 0
    assert plan(m, n, k + 1, default_lda(n, bf16), bf16)[FRO] == 1


def test_refusals():
    assert plan(129, 256, 40)[:3] == [1, 1, 2]
    assert plan(129, 256, 40, aligned=False) == [0] * 12
    assert plan(129, 256, 40, lda=258) == [0] * 12                              # rows of A not 16 bytes apart
    assert plan(129, 256, 40, lda=260)[:2] == [1, 1]
    assert plan(129, 256, 40, lda=260, bf16=True) == [0] * 12                   # 260 bf16 elements are 520 bytes
    assert plan(129, 256, 40, lda=264, bf16=True)[:2] == [1, 0]
    assert plan(129, 256, 40, lda=1024)[:2] == [1, 1] and plan(129, 256, 40, lda=1028) == [0] * 12      # lda <= 4 n
    assert plan(129, 260, 40) == [0] * 12 and plan(129, 192, 40) == [0] * 12    # n % 128
    assert plan(129, 256, 129) == [0] * 12 and plan(129, 256, 128)[:3] == [1, 1, 4]
    assert plan(129, 256, 32)[:3] == [0, 1, 1] and plan(129, 256, 1)[:3] == [0, 1, 1]


def test_the_older_exact_shapes_never_reach_a_split_kernel():
    from tests import test_gpu_exact as tg
    shapes = [p.values for p in tg.SUB + tg.FRO]
    assert len(shapes) == 13
    for m, n, k, aligned in shapes:
        assert n % 128 != 0
        for bf16 in (False, True):
            ld = ex_pitch(n, aligned, bf16)
            assert plan(m, n, k, ld, bf16, aligned) == [0] * 12, (m, n, k)


def ex_pitch(n, aligned, bf16):
    return -(-n // 4) * 4 + 4 if aligned else n + 3
