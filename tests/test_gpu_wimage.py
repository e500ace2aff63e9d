"""The MU/Frobenius W phase from a transposed image of A (csrc/dnmf_timg.hip) against the NT kernel it replaces: BIT-EQUAL on
identical inputs (mode 0 = off vs mode 2 = forced), at every shape where the new kernel takes another path -- one tile, a ragged
last block, a rotation that wraps, every rotation value, 256 tiles, clamped ranks, padded W and A, a descriptor window of 32
rows -- and the lifetime rules of the image cache in pydnmfk_amd.engine."""
import ctypes
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)


def _lib():
    from pydnmfk_amd._lib import lib
    return lib


def _plan(m, n, k, lda, a=1, w=1):
    out = (ctypes.c_int * 6)()
    assert _lib().dnmf_wimage_plan(m, n, k, lda, a, w, out) == 0
    return list(out)


def _launches():
    return _plan(128, 32, 64, 32)[5]


@pytest.fixture(autouse=True)
def _restore_mode():
    from pydnmfk_amd import engine
    was = _lib().dnmf_set_wimage(-1)
    yield
    engine.set_wimage(0)                      # drops every image
    _lib().dnmf_set_wimage(was)


def _inputs(m, n, k, seed=3, ldw=None):
    from pydnmfk_amd.engine import HIP_OPS as ops, new_gram
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.rand(m, n, device=dev, generator=g)
    H = torch.rand(k, n, device=dev, generator=g)
    W = torch.rand(m, k, device=dev, generator=g)
    G = ops.gram_hht(H, new_gram(k, dev))
    return A, H, W, G


def _both(fn, expect_image):
    """fn() -> tuple of result tensors, under mode 0 and under mode 2; asserts which path ran"""
    from pydnmfk_amd import engine
    engine.set_wimage(0)
    c0 = _launches()
    ref = fn()
    assert _launches() == c0
    engine.set_wimage(2)
    got = fn()
    assert (_launches() > c0) == expect_image
    return ref, got


def _assert_bits(ref, got):
    for r, g in zip(ref, got):
        assert torch.equal(r.view(torch.int32), g.view(torch.int32))      # every bit, NaN sentinels included


@pytest.mark.parametrize("m,n,k", [(128, 32, 64),        # one block, one k-tile
                                   (132, 64, 64),        # ragged second block
                                   (516, 96, 64),        # five blocks: rotations 0, 1, 2, 0, 1 -- the third wave's wraps at nk = 3
                                   (1024, 224, 64),      # nk = 7: every rotation value
                                   (260, 8192, 64),      # nk = 256
                                   (132096, 96, 64),     # 1032 blocks: beyond 1024 the waves go four to a workgroup
                                   (516, 96, 40), (516, 96, 60), (516, 96, 36)])      # clamped lanes of a short rank
def test_aht_update_w_bit_equal(m, n, k):
    from pydnmfk_amd.engine import HIP_OPS as ops
    A, H, W0, G = _inputs(m, n, k)

    def run():
        W = W0.clone()
        ops.aht_update_w(A, H, G, W, EPS)
        return (W,)
    ref, got = _both(run, True)
    _assert_bits(ref, got)
    assert not torch.equal(ref[0], W0) and torch.isfinite(ref[0]).all()


def test_rank_33_is_refused_and_equal():
    from pydnmfk_amd.engine import HIP_OPS as ops
    A, H, W0, G = _inputs(516, 96, 33)

    def run():
        W = W0.clone()
        ops.aht_update_w(A, H, G, W, EPS)
        return (W,)
    ref, got = _both(run, False)                                           # k % 4 != 0: rows of W are not 16-byte aligned
    _assert_bits(ref, got)


@pytest.mark.parametrize("m,n", [(516, 100), (130, 96)])
def test_refused_shapes_report_a_reason_and_return_nt_bits(m, n):
    from pydnmfk_amd import engine
    from pydnmfk_amd.engine import HIP_OPS as ops
    A, H, W0, G = _inputs(m, n, 64)
    engine.set_wimage(2)
    assert _plan(m, n, 64, n)[:2] == [0, 2]                                # shape

    def run():
        W = W0.clone()
        ops.aht_update_w(A, H, G, W, EPS)
        return (W,)
    ref, got = _both(run, False)
    _assert_bits(ref, got)


def test_padded_w_in_a_poisoned_buffer():
    from pydnmfk_amd.engine import HIP_OPS as ops
    m, n, k, ldw = 516, 96, 64, 72
    A, H, W0, G = _inputs(m, n, k)

    def run():
        buf = torch.full((m, ldw), float("nan"), device="cuda")
        buf[:, :k] = W0
        ops.aht_update_w(A, H, G, buf[:, :k], EPS)
        return (buf,)
    ref, got = _both(run, True)
    _assert_bits(ref, got)
    assert torch.isnan(got[0][:, k:]).all() and torch.isfinite(got[0][:, :k]).all()


def _c_aht_update_w(A, m, n, lda, H, G, W, image):
    """the C entry points directly: build + bind by hand (the engine's cache refuses views)"""
    lib = _lib()
    from pydnmfk_amd._lib import check
    st = torch.cuda.current_stream().cuda_stream
    k = H.shape[0]
    buf = None
    if image:
        ldat = -(-m // 4) * 4
        buf = torch.full((lib.dnmf_wimage_bytes(m, n),), 0xA5, dtype=torch.uint8, device="cuda")
        check(lib.dnmf_wimage_build(A.data_ptr(), m, n, lda, buf.data_ptr(), ldat, st))
        check(lib.dnmf_wimage_bind(A.data_ptr(), m, n, lda, buf.data_ptr(), ldat))
    try:
        check(lib.dnmf_aht_update_w(A.data_ptr(), m, n, lda, H.data_ptr(), k, H.stride(0), G.data_ptr(), W.data_ptr(), W.stride(0), EPS, st))
    finally:
        lib.dnmf_wimage_unbind()
    torch.cuda.synchronize()
    return buf


def test_padded_a_through_the_c_entry_points_and_views_refused_by_the_cache():
    from pydnmfk_amd import engine
    m, n, k = 516, 96, 64
    A, H, W0, G = _inputs(m, n, k)
    Abig = torch.full((m, n + 4), float("nan"), device="cuda")
    Abig[:, :n] = A
    Av = Abig[:, :n]
    engine.set_wimage(2)
    assert engine._wimage_lookup(Av, H, W0, G) is None and not engine._wimage_slots      # a view never gets an image
    assert _plan(m, n, k, n + 4)[:2] == [1, 0]
    c0 = _launches()
    W1 = W0.clone()
    buf = _c_aht_update_w(Av, m, n, n + 4, H, G, W1, True)
    assert _launches() == c0 + 1
    At = buf[: n * m * 4].view(torch.float32).view(n, m)
    assert torch.equal(At, A.t())                                          # the image is A^T, none of the padding
    engine.set_wimage(0)
    W2 = W0.clone()
    _c_aht_update_w(Av, m, n, n + 4, H, G, W2, False)
    _assert_bits((W2,), (W1,))


@pytest.mark.parametrize("m,n", [(516, 96), (1024, 224)])
def test_whole_steps_and_fits(m, n):
    from pydnmfk_amd.engine import HIP_OPS as ops
    k = 64
    A, H0, W0, _ = _inputs(m, n, k)

    def step():
        W, H = W0.clone(), H0.clone()
        ops.mu_fro_step(A, W, H, EPS, True, False)
        ops.mu_fro_step(A, W, H, EPS, True, True)
        return W, H
    ref, got = _both(step, True)
    _assert_bits(ref, got)

    def fit():
        W, H = W0.clone(), H0.clone()
        sq = ops.fit("mu", "fro", A, W, H, EPS, True, 12)                  # the clamp after step 10 included
        return W, H, sq.float()
    from pydnmfk_amd import engine
    engine.set_wimage(0)
    ref = fit()
    engine.set_wimage(2)
    got = fit()
    _assert_bits(ref, got)


def test_descriptor_rebase_at_32_mib_rows():
    """m = 8388736, n = 64: A is 2.1 GB, a row of the image 32 MiB -- a 2 GiB window holds 63 of them, the kernel rebases its
    descriptor every R = 32 rows, and 65537 row blocks put the last waves' rows beyond 2^31 bytes in A, the image and W."""
    m, n, k = 8388736, 64, 64
    from pydnmfk_amd import engine
    from pydnmfk_amd.engine import HIP_OPS as ops, new_gram
    engine.set_wimage(2)
    engine_plan = _plan(m, n, k, n)
    assert engine_plan[0] == 1 and engine_plan[2] < 64 and engine_plan[2] == 32
    g = torch.Generator(device="cuda").manual_seed(11)
    A = torch.rand(m, n, device="cuda", generator=g)
    H = torch.rand(k, n, device="cuda", generator=g)
    G = ops.gram_hht(H, new_gram(k, torch.device("cuda")))
    W0 = torch.rand(m, k, device="cuda", generator=g)
    parts = (slice(0, 1024), slice(m // 2 - 512, m // 2 + 512), slice(m - 1024, m))
    engine.set_wimage(0)
    W = W0.clone()
    ops.aht_update_w(A, H, G, W, EPS)
    ref = tuple(W[p].clone() for p in parts)
    engine.set_wimage(2)
    c0 = _launches()
    W.copy_(W0)
    ops.aht_update_w(A, H, G, W, EPS)
    assert _launches() == c0 + 1
    _assert_bits(ref, tuple(W[p] for p in parts))
    assert not torch.equal(ref[2], W0[parts[2]])


# ---- lifetime of the image (pydnmfk_amd.engine: one slot per device, keyed by the tensor object and its version)
def _step(A, W0, H0):
    from pydnmfk_amd.engine import HIP_OPS as ops
    W, H = W0.clone(), H0.clone()
    ops.mu_fro_step(A, W, H, EPS, True, False)
    return W, H


def test_in_place_change_of_a_drops_the_image():
    from pydnmfk_amd import engine
    A, H0, W0, _ = _inputs(516, 96, 64)
    engine.set_wimage(2)
    stale = _step(A, W0, H0)
    assert engine._wimage_slots and next(iter(engine._wimage_slots.values())).buf is not None
    A[0, 0] += 1
    c0 = _launches()
    got = _step(A, W0, H0)
    assert _launches() == c0 + 1                                           # a NEW image, not the NT kernel
    engine.set_wimage(0)
    ref = _step(A, W0, H0)
    _assert_bits(ref, got)
    assert not torch.equal(stale[0], got[0])                               # the change is visible in W: a stale image would show


def test_perturb_uniform_into_a_drops_the_image():
    from pydnmfk_amd import engine
    from pydnmfk_amd.engine import HIP_OPS as ops
    A, H0, W0, _ = _inputs(516, 96, 64)
    X = torch.rand(516, 96, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    engine.set_wimage(2)
    stale = _step(A, W0, H0)
    version = A._version
    assert ops.perturb_uniform(X, 0.3, 17, out=A) is A and A._version == version       # written behind torch's back
    assert not engine._wimage_slots
    got = _step(A, W0, H0)
    engine.set_wimage(0)
    ref = _step(A, W0, H0)
    _assert_bits(ref, got)
    assert not torch.equal(stale[0], got[0])


def test_del_a_empties_the_slot():
    from pydnmfk_amd import engine
    A, H0, W0, _ = _inputs(516, 96, 64)
    engine.set_wimage(2)
    _step(A, W0, H0)
    assert len(engine._wimage_slots) == 1
    del A
    gc.collect()
    assert not engine._wimage_slots


def test_auto_mode_builds_on_the_second_call_and_never_below_the_threshold(monkeypatch):
    from pydnmfk_amd import engine
    A, H0, W0, _ = _inputs(516, 96, 64)
    engine.set_wimage(1)
    c0 = _launches()
    for _ in range(3):
        _step(A, W0, H0)
    assert not engine._wimage_slots and _launches() == c0                  # 516 x 96 is no shape the auto rule takes
    # the second-call rule itself, at this size: forced mode decides the plan, the engine is told it is in auto mode
    engine.set_wimage(2)
    monkeypatch.setattr(engine, "_wimage_mode", lambda: 1)
    _step(A, W0, H0)
    slot = engine._wimage_slots[torch.cuda.current_device()]
    assert slot.buf is None and _launches() == c0                          # first sight: a candidate, no image
    _step(A[:256], W0[:256], H0)                                           # a row view in between neither builds nor resets
    assert engine._wimage_slots[torch.cuda.current_device()] is slot and slot.buf is None
    got = _step(A, W0, H0)
    assert slot.buf is not None and _launches() == c0 + 1                  # second consecutive call: built and used
    monkeypatch.undo()
    engine.set_wimage(0)
    _assert_bits(_step(A, W0, H0), got)


def test_no_memory_reserve_means_no_image(monkeypatch):
    from pydnmfk_amd import engine
    A, H0, W0, _ = _inputs(516, 96, 64)
    engine.set_wimage(2)
    monkeypatch.setattr(engine, "WIMAGE_RESERVE", 1 << 60)
    c0 = _launches()
    got = _step(A, W0, H0)
    slot = engine._wimage_slots[torch.cuda.current_device()]
    assert slot.buf is None and slot.refused and _launches() == c0
    engine.set_wimage(0)
    _assert_bits(_step(A, W0, H0), got)
