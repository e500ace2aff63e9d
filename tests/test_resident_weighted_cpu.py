"""dnmf_pair_resident_weighted_fit_batch (include/dnmf_resident_api.h) without a GPU: what it refuses before any HIP call, and its
binding."""
import pytest

# norm beta | A a_stride lda | V v_stride ldv | W w_stride ldw | H h_stride ldh | m n k eps w_update itr batch sq_out stream
NULLS = (None, 0, 8, None, 0, 8, None, 0, 3, None, 0, 8, 8, 8, 3, 1e-7, 1, 5, 1, None, None)


@pytest.mark.parametrize("norm, beta, k, text", [(0, 0.0, 3, b"null pointer"), (4, 0.0, 3, b"norm=4"), (3, 5.0, 3, b"beta=5"),
                                                 (0, 0.0, 33, b"1 <= k <= 32")], ids=["null", "norm", "beta", "rank"])
def test_bad_arguments_are_refused(norm, beta, k, text):
    from pydnmfk_amd._lib import lib
    args = NULLS[:14] + (k,) + NULLS[15:]
    assert lib.dnmf_pair_resident_weighted_fit_batch(norm, beta, *args) == -1
    err = lib.dnmf_last_error()
    assert b"pair_resident_weighted_fit_batch" in err and text in err, err


def test_the_resident_table_binds_the_entry_point():
    from pydnmfk_amd import _lib
    sig, plain = (_lib.RESIDENT_SIGNATURES["dnmf_pair_resident" + s + "_fit_batch"] for s in ("_weighted", ""))
    assert len(sig) == len(NULLS) + 2 and sig == plain[:5] + [_lib.c_void_p, _lib.c_long, _lib.c_long] + plain[5:]
    assert _lib.lib.dnmf_pair_resident_weighted_fit_batch.argtypes == sig
