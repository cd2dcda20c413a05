"""CPU: argument validation of the f32-faithful entry points (rr_faithful_build, rr_flat_search_faithful, rr_flat_search_f32_exact
and their workspace queries) and of the Python constructor, without a device: no compute call is made here."""
import pytest


def _seg(n=10):
    from ragroute_amd import _lib
    return (_lib.SegmentStruct * 1)(_lib.SegmentStruct(0, n, 0, -1, 0))


def _faithful(L, dtype=0, xb=None, n=10, d=768, dim=768, nq=1, k=5, list_len=32, segs=None, n_segs=1, exact=None):
    return L.rr_flat_search_faithful(xb, dtype, None, d, None, n, d, dim, _seg(n) if segs is None else segs, n_segs, None, None, nq, k,
                                     list_len, None, None, exact, None, None, 0, None, 0, None)


def test_faithful_argument_validation_without_gpu():
    from ragroute_amd import _lib
    L = _lib.lib()
    assert L.rr_version() >= 600
    assert _faithful(L, k=0) == -1 and b"list_len" in L.rr_last_error()             # k = 0
    assert _faithful(L, k=33, list_len=32) == -1                                      # list_len < k
    assert _faithful(L, k=5, list_len=2000) == -1                                     # list_len > 1024
    assert _faithful(L, dtype=7) == -1 and b"dtype" in L.rr_last_error()
    assert _faithful(L, dtype=2) == -1                                                # the int8 screening type is internal
    assert _faithful(L, d=700, dim=700) == -2                                         # unpadded dim
    assert _faithful(L, d=800, dim=768) == -1                                         # d > dim
    assert _faithful(L, n_segs=0) == -1                                               # no segment
    assert _faithful(L, nq=0) == 0                                                    # nq = 0 is a no-op
    assert _faithful(L, nq=-1) == -1
    assert _faithful(L) == -1 and b"null pointer" in L.rr_last_error()                # no query / output / workspace pointers
    S = _lib.SegmentStruct
    assert _faithful(L, segs=(S * 1)(S(0, 11, 0, -1, 0))) == -1 and b"inside the matrix" in L.rr_last_error()
    assert _faithful(L, n=1 << 33) == -1                                              # row ids are 32-bit matrix rows


def test_exact_scan_argument_validation_without_gpu():
    from ragroute_amd import _lib
    L = _lib.lib()

    def scan(k=5, d=768, ld=768, nq=4, n_idx=4, qidx=None, n=10):
        return L.rr_flat_search_f32_exact(None, ld, n, d, _seg(n), 1, None, nq, qidx, n_idx, k, None, None, None, 0, None, 0, None)
    assert scan(k=0) == -1 and scan(k=1025) == -1
    assert scan(d=9000, ld=9000) == -1                  # d > 8192
    assert scan(ld=700) == -1                           # row stride below d
    assert scan(n_idx=5, nq=4) == -1                    # no index list: n_idx <= nq
    assert scan(n_idx=0) == 0                           # nothing to scan is a no-op
    assert scan() == -1 and b"null pointer" in L.rr_last_error()


def test_faithful_build_and_workspace_queries_without_gpu():
    from ragroute_amd import _lib
    L = _lib.lib()
    assert L.rr_faithful_build(None, 768, None, 7, 10, 768, 768, None, None) == -1     # dtype (and no stats)
    assert L.rr_faithful_build(None, 768, None, 0, 10, 768, 700, None, None) == -1     # unpadded dim
    assert L.rr_faithful_build(None, 100, None, 0, 10, 768, 768, None, None) == -1     # ld_f32 < d
    assert L.rr_faithful_build(None, 768, None, 0, 10, 768, 768, None, None) == -1     # null pointers
    for args in ((0, 32, 1, 768), (33, 32, 1, 768), (5, 1025, 1, 768), (5, 32, -1, 768), (5, 32, 1, 700)):
        assert L.rr_flat_search_faithful_workspace_bytes(*args) == 0, args
    for args in ((0, 768), (1025, 768), (5, 0), (5, 8193)):
        assert L.rr_flat_search_f32_exact_workspace_bytes(*args) == 0, args


def test_python_constructor_rejects_unsupported_combinations():
    """exact_f32 with the L2 metric fails before any device is touched; build_screen() on an exact_f32 index fails too."""
    from ragroute_amd import _lib
    from ragroute_amd.flat_index import FlatIndex
    with pytest.raises(ValueError, match="exact_f32"):
        FlatIndex(768, metric="l2", exact_f32=True)
    idx = FlatIndex.__new__(FlatIndex)   # the attributes build_screen() reads, without a device
    idx.metric, idx.exact_f32, idx.dim = "ip", True, 768
    with pytest.raises(_lib.RagrouteHipError, match="exact_f32"):
        idx.build_screen()
