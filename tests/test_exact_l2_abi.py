"""CPU: the f32-faithful squared-L2 entry points (rr_flat_search_faithful_l2, its workspace query, rr_flat_search_f32_exact_l2) are
exported, declared and bound, validate their arguments as their inner-product siblings do, and the Python constructors accept
exact_l2 with the l2 metric only — without a device: no compute call is made here."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rr_flat_search_faithful_l2_workspace_bytes", "rr_flat_search_faithful_l2", "rr_flat_search_f32_exact_l2")


def _seg(n=10):
    from ragroute_amd import _lib
    return (_lib.SegmentStruct * 1)(_lib.SegmentStruct(0, n, 0, -1, 0))


def _faithful(L, dtype=0, xb=None, hn=None, n=10, d=768, dim=768, nq=1, k=5, list_len=32, segs=None, n_segs=1, ptr=None):
    """ptr: one address for every pointer the call would read or write had it passed validation (it never does here)."""
    return L.rr_flat_search_faithful_l2(xb or ptr, hn, dtype, ptr, d, ptr, n, d, dim, _seg(n) if segs is None else segs, n_segs, ptr, ptr, nq, k,
                                        list_len, ptr, ptr, ptr, None, ptr, 0, None, 0, None)


def test_symbols_are_exported_declared_and_bound():
    from ragroute_amd import _lib
    L = _lib.lib()
    assert L.rr_version() >= 800
    header = open(os.path.join(ROOT, "include", "ragroute_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in _lib.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/ragroute_hip.h"
        assert getattr(L, name).argtypes, f"{name} has no argtypes"
    assert len(L.rr_flat_search_faithful_l2.argtypes) == len(L.rr_flat_search_faithful.argtypes) + 1       # + d_half_sqnorm
    assert len(L.rr_flat_search_f32_exact_l2.argtypes) == len(L.rr_flat_search_f32_exact.argtypes)


def test_faithful_l2_argument_validation_without_gpu():
    from ragroute_amd import _lib
    L = _lib.lib()
    assert _faithful(L, k=0) == -1 and b"list_len" in L.rr_last_error()             # k = 0
    assert L.rr_last_error().startswith(b"rr_flat_search_faithful_l2:")               # the function's own name
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
    # every other pointer given, rows to scan, no norms: refused before anything is read
    assert _faithful(L, ptr=4096) == -1 and b"null half_sqnorm" in L.rr_last_error()


def test_exact_scan_l2_argument_validation_without_gpu():
    from ragroute_amd import _lib
    L = _lib.lib()

    def scan(k=5, d=768, ld=768, nq=4, n_idx=4, qidx=None, n=10):
        return L.rr_flat_search_f32_exact_l2(None, ld, n, d, _seg(n), 1, None, nq, qidx, n_idx, k, None, None, None, 0, None, 0, None)
    assert scan(k=0) == -1 and scan(k=1025) == -1
    assert L.rr_last_error().startswith(b"rr_flat_search_f32_exact_l2:")
    assert scan(d=9000, ld=9000) == -1                  # d > 8192
    assert scan(ld=700) == -1                           # row stride below d
    assert scan(n_idx=5, nq=4) == -1                    # no index list: n_idx <= nq
    assert scan(n_idx=0) == 0                           # nothing to scan is a no-op
    assert scan() == -1 and b"null pointer" in L.rr_last_error()


def test_workspace_query_without_gpu():
    from ragroute_amd import _lib
    L = _lib.lib()
    for args in ((0, 32, 1, 768), (33, 32, 1, 768), (5, 1025, 1, 768), (5, 32, -1, 768), (5, 32, 1, 700)):
        assert L.rr_flat_search_faithful_l2_workspace_bytes(*args) == 0, args


@pytest.mark.parametrize("metric", ["ip", "cosine"])
def test_python_constructors_reject_exact_l2_with_other_metrics(metric):
    """exact_l2 with a metric other than l2 fails before any device is touched, for both classes."""
    from ragroute_amd.flat_index import FlatIndex, SegmentedIndex
    with pytest.raises(ValueError, match="exact_l2"):
        FlatIndex(768, metric=metric, exact_l2=True)
    with pytest.raises(ValueError, match="exact_l2"):
        SegmentedIndex(768, [10, 20], metric=metric, exact_l2=True)
