"""CPU: the segmented squared-L2 entry point (rr_flat_search_segments_l2) is exported, declared, and validates its arguments
without a device with the statuses and messages of rr_flat_search_segments (both go through one segment-table check); the
Python constructor rejects what the metric does not serve.  No compute call is made here."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _S():
    from ragroute_amd import _lib
    return _lib.SegmentStruct


def _one(n=10):
    S = _S()
    return (S * 1)(S(0, n, 0, -1, 0))


def _call(L, xb=None, hn=None, dtype=0, n=10, dim=768, segs=None, n_segs=1, nq=1, k=5, mask=None, stride=0):
    return L.rr_flat_search_segments_l2(xb, hn, dtype, n, dim, _one(n) if segs is None else segs, n_segs, None, nq, k, None, None, None, 0,
                                        mask, stride, None)


def _ip(L, dtype=0, n=10, dim=768, segs=None, n_segs=1, nq=1, k=5, mask=None, stride=0):
    return L.rr_flat_search_segments(None, dtype, n, dim, _one(n) if segs is None else segs, n_segs, None, nq, k, None, None, None, 0,
                                     mask, stride, None)


def test_the_entry_point_is_exported_and_declared():
    from ragroute_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "rr_flat_search_segments_l2") and "rr_flat_search_segments_l2" in _lib.EXPORTS
    assert L.rr_version() >= 700
    header = open(os.path.join(ROOT, "include", "ragroute_hip.h")).read()
    decl = re.search(r"int rr_flat_search_segments_l2\(([^;]*)\);", header)
    assert decl, "rr_flat_search_segments_l2 is not declared in include/ragroute_hip.h"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert len(args) == len(L.rr_flat_search_segments_l2.argtypes) == 17
    assert args[1] == "const float* d_half_sqnorm" and args[5] == "const rr_segment* segs"
    # the call sites the function replaces are cited next to it
    for site in ("data_source.py:203", "rerank.py:28-34", "http_server.py:280-293"):
        assert site in header[header.index("int rr_flat_search_segments_l2(") - 3000: header.index("int rr_flat_search_segments_l2(")], site


def test_argument_validation_without_gpu():
    from ragroute_amd import _lib
    L, S = _lib.lib(), _S()
    assert _call(L, k=0) == -1 and b"k must be" in L.rr_last_error()
    assert _call(L, k=1025) == -1
    assert _call(L, dtype=7) == -1 and b"dtype" in L.rr_last_error()
    assert _call(L, dtype=2) == -1                                                    # the int8 screening type is internal
    assert _call(L, dim=700) == -2 and _call(L, dim=1000) == -2                       # unpadded dim
    assert _call(L, n_segs=0) == -1 and b"1 .. 32 segments" in L.rr_last_error()
    many = (S * 33)(*[S(256 * i, 10, i << 40, i, 0) for i in range(33)])
    assert _call(L, n=256 * 33, segs=many, n_segs=33) == -1 and b"1 .. 32 segments" in L.rr_last_error()
    assert _call(L, segs=(S * 1)(S(0, 11, 0, -1, 0))) == -1 and b"inside the matrix" in L.rr_last_error()
    overlap = (S * 2)(S(0, 300, 0, 0, 0), S(256, 10, 1 << 40, 1, 0))
    assert _call(L, n=1000, segs=overlap, n_segs=2) == -1 and b"non-overlapping" in L.rr_last_error()
    unaligned = (S * 2)(S(0, 100, 0, 0, 0), S(300, 10, 1 << 40, 1, 0))
    assert _call(L, n=1000, segs=unaligned, n_segs=2) == -1 and b"multiples of 256" in L.rr_last_error()
    assert _call(L, segs=(S * 1)(S(0, 10, 0, -2, 0))) == -1 and b"mask_col" in L.rr_last_error()
    assert _call(L, n=1 << 33) == -1                                                  # row ids are 32-bit matrix rows
    assert _call(L, nq=0) == 0                                                        # nq = 0 is a no-op
    assert _call(L, nq=-1) == -1
    assert _call(L) == -1 and b"half_sqnorm" in L.rr_last_error()                     # rows present, no norms
    assert _call(L, hn=1 << 20) == -1 and b"null pointer" in L.rr_last_error()        # norms given: queries / outputs / workspace missing
    assert _call(L, n=0, segs=_one(0)) == -1 and b"null pointer" in L.rr_last_error()  # an empty federation needs no norms, but its outputs


def test_messages_and_statuses_mirror_the_inner_product_entry_point():
    """Both entry points validate through the same segment-table check: same status, same text apart from the function's name."""
    from ragroute_amd import _lib
    L, S = _lib.lib(), _S()
    cases = [dict(n_segs=0), dict(segs=(S * 1)(S(0, 11, 0, -1, 0))), dict(n=1000, segs=(S * 2)(S(0, 300, 0, 0, 0), S(256, 10, 0, 1, 0)), n_segs=2),
             dict(segs=(S * 1)(S(0, 10, 0, -2, 0))), dict(n=-1), dict(k=0), dict(dim=700), dict(dtype=9),
             dict(segs=(S * 1)(S(0, 10, 0, 3, 0)), mask=1 << 20, stride=2)]
    for kw in cases:
        a = _ip(L, **kw)
        msg_a = L.rr_last_error().decode()
        b = _call(L, hn=1 << 20, **kw)
        msg_b = L.rr_last_error().decode()
        assert a == b and a < 0, kw
        assert msg_a.replace("rr_flat_search_segments", "X") == msg_b.replace("rr_flat_search_segments_l2", "X"), (msg_a, msg_b)


def test_python_constructor_rejects_exact_f32_with_l2():
    from ragroute_amd.flat_index import SegmentedIndex
    with pytest.raises(ValueError, match="exact_f32"):
        SegmentedIndex(768, [10, 20], metric="l2", exact_f32=True)
    with pytest.raises(ValueError, match="metric"):
        SegmentedIndex(768, [10, 20], metric="hamming")


def test_the_header_no_longer_says_segments_are_inner_product_only():
    header = open(os.path.join(ROOT, "include", "ragroute_hip.h")).read()
    doc = header[header.index("ONE search over several data sources"): header.index("typedef struct rr_segment")]
    assert "Inner product / cosine only" not in doc and "rr_flat_search_segments_l2" in doc
