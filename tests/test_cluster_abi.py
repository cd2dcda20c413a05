"""CPU: the clustering entry points of the C ABI (rr_cluster_assign, rr_cluster_means, rr_cluster_workspace_bytes) are declared,
exported and bound, and every validation rule returns its status and a message before any device call (the pointers here are not
device pointers; no GPU is needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rr_cluster_assign", "rr_cluster_means", "rr_cluster_workspace_bytes")
BIG = (1 << 32) - 31          # one more than 2^32 - 32
P = 16                        # a non-null, 16-byte aligned stand-in for a device pointer that must never be dereferenced


def test_new_symbols_are_declared_exported_and_bound():
    from ragroute_amd import _lib
    L = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ragroute_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None, f"{name} has no argtypes"
    assert re.search(r"RR_MAX_CLUSTERS\s*=\s*64", header) and _lib.RR_MAX_CLUSTERS == 64
    assert L.rr_version() >= 900


def test_workspace_query_returns_zero_for_bad_sizes():
    from ragroute_amd import _lib
    L = _lib.lib()
    assert L.rr_cluster_workspace_bytes(1000, 768, 10) > 0
    assert L.rr_cluster_workspace_bytes(0, 128, 1) > 0
    assert L.rr_cluster_workspace_bytes((1 << 32) - 32, 8192, 64) > 0
    for n, dim, C in ((-1, 768, 10), (BIG, 768, 10), (1000, 700, 10), (1000, 0, 10), (1000, 8320, 10), (1000, 768, 0), (1000, 768, 65)):
        assert L.rr_cluster_workspace_bytes(n, dim, C) == 0, (n, dim, C)
    # grows with neither the row count beyond its cap nor without bound: at most ~128 MiB of partials (+ counts) for the widest case
    assert L.rr_cluster_workspace_bytes(1 << 31, 8192, 64) <= (160 << 20)


def test_assign_validation_without_gpu():
    from ragroute_amd import _lib
    L = _lib.lib()

    def call(xb=P, dtype=0, n=10, dim=768, cent=P, bias=None, C=10, assign=P, score=None):
        return L.rr_cluster_assign(xb, dtype, n, dim, cent, bias, C, assign, score, None)
    for kw, status, word in (({"n": -1}, -1, b"negative"), ({"C": 0}, -1, b"n_clusters"), ({"C": 65}, -1, b"n_clusters"),
                             ({"dtype": 2}, -1, b"dtype"), ({"dtype": -1}, -1, b"dtype"), ({"cent": None}, -1, b"null"),
                             ({"xb": None}, -1, b"null"), ({"assign": None}, -1, b"null"),
                             ({"dim": 700}, -2, b"rr_padded_dim"), ({"dim": 8320}, -2, b"rr_padded_dim"), ({"n": BIG}, -2, b"2^32")):
        assert call(**kw) == status, kw
        msg = L.rr_last_error()
        assert msg.startswith(b"rr_cluster_assign:") and word in msg, (kw, msg)
    assert call(n=0, xb=None, assign=None) == 0            # n_rows == 0 is a no-op


def test_means_validation_without_gpu():
    from ragroute_amd import _lib
    L = _lib.lib()
    need = L.rr_cluster_workspace_bytes(10, 768, 10)

    def call(xb=P, dtype=1, n=10, dim=768, d=700, assign=P, C=10, cent=P, counts=P, ws=P, ws_bytes=need):
        return L.rr_cluster_means(xb, dtype, n, dim, d, assign, C, cent, counts, ws, ws_bytes, None)
    for kw, status, word in (({"n": -1}, -1, b"negative"), ({"C": 0}, -1, b"n_clusters"), ({"C": 65}, -1, b"n_clusters"),
                             ({"dtype": 5}, -1, b"dtype"), ({"d": 0}, -1, b"d must"), ({"d": 769}, -1, b"d must"),
                             ({"xb": None}, -1, b"null"), ({"assign": None}, -1, b"null"), ({"cent": None}, -1, b"null"),
                             ({"counts": None}, -1, b"null"), ({"ws": None}, -1, b"null"), ({"ws": 8}, -1, b"aligned"),
                             ({"dim": 1000, "d": 700}, -2, b"rr_padded_dim"), ({"n": BIG, "ws_bytes": 1 << 40}, -2, b"2^32"),
                             ({"ws_bytes": need - 1}, -3, b"workspace"), ({"ws_bytes": 0}, -3, b"workspace")):
        assert call(**kw) == status, kw
        msg = L.rr_last_error()
        assert msg.startswith(b"rr_cluster_means:") and word in msg, (kw, msg)
