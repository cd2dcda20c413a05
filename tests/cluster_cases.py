"""Cases and numpy / f64 references for the clustering kernels (rr_cluster_assign, rr_cluster_means) and ragroute_amd/cluster.py.
Everything here is host numpy; the GPU tests (tests/test_cluster_gpu.py) compare the library against these, and
tests/test_cluster_host.py checks these against brute-force loops."""
import numpy as np

from tests.util import half_round

U24 = 2.0 ** -24   # f32 unit roundoff


# ---- exact integer cases ------------------------------------------------------------------------------------------------------
# Values in [-8, 8], integer centroids, bias a multiple of 1/2: |score| <= 64 * 8192 + bias < 2^20 in steps of 1/2, so every
# partial sum and the one subtraction are exact in f32 in any order.  (dim, d, n_rows, C, nonzero columns): every width, row count
# and cluster count of the issue appears; `nz` small makes most rows tie between several centroids.
EXACT_SHAPES = [
    (128, 100, 1, 1, 100), (128, 100, 257, 17, 3), (128, 100, 70_001, 64, 4), (128, 100, 255, 2, 2),
    (768, 768, 255, 10, 768), (768, 768, 256, 2, 768), (768, 768, 70_001, 10, 768), (768, 768, 1, 64, 768),
    (896, 896, 257, 16, 896), (896, 896, 255, 64, 5), (896, 896, 256, 1, 896),
    (8192, 8192, 257, 64, 8192), (8192, 8192, 256, 17, 8192), (8192, 8192, 1, 2, 8192), (8192, 8192, 255, 10, 6),
]


def int_case(seed, n, d, C, nz=None, lo=-8, hi=8):
    """(x f32 [n, d], cent f32 [C, d], bias f32 [C]): integers in [lo, hi] in the first nz columns (zero behind), bias a multiple of 1/2."""
    rng = np.random.default_rng(seed)
    nz = d if nz is None else nz
    x = np.zeros((n, d), np.float32)
    c = np.zeros((C, d), np.float32)
    x[:, :nz] = rng.integers(lo, hi + 1, size=(n, nz))
    c[:, :nz] = rng.integers(lo, hi + 1, size=(C, nz))
    bias = (rng.integers(-40, 41, size=C) / 2.0).astype(np.float32)
    return x, c, bias


def ref_assign_exact(x, cent, bias=None):
    """int64 argmax with the lowest index on ties: (assign i32 [n], score f32 [n]).  Scores are kept doubled so that a bias that is a
    multiple of 1/2 stays an integer; the f64 matmul is exact on these integers (|sum| < 2^53) and is cast to int64 before the argmax."""
    s2 = 2 * np.rint(np.asarray(x, np.float64) @ np.asarray(cent, np.float64).T).astype(np.int64)
    if bias is not None:
        b2 = np.rint(2 * np.asarray(bias, np.float64)).astype(np.int64)
        assert np.array_equal(b2 / 2.0, np.asarray(bias, np.float64)), "bias must be a multiple of 1/2"
        s2 = s2 - b2[None, :]
    a = np.argmax(s2, axis=1)                     # numpy: the first maximum
    best = s2[np.arange(len(a)), a]
    assert np.abs(s2).max(initial=0) < 1 << 24
    return a.astype(np.int32), (best / 2.0).astype(np.float32)


def brute_assign(x, cent, bias=None):
    """The same by a triple loop (tiny cases only)."""
    n, d = x.shape
    out_a, out_s = np.zeros(n, np.int32), np.zeros(n, np.float32)
    for r in range(n):
        best, arg = None, -1
        for c in range(cent.shape[0]):
            s = 0.0
            for j in range(d):
                s += float(x[r, j]) * float(cent[c, j])
            if bias is not None:
                s -= float(bias[c])
            if best is None or s > best:
                best, arg = s, c
        out_a[r], out_s[r] = arg, best
    return out_a, out_s


# ---- rounded gaussian cases ---------------------------------------------------------------------------------------------------
GAUSS_SHAPES = [(70_000, 768, 768, 10), (5_000, 8192, 8192, 64), (3_000, 100, 128, 17)]   # (n, d, dim, C)
GAUSS_AMBIGUOUS_CAP = 0.15     # a condition on the case, not a tolerance: rows whose f64 reference admits more than one centroid


def gauss_case(n, d, C, dtype):
    """numpy.random.default_rng(0); rows and centroids N(0, 1/d) rounded to the index dtype (returned as f32 holding those values)."""
    rng = np.random.default_rng(0)
    x = half_round((rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32), dtype)
    c = half_round((rng.standard_normal((C, d)) / np.sqrt(d)).astype(np.float32), dtype)
    return x, c


def dot_and_abs(x, cent):
    """(x . c, sum_j |x_j c_j|) in f64, [n, C] each: the two matrix products every bound of a case shares."""
    x64, c64 = np.asarray(x, np.float64), np.asarray(cent, np.float64)
    return x64 @ c64.T, np.abs(x64) @ np.abs(c64).T


def score_bound(x, cent, bias, dim, products=None):
    """(s64 [n, C], tol [n, C]): the f64 scores x . c - bias of the stored values and the derived f32 error bound
    tol = g A + 2^-24 (|s64| + |bias| + g A), A = sum_j |x_j c_j|, g = dim 2^-24 / (1 - dim 2^-24): the standard bound of an f32 dot
    product of dim terms in any order, plus the rounding of the one subtraction (whose operand is off by at most g A).
    products: dot_and_abs(x, cent), when several biases share them."""
    dot, A = dot_and_abs(x, cent) if products is None else products
    b64 = np.zeros(dot.shape[1]) if bias is None else np.asarray(bias, np.float64)
    s64 = dot - b64[None, :]
    g = dim * U24 / (1 - dim * U24)
    return s64, g * A + U24 * (np.abs(s64) + np.abs(b64)[None, :] + g * A)


def check_assignment_within_bound(assign, s64, tol):
    """Every row: s64(assigned) + tol >= max_c (s64 - tol).  Returns the fraction of rows whose reference itself admits more than one
    centroid (some other c reaches the same condition)."""
    n = s64.shape[0]
    a = np.asarray(assign, np.int64)
    assert a.min() >= 0 and a.max() < s64.shape[1]
    need = (s64 - tol).max(axis=1)
    got = s64[np.arange(n), a] + tol[np.arange(n), a]
    bad = np.flatnonzero(got < need)
    assert bad.size == 0, f"{bad.size} rows assigned outside the bound, first {bad[:5]}: {got[bad[:5]]} < {need[bad[:5]]}"
    admitted = ((s64 + tol) >= need[:, None]).sum(axis=1)
    return float((admitted > 1).mean())


# ---- means --------------------------------------------------------------------------------------------------------------------
def ref_means64(x, assign, C, prev=None):
    """(means f64 [C, d], counts i64 [C], abs_sums f64 [C, d]); a cluster without members keeps prev's row (zeros without prev).
    Labels outside [0, C) are skipped."""
    x64 = np.asarray(x, np.float64)
    a = np.asarray(assign, np.int64)
    d = x64.shape[1]
    out = np.zeros((C, d)) if prev is None else np.asarray(prev, np.float64).copy()
    counts = np.zeros(C, np.int64)
    abs_sums = np.zeros((C, d))
    for c in range(C):
        rows = x64[a == c]
        counts[c] = rows.shape[0]
        if rows.shape[0]:
            out[c] = rows.sum(axis=0) / rows.shape[0]
            abs_sums[c] = np.abs(rows).sum(axis=0)
    return out, counts, abs_sums


def brute_means(x, assign, C):
    n, d = x.shape
    sums = [[0.0] * d for _ in range(C)]
    counts = [0] * C
    for r in range(n):
        c = int(assign[r])
        if 0 <= c < C:
            counts[c] += 1
            for j in range(d):
                sums[c][j] += float(x[r, j])
    return np.array([[s / counts[c] if counts[c] else 0.0 for s in sums[c]] for c in range(C)]), np.array(counts, np.int64)


def means_bound(means64, counts, abs_sums):
    """The accuracy contract of rr_cluster_means per element: 4098 2^-24 sum|x| / count + one f32 rounding of the mean."""
    cnt = np.maximum(counts, 1)[:, None].astype(np.float64)
    return 4098 * U24 * abs_sums / cnt + U24 * np.abs(means64)


# ---- planted blobs ------------------------------------------------------------------------------------------------------------
def blobs_case(seed=3, n=4000, d=128, blobs=8, sep=4.0, noise=0.05):
    """(x f32 [n, d] shuffled, labels [n], centres f32 [blobs, d], first_row_of_blob [blobs]): separation >> noise."""
    rng = np.random.default_rng(seed)
    centres = (sep * rng.standard_normal((blobs, d))).astype(np.float32)
    labels = rng.permutation(np.arange(n) % blobs)
    x = (centres[labels] + noise * rng.standard_normal((n, d))).astype(np.float32)
    first = np.array([int(np.flatnonzero(labels == b)[0]) for b in range(blobs)])
    return x, labels, centres, first
