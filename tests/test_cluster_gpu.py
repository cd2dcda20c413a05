"""GPU: rr_cluster_assign and rr_cluster_means against the numpy / f64 references of tests/cluster_cases.py, and ragroute_amd/cluster.py
(kmeans, federate, route_nearest, cluster_stats) through the public interface.

Exact cases use integer data (every score an exact f32 in any summation order) and compare bit for bit; rounded gaussian data is held
to the derived f32 dot-product bound of cluster_cases.score_bound, the means to the accuracy contract of include/ragroute_hip.h."""
import functools

import numpy as np
import pytest
import torch

from tests import cluster_cases as K

pytestmark = pytest.mark.gpu

TD = {"fp16": torch.float16, "bf16": torch.bfloat16}
HUGE = {"fp16": 60000.0, "bf16": 3.0e38}


def dev_half(x, dim, dtype, dev, extra_rows=0, fill=0.0):
    """f32 [n, d] holding values the dtype stores exactly -> device [n + extra_rows, dim], zero padded; extra rows hold `fill`."""
    n, d = x.shape
    t = torch.zeros((n + extra_rows, dim), dtype=TD[dtype], device=dev)
    t[:n, :d] = torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(TD[dtype])
    if extra_rows:
        t[n:] = fill
    return t


def run_assign(xb, n, ch, bias, out=None):
    from ragroute_amd import cluster
    b = None if bias is None else (bias if isinstance(bias, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(bias, np.float32)).to(xb.device))
    a, s = cluster.assign_half(xb, n, ch, b, out)
    torch.cuda.synchronize()
    return a.cpu().numpy(), s.cpu().numpy()


def assert_bit_equal(a, s, ra, rs, what=""):
    assert np.array_equal(a, ra), f"{what}: {(a != ra).sum()} of {len(a)} assignments differ, first at {np.flatnonzero(a != ra)[:5]}"
    assert np.array_equal(s.view(np.uint32), rs.view(np.uint32)), f"{what}: scores differ at {np.flatnonzero(s != rs)[:5]}"


@functools.lru_cache(maxsize=2)
def _exact(shape):
    dim, d, n, C, nz = shape
    lo, hi = (-1, 1) if nz < 10 else (-8, 8)                               # few live columns of few values: most rows tie
    x, c, bias = K.int_case(100 + dim + n + C, n, d, C, nz, lo, hi)
    return x, c, bias, K.ref_assign_exact(x, c, None), K.ref_assign_exact(x, c, bias)


# ---- assignment, exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.EXACT_SHAPES, ids=lambda s: "dim%d-d%d-n%d-C%d-nz%d" % s)
def test_assign_exact_on_integer_data(gpu, shape):
    dim, d, n, C, nz = shape
    x, c, bias, ref_ip, ref_b = _exact(shape)
    if nz < 10 and n > 100:
        s = x.astype(np.float64) @ c.astype(np.float64).T
        assert ((s == s.max(1, keepdims=True)).sum(1) > 1).mean() > 0.1, "the low-rank cases are there for their ties"
    for dtype in ("fp16", "bf16"):
        xb, ch = dev_half(x, dim, dtype, gpu), dev_half(c, dim, dtype, gpu)
        assert_bit_equal(*run_assign(xb, n, ch, None), *ref_ip, what=f"{dtype} no bias")
        assert_bit_equal(*run_assign(xb, n, ch, bias), *ref_b, what=f"{dtype} bias")


@pytest.mark.parametrize("C", [10, 17])
def test_padding_columns_never_win_when_every_score_is_negative(gpu, C):
    rng = np.random.default_rng(C)
    x = rng.integers(1, 9, size=(300, 768)).astype(np.float32)          # all positive
    c = -rng.integers(1, 9, size=(C, 768)).astype(np.float32)           # all negative: every real score < 0, a padding column scores 0
    bias = (rng.integers(0, 41, size=C) / 2.0).astype(np.float32)
    for dtype in ("fp16", "bf16"):
        xb, ch = dev_half(x, 768, dtype, gpu), dev_half(c, 768, dtype, gpu)
        for b in (None, bias):
            ra, rs = K.ref_assign_exact(x, c, b)
            assert (rs < 0).all()
            assert_bit_equal(*run_assign(xb, 300, ch, b), ra, rs, what=f"{dtype}")


@pytest.mark.parametrize("C", [17, 64])
def test_winner_in_the_last_column(gpu, C):
    x, c, bias = K.int_case(40 + C, 200, 128, C)
    x[:120] = c[C - 1]                                                    # 120 rows are (nearly) the last centroid: it wins them widely
    x[np.arange(120), np.arange(120)] = 0
    ra, rs = K.ref_assign_exact(x, c, None)
    assert (ra[:120] == C - 1).all() and (ra != C - 1).any()
    for dtype in ("fp16", "bf16"):
        assert_bit_equal(*run_assign(dev_half(x, 128, dtype, gpu), 200, dev_half(c, 128, dtype, gpu), None), ra, rs, what=dtype)


def test_asymmetric_centroid_matrix_catches_a_row_column_swap(gpu):
    """Rows are unit vectors e_r: score(r, c) = cent[c][r], a 16 x 16 matrix that differs from its transpose."""
    rng = np.random.default_rng(8)
    M = rng.integers(-8, 9, size=(16, 16)).astype(np.float32)
    assert not np.array_equal(M, M.T)
    x, c = np.zeros((16, 100), np.float32), np.zeros((16, 100), np.float32)
    x[np.arange(16), np.arange(16)] = 1
    c[:, :16] = M
    ra, rs = K.ref_assign_exact(x, c, None)
    assert not np.array_equal(ra, K.ref_assign_exact(x, np.pad(M.T, ((0, 0), (0, 84))), None)[0])
    for dtype in ("fp16", "bf16"):
        assert_bit_equal(*run_assign(dev_half(x, 128, dtype, gpu), 16, dev_half(c, 128, dtype, gpu), None), ra, rs, what=dtype)


def test_nan_rows_and_nan_centroids(gpu):
    x, c, bias = K.int_case(77, 100, 768, 10)
    ra, rs = K.ref_assign_exact(x, c, bias)
    for dtype in ("fp16", "bf16"):
        xn = x.copy()
        xn[5, 300] = np.nan                                               # one NaN in one row
        a, s = run_assign(dev_half(xn, 768, dtype, gpu), 100, dev_half(c, 768, dtype, gpu), bias)
        assert a[5] == -1 and np.isnan(s[5])
        keep = np.arange(100) != 5
        assert_bit_equal(a[keep], s[keep], ra[keep], rs[keep], what=f"{dtype}: neighbours of the NaN row")
        cn = c.copy()
        cn[3, 11] = np.nan                                                # a NaN centroid never wins
        a, s = run_assign(dev_half(x, 768, dtype, gpu), 100, dev_half(cn, 768, dtype, gpu), bias)
        s2 = x.astype(np.float64) @ c.astype(np.float64).T - bias[None, :].astype(np.float64)
        s2[:, 3] = -np.inf
        wa = np.argmax(s2, 1).astype(np.int32)
        assert (ra == 3).any(), "centroid 3 would have won some rows"
        assert_bit_equal(a, s, wa, s2[np.arange(100), wa].astype(np.float32), what=f"{dtype}: NaN centroid")
        cn[:] = np.nan                                                    # every centroid NaN: every row unassigned
        a, s = run_assign(dev_half(x, 768, dtype, gpu), 100, dev_half(cn, 768, dtype, gpu), None)
        assert (a == -1).all() and np.isnan(s).all()


@pytest.mark.parametrize("n", [1, 255, 257])
def test_nothing_is_read_or_written_behind_n_rows(gpu, n):
    x, c, bias = K.int_case(n, n, 100, 17)
    ra, rs = K.ref_assign_exact(x, c, bias)
    for dtype in ("fp16", "bf16"):
        xb = dev_half(x, 128, dtype, gpu, extra_rows=256, fill=HUGE[dtype])
        a = torch.full((n + 256,), -7, dtype=torch.int32, device=gpu)
        s = torch.full((n + 256,), 123.0, dtype=torch.float32, device=gpu)
        ga, gs = run_assign(xb, n, dev_half(c, 128, dtype, gpu), bias, out=(a, s))
        assert_bit_equal(ga[:n], gs[:n], ra, rs, what=dtype)
        assert (ga[n:] == -7).all() and (gs[n:] == 123.0).all(), "sentinels behind n_rows were overwritten"


def test_score_output_is_optional(gpu):
    from ragroute_amd import _calls, _lib
    x, c, _ = K.int_case(3, 300, 100, 10)
    xb, ch = dev_half(x, 128, "fp16", gpu), dev_half(c, 128, "fp16", gpu)
    a = torch.empty(300, dtype=torch.int32, device=gpu)
    _lib.check(_lib.lib().rr_cluster_assign(xb.data_ptr(), 0, 300, 128, ch.data_ptr(), None, 10, a.data_ptr(), None, _calls.stream_ptr()), "assign")
    assert np.array_equal(a.cpu().numpy(), K.ref_assign_exact(x, c, None)[0])


# ---- assignment, rounded gaussian data --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", K.GAUSS_SHAPES, ids=lambda s: "n%d-d%d-dim%d-C%d" % s)
def test_assign_gaussian_within_the_derived_bound(gpu, shape, dtype):
    from ragroute_amd import _calls
    n, d, dim, C = shape
    x, c = K.gauss_case(n, d, C, dtype)
    xb, ch = dev_half(x, dim, dtype, gpu), dev_half(c, dim, dtype, gpu)
    bias_dev = _calls.half_sqnorms(ch, C)                                  # the f32 bias as rr_half_sqnorms returns it
    products = K.dot_and_abs(x, c)
    for bias in (bias_dev, None):
        a, s = run_assign(xb, n, ch, bias)
        b = None if bias is None else bias.cpu().numpy()
        s64, tol = K.score_bound(x, c, b, dim, products)
        frac = K.check_assignment_within_bound(a, s64, tol)
        print(f"{shape} {dtype} bias={bias is not None}: rows admitting more than one centroid {100 * frac:.3f} %")
        assert frac <= K.GAUSS_AMBIGUOUS_CAP
        err = np.abs(s.astype(np.float64) - s64[np.arange(n), a])
        assert (err <= tol[np.arange(n), a]).all(), "a returned score is outside the bound of its own centroid"


# ---- means ------------------------------------------------------------------------------------------------------------------------
def run_means(xb, n, d, labels, C, prev=None, dtype="fp16"):
    from ragroute_amd import _calls, _lib
    L = _lib.lib()
    dev = xb.device
    cent = torch.zeros((C, d), dtype=torch.float32, device=dev) if prev is None else torch.from_numpy(np.ascontiguousarray(prev, np.float32)).to(dev)
    counts = torch.full((C,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.rr_cluster_workspace_bytes(n, xb.shape[1], C), dtype=torch.uint8, device=dev)
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(dev)
    _lib.check(L.rr_cluster_means(xb.data_ptr(), _calls.RR_DTYPE[dtype], n, xb.shape[1], d, lab.data_ptr(), C, cent.data_ptr(), counts.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _calls.stream_ptr()), "rr_cluster_means")
    torch.cuda.synchronize()
    return cent, counts


@pytest.mark.parametrize("shape", [(10_007, 100, 128, 10), (5_000, 768, 768, 64), (300, 1000, 1280, 33), (1, 8192, 8192, 1)],
                         ids=lambda s: "n%d-d%d-dim%d-C%d" % s)
def test_means_exact_on_integer_data(gpu, shape):
    n, d, dim, C = shape
    rng = np.random.default_rng(n + C)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    labels = rng.integers(0, C, size=n).astype(np.int32)
    if n > 100:
        labels[rng.integers(0, n, size=20)] = -1                          # skipped
        labels[rng.integers(0, n, size=5)] = C + 35                       # outside [0, C): skipped too
        labels[labels == C - 1] = 0                                       # the last cluster is empty: keeps its row
    prev = rng.standard_normal((C, d)).astype(np.float32)
    m64, cnt, _ = K.ref_means64(x, labels, C, prev)
    for dtype in ("fp16", "bf16"):
        cent, counts = run_means(dev_half(x, dim, dtype, gpu), n, d, labels, C, prev, dtype)
        assert np.array_equal(counts.cpu().numpy(), cnt)
        assert np.array_equal(cent.cpu().numpy().view(np.uint32), m64.astype(np.float32).view(np.uint32)), "centroid != fl32(sum / count)"
        if n > 100:
            assert cnt[C - 1] == 0 and np.array_equal(cent.cpu().numpy()[C - 1], prev[C - 1])


def test_means_exact_when_a_range_flushes_more_than_once(gpu):
    """More than 512 x 4096 rows: the ranges are longer than 4096 rows, so each adds its later f32 blocks onto its own f64 partial.
    Data and the (exact, integer) reference are made on the device."""
    n, d, dim, C = 512 * 4096 + 4097, 64, 128, 10
    g = torch.Generator(device=gpu).manual_seed(1)
    xb = torch.zeros((n, dim), dtype=torch.float16, device=gpu)
    xb[:, :d] = torch.randint(-8, 9, (n, d), generator=g, device=gpu).to(torch.float16)
    labels = torch.randint(-1, C, (n,), generator=g, device=gpu, dtype=torch.int32)
    cent, counts = run_means(xb, n, d, labels, C)
    for c in range(C):
        rows = labels == c
        m = int(rows.sum())
        total = xb[rows][:, :d].to(torch.float64).sum(0)                   # integers: exact in any order
        assert int(counts[c]) == m
        assert torch.equal(cent[c], (total / m).to(torch.float32))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_means_gaussian_within_the_contract(gpu, dtype):
    n, d, dim, C = 20_000, 768, 768, 10
    rng = np.random.default_rng(0)
    from tests.util import half_round
    x = half_round((0.5 + 0.25 * rng.standard_normal((n, d))).astype(np.float32), dtype)
    labels = (rng.integers(0, C, size=n) * (rng.random(n) < 0.7)).astype(np.int32)   # cluster 0 holds more than 4096 rows
    m64, cnt, abs_sums = K.ref_means64(x, labels, C)
    assert cnt[0] > 4096
    cent, counts = run_means(dev_half(x, dim, dtype, gpu), n, d, labels, C, None, dtype)
    assert np.array_equal(counts.cpu().numpy(), cnt)
    err = np.abs(cent.cpu().numpy().astype(np.float64) - m64)
    bound = K.means_bound(m64, cnt, abs_sums)
    print(f"{dtype}: worst error / bound = {(err / bound).max():.3e}")
    assert (err <= bound).all()


def test_means_are_deterministic(gpu):
    n, d, dim, C = 300_000, 64, 128, 10
    g = torch.Generator(device=gpu).manual_seed(2)
    xb = torch.zeros((n, dim), dtype=torch.float16, device=gpu)
    xb[:, :d] = (0.5 + torch.randn((n, d), generator=g, device=gpu)).to(torch.float16)
    labels = torch.randint(0, C, (n,), generator=g, device=gpu, dtype=torch.int32)
    c1, n1 = run_means(xb, n, d, labels, C)
    c2, n2 = run_means(xb, n, d, labels, C)
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32)) and torch.equal(n1, n2)
    assert int(n1.sum()) == n and float(c1.abs().max()) < 1.0


# ---- the public interface ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs(gpu):
    from ragroute_amd.flat_index import FlatIndex
    x, labels, centres, first = K.blobs_case()
    idx = FlatIndex(x.shape[1], metric="l2", device=gpu)
    idx.add(x)
    return idx, x, labels, centres, first


def test_kmeans_recovers_planted_blobs(blobs):
    from ragroute_amd import cluster
    idx, x, labels, centres, first = blobs
    res = cluster.kmeans(idx, 8, init=x[first])
    assert res.converged and res.iterations <= 3
    assert np.array_equal(res.assign.cpu().numpy(), labels.astype(np.int32))
    assert np.array_equal(res.counts.cpu().numpy(), np.bincount(labels, minlength=8))
    assert np.allclose(res.centroids.cpu().numpy(), centres, atol=0.05)
    again, _ = cluster.assign(idx, res.centroids)
    assert torch.equal(again, res.assign)
    stats = cluster.cluster_stats(idx, res)
    assert [s["size"] for s in stats] == np.bincount(labels, minlength=8).tolist()
    assert np.array_equal(np.asarray(stats[2]["centroid"], np.float32), res.centroids[2].cpu().numpy())   # converged: the same means


@pytest.mark.parametrize("metric", ["l2", "cosine", "ip"])
def test_kmeans_seeded_default_init_is_reproducible(gpu, metric):
    from ragroute_amd import cluster
    from ragroute_amd.flat_index import FlatIndex
    x = K.blobs_case(seed=4, n=3000, d=100, blobs=6)[0]
    idx = FlatIndex(100, metric=metric, dtype="bf16", device=gpu)
    idx.add(x)
    a, b = cluster.kmeans(idx, 6, iters=5, seed=7), cluster.kmeans(idx, 6, iters=5, seed=7)
    assert torch.equal(a.centroids.view(torch.int32), b.centroids.view(torch.int32)) and torch.equal(a.assign, b.assign)
    assert torch.equal(a.counts, b.counts) and (a.iterations, a.converged) == (b.iterations, b.converged)
    assert torch.equal(cluster.assign(idx, a.centroids)[0], a.assign)
    assert np.array_equal(a.counts.cpu().numpy(), np.bincount(a.assign.cpu().numpy(), minlength=6))
    if metric != "l2":                                                     # spherical: unit centroids
        assert np.allclose(np.linalg.norm(a.centroids.cpu().numpy().astype(np.float64), axis=1), 1.0, atol=1e-5)
    rows = sorted(int(r) for r in np.random.default_rng(7).choice(3000, 6, replace=False))
    c = cluster.kmeans(idx, 6, iters=0, seed=7)                            # no pass: the init itself = the stored rows
    assert torch.equal(c.centroids, idx.xb[rows][:, :100].float())


def test_kmeans_refuses_what_it_cannot_cluster(gpu):
    from ragroute_amd import _lib, cluster
    from ragroute_amd.flat_index import FlatIndex
    x = np.random.default_rng(1).standard_normal((20, 64)).astype(np.float32)
    idx = FlatIndex(64, metric="l2", device=gpu)
    idx.add(x)
    with pytest.raises(ValueError):
        cluster.kmeans(idx, 21)
    with pytest.raises(ValueError):
        cluster.kmeans(idx, 65)
    for kw in ({"metric": "l2", "exact_l2": True}, {"metric": "ip", "exact_f32": True}):
        faithful = FlatIndex(64, device=gpu, **kw)
        faithful.add(x)
        with pytest.raises(_lib.RagrouteHipError):
            cluster.kmeans(faithful, 2)
    screened = FlatIndex(64, metric="ip", device=gpu)
    screened.add(x)
    screened.build_screen()
    with pytest.raises(_lib.RagrouteHipError):
        cluster.kmeans(screened, 2)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_federation_searches_like_the_original_index(gpu, metric):
    from ragroute_amd import cluster
    from ragroute_amd.flat_index import FlatIndex
    rng = np.random.default_rng(12)
    n, d, k, C = 3000, 128, 10, 5
    x = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    xq = rng.integers(-2, 3, size=(32, d)).astype(np.float32)
    idx = FlatIndex(d, metric=metric, device=gpu)
    idx.add(x)
    res = cluster.kmeans(idx, C, iters=3, seed=1)
    fed = cluster.federate(idx, res)
    labels = res.assign.cpu().numpy()
    assert fed.index.rows == np.bincount(labels, minlength=C).tolist() and fed.index.metric == metric
    rows = fed.rows.cpu().numpy()
    assert np.array_equal(rows, np.argsort(labels, kind="stable"))          # cluster by cluster, ascending original row
    for c in range(C):                                                      # the stored half rows, bit for bit
        mine = rows[labels[rows] == c]
        assert torch.equal(fed.index.rows_of(c).view(torch.int16), idx.xb[torch.from_numpy(mine).to(gpu)].view(torch.int16))
    q = idx.prepare_queries(xq)
    D0, I0 = idx.search_prepared(q, k)
    D1, I1 = fed.index.search_prepared(q, k)
    assert torch.equal(D0.view(torch.int32), D1.view(torch.int32))
    I1o = fed.original_ids(I1)
    D0, I0, I1o = D0.cpu().numpy(), I0.cpu().numpy(), I1o.cpu().numpy()
    checked = 0
    for qi in range(32):
        for j in range(k):
            better = D0[qi, j] < D0[qi, k - 1] if metric == "l2" else D0[qi, j] > D0[qi, k - 1]
            if better and (D0[qi] == D0[qi, j]).sum() == 1:
                assert I0[qi, j] == I1o[qi, j]
                checked += 1
        assert set(I1o[qi].tolist()) <= set(range(n))
    assert checked > 32
    assert torch.equal(fed.original_ids(torch.tensor([[-1, 0]], device=gpu))[0, :1], torch.tensor([-1], device=gpu))
    # unassigned rows: refused, or left out on request
    bad = res._replace(assign=res.assign.clone())
    bad.assign[17] = -1
    with pytest.raises(ValueError):
        cluster.federate(idx, bad)
    part = cluster.federate(idx, bad, drop_unassigned=True)
    assert part.rows.numel() == n - 1 and 17 not in part.rows.cpu().tolist()


def test_route_nearest(blobs):
    from ragroute_amd import cluster
    idx, x, labels, centres, first = blobs
    res = cluster.kmeans(idx, 8, init=x[first])
    fed = cluster.federate(idx, res)
    k = 10
    xq = centres + 0.01
    q = idx.prepare_queries(xq)
    D_all, I_all = fed.index.search_prepared(q, k)
    full = cluster.route_nearest(res, xq, 8)
    assert full.dtype == torch.uint8 and full.shape == (8, 8) and bool(full.all())
    D8, I8 = fed.index.search_prepared(q, k, route_mask=full)
    assert torch.equal(D8, D_all) and torch.equal(I8, I_all)                # n_probe = C: as no mask
    one = cluster.route_nearest(res, xq, 1)
    assert torch.equal(one.sum(1).cpu(), torch.ones(8, dtype=torch.int64))
    D1, I1 = fed.index.search_prepared(q, k, route_mask=one)
    assert torch.equal(D1, D_all) and torch.equal(I1, I_all)                # queries at the blob centres: the exhaustive top-k
    ch, bias = cluster._half_centroids(idx, res.centroids)                  # the single set column = rr_cluster_assign of the queries
    qa, _ = cluster.assign_half(q, 8, ch, bias)
    assert torch.equal(one.to(torch.int32).argmax(1).to(torch.int32), qa) and qa.cpu().tolist() == list(range(8))
    three = cluster.route_nearest(cluster.centroid_index(res), xq, 3)       # a prebuilt centroid index serves too
    assert torch.equal(three.sum(1).cpu(), torch.full((8,), 3, dtype=torch.int64)) and bool((three >= one).all())
    with pytest.raises(ValueError):
        cluster.route_nearest(res, xq, 9)
