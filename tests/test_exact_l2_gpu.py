"""GPU: the f32-faithful exact search under the squared-L2 metric (FlatIndex / SegmentedIndex exact_l2=True,
rr_flat_search_faithful_l2, rr_flat_search_f32_exact_l2) returns, bit for bit, what the CPU oracle's flat_search_l2 returns on the
UNROUNDED f32 rows and queries — the reference's wikipedia federation reads L2 index files and keeps the lowest scores
(ragroute/config.py:59-70, rerank.py:28-34).  Data are gaussian f32 values that f16 / bf16 cannot represent."""
import numpy as np
import pytest
import torch

from tests.util import half_round

pytestmark = pytest.mark.gpu


def _gauss(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _index(gpu, xb, d, dtype="fp16"):
    from ragroute_amd.flat_index import FlatIndex
    idx = FlatIndex(d, metric="l2", dtype=dtype, device=gpu, exact_l2=True)
    idx.add(xb)
    return idx


def _plain(gpu, xb, d, dtype="fp16"):
    from ragroute_amd.flat_index import FlatIndex
    idx = FlatIndex(d, metric="l2", dtype=dtype, device=gpu)
    idx.add(xb)
    return idx


def _lib_normalised(x):
    """The f32 queries as the library itself normalises them (rr_l2_normalize_f32)."""
    from ragroute_amd.flat_index import normalize_L2
    y = np.ascontiguousarray(x, dtype=np.float32).copy()
    normalize_L2(y)
    return y


def _oracle(xb, xq, k):
    from oracle import oracle as O
    return O.flat_search_l2(xb, xq, k)


def _equal(D, I, Dref, Iref):
    assert np.array_equal(I, Iref), np.argwhere(I != Iref)[:5]
    assert np.array_equal(D, Dref)


def test_planted_near_ties_need_the_f32_rows(gpu):
    """b = half_round(q + u) and a = b moved towards q by at most 2^-14 on the elements with |b_j| >= 0.25 (half an f16 ulp there
    is at least 2^-13): a rounds to the same f16 row as b, so the half-precision search ties them and returns b (the lower id);
    on the f32 rows a is strictly nearer, and the faithful mode must return a, bit-equal to the oracle."""
    rng = np.random.default_rng(11)
    n, d, nq = 20_000, 768, 8
    xb = _gauss(rng, n, d)
    xq = _gauss(rng, nq, d)
    for i, q in enumerate(xq):
        b = half_round((q + np.float32(0.05) * _gauss(rng, 1, d)[0])[None, :])[0]
        diff = q - b
        c = np.float32(2.0 ** -14) / np.abs(diff).max()
        a = np.where(np.abs(b) >= 0.25, b + c * diff, b).astype(np.float32)
        assert np.array_equal(half_round(a[None, :])[0], b), "a and b must be one f16 row"
        q64 = q.astype(np.float64)
        assert ((q64 - a) ** 2).sum() < ((q64 - b) ** 2).sum(), "a must be strictly nearer in f64"
        xb[100 + 2 * i], xb[101 + 2 * i] = b, a              # a at the higher id
    _, Ip = _plain(gpu, xb, d).search(xq, 1)
    assert np.array_equal(Ip[:, 0], 100 + 2 * np.arange(nq)), "the rounded corpus ties a and b (lower id wins)"
    D, I = _index(gpu, xb, d).search(xq, 1)
    assert np.array_equal(I[:, 0], 101 + 2 * np.arange(nq))
    _equal(D, I, *_oracle(xb, xq, 1))


CASES = [  # dtype, d, nq, k, n, list_len
    ("fp16", 768, 64, 32, 30_001, None),
    ("bf16", 768, 300, 100, 20_011, None),      # > one query block
    ("bf16", 384, 1, 1, 9_999, None),
    ("fp16", 1024, 200, 32, 12_345, None),
    ("fp16", 2048, 64, 100, 10_007, None),
    ("fp16", 4096, 200, 32, 8_200, None),       # row-split wide-row kernel, just past the dense path
    ("bf16", 4096, 1, 1, 8_001, None),          # dense path
    ("fp16", 768, 300, 1024, 5_000, 1024),
    ("bf16", 1024, 64, 100, 50, None),          # n < k: (+inf, -1) padding
    ("fp16", 384, 64, 32, 8_193, None),
]


@pytest.mark.parametrize("dtype,d,nq,k,n,list_len", CASES)
def test_bit_equal_to_oracle_on_raw_f32(gpu, dtype, d, nq, k, n, list_len):
    rng = np.random.default_rng(d + nq + k + n)
    xb, xq = _gauss(rng, n, d), _gauss(rng, nq, d)
    idx = _index(gpu, xb, d, dtype)
    if list_len is not None:
        idx.faithful_list = list_len
    D, I = idx.search(xq, k)
    Dref, Iref = _oracle(xb, xq, k)
    _equal(D, I, Dref, Iref)
    if n < k:
        assert np.all(I[:, n:] == -1) and np.all(np.isposinf(D[:, n:]))


def _check_bound(gpu, xb, xq, d, k=32):
    """For every (q, row, D~) the plain half-precision L2 search returns: (max(0, sqrt(max(0, D~ - A)) - R))^2 <= |q - x|^2 in f64."""
    Dp, Ip = _plain(gpu, xb, d).search(xq, k)
    _, _, _, bound = _index(gpu, xb, d).search_exact_f32(torch.from_numpy(xq).to(gpu), k)
    bound = bound.cpu().numpy().astype(np.float64)
    assert bound.shape == (len(xq), 2) and np.all(np.isfinite(bound))
    A, R = bound[:, :1], bound[:, 1:]
    true = ((xq.astype(np.float64)[:, None, :] - xb[Ip].astype(np.float64)) ** 2).sum(-1)
    lower = np.maximum(0.0, np.sqrt(np.maximum(0.0, Dp.astype(np.float64) - A)) - R) ** 2
    assert np.all(lower <= true), float((lower - true).max())
    return lower, true


@pytest.mark.parametrize("d,nq,scale", [(768, 64, 1), (768, 256, 1), (2048, 16, 1), (2048, 200, 1), (4096, 200, 1), (384, 5, 1),
                                        (768, 64, 2.0 ** -18), (2048, 200, 2.0 ** -18)],
                         ids=["768-64", "768-256", "2048-16", "2048-200", "4096-200", "384-5", "768-64-subnormal", "2048-200-subnormal"])
def test_bound_holds_for_the_half_precision_scan(gpu, d, nq, scale):
    """A(q) and R(q) are not too small for the kernel family that serves this (dim, nq).  scale 2^-18: rows 3 g 2^-18 (g gaussian),
    whose half copies are mostly fp16 SUBNORMALS."""
    rng = np.random.default_rng(d * nq)
    n = 30_000
    xb, xq = _gauss(rng, n, d) * np.float32(3 * scale), _gauss(rng, nq, d)
    if scale != 1:
        stored = np.abs(half_round(xb[:256]))
        assert np.mean((stored < 2.0 ** -14) & (stored > 0)) > 0.9, "the half copies should be mostly subnormal and nonzero"
    _check_bound(gpu, xb, xq, d)


def test_bound_holds_where_the_distance_cancels(gpu):
    """Half the queries are stored rows plus 1e-3 N(0, 1): D~ = fl(qn - 2 s~) is the small difference of two large numbers."""
    rng = np.random.default_rng(77)
    n, d, nq = 30_000, 768, 64
    xb, xq = _gauss(rng, n, d), _gauss(rng, nq, d)
    xq[::2] = xb[1000: 1000 + nq // 2] + np.float32(1e-3) * _gauss(rng, nq // 2, d)
    lower, true = _check_bound(gpu, xb, xq, d)
    assert true[::2, 0].max() < 0.01 and true[1::2, 0].min() > 100      # both regimes are in the batch


def test_certified_lists_are_right_on_adversarial_data(gpu):
    """A dense cluster of near-duplicate rows around each query, list_len = k: many proofs fail, but every query the device
    certifies (exact = 1) has the oracle's result."""
    rng = np.random.default_rng(5)
    d, nq, k, per = 768, 32, 10, 300
    xq = _gauss(rng, nq, d)
    xb = np.concatenate([_gauss(rng, 5_000, d)] +
                        [q[None, :] + rng.standard_normal((per, d)).astype(np.float32) * np.float32(1e-3) for q in xq]).astype(np.float32)
    idx = _index(gpu, xb, d)
    D, I, exact, _ = idx.search_exact_f32(torch.from_numpy(xq).to(gpu), k, list_len=k)
    exact = exact.cpu().numpy().astype(bool)
    Dref, Iref = _oracle(xb, xq, k)
    assert np.array_equal(I.cpu().numpy()[exact], Iref[exact]) and np.array_equal(D.cpu().numpy()[exact], Dref[exact])
    assert (~exact).any(), "the data should defeat some proofs at list_len = k"
    D2, I2 = idx.search(xq, k)
    _equal(D2, I2, Dref, Iref)


@pytest.mark.parametrize("k", [5, 100])
def test_retry_and_exact_fallback(gpu, k):
    """3 000 rows that round to ONE f16 row: no list of 1024 proves the queries that point at them, the exact f32 scan answers
    those.  A mixed batch (ordinary queries beside them) still equals the oracle."""
    rng = np.random.default_rng(k)
    d = 768
    v = half_round(_gauss(rng, 1, d))[0]
    dup = (v[None, :] * (1 + rng.uniform(-1e-4, 1e-4, size=(3_000, d)))).astype(np.float32)
    assert np.all(half_round(dup) == v[None, :])
    xb = np.concatenate([_gauss(rng, 7_000, d), dup, _gauss(rng, 3_000, d)]).astype(np.float32)
    xq = _gauss(rng, 24, d)
    xq[::3] = v + _gauss(rng, 8, d) * np.float32(0.01)       # every third query points at the duplicates
    idx = _index(gpu, xb, d)
    D, I = idx.search(xq, k)
    _equal(D, I, *_oracle(xb, xq, k))
    assert 0 < idx.faithful_fallbacks < len(xq)
    assert idx.faithful_retries >= idx.faithful_fallbacks


def test_zero_distance_is_positive_zero(gpu):
    rng = np.random.default_rng(3)
    d, k = 768, 8
    xb = _gauss(rng, 12_000, d)
    xq = xb[[5, 4_000, 11_999]].copy()
    idx = _index(gpu, xb, d)
    D, I = idx.search(xq, k)
    assert np.all(D[:, 0] == 0) and not np.signbit(D[:, 0]).any()
    _equal(D, I, *_oracle(xb, xq, k))
    # the exact scan's own emit path
    Dt, It = torch.empty((3, k), device=gpu), torch.empty((3, k), dtype=torch.int64, device=gpu)
    idx._exact_scan(torch.from_numpy(xq).to(gpu), None, k, idx._segments(), idx.ntotal, None, 0, Dt, It)
    assert not np.signbit(Dt.cpu().numpy()[:, 0]).any()
    _equal(Dt.cpu().numpy(), It.cpu().numpy(), D, I)


def test_segmented_index_with_mask(gpu):
    from oracle import oracle as O
    from ragroute_amd.flat_index import SegmentedIndex
    rng = np.random.default_rng(21)
    d, nq, k = 768, 50, 32
    parts = [_gauss(rng, n, d) for n in (3_000, 700, 9_001, 1)]
    seg = SegmentedIndex(d, [p.shape[0] for p in parts], mask_cols=[2, 0, 3, 1], metric="l2", device=gpu, exact_l2=True)
    for s, p in enumerate(parts):
        seg.fill(s, p)
    xq = _gauss(rng, nq, d)
    mask = rng.integers(0, 2, size=(nq, 4)).astype(np.uint8)
    mask[0] = 0                                            # a query routed nowhere
    D, I = seg.search(xq, k, route_mask=mask)
    cols = []
    for s, p in enumerate(parts):
        Ds, Is = O.flat_search_l2(p, xq, k)
        keep = mask[:, seg.mask_cols[s]].astype(bool)[:, None]
        cols.append((np.where(keep, Ds, np.inf).astype(np.float32), np.where(keep & (Is >= 0), Is + (s << 40), -1)))
    Dref, Iref = O.merge_topk(np.concatenate([c[0] for c in cols], 1), np.concatenate([c[1] for c in cols], 1), k, False)
    _equal(D, I, Dref, Iref)
    assert np.all(I[0] == -1) and np.all(np.isposinf(D[0]))


def test_route_mask_column_and_id_offset(gpu):
    rng = np.random.default_rng(9)
    d, nq, k = 1024, 40, 32
    xb, xq = _gauss(rng, 20_000, d), _gauss(rng, nq, d)
    idx = _index(gpu, xb, d)
    prep = idx.prepare_queries(xq)
    assert isinstance(prep, tuple) and prep[1].dtype == torch.float32
    Du, Iu = (t.cpu().numpy() for t in idx.search_prepared(prep, k))
    _equal(Du, Iu, *_oracle(xb, xq, k))
    mask2 = torch.from_numpy(rng.integers(0, 2, size=(nq, 3)).astype(np.uint8)).to(gpu)
    mask = mask2[:, 1]                                     # a strided column of the router's mask
    D, I = (t.cpu().numpy() for t in idx.search_prepared(prep, k, id_offset=7 << 40, route_mask=mask))
    keep = mask.cpu().numpy().astype(bool)
    assert np.all(I[~keep] == -1) and np.all(np.isposinf(D[~keep]))
    assert np.array_equal(I[keep], Iu[keep] + (7 << 40)) and np.array_equal(D[keep], Du[keep])


def test_two_adds_equal_one(gpu):
    rng = np.random.default_rng(4)
    d, k = 768, 32
    xb, xq = _gauss(rng, 30_000, d), _gauss(rng, 20, d)
    one = _index(gpu, xb, d)
    two = _index(gpu, xb[:11_111], d)
    two.add(xb[11_111:])
    D1, I1 = one.search(xq, k)
    D2, I2 = two.search(xq, k)
    _equal(D2, I2, D1, I1)
    assert torch.equal(one._fstats, two._fstats)
    assert torch.equal(one._hn[: one.ntotal], two._hn[: two.ntotal])


def test_deterministic(gpu):
    rng = np.random.default_rng(6)
    d, k = 2048, 100
    xb, xq = _gauss(rng, 20_000, d), _gauss(rng, 100, d)
    idx = _index(gpu, xb, d, dtype="bf16")
    a = idx.search_exact_f32(torch.from_numpy(xq).to(gpu), k)
    b = idx.search_exact_f32(torch.from_numpy(xq).to(gpu), k)
    assert len(a) == 4
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_refusals_on_device(gpu):
    from ragroute_amd import _lib
    from ragroute_amd.flat_index import SegmentedIndex
    idx = _index(gpu, _gauss(np.random.default_rng(0), 10, 128), 128)
    with pytest.raises(_lib.RagrouteHipError):
        idx.build_screen()
    with pytest.raises(_lib.RagrouteHipError):
        idx.adopt(idx.xb)
    with pytest.raises(_lib.RagrouteHipError):
        SegmentedIndex.from_indexes([idx])


def test_data_source_serves_f32_distances(gpu, monkeypatch):
    from ragroute_amd import data_source as DS
    monkeypatch.setenv("RAGROUTE_EXACT_F32", "1")
    rng = np.random.default_rng(8)
    n, d, k = 4_000, 768, 32
    xb, xq = _gauss(rng, n, d), _gauss(rng, 6, d)
    ws = DS.DataSource(3, "wikipedia", "3")
    ws.index_metric = "l2"                                 # what load_faiss_index() reads from an IxF2 file
    ws.set_index(xb, [], [f"title {i}" for i in range(n)], [f"text {i}" for i in range(n)])
    assert ws.faiss_indexes[0].exact_l2 and not ws.faiss_indexes[0].exact_f32
    replies = ws.retrieve_docs_wikipedia(xq.copy(), k)     # (the wikipedia sources normalise their queries, in place)
    Dref, Iref = _oracle(xb, _lib_normalised(xq), k)
    for q, (rows, docs, scores) in enumerate(replies):
        assert list(rows) == Iref[q].tolist()
        assert np.array_equal(np.asarray(scores, np.float32), Dref[q])
        assert docs[0] == (f"title {Iref[q, 0]}", f"text {Iref[q, 0]}")
