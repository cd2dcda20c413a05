"""GPU: the f32-faithful exact search (FlatIndex / SegmentedIndex exact_f32=True, rr_flat_search_faithful, rr_flat_search_f32_exact)
returns, bit for bit, what the CPU oracle returns on the UNROUNDED f32 rows and queries — the reference's faiss.IndexFlatIP reads
f32 rows (ragroute/data_source.py:71, 158, 186, 203).  Data are gaussian f32 values that f16 / bf16 cannot represent."""
import numpy as np
import pytest
import torch

from tests.util import half_round

pytestmark = pytest.mark.gpu


def _gauss(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _index(gpu, xb, d, metric="ip", dtype="fp16", **kw):
    from ragroute_amd.flat_index import FlatIndex
    idx = FlatIndex(d, metric=metric, dtype=dtype, device=gpu, exact_f32=True, **kw)
    idx.add(xb)
    return idx


def _lib_normalised(x):
    """The f32 rows the library itself normalises (rr_l2_normalize_f32): the cosine oracle's inputs."""
    from ragroute_amd.flat_index import normalize_L2
    y = np.ascontiguousarray(x, dtype=np.float32).copy()
    normalize_L2(y)
    return y


def _oracle(xb, xq, k, metric="ip"):
    from oracle import oracle as O
    if metric == "cosine":
        xb, xq = _lib_normalised(xb), _lib_normalised(xq)
    return O.flat_search_ip(xb, xq, k)


def _equal(D, I, Dref, Iref):
    assert np.array_equal(I, Iref), np.argwhere(I != Iref)[:5]
    assert np.array_equal(D, Dref)


def test_planted_near_ties_need_the_f32_rows(gpu):
    """Row a = b + delta q/|q|^2 rounds to the same f16 row as b, so the half-precision search ties them and returns b (the
    lower id); on the f32 rows a scores delta higher, and the faithful mode must return a, bit-equal to the oracle."""
    from ragroute_amd.flat_index import FlatIndex
    rng = np.random.default_rng(11)
    n, d, nq = 20_000, 768, 8
    xb = _gauss(rng, n, d)
    xq = _gauss(rng, nq, d)
    for i, q in enumerate(xq):
        b = half_round(4.0 * q[None, :])[0]                # far above every gaussian row (4 |q|^2 vs ~ N(0, |q|^2))
        a = (b + np.float32(0.05) * q / np.float32(q @ q)).astype(np.float32)
        assert np.array_equal(half_round(a[None, :])[0], b), "a and b must be one f16 row"
        assert np.float32(np.float64(q) @ np.float64(a)) > np.float32(np.float64(q) @ np.float64(b))
        xb[100 + 2 * i], xb[101 + 2 * i] = b, a              # a at the higher id
    plain = FlatIndex(d, device=gpu)
    plain.add(xb)
    _, Ip = plain.search(xq, 1)
    assert np.array_equal(Ip[:, 0], 100 + 2 * np.arange(nq)), "the rounded corpus ties a and b (lower id wins)"
    idx = _index(gpu, xb, d)
    D, I = idx.search(xq, 1)
    assert np.array_equal(I[:, 0], 101 + 2 * np.arange(nq))
    _equal(D, I, *_oracle(xb, xq, 1))


CASES = [  # metric, dtype, d, nq, k, n, list_len
    ("ip", "fp16", 768, 64, 32, 50_001, None),
    ("cosine", "bf16", 768, 300, 100, 30_011, None),     # > one query block
    ("ip", "bf16", 384, 1, 1, 9_999, None),
    ("cosine", "fp16", 1024, 200, 32, 20_003, None),
    ("ip", "fp16", 2048, 64, 100, 12_345, None),
    ("ip", "fp16", 4096, 200, 32, 10_007, None),          # row-split wide-row kernel
    ("cosine", "bf16", 4096, 1, 1, 8_001, None),
    ("ip", "fp16", 768, 300, 1024, 5_000, 1024),
    ("ip", "bf16", 1024, 64, 100, 50, None),              # n < k: padding
    ("cosine", "fp16", 384, 64, 32, 8_193, None),         # dense path boundary
]


@pytest.mark.parametrize("metric,dtype,d,nq,k,n,list_len", CASES)
def test_bit_equal_to_oracle_on_raw_f32(gpu, metric, dtype, d, nq, k, n, list_len):
    rng = np.random.default_rng(d + nq + k + n)
    xb, xq = _gauss(rng, n, d), _gauss(rng, nq, d)
    idx = _index(gpu, xb, d, metric, dtype)
    if list_len is not None:
        idx.faithful_list = list_len
    D, I = idx.search(xq, k)
    _equal(D, I, *_oracle(xb, xq, k, metric))


@pytest.mark.parametrize("d,nq,scale", [(768, 64, 1), (768, 256, 1), (2048, 16, 1), (2048, 200, 1), (4096, 200, 1), (384, 5, 1),
                                        (768, 64, 2.0 ** -18), (2048, 200, 2.0 ** -18)],
                         ids=["768-64", "768-256", "2048-16", "2048-200", "4096-200", "384-5", "768-64-subnormal", "2048-200-subnormal"])
def test_eps_bounds_the_half_precision_scan(gpu, d, nq, scale):
    """Every score the plain fp16 search returns is within eps(q) of the true (f64) dot product of the f32 inputs: the bound
    gamma(dim) is not too small for the kernel family that serves this (dim, nq).  scale 2^-18: rows 3 g 2^-18 (g gaussian), whose
    half copies are mostly fp16 SUBNORMALS (|v| < 2^-14 for |g| < 5.3) - the proof assumes the matrix cores take subnormal fp16
    inputs as they are, and eps(q) has no term for a flushed operand."""
    from ragroute_amd.flat_index import FlatIndex
    rng = np.random.default_rng(d * nq)
    n, k = 30_000, 32
    xb, xq = _gauss(rng, n, d) * np.float32(3 * scale), _gauss(rng, nq, d)
    if scale != 1:
        stored = np.abs(half_round(xb[:256]))
        assert np.mean((stored < 2.0 ** -14) & (stored > 0)) > 0.9, "the half copies should be mostly subnormal and nonzero"
    plain = FlatIndex(d, device=gpu)
    plain.add(xb)
    Dp, Ip = plain.search(xq, k)
    idx = _index(gpu, xb, d)
    _, _, _, eps = idx.search_exact_f32(torch.from_numpy(xq).to(gpu), k)
    eps = eps.cpu().numpy().astype(np.float64)
    true = np.einsum("qd,qkd->qk", xq.astype(np.float64), xb[Ip].astype(np.float64))
    err = np.abs(Dp.astype(np.float64) - true)
    assert np.all(np.isfinite(eps)) and np.all(err <= eps[:, None]), float((err / eps[:, None]).max())


def test_certified_lists_are_right_on_adversarial_data(gpu):
    """A dense cluster of near-duplicate rows around each query, list_len = k: many proofs fail, but every query the device
    certifies (exact = 1) has the oracle's ids."""
    rng = np.random.default_rng(5)
    d, nq, k, per = 768, 32, 10, 300
    xq = _gauss(rng, nq, d)
    xb = np.concatenate([_gauss(rng, 5_000, d)] +
                        [q[None, :] + rng.standard_normal((per, d)).astype(np.float32) * np.float32(s) for q in xq for s in (1e-3,)]).astype(np.float32)
    idx = _index(gpu, xb, d)
    D, I, exact, _ = idx.search_exact_f32(torch.from_numpy(xq).to(gpu), k, list_len=k)
    exact = exact.cpu().numpy().astype(bool)
    Dref, Iref = _oracle(xb, xq, k)
    assert np.array_equal(I.cpu().numpy()[exact], Iref[exact]) and np.array_equal(D.cpu().numpy()[exact], Dref[exact])
    assert (~exact).any(), "the data should defeat some proofs at list_len = k"
    D2, I2 = idx.search(xq, k)
    _equal(D2, I2, Dref, Iref)


def _duplicates(rng, n_dup, d):
    """n_dup rows that all round to ONE f16 row (relative perturbations below half an f16 ulp) but differ in f32."""
    v = half_round(_gauss(rng, 1, d))[0]
    return (v[None, :] * (1 + rng.uniform(-1e-4, 1e-4, size=(n_dup, d)))).astype(np.float32), v


@pytest.mark.parametrize("k", [5, 100])
def test_retry_and_exact_fallback(gpu, k):
    """More than 1024 rows within eps of the k-th score (near duplicates of one f16 row): no list proves those queries, the
    exact f32 scan answers them.  A mixed batch (ordinary queries beside them) still equals the oracle."""
    rng = np.random.default_rng(k)
    d = 768
    dup, v = _duplicates(rng, 3_000, d)
    xb = np.concatenate([_gauss(rng, 7_000, d), dup, _gauss(rng, 3_000, d)]).astype(np.float32)
    xq = _gauss(rng, 24, d)
    xq[::3] = v + _gauss(rng, 8, d) * np.float32(0.01)       # every third query points at the duplicates
    idx = _index(gpu, xb, d)
    D, I = idx.search(xq, k)
    _equal(D, I, *_oracle(xb, xq, k))
    assert idx.faithful_fallbacks > 0 and idx.faithful_fallbacks < len(xq)
    assert idx.faithful_retries >= idx.faithful_fallbacks


def test_route_mask(gpu):
    rng = np.random.default_rng(9)
    d, nq, k = 1024, 40, 32
    xb, xq = _gauss(rng, 20_000, d), _gauss(rng, nq, d)
    idx = _index(gpu, xb, d)
    prep = idx.prepare_queries(xq)
    Du, Iu = (t.cpu().numpy() for t in idx.search_prepared(prep, k))
    mask2 = torch.from_numpy(rng.integers(0, 2, size=(nq, 3)).astype(np.uint8)).to(gpu)
    mask = mask2[:, 1]                                     # a strided column of the router's mask
    D, I = (t.cpu().numpy() for t in idx.search_prepared(prep, k, id_offset=7 << 40, route_mask=mask))
    keep = mask.cpu().numpy().astype(bool)
    assert np.all(I[~keep] == -1) and np.all(np.isneginf(D[~keep]))
    assert np.array_equal(I[keep], Iu[keep] + (7 << 40)) and np.array_equal(D[keep], Du[keep])


def test_segmented_index_with_mask(gpu):
    from oracle import oracle as O
    from ragroute_amd.flat_index import SegmentedIndex
    rng = np.random.default_rng(21)
    d, nq, k = 768, 50, 32
    parts = [_gauss(rng, n, d) for n in (3_000, 700, 9_001, 1)]
    seg = SegmentedIndex(d, [p.shape[0] for p in parts], mask_cols=[2, 0, 3, 1], device=gpu, exact_f32=True)
    for s, p in enumerate(parts):
        seg.fill(s, p)
    xq = _gauss(rng, nq, d)
    mask = rng.integers(0, 2, size=(nq, 4)).astype(np.uint8)
    mask[0] = 0                                            # a query routed nowhere
    D, I = seg.search(xq, k, route_mask=mask)
    cols = []
    for s, p in enumerate(parts):
        Ds, Is = O.flat_search_ip(p, xq, k)
        keep = mask[:, seg.mask_cols[s]].astype(bool)[:, None]
        cols.append((np.where(keep, Ds, -np.inf).astype(np.float32), np.where(keep & (Is >= 0), Is + (s << 40), -1)))
    Dref, Iref = O.merge_topk(np.concatenate([c[0] for c in cols], 1), np.concatenate([c[1] for c in cols], 1), k, True)
    _equal(D, I, Dref, Iref)
    assert np.all(I[0] == -1)


def test_two_adds_equal_one(gpu):
    rng = np.random.default_rng(4)
    d, k = 768, 32
    xb, xq = _gauss(rng, 30_000, d), _gauss(rng, 20, d)
    one = _index(gpu, xb, d, "cosine")
    two = _index(gpu, xb[:11_111], d, "cosine")
    two.add(xb[11_111:])
    D1, I1 = one.search(xq, k)
    D2, I2 = two.search(xq, k)
    _equal(D2, I2, D1, I1)
    assert torch.equal(one._fstats, two._fstats)


def test_deterministic(gpu):
    rng = np.random.default_rng(6)
    d, k = 2048, 100
    xb, xq = _gauss(rng, 20_000, d), _gauss(rng, 100, d)
    idx = _index(gpu, xb, d, dtype="bf16")
    a = idx.search_exact_f32(torch.from_numpy(xq).to(gpu), k)
    b = idx.search_exact_f32(torch.from_numpy(xq).to(gpu), k)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_constructor_rejections_on_device(gpu):
    from ragroute_amd import _lib
    idx = _index(gpu, _gauss(np.random.default_rng(0), 10, 128), 128)
    with pytest.raises(_lib.RagrouteHipError):
        idx.build_screen()
    with pytest.raises(_lib.RagrouteHipError):
        idx.adopt(idx.xb)


def test_data_source_serves_f32_scores(gpu, monkeypatch):
    from ragroute_amd import data_source as DS
    monkeypatch.setenv("RAGROUTE_EXACT_F32", "1")
    rng = np.random.default_rng(8)
    n, d, k = 4_000, 768, 32
    xb, xq = _gauss(rng, n, d), _gauss(rng, 6, d)
    ws = DS.DataSource(3, "wikipedia", "3")
    ws.set_index(xb, [], [f"title {i}" for i in range(n)], [f"text {i}" for i in range(n)])
    assert ws.faiss_indexes[0].exact_f32
    replies = ws.retrieve_docs_wikipedia(xq.copy(), k)     # (normalised in place by the data source)
    Dref, Iref = _oracle(xb, _lib_normalised(xq), k)
    for q, (rows, docs, scores) in enumerate(replies):
        assert list(rows) == Iref[q].tolist()
        assert np.array_equal(np.asarray(scores, np.float32), Dref[q])
        assert docs[0] == (f"title {Iref[q, 0]}", f"text {Iref[q, 0]}")
