"""GPU parity of the segmented squared-L2 search (`rr_flat_search_segments_l2`, SegmentedIndex(metric="l2")): ONE pass over the
sources of one encoder under the L2 metric, against the oracle CHAIN of the reference's wikipedia flow — every selected source
answers with its own k nearest rows (`index.search` on an IndexFlatL2 file, data_source.py:203), the front-end concatenates the
replies (http_server.py:280-293) and keeps the k LOWEST scores (rerank.py:28-34).  Embeddings are small integers, so every dot
product, every |x|^2 / 2 and every distance is exact in f32: ids and distances must match bit for bit, ties included (ties:
ascending global id = (source order, row)).  The oracle is the checker only."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_segments_gpu import CASES
from tests.util import half_round, int_data

pytestmark = pytest.mark.gpu
SHIFT = 40


def oracle_chain_l2(parts, xq, k, mask, sids=None):
    """per-source oracle L2 top-k (ids + sid << 40) -> unrouted sources (+inf, -1) -> concat -> oracle ascending merge"""
    from oracle import oracle as O
    nq = xq.shape[0]
    sids = list(range(len(parts))) if sids is None else sids
    Ds, Is = [], []
    for p, sid in zip(parts, sids):
        if p.shape[0] == 0:
            D, I = np.full((nq, k), np.inf, np.float32), np.full((nq, k), -1, np.int64)
        else:
            D, I = O.flat_search_l2(p, xq, k)
            I = np.where(I >= 0, I + (sid << SHIFT), -1)
        if mask is not None:
            keep = mask[:, sid][:, None]
            D, I = np.where(keep, D, np.inf).astype(np.float32), np.where(keep, I, -1)
        Ds.append(D)
        Is.append(I)
    return O.merge_topk(np.concatenate(Ds, 1), np.concatenate(Is, 1), k, False)


def build(parts, d, gpu, dtype="fp16", sids=None, poison=True):
    """SegmentedIndex(metric="l2") whose alignment gaps hold garbage in the matrix (NaN, 60000) AND in the norm array (NaN, +-inf,
    -60000: a gap row may score anything, +inf included) before the sources are filled in: scanned, never returned, never counted."""
    from ragroute_amd.flat_index import SegmentedIndex
    sids = list(range(len(parts))) if sids is None else sids
    seg = SegmentedIndex(d, [p.shape[0] for p in parts], id_offsets=[s << SHIFT for s in sids], mask_cols=sids, metric="l2",
                         dtype=dtype, device=gpu)
    if poison and seg.n_rows_total > 0:
        seg._xb.fill_(float("nan"))
        seg._xb[::7] = 60000.0
        seg._hn.fill_(float("nan"))
        seg._hn[::3] = float("-inf")
        seg._hn[1::3] = -60000.0
        seg._hn[::11] = float("inf")
    for s, p in enumerate(parts):
        if p.shape[0]:
            seg.fill(s, p)
    return seg


def check(D, I, Dr, Ir):
    assert np.array_equal(I, Ir), (np.argwhere(I != Ir)[:5], I[I != Ir][:5], Ir[I != Ir][:5])
    assert np.array_equal(D, Dr), (np.argwhere(D != Dr)[:5], D[D != Dr][:5], Dr[D != Dr][:5])


@pytest.mark.parametrize("d,rows,nq,k", CASES)
def test_segmented_l2_search_equals_the_oracle_chain(gpu, d, rows, nq, k):
    rng = np.random.default_rng(sum(rows) + d + nq + 1)
    parts = [int_data(rng, n, d, -2, 3) for n in rows]
    xq = int_data(rng, nq, d, -2, 3)
    mask = rng.integers(0, 2, size=(nq, len(rows))).astype(bool)
    mask[0] = False                    # a query routed nowhere: all padding (+inf, -1)
    if nq > 1:
        mask[1] = True
    seg = build(parts, d, gpu)
    for m in (mask, None):
        D, I = seg.search(xq, k, route_mask=m)
        Dr, Ir = oracle_chain_l2(parts, xq, k, m)
        check(D, I, Dr, Ir)
        if m is not None:
            assert np.all(I[0] == -1) and np.all(np.isposinf(D[0]))
    assert (I[1] >= 0).sum() == min(k, sum(rows))


def test_segmented_l2_fewer_rows_than_k_pads_with_plus_inf(gpu):
    rng = np.random.default_rng(5)
    parts = [int_data(rng, n, 768) for n in (3, 0, 4)]
    xq = int_data(rng, 9, 768)
    D, I = build(parts, 768, gpu).search(xq, 10)
    Dr, Ir = oracle_chain_l2(parts, xq, 10, None)
    check(D, I, Dr, Ir)
    assert np.all(I[:, 7:] == -1) and np.all(np.isposinf(D[:, 7:])) and np.all(I[:, :7] >= 0)


def test_segmented_l2_all_ties(gpu):
    """Every row is at the same distance: the k lowest global ids of the routed sources, whatever the scan order."""
    parts = [np.ones((5000, 256), np.float32), np.ones((300, 256), np.float32), np.ones((12_000, 256), np.float32)]
    xq = np.ones((20, 256), np.float32)
    mask = np.ones((20, 3), bool)
    mask[3, 0] = False
    mask[4, :2] = False
    seg = build(parts, 256, gpu)
    D, I = seg.search(xq, 32, route_mask=mask)
    Dr, Ir = oracle_chain_l2(parts, xq, 32, mask)
    check(D, I, Dr, Ir)
    assert I[3, 0] == (1 << SHIFT) and I[4, 0] == (2 << SHIFT) and I[0, 0] == 0
    assert np.array_equal(I[0], np.arange(32)) and np.all(D == 0)


def test_segmented_l2_bf16_storage_and_a_single_query(gpu):
    rng = np.random.default_rng(41)
    parts = [int_data(rng, n, 768) for n in (30_000, 77, 12_345)]
    for nq in (1, 33):
        xq = int_data(rng, nq, 768)
        mask = rng.integers(0, 2, size=(nq, 3)).astype(bool)
        mask[0, 2] = True
        seg = build(parts, 768, gpu, dtype="bf16")
        D, I = seg.search(xq, 10, route_mask=mask)
        Dr, Ir = oracle_chain_l2(parts, xq, 10, mask)
        check(D, I, Dr, Ir)


def test_segmented_l2_mask_columns_and_id_offsets_are_the_callers(gpu):
    rng = np.random.default_rng(3)
    sids = [2, 5, 11]
    parts = [int_data(rng, n, 768) for n in (20_000, 700, 33_000)]
    xq = int_data(rng, 64, 768)
    mask = rng.integers(0, 2, size=(64, 13)).astype(bool)
    D, I = build(parts, 768, gpu, sids=sids).search(xq, 10, route_mask=mask)
    Dr, Ir = oracle_chain_l2(parts, xq, 10, mask, sids)
    check(D, I, Dr, Ir)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_segmented_l2_gaussian(gpu, dtype):
    """Real-valued rows rounded to the storage type: the tolerances of tests/test_flat_search_gpu.py::test_l2_metric_gaussian, the
    project's figures for this metric (the distance is |q|^2 - 2 (q.x - |x|^2/2) in f32 on both sides of ~d-sized terms)."""
    rng = np.random.default_rng(12)
    rows, d, nq, k = [60_000, 2_000, 45_000], 768, 16, 10
    parts = [half_round(rng.standard_normal((n, d)).astype(np.float32), dtype) for n in rows]
    xq = half_round(rng.standard_normal((nq, d)).astype(np.float32), dtype)
    mask = rng.integers(0, 2, size=(nq, 3)).astype(bool)
    mask[:, 0] |= ~mask.any(1)
    D, I = build(parts, d, gpu, dtype=dtype).search(xq, k, route_mask=mask)
    Dr, Ir = oracle_chain_l2(parts, xq, k, mask)
    print("max |D - Dref|", float(np.abs(D - Dr).max()), "mean id overlap", np.mean([len(set(I[q]) & set(Ir[q])) / k for q in range(nq)]))
    assert np.allclose(D, Dr, rtol=2e-5, atol=2e-2)
    assert np.mean([len(set(I[q]) & set(Ir[q])) / k for q in range(nq)]) >= 0.99


def test_segment_slices_serve_the_per_source_l2_surface_on_the_same_memory(gpu):
    """SegmentedIndex.source(s) is an L2 FlatIndex on the slice and on the matching slice of the norms (no copy); it answers like a
    standalone L2 FlatIndex on the same rows, and the per-source answers merged ascending are the one-pass answer."""
    from ragroute_amd.flat_index import FlatIndex
    from ragroute_amd.rerank import merge_topk
    rng = np.random.default_rng(12)
    parts = [int_data(rng, n, 768) for n in (15_000, 333, 21_000)]
    xq = int_data(rng, 32, 768)
    seg = build(parts, 768, gpu)
    Ds, Is = [], []
    for s, p in enumerate(parts):
        idx = seg.source(s)
        assert idx.metric == "l2" and idx.xb.data_ptr() == seg.rows_of(s).data_ptr() and idx._hn.data_ptr() == seg.norms_of(s).data_ptr()
        alone = FlatIndex(768, metric="l2", device=gpu)
        alone.add(p)
        assert torch.equal(alone._hn[: alone.ntotal], idx._hn)
        D, I = idx.search_prepared(idx.prepare_queries(xq), 32, id_offset=s << SHIFT)
        Da, Ia = alone.search_prepared(alone.prepare_queries(xq), 32, id_offset=s << SHIFT)
        assert torch.equal(I, Ia) and torch.equal(D, Da)
        Ds.append(D)
        Is.append(I)
    Dm, Im = merge_topk(torch.cat(Ds, 1), torch.cat(Is, 1), 32, False)
    D1, I1 = seg.search_prepared(seg.prepare_queries(xq), 32)
    assert torch.equal(I1, Im) and torch.equal(D1, Dm)


def test_from_indexes_carries_the_norms_over(gpu):
    from ragroute_amd.flat_index import FlatIndex, SegmentedIndex
    rng = np.random.default_rng(9)
    parts = [int_data(rng, n, 384) for n in (9_000, 0, 5_001)]
    idxs = []
    for p in parts:
        idx = FlatIndex(384, metric="l2", device=gpu)
        if p.shape[0]:
            idx.add(p)
        idxs.append(idx)
    xq = int_data(rng, 17, 384)
    before = [i.search(xq, 5) for i in idxs]
    seg = SegmentedIndex.from_indexes(idxs)
    assert seg.metric == "l2"
    for s, (i, (D0, I0)) in enumerate(zip(idxs, before)):
        assert i.xb.data_ptr() == seg.rows_of(s).data_ptr() or i.ntotal == 0
        D, I = i.search(xq, 5)
        assert np.array_equal(I, I0) and np.array_equal(D, D0)
    D, I = seg.search(xq, 5)
    Dr, Ir = oracle_chain_l2(parts, xq, 5, None)
    check(D, I, Dr, Ir)


def test_three_repeated_searches_are_identical(gpu):
    rng = np.random.default_rng(77)
    parts = [int_data(rng, n, 1024) for n in (30_000, 3_633, 8_674, 25_000)]
    xq = int_data(rng, 256, 1024)
    mask = torch.from_numpy(rng.integers(0, 2, size=(256, 4)).astype(bool)).to(gpu)
    seg = build(parts, 1024, gpu)
    q = seg.prepare_queries(xq)
    res = [tuple(t.clone() for t in seg.search_prepared(q, 10, route_mask=mask)) for _ in range(3)]
    for D, I in res[1:]:
        assert torch.equal(I, res[0][1]) and torch.equal(D, res[0][0])


def test_torch_op_reaches_the_segmented_l2_search(gpu):
    import ragroute_amd.torch_ops  # noqa: F401  (registers the ops)
    rng = np.random.default_rng(31)
    parts = [int_data(rng, n, 768) for n in (9_000, 100, 30_000)]
    xq = int_data(rng, 24, 768)
    mask = rng.integers(0, 2, size=(24, 3)).astype(bool)
    seg = build(parts, 768, gpu)
    q = seg.prepare_queries(xq)
    m = torch.from_numpy(mask).to(gpu)
    Dr, Ir = oracle_chain_l2(parts, xq, 10, mask)
    D, I = torch.ops.ragroute.flat_topk_segments(seg._xb, seg.begins, seg.rows, seg.id_offsets, seg.mask_cols, q, 10, m, True, seg._hn)
    check(D.cpu().numpy(), I.cpu().numpy(), Dr, Ir)
    # without the norms the op computes them itself (gap rows hold NaN / 60000: their norms are garbage again, and unused)
    D, I = torch.ops.ragroute.flat_topk_segments(seg._xb, seg.begins, seg.rows, seg.id_offsets, seg.mask_cols, q, 10, m, l2=True)
    check(D.cpu().numpy(), I.cpu().numpy(), Dr, Ir)


# ---- guard pages: the matrix AND the norm array end flush against unmapped addresses --------------------------------------------
def _run_guarded(dev):
    from ragroute_amd.flat_index import SegmentedIndex
    from tests.test_guard_pages_gpu import _flush_to_end
    rng = np.random.default_rng(23)
    for d, rows, nqs in [(768, [20_000, 333, 13_001], (1, 256)), (1024, [9_000, 17_777], (100, 200, 256)), (4096, [9_001, 5_003], (3, 180, 256)),
                         (768, [300, 5, 4100], (7,))]:
        parts = [int_data(rng, n, d) for n in rows]
        seg = SegmentedIndex(d, rows, metric="l2", device=dev)
        host = torch.zeros((seg.n_rows_total, seg.dim), dtype=torch.float16)
        norms = torch.zeros(seg.n_rows_total, dtype=torch.float32)
        for s_, p in enumerate(parts):
            host[seg.begins[s_]: seg.begins[s_] + rows[s_], :d] = torch.from_numpy(p).half()
            norms[seg.begins[s_]: seg.begins[s_] + rows[s_]] = torch.from_numpy(0.5 * (p.astype(np.float64) ** 2).sum(1)).float()
        keep_b, arena = _flush_to_end(host, dev)
        keep_n, hn = _flush_to_end(norms, dev)
        seg._xb, seg._hn = arena, hn                              # matrix and norms now end with their device mappings
        for nq in nqs:
            xq = int_data(rng, nq, d)
            xq_h = torch.zeros((nq, seg.dim), dtype=torch.float16)
            xq_h[:, :d] = torch.from_numpy(xq).half()
            keep_q, xq_dev = _flush_to_end(xq_h, dev)
            mask = torch.from_numpy(rng.integers(0, 2, size=(nq, len(rows))).astype(np.uint8)).to(dev)
            D, I = seg.search_prepared(xq_dev, 10, route_mask=mask)
            torch.cuda.synchronize()
            Dr, Ir = oracle_chain_l2(parts, xq, 10, mask.cpu().numpy().astype(bool))
            assert np.array_equal(I.cpu().numpy(), Ir) and np.array_equal(D.cpu().numpy(), Dr), (d, rows, nq)
            del keep_q
        del keep_b, keep_n


def test_no_read_past_the_end_of_matrix_or_norms(gpu):
    """tests/test_guard_pages_gpu.py's layout for rr_flat_search_segments_l2: an over-read is a GPU fault that takes the process down,
    so the layout runs in a child process and fails this one test."""
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    code = "import torch, tests.test_segments_l2_gpu as t; t._run_guarded(torch.device('cuda:0')); print('ok')"
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "ok" in res.stdout, (res.returncode, res.stdout[-500:], res.stderr[-2000:])


# ---- pipeline and placement -----------------------------------------------------------------------------------------------------
class _FixedRouter:
    def __init__(self, mask):
        self.mask = mask

    def run(self, xq_models):
        return None, self.mask


def _wikipedia_like(rng, d=768):
    """Ten L2 sources of one key (the reference's wikipedia federation: ten clusters behind one DPR encoder, config.py:59-70)."""
    rows = [12_000, 5_000, 3_633, 9_000, 700, 20_000, 1, 8_192, 257, 15_000]
    return rows, [int_data(rng, n, d) for n in rows]


@pytest.mark.parametrize("routed", [True, False])
def test_pipeline_packs_l2_sources_of_one_key(gpu, routed):
    from ragroute_amd.flat_index import FlatIndex
    from ragroute_amd.pipeline import RetrievalPipeline
    rng = np.random.default_rng(21)
    rows, parts = _wikipedia_like(rng)
    nq, k = 40, 10
    xq = int_data(rng, nq, 768)
    mask = rng.integers(0, 2, size=(nq, 10)).astype(bool)
    mask[0] = False
    router = _FixedRouter(torch.from_numpy(mask).to(gpu)) if routed else None

    def make():
        out = []
        for p in parts:
            idx = FlatIndex(768, metric="l2", device=gpu)
            idx.add(p)
            out.append(idx)
        return out

    plain = RetrievalPipeline(make(), list(range(10)), router=router)
    packed = RetrievalPipeline(make(), list(range(10)), router=router, share_queries=["dpr"] * 10)
    assert [u[0] for u in packed.units] == ["segments"] and packed.units[0][1].metric == "l2"
    assert not plain.descending and not packed.descending
    q = torch.from_numpy(xq).to(gpu)
    zeros = torch.zeros(nq, 1, 1, device=gpu)
    D0, I0 = plain.search(q, k, xq_models=zeros)
    D1, I1 = packed.search(q, k, xq_models=zeros)
    assert packed.slots == 1 and plain.slots == 10
    assert torch.equal(I0, I1) and torch.equal(D0, D1)
    Dr, Ir = oracle_chain_l2(parts, xq, k, mask if routed else None)
    check(D1.cpu().numpy(), I1.cpu().numpy(), Dr, Ir)
    # more exchange slots than units: the unused slots are padding that must lose an ASCENDING merge
    spare = RetrievalPipeline(make(), list(range(10)), router=router, share_queries=["dpr"] * 10, slots=3)
    D2, I2 = spare.search(q, k, xq_models=zeros)
    assert torch.equal(I2, I1) and torch.equal(D2, D1)


def test_placement_with_grouped_l2_sources_gives_the_one_gpu_result(gpu):
    """plan(..., 4, group_l2=True): the federation's L2 sources cut into row slices over four ranks, every rank's units searched here
    in turn (one device) and merged ascending, as the exchange + merge of four processes would."""
    from ragroute_amd import placement as PL
    from ragroute_amd.flat_index import SegmentedIndex
    from ragroute_amd.pipeline import RetrievalPipeline
    from ragroute_amd.rerank import merge_topk
    rng = np.random.default_rng(22)
    rows, parts = _wikipedia_like(rng)
    nq, k = 40, 10
    xq = int_data(rng, nq, 768)
    mask = rng.integers(0, 2, size=(nq, 10)).astype(bool)
    mask[0] = False
    fed = [PL.Source(s, n, 768, "dpr", "l2", "fp16", f"cluster{s}") for s, n in enumerate(rows)]
    plan = PL.plan(fed, 4, cost=PL.CostModel(fixed_ms=1e-6, segment_ms=0.0), min_slice_rows=2048, group_l2=True)
    assert sum(len(plan.slices_of(s.sid)) - 1 for s in fed) >= 1, "the plan should cut a source"
    assert all(len(units) == 1 for units in plan.ranks), "one unit per rank: the L2 pieces of one encoder share a search"
    q = torch.from_numpy(xq).to(gpu)
    zeros = torch.zeros(nq, 1, 1, device=gpu)
    router = _FixedRouter(torch.from_numpy(mask).to(gpu))
    per_rank = []
    for rk in range(4):
        pipe = RetrievalPipeline.from_placement(plan, rk, rows_f32=lambda sid, a, b: parts[sid][a:b], router=router, device=gpu)
        assert not pipe.descending
        assert len(pipe.units) == 1 and isinstance(pipe.units[0][1], SegmentedIndex) and pipe.units[0][1].metric == "l2"
        per_rank.append(pipe.search({s.sid: q for s in fed}, k, xq_models=zeros))
    D, I = merge_topk(torch.cat([d for d, _ in per_rank], 1), torch.cat([i for _, i in per_rank], 1), k, False)
    one = RetrievalPipeline.from_placement(PL.plan(fed, 1, group_l2=True), 0, rows_f32=lambda sid, a, b: parts[sid][a:b], router=router, device=gpu)
    D1, I1 = one.search({s.sid: q for s in fed}, k, xq_models=zeros)
    assert torch.equal(I, I1) and torch.equal(D, D1)
    Dr, Ir = oracle_chain_l2(parts, xq, k, mask)
    check(D.cpu().numpy(), I.cpu().numpy(), Dr, Ir)


def test_a_pipeline_of_mixed_metrics_raises(gpu):
    from ragroute_amd.flat_index import FlatIndex
    from ragroute_amd.pipeline import RetrievalPipeline
    a, b, c = FlatIndex(768, metric="l2", device=gpu), FlatIndex(768, metric="ip", device=gpu), FlatIndex(768, metric="cosine", device=gpu)
    with pytest.raises(ValueError, match="l2"):
        RetrievalPipeline([a, b], [0, 1])
    with pytest.raises(ValueError, match="l2"):
        RetrievalPipeline([a, c], [0, 1], share_queries=["x", "x"])
    with pytest.raises(ValueError, match="l2"):
        RetrievalPipeline([], [], units=[(a, [0]), (b, [1])])
    RetrievalPipeline([b, c], [0, 1])          # scores of ip and cosine sources merge as before
