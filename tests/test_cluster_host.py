"""CPU: the host side of ragroute_amd/cluster.py (write_federation writes what DataSource("wikipedia") and Router.load_router read) and
the numpy references of tests/cluster_cases.py against brute-force loops."""
import json
import os
import pickle

import numpy as np
import pytest

from tests import cluster_cases as K
from tests.util import synth_router_case


def test_write_federation_layout_round_trips(tmp_path):
    from ragroute_amd.cluster import write_federation
    from ragroute_amd.data_source import read_faiss_flat_index
    rng = np.random.default_rng(5)
    n, d, C = 41, 12, 3
    x = rng.standard_normal((n, d)).astype(np.float32)
    assign = rng.integers(0, C, size=n)
    assign[7] = -1                                                   # an unassigned row belongs to no file
    titles = [f"title {r}" for r in range(n)]
    texts = [f"text of row {r}" for r in range(n)]
    stats = [{"centroid": x[assign == c].mean(0).tolist(), "size": int((assign == c).sum())} for c in range(C)]
    for metric, fourcc in (("l2", b"IxF2"), ("ip", b"IxFI")):
        root = tmp_path / metric
        write_federation(str(root), x, assign, stats, titles, texts, metric=metric)
        base = root / "faiss_clusters"
        for c in range(C):
            path = base / "normalized_indexes" / f"faiss_index_{c}_normalized.index"
            assert open(path, "rb").read(4) == fourcc
            got, m = read_faiss_flat_index(str(path), mmap=False)
            rows = np.flatnonzero(assign == c)                       # ascending original order
            assert m == metric and np.array_equal(got, x[rows])
            split = base / "split_texts_titles"
            assert open(split / f"titles_{c}.txt", encoding="utf-8").read().splitlines() == [titles[r] for r in rows]
            assert open(split / f"texts_{c}.txt", encoding="utf-8").read().splitlines() == [texts[r] for r in rows]
        assert json.load(open(base / "cluster_stats.json")) == stats
    # without titles / texts the layout still loads: one (empty) line per row
    write_federation(str(tmp_path / "bare"), x, assign, stats)
    lines = open(tmp_path / "bare" / "faiss_clusters" / "split_texts_titles" / "texts_1.txt").read().splitlines()
    assert lines == [""] * int((assign == 1).sum())
    with pytest.raises(ValueError):
        write_federation(str(tmp_path / "bad"), x, assign[:-1], stats)


def test_cluster_stats_file_loads_through_the_router(tmp_path):
    """cluster_stats.json as write_federation writes it is the list Router.load_router indexes by cluster number (wikipedia)."""
    import torch
    from sklearn.preprocessing import StandardScaler
    from ragroute_amd.cluster import write_federation
    from ragroute_amd.router import Router
    case = synth_router_case("wikipedia", 32)
    C, d = len(case["sources"]), 40
    rng = np.random.default_rng(6)
    x = rng.standard_normal((200, d)).astype(np.float32)
    assign = np.arange(200) % C
    stats = [{"centroid": x[assign == c].mean(0).tolist(), "size": int((assign == c).sum())} for c in range(C)]
    write_federation(str(tmp_path), x, assign, stats)
    model, pk = tmp_path / "best_model.pth", tmp_path / "scaler.pkl"
    torch.save({k: torch.from_numpy(v) for k, v in case["sd"].items()}, model)
    sc = StandardScaler()
    sc.mean_, sc.scale_ = case["scaler"]
    pickle.dump(sc, open(pk, "wb"))
    f = os.path.join(str(tmp_path), "faiss_clusters", "cluster_stats.json")
    r = Router("wikipedia", case["sources"], "ragroute")
    r.load_router(model_path=str(model), scaler_path=str(pk), stats_files={c: f for c in case["sources"]})
    for c in case["sources"]:
        want = np.asarray(stats[int(c)]["centroid"], np.float32)
        assert np.array_equal(r.centroids[c][:d], want) and not r.centroids[c][d:].any()


def test_references_agree_with_brute_force():
    x, c, bias = K.int_case(11, 23, 7, 5, nz=2)                      # two live columns: many ties
    for b in (None, bias):
        a, s = K.ref_assign_exact(x, c, b)
        ab, sb = K.brute_assign(x, c, b)
        assert np.array_equal(a, ab) and np.array_equal(s, sb)
    s64, tol = K.score_bound(x, c, bias, 128)
    assert np.array_equal(s64, (x.astype(np.float64) @ c.astype(np.float64).T) - bias[None, :]) and (tol >= 0).all()
    ties = ((s64 == s64.max(1, keepdims=True)).sum(1) > 1).mean()
    assert K.check_assignment_within_bound(K.ref_assign_exact(x, c, bias)[0], s64, tol) >= ties
    with pytest.raises(AssertionError):                                # a wrong assignment on a row with a clear winner is caught
        worst = np.argmin(s64, axis=1).astype(np.int32)
        K.check_assignment_within_bound(worst, s64, tol)
    labels = np.array([0, 2, 2, -1, 4, 0, 7] + [1] * 16)              # -1 and 7 are skipped, cluster 3 is empty
    m, cnt, abs_sums = K.ref_means64(x, labels, 5)
    mb, cb = K.brute_means(x, labels, 5)
    assert np.array_equal(cnt, cb) and np.allclose(m, mb, rtol=0, atol=1e-12) and cnt[3] == 0 and cnt.sum() == 21
    prev = np.full((5, 7), 9.0)
    assert (K.ref_means64(x, labels, 5, prev)[0][3] == 9.0).all()
    assert (K.means_bound(m, cnt, abs_sums) >= 0).all()


def test_gauss_recipe_is_the_issue_s():
    x, c = K.gauss_case(50, 100, 17, "bf16")
    rng = np.random.default_rng(0)
    want = (rng.standard_normal((50, 100)) / 10.0).astype(np.float32)
    import torch
    assert np.array_equal(x, torch.from_numpy(want).to(torch.bfloat16).float().numpy())
    assert c.shape == (17, 100) and abs(float((x.astype(np.float64) ** 2).sum(1).mean()) - 1.0) < 0.1
